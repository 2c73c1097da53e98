"""Worker of tests/test_gpu_desc_head_2wg.py and tests/test_gpu_convpb_stores.py (not a test module).

    python tests/_tail_ab.py desc|convpb <superpoint.safetensors> <out.npz>

Runs every case of one of the two tail kernels of csrc/sp_convs.hip through the test-only entries sship_sp_debug_desc_head /
sship_sp_debug_convpb on seeded inputs and saves the raw outputs.  The kernel form is chosen by the caller: the developer-build switches
SUPERSLAM_HIP_DESC_HEAD / SUPERSLAM_HIP_CONVPB are read once per process, so every form runs in its own interpreter (SSHIP_DEV_LIBRARY names
the developer build, as in tests/test_gpu_alt_paths.py); without them the shipped library runs its one path."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MAPS = ((2, 3), (8, 12), (47, 172))          # Hc x Wc: smaller than a patch, a few tiles, the KITTI map
BATCHES = (1, 2, 5)
MAX_KP = 200                                  # not a multiple of 64: the last workgroup of an image is ragged
COUNTS = (0, 1, 63, 64, 65, 130, MAX_KP)      # per image; image b of rotation r gets COUNTS[(r + b) % 7], so every batch of 2 or 5 has an n = 0 image
BIG = (47, 172, 5, 1700)                      # Hc, Wc, batch, max_kp: 135 workgroups, the throughput form by the launcher's own rule
DESC_FILL = 0x7B7B                            # rows past an image's count stay as they were
CONVPB_P = (1, 15, 16, 17, 33, 80, 197)       # 80 = 5 tiles on 2 workgroups: three waves without a tile; 197: every wave one tile, a ragged 13th
LOGIT_FILL = 0x7FC12345                       # a NaN pattern no kernel produces


def cells_for(hc, wc, count, rot, rng):
    """`count` cells: the four corners, cells on all four edges, then the interior (where the map has one), rotated by `rot`."""
    corner = [(0, 0), (0, wc - 1), (hc - 1, 0), (hc - 1, wc - 1)]
    edge = [(0, wc // 2), (hc - 1, wc // 2), (hc // 2, 0), (hc // 2, wc - 1)]
    edge += [(0, int(x)) for x in rng.integers(0, wc, 4)] + [(hc - 1, int(x)) for x in rng.integers(0, wc, 4)]
    edge += [(int(y), 0) for y in rng.integers(0, hc, 4)] + [(int(y), wc - 1) for y in rng.integers(0, hc, 4)]
    inner = []
    if hc > 2 and wc > 2:
        inner = [(int(y), int(x)) for y, x in zip(rng.integers(1, hc - 1, 24), rng.integers(1, wc - 1, 24))]
    base = corner + edge + inner
    base = base[rot % len(base):] + base[:rot % len(base)]
    rest = [(int(y), int(x)) for y, x in zip(rng.integers(0, hc, max(0, count - len(base))), rng.integers(0, wc, max(0, count - len(base))))]
    return (base + rest)[:count]


def desc_cases():
    for hc, wc in MAPS:
        for b in BATCHES:
            for rot in range(len(COUNTS)):
                yield hc, wc, b, MAX_KP, [COUNTS[(rot + i) % len(COUNTS)] for i in range(b)], rot
    hc, wc, b, mk = BIG
    yield hc, wc, b, mk, [mk, 0, 1601, 65, 1], 0


def desc_key(hc, wc, b, rot, mk):
    return "d_%dx%d_b%d_r%d_k%d" % (hc, wc, b, rot, mk)


def desc_map(hc, wc, images=5):
    """One conv4b-like map per size (ReLU output: non-negative, a third zeros), [images, hc, wc, 128] fp16."""
    return np.maximum(np.random.default_rng(hc * wc).standard_normal((images, hc, wc, 128)).astype(np.float32) - 0.4, 0).astype(np.float16)


def desc_cells(hc, wc, b, mk, counts, rot):
    """(cell_h, cell_w) [b, mk] int32 of one case: cells_for per image, zeros past an image's count."""
    rng = np.random.default_rng(1000 * hc + 10 * b + rot)
    ch = np.zeros((b, mk), np.int32)
    cw = np.zeros((b, mk), np.int32)
    for i, n in enumerate(counts):
        c = cells_for(hc, wc, n, rot + i, rng)
        ch[i, :n] = [y for y, _ in c]
        cw[i, :n] = [x for _, x in c]
    return ch, cw


def bind_desc_head(L):
    L.sship_sp_debug_desc_head.restype = C.c_int
    L.sship_sp_debug_desc_head.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]


def run_desc_case(sp, L, dmap, hc, wc, b, mk, counts, ch, cw):
    """One sship_sp_debug_desc_head call on a device map -> the descriptor rows as int16 [b, mk, 256] (DESC_FILL where nothing was written)."""
    import torch

    d = torch.full((b, mk, 256), DESC_FILL, dtype=torch.int16).cuda()
    tch, tcw, tn = torch.from_numpy(ch).cuda(), torch.from_numpy(cw).cuda(), torch.tensor(counts, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    rc = L.sship_sp_debug_desc_head(sp._h, dmap.data_ptr(), b, hc, wc, tch.data_ptr(), tcw.data_ptr(), tn.data_ptr(), mk, d.data_ptr())
    assert rc == 0, (rc, L.sship_last_error())
    return d.cpu().numpy()


def run_desc(sp, L, out):
    import torch

    bind_desc_head(L)
    maps = {}
    for hc, wc, b, mk, counts, rot in desc_cases():
        if (hc, wc) not in maps:
            maps[(hc, wc)] = torch.from_numpy(desc_map(hc, wc)).cuda()
        ch, cw = desc_cells(hc, wc, b, mk, counts, rot)
        out[desc_key(hc, wc, b, rot, mk)] = run_desc_case(sp, L, maps[(hc, wc)], hc, wc, b, mk, counts, ch, cw)


def run_convpb(sp, L, out):
    import torch

    from superslam_amd.synth import make_frame

    L.sship_sp_debug_convpb.restype = C.c_int
    L.sship_sp_debug_convpb.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    for p in CONVPB_P:
        x = torch.from_numpy(np.maximum(np.random.default_rng(p).standard_normal((p, 256)).astype(np.float32), 0).astype(np.float16)).cuda()
        o = torch.from_numpy(np.full((p + 2, 68), LOGIT_FILL, np.uint32).view(np.int32)).cuda()   # two guard rows behind the last pixel
        torch.cuda.synchronize()
        rc = L.sship_sp_debug_convpb(sp._h, x.data_ptr(), p, o.data_ptr())
        assert rc == 0, (rc, L.sship_last_error())
        out["l_%d" % p] = o.cpu().numpy().view(np.uint32)
    imgs = torch.from_numpy(np.stack([make_frame(64, 96, 5), make_frame(64, 96, 6)])).cuda()
    desc, kp, n = sp.extract_batch_device(imgs)
    torch.cuda.synchronize()
    out["kp"], out["n"], out["desc"] = kp.cpu().numpy().view(np.uint32), n.cpu().numpy(), desc.cpu().numpy().view(np.uint16)


DEV_LIB = os.path.join(ROOT, "superslam_amd", "lib", "variants", "dev.so")


def run_worker(kind, mode_env, weights_dir, out):
    """Called by the tests: one form in its own interpreter; a mode with switches runs on the developer build, one without on the shipped library."""
    import subprocess

    env = dict(os.environ, **mode_env)
    env.pop("SSHIP_DEV_LIBRARY", None)
    if mode_env:
        assert os.path.exists(DEV_LIB), "superslam_amd/lib/variants/dev.so is missing: __graft_entry__.build() produces it"
        env["SSHIP_DEV_LIBRARY"] = DEV_LIB
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_tail_ab.py"), kind, weights_dir["sp_path"], out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


def main():
    import _devlib

    _devlib.use_dev_library()
    from superslam_amd import SuperPoint, _lib

    kind, sp_path, out_path = sys.argv[1:4]
    _lib.init(0)
    sp = SuperPoint(sp_path, 600, 0.005, 4, max_batch=2)
    assert sp.initialize(), sp.last_error
    out = {}
    (run_desc if kind == "desc" else run_convpb)(sp, _lib.lib(), out)
    sp.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
