"""GPU: steered BRIEF descriptors and the Hamming matcher (sship_brief_*, sship_hm_*; csrc/brief_kernels.hip k_brief_describe, k_hm_best,
k_hm_final) against tests/_brief_ref.py, the numpy restatement of include/sship.h "Binary descriptors" and "Hamming matcher".

Both rules are integers and comparisons, so every output equals the restatement with np.array_equal: no tolerance, nothing left out.
Sizes sit at the kernels' own edges - the smallest image (one describable pixel), keypoints on both sides of the reach, keypoint counts
around k_brief_describe's 4 waves per workgroup and k_hm_best's two numbers, ROWS and TILE below - not at the workload's size."""
import struct
import subprocess

import numpy as np
import pytest

import _brief_ref as R
import _fast_ref as F
import _pose_ref as P
from test_brief_cpu import host_layer_binary

pytestmark = pytest.mark.gpu

ROWS = 128   # kHmRows: rows of one set per workgroup of k_hm_best (one per lane)
TILE = 64    # kHmTile: rows of the other set per LDS tile
QNAN = np.float32(np.nan)
MODES = (("steered", R.STEERED), ("upright", R.UPRIGHT))


def dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == np.int32 and want.dtype == np.uint32:
        got = got.view(np.uint32)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name} {want.shape}: {len(bad)} entries differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def contents(h, w, seed):
    rng = np.random.default_rng(seed)
    return np.stack([F.smooth_noise(rng, h, w), F.white_noise(rng, h, w), F.constant(h, w), F.checkerboard(h, w)])


def keypoints(h, w, mk, seed):
    """f32 [mk, 3]: both sides of the reach in x and y, .5 fractions, NaN / Inf / negative rows, then seeded positions over the whole image"""
    rng = np.random.default_rng(seed)
    xs, ys = (15, 16, w - 17, w - 16), (15, 16, h - 17, h - 16)
    rows = [(x, y) for x in xs for y in ys]
    rows += [(15.5, 16), (15.49, 16.2), (w - 16.5, h - 17), (w - 16.51, h - 16.5), (16, 15.5), (w / 2 + 0.5, h / 2 - 0.5)]
    rows += [(QNAN, 20), (20, QNAN), (np.inf, 20), (20, -np.inf), (-1, 20), (20, -0.6), (16384, 20), (w / 2, h / 2)]
    kp = np.zeros((mk, 3), np.float32)
    kp[:, 0] = rng.uniform(0, w, mk)
    kp[:, 1] = rng.uniform(0, h, mk)
    kp[:, 2] = rng.uniform(0, 255, mk)
    m = min(len(rows), mk)
    kp[:m, :2] = np.array(rows[:m], np.float32)
    return kp[rng.permutation(mk)] if mk > 1 else kp


def describe(imgs_dev, kp, n, mode, unit_stride=1):
    from superslam_amd import brief_describe_batch

    d, s, b = brief_describe_batch(imgs_dev, dev(kp), dev(np.asarray(n, np.int32)), mode=mode, unit_stride=unit_stride, return_status=True,
                                   return_bins=True)
    return d.cpu().numpy(), s.cpu().numpy(), b.cpu().numpy()


def check_describe(name, got, want):
    for part, g, w in zip(("desc", "status", "bin"), got, want):
        same(f"{name} {part}", g, w)


# ------------------------------------------------------------------------------------------------------
# describe
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(33, 33), (40, 57), (96, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_describe_every_size_content_and_mode(size):
    h, w = size
    imgs = contents(h, w, seed=h * 3 + w)
    mk = 64
    kp = np.stack([keypoints(h, w, mk, seed=10 + i) for i in range(len(imgs))])
    if (h, w) == (33, 33):
        kp[:, 0, :2] = 16                                       # the one describable pixel
    n = np.full(len(imgs), mk, np.int32)
    src = dev(imgs)
    for name, mode in MODES:
        want = R.describe_batch(imgs, kp, n, mode)
        check_describe(f"{h}x{w} {name}", describe(src, kp, n, name), want)
        assert (want[1] == R.OK).any() and (want[1] == R.BORDER).any()
        ok = want[1][2] == R.OK                                 # the constant image: bin 0, no bit set
        assert not want[2][2][ok].any() and not want[0][2][ok].any()
    if (h, w) == (33, 33):
        assert (want[1][:, 0] == R.OK).all()


@pytest.mark.parametrize("mk", [1, 63, 64, 65, 130])
def test_describe_counts_and_max_keypoints(mk):
    h, w = 40, 57
    rng = np.random.default_rng(mk)
    imgs = np.stack([F.smooth_noise(rng, h, w) for _ in range(5)])
    kp = np.stack([keypoints(h, w, mk, seed=mk + i) for i in range(5)])
    kp[:, :, 0] = np.clip(kp[:, :, 0], 14, w - 15)              # mostly describable
    n = np.array([0, mk, mk + 7, -3, max(mk // 2, 1)], np.int32)
    for name, mode in MODES:
        want = R.describe_batch(imgs, kp, n, mode)
        check_describe(f"mk {mk} {name}", describe(dev(imgs), kp, n, name), want)
    assert not want[1][0].any() and not want[1][3].any() and (want[1][1] != R.NONE).all() and (want[1][2] != R.NONE).all()


def test_describe_strides_units_and_batch_position():
    """unit_stride 2, rows of w + 3 bytes at an odd address, image_stride 0 and 2 h stride, 70 images (17 x 70 workgroups of 4 keypoints:
    several per compute unit), row b of the batch against the same image alone, and the host entry"""
    import torch

    from superslam_amd import brief_describe

    h, w, mk, B = 40, 57, 65, 70
    rng = np.random.default_rng(5)
    imgs = np.stack([F.smooth_noise(rng, h, w) if i % 2 else F.white_noise(rng, h, w) for i in range(B)])
    kp = np.stack([keypoints(h, w, mk, seed=100 + i) for i in range(2 * B)])
    n = rng.integers(0, mk + 3, 2 * B).astype(np.int32)
    n[:4] = mk
    # rows of w + 3 bytes from an odd address
    flat = torch.full((1 + B * h * (w + 3),), 0xEE, dtype=torch.uint8, device="cuda")
    view = flat[1:].view(B, h, w + 3)[:, :, :w]
    view.copy_(dev(imgs))
    assert view.data_ptr() % 2 == 1
    for name, mode in MODES:
        want1 = R.describe_batch(imgs, kp, n, mode)
        got1 = describe(view, kp[:B], n[:B], name)
        check_describe(f"odd rows {name}", got1, want1)
        check_describe(f"contiguous {name}", describe(dev(imgs), kp[:B], n[:B], name), want1)
        want2 = R.describe_batch(imgs, kp, n, mode, unit_stride=2)
        check_describe(f"unit_stride 2 {name}", describe(view, kp, n, name, unit_stride=2), want2)
        # image_stride = 2 h stride: the left images of an L0, R0, ... batch
        half = dev(imgs)[0::2]
        check_describe(f"[0::2] {name}", describe(half, kp[:B // 2], n[:B // 2], name), R.describe_batch(imgs[0::2], kp, n, mode))
        # image_stride = 0: one image under every keypoint list
        one = dev(imgs[3:4]).expand(6, h, w)
        check_describe(f"expand {name}", describe(one, kp[:6], n[:6], name), R.describe_batch(np.repeat(imgs[3:4], 6, 0), kp, n, mode))
        # row b alone, on the device and through the host entry
        for b in (0, 1, 37, B - 1):
            alone = describe(dev(imgs[b:b + 1]), kp[b:b + 1], n[b:b + 1], name)
            check_describe(f"row {b} alone {name}", alone, tuple(g[b:b + 1] for g in got1))
            nb = min(max(int(n[b]), 0), mk)
            d, s, k = brief_describe(imgs[b], kp[b, :nb], mode=name, return_status=True, return_bins=True)
            same(f"host desc {b}", d, got1[0][b, :nb].view(np.uint32))
            same(f"host status {b}", s, got1[1][b, :nb])
            same(f"host bin {b}", k, got1[2][b, :nb])
    host = flat.cpu().numpy()
    assert host[0] == 0xEE and (host[1:].reshape(B, h, w + 3)[:, :, w:] == 0xEE).all()
    # a strided host image
    wide = np.zeros((h, w + 9), np.uint8)
    wide[:, :w] = imgs[1]
    same("host strided", brief_describe(wide[:, :w], kp[1, :mk]), brief_describe(imgs[1], kp[1, :mk]))


# ------------------------------------------------------------------------------------------------------
# match
# ------------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 2, TILE - 1, TILE, TILE + 1, ROWS - 1, ROWS, ROWS + 1)
MK = ROWS + 2
_CASE = {}


def grid_case():
    """81 pairs, every (n0, n1) of COUNTS x COUNTS, in the stereo layout: descriptors out of a small pool with a few flipped bits (many
    ties and duplicated best rows), status with holes, keypoints with NaN rows.  Shared and read-only."""
    if not _CASE:
        rng = np.random.default_rng(11)
        pairs = [(a, b) for a in COUNTS for b in COUNTS]
        U = 2 * len(pairs)
        pool = rng.integers(0, 2 ** 32, (24, 8), dtype=np.uint64).astype(np.uint32)
        desc = pool[rng.integers(0, len(pool), (U, MK))]
        flips = rng.integers(0, 4, (U, MK))
        for _ in range(3):
            word, bit = rng.integers(0, 8, (U, MK)), rng.integers(0, 32, (U, MK)).astype(np.uint32)
            sel = flips > 0
            uu, kk = np.nonzero(sel)
            desc[uu, kk, word[sel]] ^= (np.uint32(1) << bit[sel])
            flips -= 1
        n = np.array([c for p in pairs for c in p], np.int32)
        status = np.where(rng.uniform(size=(U, MK)) < 0.8, R.OK, rng.integers(0, 3, (U, MK))).astype(np.uint8)
        kp = np.zeros((U, MK, 3), np.float32)
        kp[:, :, 0] = rng.uniform(0, 200, (U, MK))
        kp[:, :, 1] = rng.uniform(0, 20, (U, MK))
        kp[rng.uniform(size=(U, MK)) < 0.05, 0] = QNAN
        kp[rng.uniform(size=(U, MK)) < 0.02, 1] = np.inf
        _CASE.update(pairs=pairs, desc=desc, n=n, status=status, kp=kp)
    return _CASE


def matcher(mk, max_pairs, **kw):
    from superslam_amd import HammingMatcher

    m = HammingMatcher(mk, max_pairs, **kw)
    assert m.initialize(), m.last_error
    return m


def ref_batch(c, layout, pairs, status=True, gate=None, **params):
    f0, s0, f1, s1 = layout
    out = []
    for p in range(pairs):
        a, b = f0 + p * s0, f1 + p * s1
        out.append(R.match(c["desc"][a], c["n"][a], c["desc"][b], c["n"][b], c["status"][a] if status else None, c["status"][b] if status else None,
                           c["kp"][a], c["kp"][b], gate, **params))
    return tuple(np.stack([o[j] for o in out]) for j in range(3))


def run_batch(m, c, layout, pairs, status=True):
    got = m.match_batch(dev(c["n"]), dev(c["desc"].view(np.int32)), dev(c["status"]) if status else None, dev(c["kp"]), layout=layout, pairs=pairs,
                        return_scores=True)
    return tuple(g.cpu().numpy() for g in got)


def check_match(name, got, want):
    for part, g, w in zip(("matches0", "dist0", "mscores0"), got, want):
        same(f"{name} {part}", g, w)


@pytest.mark.parametrize("params", [dict(), dict(max_distance=40), dict(ratio_percent=80), dict(mutual_check=False),
                                    dict(max_distance=100, ratio_percent=95, mutual_check=False)], ids=str)
def test_match_every_count_pair(params):
    c = grid_case()
    P_ = len(c["pairs"])
    assert P_ >= 70
    m = matcher(MK, P_, **params)
    for status in (False, True):
        want = ref_batch(c, (0, 2, 1, 2), P_, status=status, **params)
        check_match(f"{params} status {status}", run_batch(m, c, (0, 2, 1, 2), P_, status=status), want)
    assert (want[0] >= 0).any() and (want[0] < 0).any()


def test_match_ties_take_the_smallest_index():
    """identical descriptors everywhere: every entry ties, row 0 and column 0 win, the mutual check keeps (0, 0) alone; then a duplicated
    best row"""
    m = matcher(MK, 2)
    one = np.full((2, MK, 8), 0x5a5a5a5a, np.uint32)
    n = np.array([MK - 1, TILE + 1], np.int32)
    c = dict(desc=one, n=n, status=np.ones((2, MK), np.uint8), kp=np.zeros((2, MK, 3), np.float32))
    got = run_batch(m, c, (0, 2, 1, 2), 1, status=False)
    check_match("all equal", got, ref_batch(c, (0, 2, 1, 2), 1, status=False))
    assert got[0][0, 0] == 0 and (got[0][0, 1:] == -1).all() and got[1][0, 0] == 0 and got[2][0, 0] == 1.0
    m.set_params(mutual_check=False)
    got = run_batch(m, c, (0, 2, 1, 2), 1, status=False)
    assert (got[0][0, :MK - 1] == 0).all() and got[0][0, MK - 1] == -1
    rng = np.random.default_rng(2)
    d = rng.integers(0, 2 ** 32, (2, MK, 8), dtype=np.uint64).astype(np.uint32)
    d[1, 70] = d[0, 5]
    d[1, 3] = d[0, 5]                                           # two exact copies of row 5's best: column 3 wins
    d[1, 3 + TILE] = d[0, 5]
    c = dict(c, desc=d, n=np.array([MK, MK], np.int32))
    got = run_batch(m, c, (0, 2, 1, 2), 1, status=False)
    check_match("duplicated best", got, ref_batch(c, (0, 2, 1, 2), 1, status=False, mutual_check=False))
    assert got[0][0, 5] == 3 and got[1][0, 5] == 0


@pytest.mark.parametrize("gate", [(0.0, 64.0, -2.0, 2.0), (-12.0, 12.0, -12.0, 12.0), (-np.inf, np.inf, -np.inf, np.inf), (500.0, 600.0, 0.0, 0.0)],
                         ids=["stereo band", "track window", "open", "nothing"])
def test_match_gates(gate):
    c = grid_case()
    P_ = len(c["pairs"])
    m = matcher(MK, P_, gate=gate, ratio_percent=90)
    assert m.gate() == tuple(float(np.float32(v)) for v in gate)
    want = ref_batch(c, (0, 2, 1, 2), P_, gate=gate, ratio_percent=90)
    got = run_batch(m, c, (0, 2, 1, 2), P_)
    check_match(f"gate {gate}", got, want)
    if gate[0] == 500.0:
        assert (got[0] == -1).all()
    if np.isinf(gate[0]):
        # the open gate gives the ungated bits where no coordinate is NaN
        clean = dict(c, kp=np.nan_to_num(c["kp"], nan=1.0, posinf=2.0))
        m.clear_gate()
        assert m.gate() is None
        ungated = run_batch(m, clean, (0, 2, 1, 2), P_)
        m.set_gate(*gate)
        check_match("open == ungated", run_batch(m, clean, (0, 2, 1, 2), P_), ungated)
    with pytest.raises(ValueError):
        m.match_batch(dev(c["n"]), dev(c["desc"].view(np.int32)), layout=(0, 2, 1, 2))     # gated, no keypoints


@pytest.mark.parametrize("layout,pairs", [((0, 2, 1, 2), 9), ((0, 1, 1, 1), 17), ((0, 0, 1, 1), 17), ((5, 3, 4, 0), 4)],
                         ids=["stereo", "consecutive", "keyframe against many", "general"])
def test_match_layouts_and_batch_position(layout, pairs):
    c0 = grid_case()
    U = 18
    pick = [2 * i + 1 for i in range(U)]                        # units with every n1 of COUNTS, twice
    c = dict(desc=c0["desc"][pick], n=c0["n"][pick], status=c0["status"][pick], kp=c0["kp"][pick])
    m = matcher(MK, 32, max_distance=120)
    want = ref_batch(c, layout, pairs, max_distance=120)
    got = run_batch(m, c, layout, pairs)
    check_match(f"layout {layout}", got, want)
    f0, s0, f1, s1 = layout
    for p in (0, pairs // 2, pairs - 1):                        # the pair alone, at position 0 of its own call
        alone = run_batch(m, c, (f0 + p * s0, 0, f1 + p * s1, 0), 1)
        check_match(f"pair {p} alone", alone, tuple(g[p:p + 1] for g in got))
    with pytest.raises(ValueError):
        m.match_batch(dev(c["n"]), dev(c["desc"].view(np.int32)), layout=layout, pairs=pairs + 20)


def test_match_host_entry_and_bench():
    c = grid_case()
    m = matcher(MK, 1, ratio_percent=85)
    for p in (4, 40, 44, 76, 80, 8, 72):
        a, b = 2 * p, 2 * p + 1
        n0, n1 = int(c["n"][a]), int(c["n"][b])
        for gate in (None, (-30.0, 90.0, -5.0, 5.0)):
            m.clear_gate() if gate is None else m.set_gate(*gate)
            for status in (False, True):
                s0, s1 = (c["status"][a, :n0], c["status"][b, :n1]) if status else (None, None)
                got = m.match(c["desc"][a, :n0], c["desc"][b, :n1], s0, s1, c["kp"][a, :n0], c["kp"][b, :n1], return_scores=True)
                want = R.match(c["desc"][a, :n0], n0, c["desc"][b, :n1], n1, s0, s1, c["kp"][a, :n0], c["kp"][b, :n1], gate, ratio_percent=85)
                check_match(f"host pair {p} gate {gate} status {status}", got, want)
    assert m.bench(2) > 0.0


# ------------------------------------------------------------------------------------------------------
# the chain
# ------------------------------------------------------------------------------------------------------
def test_chain_detect_describe_match_observations():
    """FastDetector.detect on two shifted images independently -> brief_describe_batch -> HammingMatcher with a track-window gate ->
    sship_pose_obs_from_matches_batch_device takes matches0 unchanged; every stage equals the same chain on the restatements"""
    import torch

    from superslam_amd import FastDetector, PoseSolver, brief_describe_batch

    h, w, mk, shift = 96, 160, 128, (3, 2)
    rng = np.random.default_rng(21)
    big = F.smooth_noise(rng, h + 8, w + 8)
    imgs = np.stack([big[4:4 + h, 4:4 + w], big[4 - shift[1]:4 - shift[1] + h, 4 - shift[0]:4 - shift[0] + w]])
    f = FastDetector(h, w, mk, 2, border=20)
    assert f.initialize(), f.last_error
    src = dev(imgs)
    kp, n = f.detect(src)
    ref = [F.detect(I, mk, border=20) for I in imgs]
    same("kp", kp.cpu().numpy(), np.stack([r["kp"] for r in ref]))
    n_ref = np.array([r["n_out"] for r in ref], np.int32)
    same("n", n.cpu().numpy(), n_ref)
    assert n_ref.min() >= 20
    desc, status = brief_describe_batch(src, kp, n, return_status=True)
    kp_ref = np.stack([r["kp"] for r in ref])
    d_ref, s_ref, _ = R.describe_batch(imgs, kp_ref, n_ref)
    same("desc", desc.cpu().numpy(), d_ref)
    same("status", status.cpu().numpy(), s_ref)
    gate = (-6.0, 0.0, -5.0, 1.0)                               # x0 - x1 = -3, y0 - y1 = -2, +- 3
    m = matcher(mk, 1, gate=gate, max_distance=64)
    m0, dist = m.match_batch(n, desc, status, kp, layout=(0, 1, 1, 1))
    w0, wd, _ = R.match(d_ref[0], n_ref[0], d_ref[1], n_ref[1], s_ref[0], s_ref[1], kp_ref[0], kp_ref[1], gate, max_distance=64)
    same("matches0", m0.cpu().numpy()[0], w0)
    same("dist0", dist.cpu().numpy()[0], wd)
    matched = np.flatnonzero(w0 >= 0)
    assert len(matched) >= 10
    d = kp_ref[1][w0[matched], :2] - kp_ref[0][matched, :2]
    assert (d == np.array(shift, np.float32)).mean() >= 0.9      # the scene moved by `shift`
    # observations: a made-up disparity of 8 px for every keypoint
    cam = P.Camera()
    stereo = np.concatenate([kp_ref[:, :, :2], kp_ref[:, :, :1] - 8.0], 2).astype(np.float32)
    hd = (np.arange(mk)[None, :] < n_ref[:, None]).astype(np.uint8)
    ps = PoseSolver(cam.tuple(), mk, 1)
    assert ps.initialize(), ps.last_error
    pts, ms, va = ps.obs_from_matches(dev(stereo[:1]), dev(hd[:1]), dev(stereo[1:]), dev(hd[1:]), m0, n[:1], n[1:])
    torch.cuda.synchronize()
    wp, wm, wv = P.gather(stereo[0], hd[0], stereo[1], hd[1], w0, n_ref[0], n_ref[1], cam)
    assert va.cpu().numpy()[0].tobytes() == wv.tobytes() and pts.cpu().numpy()[0].tobytes() == wp.tobytes() and ms.cpu().numpy()[0].tobytes() == wm.tobytes()
    assert int(wv.sum()) == len(matched)


def test_cpp_host_layer(tmp_path):
    """superslam_hip::describe_brief and HammingMatcher::match_host (tests/cpp/test_binary_descriptor.cc gpu <file>) give the restatement's bits"""
    h, w, n, n1 = 40, 57, 65, 50
    rng = np.random.default_rng(31)
    I = F.smooth_noise(rng, h, w)
    kp = keypoints(h, w, n, seed=32)
    kp[~np.isfinite(kp)] = -3.0                                  # finite rows: the open gate then gives the ungated bits
    for mode in (R.STEERED, R.UPRIGHT):
        desc, status, bins = R.describe(I, kp, n, mode)
        d1 = desc[rng.permutation(n)[:n1]].copy()
        d1[::3, 1] ^= np.uint32(0x0f0f)
        s1 = np.where(np.arange(n1) % 7 == 0, R.BORDER, R.OK).astype(np.uint8)
        m0, dist, _ = R.match(desc, n, d1, n1, status, s1, max_distance=30)
        assert (m0 >= 0).sum() >= 5
        path = tmp_path / f"case{mode}.bin"
        path.write_bytes(struct.pack("6i", h, w, n, mode, n1, 30) + I.tobytes() + kp.tobytes() + desc.tobytes() + status.tobytes() + bins.tobytes()
                         + d1.tobytes() + s1.tobytes() + m0.tobytes() + dist.tobytes())
        out = subprocess.run([host_layer_binary(), "gpu", str(path)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "all checks passed (gpu)" in out.stdout, out.stdout + out.stderr
