"""GPU (-m gpu): the EigenPlaces batch entries against THE RULE of include/sship.h ("EigenPlaces: batches"): descriptor b of a batch call has
exactly the bits sship_ep_infer_u8_device gives for image b alone, and so has every captured stage.  Every comparison is on the uint32 / uint16
views, no tolerance, no element excluded.  The fp64 accuracy of every stage is held by tests/test_gpu_ep_layers.py on the single-image path;
bit equality transfers it.

The cases are _ep_batch_ref.GPU_CASES; test_ep_batch_cpu.py asserts from the dispatch mirror that they reach both forms of every deep layer
(batched split-K, grouped) at both tile heights, k = 2, 4, 8 and the three split epilogue forms in both forms.

Shipped library, no developer switches, weights make_eigenplaces_weights(2), images make_frame with a different seed per slot."""
import ctypes as C

import numpy as np
import pytest
import torch

import _ep_batch_ref as B
import _ep_layer_ref as R
from superslam_amd import _lib
from superslam_amd.synth import make_frame
from superslam_amd.weights import make_eigenplaces_weights, save_safetensors

pytestmark = pytest.mark.gpu

CANARY = np.uint32(0x7FC0BEEF)   # a NaN payload no kernel writes


@pytest.fixture(scope="module")
def ep_path(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("epb") / "eigenplaces_resnet18_512.safetensors")
    save_safetensors(make_eigenplaces_weights(2), p)
    return p


@pytest.fixture(scope="module")
def L():
    _lib.init(0)
    assert torch.cuda.is_available()
    return _lib.lib()


def _frames(n, channels, h, w, seed0=100):
    """[n, h, w] or [n, h, w, 3] uint8, a different seed per slot (and per channel)."""
    if channels == 1:
        return np.stack([make_frame(h, w, seed0 + i, n_rects=12) for i in range(n)])
    return np.ascontiguousarray(np.stack([np.stack([make_frame(h, w, seed0 + 3 * i + c, n_rects=12) for c in range(3)], -1) for i in range(n)]))


def _source_size(in_w):
    return (188, 620) if in_w >= 512 else (96, 128)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


class Handle:
    def __init__(self, L, path, in_w, in_h, reserve=1):
        self.L, self.in_w, self.in_h = L, in_w, in_h
        self.h = C.c_void_p()
        _lib.check(L.sship_ep_create(path.encode(), in_w, in_h, C.byref(self.h)))
        if reserve > 1:
            _lib.check(L.sship_ep_reserve_batch(self.h, reserve))

    def close(self):
        self.L.sship_ep_destroy(self.h)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def single(self, img_dev, stream=0):
        """sship_ep_infer_u8_device on one contiguous device image -> numpy [512]."""
        h, w = int(img_dev.shape[0]), int(img_dev.shape[1])
        ch = 1 if img_dev.dim() == 2 else 3
        out = torch.zeros(512, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(self.L.sship_ep_infer_u8_device(self.h, img_dev.data_ptr(), h, w, w * ch, ch, out.data_ptr(), stream))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def singles(self, imgs_dev):
        return np.stack([self.single(imgs_dev[i]) for i in range(imgs_dev.shape[0])])

    def batch_rc(self, imgs_dev, stream=0, batch=None):
        """sship_ep_infer_u8_batch_device on a contiguous [B, h, w(, 3)] device tensor -> (rc, numpy [B, 512])."""
        b, h, w = (int(v) for v in imgs_dev.shape[:3])
        ch = 1 if imgs_dev.dim() == 3 else 3
        b = b if batch is None else batch
        out = torch.zeros((max(b, 1), 512), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc = self.L.sship_ep_infer_u8_batch_device(self.h, imgs_dev.data_ptr(), b, h, w, w * ch, h * w * ch, ch, out.data_ptr(), 512, stream)
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()

    def batch(self, imgs_dev, stream=0):
        rc, out = self.batch_rc(imgs_dev, stream)
        _lib.check(rc)
        return out

    def stages(self):
        out = {}
        for stage, (shape, dtype) in R.stage_shapes(self.in_w, self.in_h).items():
            a = np.empty(shape, dtype)
            _lib.check(self.L.sship_ep_debug_activation(self.h, stage, a.ctypes.data, a.nbytes))
            out[stage] = a
        return out


def _assert_rows_equal(got, ref, what):
    assert got.shape == ref.shape and np.isfinite(ref).all()
    diff = _bits(got) != _bits(ref)
    assert not diff.any(), f"{what}: {int(diff.sum())} differing elements in rows {sorted(set(np.nonzero(diff)[0].tolist()))[:16]}"


@pytest.mark.parametrize("in_w,in_h,channels,batch", B.GPU_CASES, ids=[f"{w}x{h}-b{b}" for w, h, _, b in B.GPU_CASES])
def test_batch_rows_and_stages_equal_the_single_image_call(L, ep_path, in_w, in_h, channels, batch):
    sh, sw = _source_size(in_w)
    imgs = torch.from_numpy(_frames(batch, channels, sh, sw)).cuda()
    with Handle(L, ep_path, in_w, in_h, reserve=batch) as H:
        assert L.sship_ep_max_batch(H.h) == batch
        ref = H.singles(imgs)
        assert len({r.tobytes() for r in ref}) == batch                       # the slots really hold different images
        got = H.batch(imgs)
        _assert_rows_equal(got, ref, f"{in_w}x{in_h} batch {batch}")
        # every captured stage of image b in {0, last}
        _lib.check(L.sship_ep_debug_capture(H.h, 1))
        for b in sorted({0, batch - 1}):
            H.single(imgs[b])
            want = H.stages()
            _lib.check(L.sship_ep_debug_capture_image(H.h, b))
            got_on = H.batch(imgs)
            have = H.stages()
            assert len(want) == 29 - 5 and set(have) == set(want)             # 29 stage numbers, five blocks without a downsample
            for s in want:
                d = _bits(have[s]) != _bits(want[s])
                assert not d.any(), f"{in_w}x{in_h} batch {batch} image {b} stage {s}: {int(d.sum())} of {d.size} elements differ"
            _assert_rows_equal(got_on, ref, "capture on")
        _lib.check(L.sship_ep_debug_capture(H.h, 0))
        _assert_rows_equal(H.batch(imgs), ref, "capture off again")


def test_position_independence_and_identical_images(L, ep_path):
    in_w, in_h = 130, 100
    nb = B.first_all_grouped_batch(in_w, in_h)            # 64 with the rule's threshold: the grouped form
    frames = _frames(5, 1, 96, 128, seed0=300)
    with Handle(L, ep_path, in_w, in_h, reserve=nb) as H:
        x = torch.from_numpy(frames[0]).cuda()
        want = H.single(x)
        # the same image at slots 0, middle and last of a batched split-K batch ...
        mixed = torch.from_numpy(frames[[0, 1, 0, 2, 0]]).cuda()
        got = H.batch(mixed)
        for slot in (0, 2, 4):
            _assert_rows_equal(got[slot], want, f"slot {slot} of 5")
        # ... and of a grouped one, the other slots holding other images
        idx = np.arange(nb) % 4 + 1
        idx[[0, nb // 2, nb - 1]] = 0
        got = H.batch(torch.from_numpy(frames[idx]).cuda())
        for slot in (0, nb // 2, nb - 1):
            _assert_rows_equal(got[slot], want, f"slot {slot} of {nb}")
        # a batch of identical images gives identical rows, in both forms
        for n in (3, nb):
            got = H.batch(x[None].expand(n, -1, -1).contiguous())
            _assert_rows_equal(got, np.broadcast_to(want, (n, 512)), f"{n} identical images")


def test_layout_interleaved_strided_unaligned_with_canaries(L, ep_path):
    """The interleaved L0, R0, L1, R1, ... buffer read with image_stride = 2 h stride: only the left images are read.  Row stride w + 3, base
    pointer 1 byte off, desc_stride 515 with canary floats between the rows and after the last one."""
    in_w, in_h, nb, h, w = 40, 40, 5, 50, 70
    stride = w + 3
    left = _frames(nb, 1, h, w, seed0=500)
    ds = 515
    with Handle(L, ep_path, in_w, in_h, reserve=nb) as H:
        ref = H.singles(torch.from_numpy(left).cuda())
        results = []
        for right_fill in (0, 255, None):
            buf = np.full(1 + 2 * nb * h * stride, 77, np.uint8)
            v = buf[1:].reshape(2 * nb, h, stride)
            v[0::2, :, :w] = left
            v[1::2] = np.random.default_rng(9).integers(0, 256, v[1::2].shape, dtype=np.uint8) if right_fill is None else right_fill
            dbuf = torch.from_numpy(buf).cuda()
            out = torch.from_numpy(np.full(nb * ds + 64, CANARY, np.uint32).view(np.float32)).cuda()
            torch.cuda.synchronize()
            _lib.check(L.sship_ep_infer_u8_batch_device(H.h, dbuf.data_ptr() + 1, nb, h, w, stride, 2 * h * stride, 1, out.data_ptr(), ds, 0))
            torch.cuda.synchronize()
            o = out.cpu().numpy().view(np.uint32)
            rows = o[:nb * ds].reshape(nb, ds)
            assert (rows[:, 512:] == CANARY).all() and (o[nb * ds:] == CANARY).all()     # nothing between the rows or after the last one
            results.append(rows[:, :512].copy().view(np.float32))
        for r in results:
            _assert_rows_equal(r, ref, "interleaved buffer")
        # the strides are minima, nothing else: below them the call is refused and writes nothing
        out = torch.zeros(nb * ds, dtype=torch.float32, device="cuda")
        dbuf = torch.zeros(1 + 2 * nb * h * stride, dtype=torch.uint8, device="cuda")
        for args in ((nb, h, w, w - 1, 2 * h * stride, 1, ds), (nb, h, w, stride, h * stride - 1, 1, ds), (nb, h, w, stride, 2 * h * stride, 1, 511),
                     (nb, h, w, stride, 2 * h * stride, 2, ds), (0, h, w, stride, 2 * h * stride, 1, ds), (nb, 0, w, stride, 2 * h * stride, 1, ds)):
            b_, h_, w_, st_, ist_, ch_, ds_ = args
            assert L.sship_ep_infer_u8_batch_device(H.h, dbuf.data_ptr(), b_, h_, w_, st_, ist_, ch_, out.data_ptr(), ds_, 0) == _lib.ERR_INVALID, args
        assert L.sship_ep_infer_u8_batch_device(H.h, None, nb, h, w, stride, 2 * h * stride, 1, out.data_ptr(), ds, 0) == _lib.ERR_INVALID
        assert L.sship_ep_infer_u8_batch_device(H.h, dbuf.data_ptr(), nb, h, w, stride, 2 * h * stride, 1, None, ds, 0) == _lib.ERR_INVALID
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()


def test_capture_off_costs_nothing_and_image_index_is_checked(L, ep_path):
    in_w, in_h, nb = 130, 100, 3
    imgs = torch.from_numpy(_frames(nb, 1, 96, 128, seed0=700)).cuda()
    probe = np.zeros(512, np.float32)
    with Handle(L, ep_path, in_w, in_h, reserve=nb) as H:
        d_off = H.batch(imgs)
        assert L.sship_ep_debug_activation(H.h, R.STAGE_DESC, probe.ctypes.data, probe.nbytes) == _lib.ERR_INVALID     # capture is off
        # capture off: no allocation by a call (the device's free memory does not move over further calls)
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            _assert_rows_equal(H.batch(imgs), d_off, "repeat, capture off")
        assert torch.cuda.mem_get_info()[0] == free0
        _lib.check(L.sship_ep_debug_capture(H.h, 1))
        assert L.sship_ep_debug_capture_image(H.h, -1) == _lib.ERR_INVALID
        assert L.sship_ep_debug_capture_image(H.h, 1024) == _lib.ERR_INVALID
        # an image the batch does not hold: nothing is captured
        _lib.check(L.sship_ep_debug_capture_image(H.h, nb))
        _assert_rows_equal(H.batch(imgs), d_off, "capture on, image index == batch")
        assert L.sship_ep_debug_activation(H.h, R.STAGE_DESC, probe.ctypes.data, probe.nbytes) == _lib.ERR_INVALID
        _lib.check(L.sship_ep_debug_capture_image(H.h, nb - 1))
        assert L.sship_ep_debug_activation(H.h, R.STAGE_DESC, probe.ctypes.data, probe.nbytes) == _lib.ERR_INVALID     # selecting forgets
        _assert_rows_equal(H.batch(imgs), d_off, "capture on")
        _lib.check(L.sship_ep_debug_activation(H.h, R.STAGE_DESC, probe.ctypes.data, probe.nbytes))
        _assert_rows_equal(probe, d_off[nb - 1], "captured descriptor of the last image")
        # the single-image entry is not affected by the selection: it captures its own image
        one = H.single(imgs[0])
        _lib.check(L.sship_ep_debug_activation(H.h, R.STAGE_DESC, probe.ctypes.data, probe.nbytes))
        _assert_rows_equal(probe, one, "single call with a batch image selected")


def test_state_reservation_streams_and_repeat(L, ep_path):
    in_w, in_h, nb = 130, 100, 4
    imgs = torch.from_numpy(_frames(nb + 1, 1, 96, 128, seed0=900)).cuda()
    with Handle(L, ep_path, in_w, in_h) as H:
        assert L.sship_ep_max_batch(H.h) == 1
        before = H.single(imgs[0])
        _assert_rows_equal(H.batch(imgs[:1]), before[None], "batch of 1 without a reservation")
        rc, _ = H.batch_rc(imgs[:2])
        assert rc == _lib.ERR_INVALID and L.sship_ep_max_batch(H.h) == 1      # a call never grows the reservation
        for bad in (0, -3, 1025):
            assert L.sship_ep_reserve_batch(H.h, bad) == _lib.ERR_INVALID
        _lib.check(L.sship_ep_reserve_batch(H.h, nb))
        assert L.sship_ep_max_batch(H.h) == nb
        _lib.check(L.sship_ep_reserve_batch(H.h, 2))                             # smaller: a no-op
        assert L.sship_ep_max_batch(H.h) == nb
        _assert_rows_equal(H.single(imgs[0]), before, "single call after reserve_batch")
        ref = H.singles(imgs[:nb])
        first = H.batch(imgs[:nb])
        _assert_rows_equal(first, ref, "batch")
        _assert_rows_equal(H.single(imgs[0]), before, "single call after a batch call")
        rc, out = H.batch_rc(imgs)                                               # nb + 1 images
        assert rc == _lib.ERR_INVALID and not out.any()
        assert b"reserve_batch" in L.sship_last_error()
        _assert_rows_equal(H.batch(imgs[:nb]), first, "the next valid call / a second identical call")
        _assert_rows_equal(H.batch(imgs[1:3]), ref[1:3], "a smaller batch than reserved")
        st = torch.cuda.Stream()
        _assert_rows_equal(H.batch(imgs[:nb], stream=st.cuda_stream), first, "side stream")


def test_host_entry_and_python_wrappers(L, ep_path):
    from superslam_amd.eigenplaces import EigenPlaces

    in_w, in_h, n = 130, 100, 7
    frames = _frames(n, 3, 60, 90, seed0=1100)
    with Handle(L, ep_path, in_w, in_h, reserve=n) as H:
        dev = H.batch(torch.from_numpy(frames).cuda())
        # host entry on a padded host layout: row stride w * 3 + 5, image stride with 11 spare bytes
        h, w = frames.shape[1:3]
        stride, ist = w * 3 + 5, h * (w * 3 + 5) + 11
        buf = np.full(n * ist, 200, np.uint8)
        for b in range(n):
            buf[b * ist:b * ist + h * stride].reshape(h, stride)[:, :w * 3] = frames[b].reshape(h, w * 3)
        host = np.zeros((n, 512), np.float32)
        _lib.check(L.sship_ep_infer_u8_batch(H.h, buf.ctypes.data, n, h, w, stride, ist, 3, host.ctypes.data))
        _assert_rows_equal(host, dev, "host entry")
        assert L.sship_ep_infer_u8_batch(H.h, buf.ctypes.data, n + 1, h, w, stride, ist, 3, host.ctypes.data) == _lib.ERR_INVALID
    ep = EigenPlaces(ep_path, in_w, in_h)
    assert ep.initialize() and ep.max_batch() == 1
    try:
        loop = np.stack([ep.compute_global_descriptor(f) for f in frames])
        _assert_rows_equal(ep.compute_global_descriptors(list(frames)), loop, "compute_global_descriptors, chunks of 1")
        ep.reserve_batch(3)
        assert ep.max_batch() == 3
        _assert_rows_equal(ep.compute_global_descriptors(frames), loop, "compute_global_descriptors, chunks of 3, 3, 1")
        # the device wrapper on a strided view: the left images of an interleaved tensor, and a column crop
        inter = torch.from_numpy(np.repeat(frames[:3], 2, axis=0)).cuda()
        inter[1::2] = 255 - inter[1::2]
        got = ep.infer_u8_batch_device(inter[0::2])
        torch.cuda.synchronize()
        _assert_rows_equal(got.cpu().numpy(), dev[:3], "infer_u8_batch_device(imgs[0::2])")
        with pytest.raises(ValueError, match="exceeds max_batch"):
            ep.infer_u8_batch_device(inter)
        gray = torch.from_numpy(np.ascontiguousarray(frames[:2, :, :, 0])).cuda()
        crop = gray[:, 3:, 5:]
        a = ep.infer_u8_batch_device(crop)
        b = ep.infer_u8_batch_device(crop.contiguous())
        torch.cuda.synchronize()
        _assert_rows_equal(a.cpu().numpy(), b.cpu().numpy(), "a crop view against its contiguous copy")
    finally:
        ep.close()


def test_cpp_host_layer_batches_equal_its_single_calls(L, ep_path):
    """tests/cpp/test_place_recognizer_batch.cc with the weights: superslam_hip::EigenPlaces::compute_global_descriptors on five BGR images in
    buffers of their own with padded rows, in chunks of 1, of 2 and in one chunk, memcmp-equal to compute_global_descriptor per image."""
    import subprocess

    import test_ep_batch_cpu

    r = subprocess.run([test_ep_batch_cpu._build(), ep_path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_rows_go_straight_into_the_place_index(L, ep_path):
    from superslam_amd.eigenplaces import EigenPlaces
    from superslam_amd.place_index import PlaceIndex

    in_w, in_h, n = 130, 100, 6
    imgs = torch.from_numpy(_frames(n, 1, 96, 128, seed0=1300)).cuda()
    ep = EigenPlaces(ep_path, in_w, in_h)
    ia, ib = PlaceIndex(512, 16, max_queries=8, max_top_k=4), PlaceIndex(512, 16, max_queries=8, max_top_k=4)
    assert ep.initialize() and ia.initialize() and ib.initialize()
    try:
        ep.reserve_batch(n)
        ids = np.arange(10, 10 + n)
        rows = ep.infer_u8_batch_device(imgs)                     # [n, 512], as it comes
        assert ia.add(ids, rows)
        ra = [t.cpu().numpy() for t in ia.query_batch(rows, exclude_recent=0, top_k=4)]
        singles = []
        for i in range(n):
            d = ep.infer_u8_device(imgs[i]).clone()
            singles.append(d)
            assert ib.add(int(ids[i]), d)
        rb = [t.cpu().numpy() for t in ib.query_batch(torch.stack(singles), exclude_recent=0, top_k=4)]
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ia.read()[1], ib.read()[1])
        _assert_rows_equal(ia.read()[0], ib.read()[0], "stored rows")
        np.testing.assert_array_equal(ra[2], rb[2])
        np.testing.assert_array_equal(ra[0], rb[0])
        _assert_rows_equal(ra[1], rb[1], "scores")
        assert (ra[0][:, 0] == np.arange(n)).all()                # every image retrieves itself first
    finally:
        ep.close(); ia.close(); ib.close()
