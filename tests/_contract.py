"""The stream and memory contract of the asynchronous device entries (include/sship.h: "asynchronous on `stream`, no host
synchronisation inside", every output entry written and nothing beyond it), checked from outside:

  Arena          one uint8 device allocation per case; every input and output of the entry is a view carved out of it at a 256-byte
                 aligned offset between two guard bands of GUARD bytes.  The bands next to floating-point inputs hold NaN bit patterns
                 (0xFF bytes), the ones next to integer inputs 0x7F bytes (2139062143 as an int32: no count, index or id), the ones next
                 to outputs 0xA5.  check() names the carves whose bands changed.  Nothing is ever placed at the end of the allocation:
                 an overrun lands in memory the test owns and is found by comparison.
  delay(s, ms)   a spin of `ms` milliseconds enqueued on stream `s` (torch.cuda._sleep; cycles per millisecond measured once).
  side_stream()  the non-blocking stream of the delayed runs: one that is shown to run concurrently with the NULL stream.
  run_contract   the sequence of tests/test_gpu_stream_contract.py: references on the NULL stream, then the entry twice back to back
                 behind a delay on a non-blocking side stream, with the inputs arriving on that stream only.  A launch, a memset or a
                 copy that goes to another stream runs while the carves still hold the decoy; a host synchronisation inside the entry
                 returns after the delay; a store past an output changes a guard band.

An entry is described by an `Entry`: `inputs(variant)` -> ({name: numpy array}, {scalars}) for variant 0 (true), 1 (decoy), 2 (second
decoy) with the same array shapes in every variant; `outputs` -> [(name, shape, numpy dtype)]; `launch(ins, outs, scalars, stream)` with
`ins` / `outs` dicts of carved tensors and `stream` the raw handle (0 = the NULL stream)."""
from __future__ import annotations

import functools
import time
from dataclasses import dataclass, field

import numpy as np

GUARD = 4096
ALIGN = 256
TAIL = 1 << 16           # slack after the last guard band, so that no carve lies near the end of the allocation
PAT_FLOAT_IN, PAT_INT_IN, PAT_OUT = 0xFF, 0x7F, 0xA5
OUT_FILL = 0x5A          # what an output carve holds before a reference run: a byte left at it was not written


def _torch():
    import torch

    return torch


def _tdtype(dt):
    torch = _torch()
    return {np.dtype(np.uint8): torch.uint8, np.dtype(np.int8): torch.int8, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32,
            np.dtype(np.int64): torch.int64, np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32,
            np.dtype(np.float64): torch.float64, np.dtype(np.uint16): torch.int16, np.dtype(np.uint32): torch.int32}[np.dtype(dt)]


def _round_up(v, a):
    return (v + a - 1) // a * a


class Arena:
    """One device allocation, carved into guarded views."""

    def __init__(self, nbytes: int, device="cuda"):
        torch = _torch()
        self.buf = torch.empty(int(nbytes) + ALIGN + TAIL, dtype=torch.uint8, device=device)     # TAIL bytes past the last band are never carved
        self._base = (-self.buf.data_ptr()) % ALIGN      # the first 256-byte aligned byte of the allocation
        self._top = self._base
        self._carves = []                                # (name, guard_lo, lo, hi, guard_hi, pattern), byte offsets into buf
        self._expect = None

    @staticmethod
    def bytes_needed(specs) -> int:
        """The arena size for carves of these (shape, dtype) pairs."""
        total = 0
        for shape, dt in specs:
            total += GUARD + _round_up(int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize, ALIGN) + ALIGN + GUARD
        return total + ALIGN

    def carve(self, shape, dtype, fill=None, name=None, role="output"):
        """A contiguous `dtype` view of `shape` between two guard bands.  role: "output", or "input" (then the bands are poison for a
        read past the view).  fill: None, a byte value, or an array of the view's shape and dtype."""
        torch = _torch()
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        pat = PAT_OUT if role == "output" else (PAT_FLOAT_IN if dt.kind == "f" else PAT_INT_IN)
        g_lo = self._top
        lo = _round_up(g_lo + GUARD, ALIGN)
        hi = lo + nbytes
        g_hi = _round_up(hi, ALIGN) + GUARD              # the upper band starts at `hi`, so the first byte past the view is watched
        if g_hi > self.buf.numel() - TAIL:
            raise ValueError(f"arena of {self.buf.numel()} bytes is too small for carve {name}")
        self.buf[g_lo:lo] = pat
        self.buf[hi:g_hi] = pat
        self._top = g_hi
        name = name or f"carve{len(self._carves)}"
        self._carves.append((name, g_lo, lo, hi, g_hi, pat))
        self._expect = None
        view = self.buf[lo:hi].view(_tdtype(dt)).reshape(tuple(int(v) for v in shape))
        assert view.data_ptr() % ALIGN == 0 and view.is_contiguous()
        if fill is not None:
            if np.isscalar(fill):
                self.buf[lo:hi] = int(fill)
            else:
                view.copy_(to_device(np.asarray(fill, dt).reshape(shape)))
        return view

    def _sealed(self):
        torch = _torch()
        if self._expect is None:
            mask = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
            want = torch.zeros_like(self.buf)
            for _, g_lo, lo, hi, g_hi, pat in self._carves:
                mask[g_lo:lo] = True
                mask[hi:g_hi] = True
                want[g_lo:lo] = pat
                want[hi:g_hi] = pat
            self._expect = (mask, want)
        return self._expect

    def check(self):
        """The names of the carves whose guard bands no longer hold their pattern (synchronises the device)."""
        torch = _torch()
        torch.cuda.synchronize()
        mask, want = self._sealed()
        bad = (self.buf != want) & mask
        if not bool(bad.any()):
            return []
        return [name for name, g_lo, lo, hi, g_hi, _ in self._carves if bool(bad[g_lo:lo].any()) or bool(bad[hi:g_hi].any())]


def to_device(a: np.ndarray):
    """A device tensor with the bytes of `a` (unsigned 16/32-bit arrays travel as the signed type of the same width)."""
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.dtype in (np.dtype(np.uint16), np.dtype(np.uint32)):
        a = a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])
    return torch.from_numpy(a.copy()).cuda()


def bytes_of(t) -> np.ndarray:
    """The bytes of a device tensor, on the host."""
    torch = _torch()
    return t.contiguous().view(torch.uint8).reshape(-1).cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def cycles_per_ms() -> float:
    """torch.cuda._sleep cycles per millisecond of stream time, measured once per process with two events."""
    torch = _torch()
    torch.cuda._sleep(1_000_000)          # first use loads the kernel
    torch.cuda.synchronize()
    n = 20_000_000
    best = None
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return n / best


def delay(stream, ms: float) -> None:
    """Keep `stream` busy for about `ms` milliseconds."""
    torch = _torch()
    cycles = int(ms * cycles_per_ms())
    with torch.cuda.stream(stream):
        while cycles > 0:                  # _sleep takes a 64-bit count; chunks keep one launch well inside any counter width
            c = min(cycles, 1 << 30)
            torch.cuda._sleep(c)
            cycles -= c


@functools.lru_cache(maxsize=None)
def side_stream():
    """A non-blocking stream whose work runs while the NULL stream's does, found once per process.  The runtime serves its streams from a
    few hardware queues (four by default), and two streams that share one run in order whatever their flags say: work that an entry sent
    to the NULL stream by mistake would then wait for the delay like the rest and come out right.  So candidates are probed: a delay on
    the candidate, then an op on the NULL stream, which must finish while the candidate is still busy.  The same cannot be arranged for a
    handle's own stream, which the library creates: see DESIGN.md for what that leaves uncovered."""
    torch = _torch()
    flag = torch.zeros(1, device="cuda")
    for _ in range(32):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        delay(s, 20.0)
        gate = torch.cuda.Event()
        gate.record(s)
        done = torch.cuda.Event()
        with torch.cuda.stream(torch.cuda.default_stream()):
            flag.add_(1)
            done.record()
        done.synchronize()
        independent = not gate.query()
        s.synchronize()
        if independent:
            return s
    raise RuntimeError("no torch stream runs concurrently with the NULL stream on this device")


@dataclass
class Entry:
    name: str
    inputs: object                 # variant -> ({name: ndarray}, {scalar name: value})
    outputs: object                # [(name, shape, dtype)]
    launch: object                 # (ins, outs, scalars, stream) -> None
    same_ok: dict = field(default_factory=dict)    # count / status outputs that cannot differ between true and decoy: name -> reason
    bar: dict = None               # not bit-reproducible: {output name: absolute bar}; then compared under it (teeth: 100 x bar)
    inplace: dict = field(default_factory=dict)    # output name -> input name it aliases (an in-place entry)
    ragged: dict = field(default_factory=dict)     # output name -> count output name: rows [b, count[b]:] are unspecified by the header
    synchronous: str = ""       # non-empty: the header states that the entry synchronises `stream` before it returns, and why
    note: str = ""


@dataclass
class Report:
    name: str
    findings: list
    t_host_ms: float = 0.0
    t_warm_ms: float = 0.0
    delay_ms: float = 0.0
    delay_asked_ms: float = 0.0
    exact: bool = True
    wall_s: float = 0.0
    no_host_sync_checked: bool = True

    def record(self) -> dict:
        return {"t_host_ms": round(self.t_host_ms, 4), "t_host_warm_ms": round(self.t_warm_ms, 4), "delay_ms": round(self.delay_ms, 3),
                "delay_asked_ms": round(self.delay_asked_ms, 3), "comparison": "bit-exact" if self.exact else "under the module's bar",
                "no_host_sync_checked": self.no_host_sync_checked, "wall_s": round(self.wall_s, 3)}


def _same(entry, name, got: np.ndarray, want: np.ndarray, dtype) -> bool:
    if entry.bar and name in entry.bar:
        g, w = got.view(dtype).astype(np.float64), want.view(dtype).astype(np.float64)
        return bool(np.all(np.isfinite(g) == np.isfinite(w)) and np.all(np.abs(np.where(np.isfinite(g), g - w, 0.0)) <= entry.bar[name]))
    return bool(np.array_equal(got, want))


def _far(entry, name, a: np.ndarray, b: np.ndarray, dtype) -> bool:
    """Teeth: do the true and the decoy reference of this output differ (by 100 x the bar where the entry has one)?"""
    if entry.bar and name in entry.bar:
        x, y = a.view(dtype).astype(np.float64), b.view(dtype).astype(np.float64)
        ok = np.isfinite(x) & np.isfinite(y)
        return bool(np.any(np.isfinite(x) != np.isfinite(y)) or (ok.any() and np.abs(x[ok] - y[ok]).max() >= 100 * entry.bar[name]))
    return not np.array_equal(a, b)


def _trim(entry, spec, outs: dict, ref: dict) -> dict:
    """`outs` with the rows past the counts of `ref` zeroed, for the outputs whose tail rows the header leaves unspecified."""
    for name, cname in entry.ragged.items():
        shape, dt = spec[name]
        a = outs[name].view(dt).reshape(shape).copy()
        n = ref[cname].view(np.int32).reshape(-1)
        for b in range(shape[0]):
            a[b, min(max(int(n[b]), 0), shape[1]):] = 0
        outs[name] = a.reshape(-1).view(np.uint8)
    return outs


def run_contract(entry: Entry, calls: int = 2, min_delay_ms: float = 100.0) -> Report:
    """The sequence (a)-(e) of the module's docstring for one entry.  calls=1 enqueues only the true call behind the delay (the harness's
    own checks use it to show what only two back-to-back calls catch).  Returns the findings; an empty list is a pass."""
    torch = _torch()
    t_begin = time.perf_counter()
    variants = [entry.inputs(v) for v in range(3)]
    arrays = [{k: np.ascontiguousarray(a) for k, a in v[0].items()} for v in variants]
    scalars = [v[1] for v in variants]
    for v in (1, 2):
        assert arrays[v].keys() == arrays[0].keys()
        for k in arrays[0]:
            assert arrays[v][k].shape == arrays[0][k].shape and arrays[v][k].dtype == arrays[0][k].dtype, (entry.name, k)
    outs_spec = list(entry.outputs)
    free_out = [(n, s, d) for n, s, d in outs_spec if n not in entry.inplace]
    specs = [(a.shape, a.dtype) for a in arrays[0].values()] + 2 * [(s, d) for _, s, d in free_out]
    arena = Arena(Arena.bytes_needed(specs))
    ins = {k: arena.carve(a.shape, a.dtype, fill=arrays[1][k], name="in:" + k, role="input") for k, a in arrays[0].items()}
    out_sets = []
    for tag in ("A", "B"):
        o = {n: arena.carve(s, d, fill=OUT_FILL, name=f"out{tag}:{n}") for n, s, d in free_out}
        for n, src in entry.inplace.items():
            o[n] = ins[src]
        out_sets.append(o)
    staged = [{k: to_device(a) for k, a in arr.items()} for arr in arrays]      # ordinary allocations: the sources of the copies
    dtypes = {n: np.dtype(d) for n, _, d in outs_spec}
    null = torch.cuda.default_stream()

    def load(v, stream):
        with torch.cuda.stream(stream):
            for k, t in ins.items():
                t.copy_(staged[v][k], non_blocking=True)

    def reference(v, outs):
        torch.cuda.synchronize()
        load(v, null)
        for n, t in outs.items():
            if n not in entry.inplace:
                t.view(torch.uint8).fill_(OUT_FILL)
        torch.cuda.synchronize()
        entry.launch(ins, outs, scalars[v], 0)
        torch.cuda.synchronize()
        got = {n: bytes_of(t) for n, t in outs.items()}
        return _trim(entry, spec, got, got)

    spec = {n: (tuple(s), np.dtype(d)) for n, s, d in outs_spec}
    findings = []
    # warm-up on an idle side stream: first-call allocations happen here, and the host time of the sequence sizes the delay
    s = side_stream()
    assert s.cuda_stream != 0
    torch.cuda.synchronize()

    def sequence():
        t0 = time.perf_counter()
        if calls == 2:
            load(2, s)
            entry.launch(ins, out_sets[0], scalars[2], s.cuda_stream)
        load(0, s)
        entry.launch(ins, out_sets[1], scalars[0], s.cuda_stream)
        return (time.perf_counter() - t0) * 1e3

    sequence()
    s.synchronize()
    t_warm = sequence()
    s.synchronize()
    # (a) references on the NULL stream, the decoy last and into both output sets
    R = reference(0, out_sets[1])
    D2 = reference(2, out_sets[0])
    D = reference(1, out_sets[0])
    reference(1, out_sets[1])
    for n, _, _ in outs_spec:                                              # (e) teeth
        if n in entry.same_ok:
            continue
        if not _far(entry, n, D[n], R[n], dtypes[n]):
            findings.append(f"teeth: output {n} is the same for the true and the decoy inputs")
        if calls == 2 and not _far(entry, n, D2[n], R[n], dtypes[n]):
            findings.append(f"teeth: output {n} is the same for the true and the second decoy inputs")
    # (b) the delayed run
    T = max(min_delay_ms, 20.0 * t_warm)
    e0, gate = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    delay(s, T)
    gate.record(s)
    t_host = sequence()
    early = gate.query()                                                   # (c)
    s.synchronize()
    real = e0.elapsed_time(gate)
    if entry.synchronous:
        pass               # the header says this entry returns after synchronising the stream: (c) does not apply, the rest does
    elif early and real >= 2.0 * t_warm:
        # the same sequence took t_warm on an idle stream, so the delay was long enough: the calls waited for it
        findings.append(f"host synchronisation: the delay of {real:.1f} ms had passed when the calls returned after {t_host:.2f} ms "
                        f"({t_warm:.3f} ms on an idle stream)")
    elif real < 2.0 * t_host:
        findings.append(f"delay too short: {real:.2f} ms of delay against {t_host:.2f} ms of host time")
    elif early:
        findings.append(f"host synchronisation: the delay of {real:.1f} ms had passed when the calls returned after {t_host:.2f} ms")

    def compare(when):                                                     # (d)
        second = _trim(entry, spec, {n: bytes_of(t) for n, t in out_sets[1].items()}, R)
        for n in second:
            if not _same(entry, n, second[n], R[n], dtypes[n]):
                findings.append(f"mismatch {when}: output {n} of the call on the true inputs differs from its NULL-stream reference"
                                + (" (it equals the decoy's)" if np.array_equal(second[n], D[n]) else ""))
        if calls == 2:
            first = _trim(entry, spec, {n: bytes_of(t) for n, t in out_sets[0].items()}, D2)
            for n in first:
                if n in entry.inplace:             # the true inputs were copied over it for the second call
                    continue
                if not _same(entry, n, first[n], D2[n], dtypes[n]):
                    findings.append(f"mismatch {when}: output {n} of the call on the second decoy differs from its NULL-stream reference")

    compare("after stream.synchronize()")
    torch.cuda.synchronize()
    compare("after device synchronize")
    for name in arena.check():
        findings.append(f"guard band of {name} changed")
    return Report(entry.name, findings, t_host, t_warm, real, T, not entry.bar, time.perf_counter() - t_begin, not entry.synchronous)
