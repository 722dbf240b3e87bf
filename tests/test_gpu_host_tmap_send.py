"""GPU: the send step through a typemap over host memory (lampi_host_tmap_send_pack).

A datatype's elements in a host buffer, a host NIC ring prefilled with a pattern and guarded on both sides.  After the
call the whole ring -- every slot, every byte the call must not touch, the guards -- is compared byte for byte with
three references:

  (1) the model of the host send step (_msg_want of tests/test_gpu_send_pack.py, msg_send_expect of
      tests/quadrics_model.py: the oracle alone) fed the packed bytes tmap_model.packed(...) of the window;
  (2) lampi_host_msg_send_pack of those packed bytes, k_first = 0 and every fragment;
  (3) for GM and IB at 8-byte-aligned rings, the device form lampi_tmap_send_pack on an uploaded copy.

The host buffer must come back unchanged.  The pipeline chunk (LAMPI_HOST_CHUNK_BYTES) is set so that every window
spans at least 7 chunks -- the 3-deep ring of device buffers wraps twice -- and, for every type with a pair of two
bytes or more, at least one chunk boundary falls inside a pair.  Fragment lengths 52, 53, 100, 1976 and 4200, the
three header kinds and the three modes rotate over the typemaps and the window starts of tmap_model.pack_offsets.
"""
import threading

import numpy as np
import pytest

import quadrics_model as qm
import tmap_model as tmm
from test_gpu_send_pack import CRC, FILL, GM, HDR, IB, NONE, SUM, _msg_want

pytestmark = pytest.mark.gpu

QUADRICS = 3
GUARD = 512
FRAG_LENS = [52, 53, 100, 1976, 4200]
KINDS = [GM, IB, QUADRICS]
MODES = [CRC, SUM, NONE]

# beside tmap_model's: elements that overlap (legal to send), and one type either side of the span rules of
# lampi_amd/csrc/host_tmap_plan.h (gaps of a page, 176 host bytes per DMA row)
EXT0 = tmm.Typemap("extent0", [8], [0], 0, overlap_ok=True)
EXT_LT = tmm.Typemap("extent<size", [16], [0], 8, overlap_ok=True)
NEG = tmm.Typemap("negative", [8, 3], [0, 9], -24, overlap_ok=True)
def _gap(name, gap):
    """65 pieces of 64 bytes two bytes apart, the last one behind a gap of `gap` bytes: about 130 host bytes per DMA
    row, so only the gap decides the route."""
    offs = [66 * j for j in range(64)] + [66 * 63 + 64 + gap]
    return tmm.Typemap(name, [64] * 65, offs, offs[64] + 64 + 3)


GAP_IN, GAP_OUT = _gap("gap4095", 4095), _gap("gap4096", 4096)
RATIO_IN = tmm.Typemap("row176", [8], [0], 176)
RATIO_OUT = tmm.Typemap("row177", [8], [0], 177)
TYPEMAPS = [tmm.T1, tmm.T2, tmm.T3, tmm.T5, tmm.S1, tmm.S65, tmm.T4A, EXT0, EXT_LT, NEG, GAP_IN, GAP_OUT, RATIO_IN,
            RATIO_OUT]
CASES = [(t, w) for t in range(len(TYPEMAPS)) for w in range(3)]


def _buffer(oracle, tm, count, seed):
    """(host buffer, origin) around the pieces of `count` elements, 32 bytes of margin (any extent)."""
    idx = tmm.index_map(tm, np.arange(count * tm.packed_size, dtype=np.int64))
    lo, hi = int(idx.min()), int(idx.max()) + 1
    origin = 32 - min(lo, 0)
    return np.ascontiguousarray(oracle.stream(seed, 0, origin + max(hi, 0) + 32)), origin


def pack_offsets(tm):
    """tmap_model.pack_offsets, and for a type without a pair of 8 bytes the middle of element 1."""
    if int(tm.size.max()) >= 8:
        return tmm.pack_offsets(tm)
    return [0, tm.packed_size + tm.packed_size // 2, 2 * tm.packed_size]


def _stride(kind, L, unaligned):
    if unaligned:
        return 585
    return (qm.HDR if kind == QUADRICS else HDR) + (L + 7) // 8 * 8


class _Case:
    """A typemap, a window of at least 7 chunks, the ring before the call and the ring reference (1) expects."""

    def __init__(self, oracle, t, w, L=None, kind=None, mode=None, unaligned=False, last=None, nchunks=7):
        i = 3 * t + w
        self.tm = tm = TYPEMAPS[t]
        self.L = L = FRAG_LENS[i % 5] if L is None else L
        self.kind = KINDS[i % 3] if kind is None else kind
        self.mode = MODES[(i // 3 + i) % 3] if mode is None else mode
        self.pack_off = pack_offsets(tm)[w]
        # fragments per chunk: the first count from 4 KiB up that puts a chunk boundary inside a pair (none does
        # where the fragment length and the window start are multiples of every pair's size)
        fpc0 = (4096 + L - 1) // L
        inside = [f for f in range(fpc0, fpc0 + 8)
                  if not np.isin((self.pack_off + np.arange(1, nchunks + 1) * f * L) % tm.packed_size, tm.seq).all()]
        self.inside = bool(inside)
        self.fpc = inside[0] if inside else fpc0
        self.chunk = self.fpc * L
        nf = nchunks * self.fpc + 1
        last = [1, 15, 17, None][i % 4] if last is None else last
        self.pack_len = tmm.window_len(L, nf, last)
        self.n = nf
        self.count = tmm.count_for(tm, self.pack_off + self.pack_len) + 1
        self.buf, self.origin = _buffer(oracle, tm, self.count, 1500 + i)
        self.stride = _stride(self.kind, L, unaligned)
        self.at = GUARD + (3 if unaligned else 0)
        self.tmpl = np.random.default_rng(1501 + i).integers(0, 256, size=HDR, dtype=np.uint8)
        self.before = np.ascontiguousarray(oracle.stream(1502, 0, self.at + self.n * self.stride + GUARD))
        self.msg = np.ascontiguousarray(tmm.packed(tm, self.buf, self.origin, self.pack_off, self.pack_len))
        self.want = self.before.copy()
        sub = self.want[self.at:self.at + self.n * self.stride]  # (a view: the model writes through it)
        if self.kind == QUADRICS:
            n = qm.msg_send_expect(oracle, self.msg, L, sub, self.stride, self.tmpl, FILL["frag_seq0"],
                                   FILL["frag_seq_step"], FILL["desc_ptr0"], FILL["desc_ptr_stride"],
                                   FILL["seq_offset0"], self.mode)
        else:
            n, _ = _msg_want(oracle, sub, self.msg, self.kind, L, self.stride, self.pack_len, self.tmpl, FILL,
                             self.mode)
        assert n == self.n

    def boundaries_inside_a_pair(self):
        p = self.pack_off + np.arange(1, self.n // self.fpc + 1, dtype=np.int64) * self.fpc * self.L
        return ~np.isin(p % self.tm.packed_size, self.tm.seq)

    def htm(self):
        from lampi_amd import host

        return host.make_host_tmap(self.tm.size, self.tm.offset, self.tm.extent, self.count)

    def send(self, ring):
        from lampi_amd import host

        host.host_tmap_send_pack(self.buf, self.origin, self.htm(), self.pack_off, self.pack_len, self.L, ring,
                                 self.stride, host.make_fill(self.tmpl, **FILL), kind=self.kind, mode=self.mode,
                                 ring_offset=self.at)
        return ring


def _diff(got, want, x):
    d = np.nonzero(got != want)[0]
    if d.size == 0:
        return None
    i = int(d[0]) - x.at
    return dict(tm=x.tm.name, L=x.L, kind=x.kind, mode=x.mode, slot=i // x.stride, byte=i % x.stride,
                differing=int(d.size), got=int(got[d[0]]), want=int(want[d[0]]))


@pytest.fixture
def chunked(monkeypatch):
    def set_chunk(x):
        monkeypatch.setenv("LAMPI_HOST_CHUNK_BYTES", str(x.chunk))
        assert (x.n + x.fpc - 1) // x.fpc >= 7, "the window must span at least 7 chunks"
        assert x.inside == x.boundaries_inside_a_pair().any()
        if x.tm in (tmm.T1, tmm.T2, tmm.T3, tmm.T4A, GAP_IN, GAP_OUT):
            assert x.inside, "a chunk boundary must fall inside a pair"
    return set_chunk


@pytest.mark.parametrize("t,w", CASES, ids=[f"{TYPEMAPS[t].name}-w{w}" for t, w in CASES])
def test_ring_byte_for_byte(cuda, oracle, chunked, t, w):
    """References (1), (2) and, where the device form serves the case, (3)."""
    import torch

    from lampi_amd import device as dv
    from lampi_amd import host

    x = _Case(oracle, t, w)
    chunked(x)
    src = x.buf.copy()
    ring = x.send(x.before.copy())
    assert np.array_equal(ring, x.want), _diff(ring, x.want, x)
    assert np.array_equal(x.buf, src)
    ring2 = x.before.copy()
    host.host_msg_send_pack(x.msg, x.L, ring2, x.stride, host.make_fill(x.tmpl, **FILL), kind=x.kind, mode=x.mode,
                            ring_offset=x.at)
    assert np.array_equal(ring, ring2), _diff(ring, ring2, x)
    if x.kind != QUADRICS and x.tm.extent > 0 and x.tm not in (EXT_LT,):
        dbase = torch.from_numpy(x.buf).to(cuda)
        dring = torch.from_numpy(x.before).to(cuda)
        dtm = dv.make_tmap(x.tm.pairs(), x.tm.extent, x.count, cuda)
        dv.tmap_send_pack(dbase, dtm, x.L, dring[x.at:], x.stride, x.tmpl, kind=x.kind, mode=x.mode,
                          pack_off=x.pack_off, pack_len=x.pack_len, base_offset=x.origin, **FILL)
        torch.cuda.synchronize()
        dev = dring.cpu().numpy()
        assert np.array_equal(ring, dev), _diff(ring, dev, x)


def test_every_kind_mode_and_length_ran():
    """The rotation reaches every kind x mode and every fragment length x kind."""
    seen = [(FRAG_LENS[(3 * t + w) % 5], KINDS[(3 * t + w) % 3], MODES[((3 * t + w) // 3 + 3 * t + w) % 3])
            for t, w in CASES]
    assert {(k, m) for _, k, m in seen} == {(k, m) for k in KINDS for m in MODES}
    assert {(L, k) for L, k, _ in seen} == {(L, k) for L in FRAG_LENS for k in KINDS}


@pytest.mark.parametrize("kind", KINDS, ids=["gm", "ib", "quadrics"])
@pytest.mark.parametrize("ring_kind", ["pageable", "registered", "unaligned585", "unaligned585-registered"])
@pytest.mark.parametrize("t", [0, 1], ids=["T1", "T2"])
def test_rings(cuda, oracle, chunked, kind, ring_kind, t):
    """Pageable and page-locked rings, and a ring at an odd address with a stride of 585 bytes."""
    from lampi_amd import host

    unaligned = ring_kind.startswith("unaligned")
    x = _Case(oracle, t, 1, L=100 if unaligned else 1976, kind=kind, mode=[CRC, SUM, NONE][(kind + t) % 3],
              unaligned=unaligned)
    chunked(x)
    ring = x.before.copy()
    registered = ring_kind.endswith("registered")
    if registered:
        host.host_register(ring)
        host.host_register(x.buf)
    try:
        x.send(ring)
    finally:
        if registered:
            host.host_unregister(ring)
            host.host_unregister(x.buf)
    assert np.array_equal(ring, x.want), _diff(ring, x.want, x)


@pytest.mark.parametrize("kind", KINDS, ids=["gm", "ib", "quadrics"])
@pytest.mark.parametrize("mode", MODES, ids=["crc", "sum", "none"])
def test_empty_window(cuda, oracle, kind, mode):
    """pack_len == 0: one empty fragment whose header is still written, at the start, inside and at the end of the
    message."""
    from lampi_amd import host

    tm = tmm.T2
    buf, origin = _buffer(oracle, tm, 5, 1510)
    stride = _stride(kind, 100, False)
    tmpl = np.random.default_rng(1511).integers(0, 256, size=HDR, dtype=np.uint8)
    before = np.ascontiguousarray(oracle.stream(1512, 0, 2 * GUARD + stride))
    want = before.copy()
    sub = want[GUARD:GUARD + stride]
    empty = np.zeros(0, np.uint8)
    if kind == QUADRICS:
        qm.msg_send_expect(oracle, empty, 100, sub, stride, tmpl, FILL["frag_seq0"], FILL["frag_seq_step"],
                           FILL["desc_ptr0"], FILL["desc_ptr_stride"], FILL["seq_offset0"], mode)
    else:
        _msg_want(oracle, sub, empty, kind, 100, stride, 0, tmpl, FILL, mode)
    htm = host.make_host_tmap(tm.size, tm.offset, tm.extent, 5)
    for pack_off in (0, 77, 5 * tm.packed_size):
        ring = before.copy()
        host.host_tmap_send_pack(buf, origin, htm, pack_off, 0, 100, ring, stride, host.make_fill(tmpl, **FILL),
                                 kind=kind, mode=mode, ring_offset=GUARD)
        assert np.array_equal(ring, want), pack_off


def test_two_threads_and_release(cuda, oracle, monkeypatch):
    """Two threads send at once, each on its own pipeline; after lampi_host_release() on every thread no pinned
    staging is left."""
    from lampi_amd import lib

    xs = [_Case(oracle, 0, 1, L=1976, kind=GM, mode=CRC), _Case(oracle, 1, 1, L=1976, kind=QUADRICS, mode=SUM)]
    assert xs[0].chunk == xs[1].chunk
    monkeypatch.setenv("LAMPI_HOST_CHUNK_BYTES", str(xs[0].chunk))
    rings = [x.before.copy() for x in xs]
    errs = []

    def work(x, ring):
        try:
            for _ in range(3):
                ring[:] = x.before
                x.send(ring)
        except Exception as e:  # noqa: BLE001 -- reported below, on the test's thread
            errs.append(repr(e))
        finally:
            lib().lampi_host_release()

    th = [threading.Thread(target=work, args=a) for a in zip(xs, rings)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for x, ring in zip(xs, rings):
        assert np.array_equal(ring, x.want), _diff(ring, x.want, x)
    lib().lampi_host_release()
    assert lib().lampi_host_pinned_bytes() == 0


def test_refusals_write_nothing(cuda, oracle):
    """With a device present: refusals return hipErrorInvalidValue and leave the ring as it was."""
    import ctypes

    from lampi_amd import host, lib

    x = _Case(oracle, 1, 0, L=100, kind=IB, mode=CRC)
    ring = x.before.copy()
    f, fill, htm = lib().lampi_host_tmap_send_pack, host.make_fill(x.tmpl, **FILL), x.htm()
    b, r, fp, tp = x.buf.ctypes.data + x.origin, ring.ctypes.data + x.at, ctypes.addressof(fill), htm.addr()
    total = x.count * x.tm.packed_size
    assert f(b, tp, 0, x.pack_len, x.L, r, x.stride, None, IB, CRC) == 1
    assert f(b, tp, 0, x.pack_len, x.L, r, x.stride, fp, 2, CRC) == 1
    assert f(b, tp, 0, x.pack_len, x.L, r, x.stride, fp, IB, 3) == 1
    assert f(b, tp, 0, x.pack_len, x.L, r, x.L + HDR - 1, fp, IB, CRC) == 1
    assert f(b, tp, 1, total, x.L, r, x.stride, fp, IB, CRC) == 1
    assert f(b, None, 0, x.pack_len, x.L, r, x.stride, fp, IB, CRC) == 1
    bad = host.make_host_tmap(x.tm.size, x.tm.offset, x.tm.extent, x.count)
    bad.pairs["seq_offset"][1] += 1
    assert f(b, bad.addr(), 0, x.pack_len, x.L, r, x.stride, fp, IB, CRC) == 1
    assert np.array_equal(ring, x.before)
