"""GPU: the send step in one call over host memory (lampi_host_msg_send_pack).

A message in host memory, a host NIC ring prefilled with a pattern and guarded on both sides; after the call every
slot is compared byte for byte with the model of the device form -- _msg_want (tests/test_gpu_send_pack.py) for GM and
IB, msg_send_expect (tests/quadrics_model.py) for Quadrics, both from the oracle alone -- and so is every byte the
call must not touch: past header + length in each slot, and the guards.  The same ring must come out of the device
form lampi_msg_send_pack on the same bytes, and out of three calls over fragment sub-ranges.

The pipeline chunk is set (LAMPI_HOST_CHUNK_BYTES) so that each message spans at least 7 chunks: the 3-deep ring of
device buffers wraps twice and the last chunk is partial.
"""
import numpy as np
import pytest

import quadrics_model as qm
from test_gpu_send_pack import CRC, FILL, GM, HDR, IB, NONE, SUM, _msg_want

pytestmark = pytest.mark.gpu

QUADRICS = 3
GUARD = 4096  # bytes of pattern before and after the ring
MODES = pytest.mark.parametrize("mode", [CRC, SUM, NONE], ids=["crc", "sum", "none"])

# name: (kind, frag_len, slot_stride, msg_len, chunk bytes, ring base offset past the guard)
CASES = {
    "gm": (GM, 65456, 65536, 9 * 65456 + 1234, 65536, 0),           # 10 chunks of one fragment
    "ib": (IB, 1976, 2048, 300 * 1976 + 7, 40 * 1976, 0),           # 8 chunks of 40, the last 21 fragments
    "ib_odd": (IB, 1976, 2051, 300 * 1976 + 7, 40 * 1976, 3),       # an odd stride from an odd address
    "ib_dense": (IB, 1976, 2048, 100 * 1976, 12 * 1976, 0),         # frag_len + 72 == stride: 1D copies out
    "q2048": (QUADRICS, 2048, 2304, 60 * 2048 + 1000, 8 * 2048, 0),
    "q52_bare": (QUADRICS, 52, 128, 52 * 700 + 17, 4096, 0),        # inline fragments at strides 128 and 192
    "q52_192": (QUADRICS, 52, 192, 52 * 700 + 17, 4096, 0),
    "q_tail40": (QUADRICS, 4096, 4224, 4096 * 20 + 40, 3 * 4096, 0),  # a 40-byte (inline) tail after longer ones
    "q_bare4096": (QUADRICS, 4096, 128, 4096 * 20 + 100, 3 * 4096, 0),  # a bare queue: checksummed only
    "empty_gm": (GM, 65456, 65536, 0, 4096, 0),
    "empty_ib": (IB, 1976, 2048, 0, 4096, 0),
    "empty_q": (QUADRICS, 2048, 2304, 0, 4096, 0),
    "big_frag": (GM, 10000, 10080, 10000 * 7 + 4097, 4096, 0),      # one fragment larger than a chunk
}
CASE = pytest.mark.parametrize("case", list(CASES))


def _nfrags(mlen, L):
    return (mlen + L - 1) // L if mlen else 1


class _Host:
    """The message, the ring before the call (pattern, guards included) and the ring the model expects."""

    def __init__(self, oracle, case, mode):
        self.kind, self.L, self.stride, self.mlen, self.chunk, off = CASES[case]
        self.mode = mode
        self.n = _nfrags(self.mlen, self.L)
        rng = np.random.default_rng(1200 + mode)
        self.msg = oracle.stream(1201, 3, self.mlen) if self.mlen else np.zeros(0, np.uint8)
        self.msg = np.ascontiguousarray(self.msg)
        self.tmpl = rng.integers(0, 256, size=HDR, dtype=np.uint8)
        self.at = GUARD + off
        span = self.n * self.stride
        self.before = np.ascontiguousarray(oracle.stream(1202, 0, self.at + span + GUARD))
        self.want = self.before.copy()
        sub = self.want[self.at:self.at + span]  # (a view: the model writes through it)
        if self.kind == QUADRICS:
            n = qm.msg_send_expect(oracle, self.msg, self.L, sub, self.stride, self.tmpl, FILL["frag_seq0"],
                                   FILL["frag_seq_step"], FILL["desc_ptr0"], FILL["desc_ptr_stride"],
                                   FILL["seq_offset0"], mode)
        else:
            n, _ = _msg_want(oracle, sub, self.msg, self.kind, self.L, self.stride, self.mlen, self.tmpl, FILL, mode)
        assert n == self.n

    def fill(self):
        from lampi_amd import host

        return host.make_fill(self.tmpl, **FILL)

    def send(self, ring, k_first=0, k_count=None):
        from lampi_amd import host

        host.host_msg_send_pack(self.msg, self.L, ring, self.stride, self.fill(), kind=self.kind, mode=self.mode,
                                k_first=k_first, k_count=k_count, ring_offset=self.at + k_first * self.stride)


def _diff(got, want, x):
    d = np.nonzero(got != want)[0]
    if d.size == 0:
        return None
    i = int(d[0]) - x.at
    return dict(slot=i // x.stride, byte=i % x.stride, differing=int(d.size), got=int(got[d[0]]), want=int(want[d[0]]))


@pytest.fixture
def chunked(monkeypatch):
    def set_chunk(x):
        monkeypatch.setenv("LAMPI_HOST_CHUNK_BYTES", str(x.chunk))
        per = max(1, x.chunk // x.L)
        if x.mlen:
            assert (x.n + per - 1) // per >= 7, "the message must span at least 7 chunks"
    return set_chunk


@CASE
@MODES
@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "registered"])
def test_ring_byte_for_byte(cuda, oracle, chunked, case, mode, registered):
    from lampi_amd import host

    x = _Host(oracle, case, mode)
    chunked(x)
    ring = x.before.copy()
    if registered:
        host.host_register(ring)
    try:
        x.send(ring)
    finally:
        if registered:
            host.host_unregister(ring)
    assert np.array_equal(ring, x.want), _diff(ring, x.want, x)


@pytest.mark.parametrize("case", [c for c in CASES if c != "ib_odd"])
@MODES
def test_equals_the_device_form(cuda, oracle, chunked, case, mode):
    """Upload, lampi_msg_send_pack, download: the same ring (the device form takes 8-byte-aligned rings and
    strides only, so the odd case is left to the model)."""
    import torch

    from lampi_amd import device as dv

    x = _Host(oracle, case, mode)
    assert x.stride % 8 == 0 and x.at % 8 == 0
    chunked(x)
    ring = x.before.copy()
    x.send(ring)
    dmsg = torch.from_numpy(x.msg if x.mlen else np.zeros(8, np.uint8)).to(cuda)
    dring = torch.from_numpy(x.before).to(cuda)
    # (the ring tensor's base is 256-byte aligned and x.at is a multiple of 8)
    dv.msg_send_pack(dmsg, x.L, dring[x.at:], x.stride, x.tmpl, kind=x.kind, mode=mode, msg_len=x.mlen, **FILL)
    torch.cuda.synchronize()
    dev = dring.cpu().numpy()
    assert np.array_equal(ring, dev), _diff(ring, dev, x)


@pytest.mark.parametrize("case", ["gm", "ib", "ib_odd", "q2048", "q52_192", "q_tail40", "q_bare4096", "big_frag"])
@MODES
def test_sub_ranges_give_the_same_ring(cuda, oracle, chunked, case, mode):
    """[0, 3), [3, 4) and [4, n) in three calls -- a message sent through a gated window -- against the model of
    one call: the series are indexed by the fragment's place in the whole message."""
    x = _Host(oracle, case, mode)
    chunked(x)
    ring = x.before.copy()
    for k0, k1 in [(4, x.n), (0, 3), (3, 4)]:
        x.send(ring, k0, k1 - k0)
    assert np.array_equal(ring, x.want), _diff(ring, x.want, x)
    # an empty range writes nothing, wherever it starts
    for k0 in (0, 3, x.n):
        x.send(ring, k0, 0)
    assert np.array_equal(ring, x.want)


def test_refusals_write_nothing(cuda, oracle):
    """With a device present: every refusal returns hipErrorInvalidValue and leaves the ring as it was."""
    import ctypes

    from lampi_amd import lib

    x = _Host(oracle, "ib", CRC)
    ring = x.before.copy()
    f, fill = lib().lampi_host_msg_send_pack, x.fill()
    m, r, fp = x.msg.ctypes.data, ring.ctypes.data + x.at, ctypes.addressof(fill)
    assert f(m, x.mlen, x.L, 0, x.n, r, x.stride, None, IB, CRC) == 1
    assert f(m, x.mlen, x.L, 0, x.n, r, x.stride, fp, 2, CRC) == 1
    assert f(m, x.mlen, x.L, 0, x.n, r, x.stride, fp, IB, 3) == 1
    assert f(m, x.mlen, x.L, 0, x.n, r, x.stride, fp, IB, CRC | (16 << 16)) == 1
    assert f(m, x.mlen, x.L, 0, x.n, r, x.L + HDR - 1, fp, IB, CRC) == 1
    assert f(m, x.mlen, x.L, 0, x.n, r, x.L + 127, fp, QUADRICS, CRC) == 1
    assert f(m, x.mlen, x.L, 1, x.n, r, x.stride, fp, IB, CRC) == 1
    assert f(None, x.mlen, x.L, 0, x.n, r, x.stride, fp, IB, CRC) == 1
    assert f(m, x.mlen, x.L, 0, x.n, None, x.stride, fp, IB, CRC) == 1
    assert f(m, x.mlen, x.L, 0, 0, r, x.stride, fp, IB, CRC) == 0
    assert np.array_equal(ring, x.before)
