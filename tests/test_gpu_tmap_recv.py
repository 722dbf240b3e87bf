"""GPU parity of the receive step through a typemap (lampi_tmap_recv_unpack) against the models.

The ring form's model (tests/recv_unpack_model.py: pack_slots, expect_ring -- the header test, the drop, CopyToApp
against the word @64, from the oracle) runs over the packed bytes; tests/tmap_model.py's address rule maps the
packed application buffer it leaves onto the typemap's pieces.  Rings are built in shuffled slot order with faults
of every class; d_copied, d_csum, both masks (no stray bits) and both counts must be exact and the application
buffer is compared whole: the gaps between the pieces and the pieces of dropped fragments keep their sentinel.
"""
import numpy as np
import pytest

import tmap_model as tmm
from recv_unpack_model import LEN_AT, check, expect_ring, flip_bit, pack_slots
from test_gpu_send_pack import CRC, DCSUM, GM, HCSUM, HDR, IB, NONE, SUM, _stamp_all

pytestmark = pytest.mark.gpu

NFRAG = {100: 300, 1976: 61, 4096: 37, 65456: 7}
SEQ0 = 2**64 - 4096 * 3 - 5  # dataSeqOffset wraps within the first fragments


def _dv():
    from lampi_amd import device as dv

    return dv


def _stride(frag_len):
    return (HDR + frag_len + 8 + 7) // 8 * 8


def _restamp(oracle, hring, at, kind, mode, wrong_bit=None):
    """The words @64 / @68 of the header at hring[at] made consistent with its bytes [0, 64) again (wrong_bit: with
    that bit of dataChecksum flipped first)."""
    if mode == NONE:
        return
    v = int(hring[at + DCSUM:at + HCSUM].view("<u4")[0])
    if wrong_bit is not None:
        v ^= 1 << wrong_bit
    n = int(hring[at + LEN_AT:at + LEN_AT + 4].view("<u4")[0])
    w = _stamp_all(oracle, hring[None, at:at + DCSUM], np.array([v], np.uint32), np.array([n == 0]), kind, mode)
    hring[at + DCSUM:at + HCSUM] = w[0].astype("<u4").view(np.uint8)
    hring[at + HCSUM:at + HDR] = w[1].astype("<u4").view(np.uint8)


class _Recv:
    """A message of mlen packed bytes as slots in shuffled order, faults by fragment index, and the typemap-shaped
    application buffer (sentinel bytes) of `count` elements."""

    def __init__(self, cuda, oracle, tm, count, frag_len, mlen, kind, mode, seed, faults=True):
        import torch

        dv = _dv()
        rng = np.random.default_rng(seed)
        self.tm, self.count, self.kind, self.mode, self.cuda = tm, count, kind, mode, cuda
        self.L, self.stride = frag_len, _stride(frag_len)
        self.app_len = count * tm.packed_size
        m = rng.integers(0, 256, size=mlen, dtype=np.uint8)
        n = (mlen + frag_len - 1) // frag_len if mlen else 1
        self.n = n
        ring_t = torch.empty(n * self.stride, dtype=torch.uint8, device=cuda)
        dv.fill_stream(ring_t, seed=seed + 1)
        hring = ring_t.cpu().numpy()
        order = rng.permutation(n)
        pack_slots(oracle, rng, hring, m, frag_len, self.stride, SEQ0, kind, mode, order)
        lens = np.minimum(frag_len, mlen - np.arange(n, dtype=np.int64) * frag_len)
        hdr_ranges = [(0, 20 if mode == NONE else DCSUM), (DCSUM, HCSUM), (HCSUM, HDR)]
        nh = 0
        for k in range(n if faults else 0):
            at, c = int(order[k]) * self.stride, int(lens[k])
            cls = k % 10
            if cls in (1, 7):  # a header bit: in [0, 64), the word @64, the word @68 in turn
                flip_bit(hring, at, rng, *hdr_ranges[nh % 3])
                nh += 1
            if cls in (3, 7) and c:  # a payload byte, every other time the last one
                hring[at + HDR + (c - 1 if k % 20 == 3 else int(rng.integers(0, c)))] ^= np.uint8(0x10)
            if cls == 5:  # a consistent header with a wrong dataChecksum
                _restamp(oracle, hring, at, kind, mode, wrong_bit=int(rng.integers(0, 32)))
            if k == 9 or (n < 10 and k == 2):  # a dataLength past the slot, the header otherwise consistent
                hring[at + LEN_AT:at + LEN_AT + 4] = np.array([self.stride - HDR + 1], "<u4").view(np.uint8)
                _restamp(oracle, hring, at, kind, mode)
        self.hring = hring
        self.ring = torch.from_numpy(hring).to(cuda)
        self.hbuf, self.origin = tmm.host_buffer(tm, count, seed + 2)
        self.buf = torch.from_numpy(self.hbuf).to(cuda)
        self.dtm = dv.make_tmap(tm.pairs(), tm.extent, count, cuda)
        # the model: the ring form over the packed view of the buffer, mapped back through the address rule
        idx = self.origin + tmm.index_map(tm, np.arange(self.app_len, dtype=np.int64))
        app = self.hbuf[idx]
        self.want = expect_ring(oracle, hring, n, self.stride, app, self.app_len, SEQ0, kind, mode)
        self.want_buf = self.hbuf.copy()
        self.want_buf[idx] = app

    def run(self, what=""):
        got = _dv().tmap_recv_unpack(self.ring, self.n, self.stride, self.buf, self.dtm, kind=self.kind, mode=self.mode,
                                     seq_offset0=SEQ0, base_offset=self.origin)
        check(got, self.want, self.n, self.buf, self.want_buf, self.tm.extent, what)
        assert np.array_equal(self.ring.cpu().numpy(), self.hring), (what, "ring changed")
        return got


def _clipped(tm, frag_len, nf):
    """(count, mlen): most fragments inside count elements, one cut by the end, the rest at Offset >= app_len --
    where one element is not longer than the whole message."""
    count = max(1, ((nf - 2) * frag_len + frag_len // 3) // tm.packed_size)
    return count, nf * frag_len


@pytest.mark.parametrize("kind", [GM, IB], ids=["gm", "ib"])
@pytest.mark.parametrize("frag_len", tmm.FRAG_LENS)
@pytest.mark.parametrize("tm", tmm.TYPEMAPS, ids=[t.name for t in tmm.TYPEMAPS])
def test_outputs_and_buffer(cuda, oracle, tm, frag_len, kind):
    """Every mode, LAMPI_CSUM_NONE included; the last fragment 1, 15, 17 bytes or whole in turn."""
    nf = NFRAG[frag_len]
    turn = tmm.TYPEMAPS.index(tm) + tmm.FRAG_LENS.index(frag_len) + kind
    for mode in (CRC, SUM, NONE):
        count, _ = _clipped(tm, frag_len, nf)
        mlen = tmm.window_len(frag_len, nf, tmm.LAST_LENS[(turn + mode) % 4])
        r = _Recv(cuda, oracle, tm, count, frag_len, mlen, kind, mode, seed=1000 + 7 * turn + mode)
        r.run(f"mode {mode}")


@pytest.mark.parametrize("kind,mode", [(k, m) for k in (GM, IB) for m in (CRC, SUM, NONE)])
def test_every_fault_class_is_in_the_ring(cuda, oracle, kind, mode):
    """T2 at IB's 1,976 bytes, 61 fragments: the model's verdicts show every class -- dropped headers, corrupt
    payloads, a clipped delivery, fragments beyond the buffer -- and the device gives the same."""
    tm, L, nf = tmm.T2, 1976, 61
    count, mlen = _clipped(tm, L, nf)
    r = _Recv(cuda, oracle, tm, count, L, mlen - L + 17, kind, mode, seed=1100 + mode)
    copied, _, hbad, dbad = r.want
    assert int(hbad.sum()) >= (1 if mode == NONE else 6)      # NONE: the dataLength past the slot alone
    assert int(dbad.sum()) >= (0 if mode == NONE else 10)
    assert np.any((copied > 0) & (copied < L) & (copied != 17))  # Offset + dataLength > app_len, clipped
    assert int((copied == 0).sum()) >= 1                      # Offset >= app_len
    r.run()


@pytest.mark.parametrize("kind,mode", [(k, m) for k in (GM, IB) for m in (CRC, SUM, NONE)])
def test_contiguous_typemap_equals_msg_recv_unpack(cuda, oracle, kind, mode):
    import torch

    dv = _dv()
    for L, nf in ((65456, 7), (1976, 61), (100, 300)):
        count, mlen = _clipped(tmm.T5, L, nf)
        r = _Recv(cuda, oracle, tmm.T5, count, L, mlen - L + 15, kind, mode, seed=1200 + mode)
        before = r.buf.clone()
        ours = r.run(f"L {L}")
        mine = r.buf.clone()
        r.buf.copy_(before)
        ring_form = dv.msg_recv_unpack(r.ring, r.n, r.stride, r.buf[r.origin:], kind=kind, mode=mode, seq_offset0=SEQ0,
                                       app_len=r.app_len)
        torch.cuda.synchronize()
        for a, b in zip(ours, ring_form):
            assert torch.equal(a, b), L
        assert torch.equal(mine, r.buf), L


def test_refusals_write_nothing(cuda, oracle):
    """Every refusal returns hipErrorInvalidValue and leaves the outputs and the buffer untouched."""
    import ctypes

    import torch

    from lampi_amd import lib
    from lampi_amd._lib import Tmap

    tm = tmm.T2
    r = _Recv(cuda, oracle, tm, 40, 500, 2300, GM, CRC, seed=1300, faults=False)
    f = lib().lampi_tmap_recv_unpack
    outs = [torch.full((16,), 0x5A5A5A5A, dtype=torch.int32, device=cuda) for _ in range(5)]
    copied, csum, hm, dm, nbad = [o.data_ptr() for o in outs]
    before = r.buf.clone()

    def tmap(**kw):
        t = Tmap()
        ctypes.memmove(ctypes.addressof(t), ctypes.addressof(r.dtm.struct), ctypes.sizeof(Tmap))
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    good = tmap()

    def call(ring=r.ring.data_ptr(), n=r.n, stride=r.stride, kind=GM, base=r.buf.data_ptr() + r.origin,
             t=ctypes.addressof(good), nb=nbad, mode=CRC, cp=copied):
        return f(ring, n, stride, kind, base, t, SEQ0, cp, csum, hm, dm, nb, mode, None)

    for t in (tmap(d_pairs=None), tmap(num_pairs=0), tmap(packed_size=0), tmap(reserved=7),
              tmap(count=(1 << 63) // tm.packed_size + 1)):
        assert call(t=ctypes.addressof(t)) == 1
    assert call(t=None) == 1
    for mode in (3, -1, CRC | 0x100, SUM | (4 << 16)):
        assert call(mode=mode) == 1
    for kind in (2, 3, -1):  # Quadrics (3) is refused
        assert call(kind=kind) == 1
    assert call(n=1 << 32) == 1
    assert call(stride=64) == 1
    assert call(stride=r.stride + 4) == 1
    assert call(ring=r.ring.data_ptr() + 4) == 1
    assert call(ring=None) == 1
    assert call(base=None) == 1
    assert call(nb=None) == 1
    assert call(cp=None) == 1
    torch.cuda.synchronize()
    assert torch.equal(r.buf, before)
    for o in outs:
        assert bool((o == 0x5A5A5A5A).all())
    assert call(n=0) == 0  # no slots: both counts zeroed, nothing else
    torch.cuda.synchronize()
    assert [int(x) for x in outs[4][:2].cpu()] == [0, 0] and bool((outs[0] == 0x5A5A5A5A).all())
    assert torch.equal(r.buf, before)
