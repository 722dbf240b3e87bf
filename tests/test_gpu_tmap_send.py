"""GPU parity of the send step through a typemap (lampi_tmap_send_pack) against tests/tmap_model.py.

Whole rings are compared byte for byte: the payloads against the model's packed bytes (the address rule), the
72-byte headers against the flavour table of tests/test_gpu_send_pack.py (_msg_want, _stamp_all), the bytes between
a payload's end and the next slot against their sentinel; the source must be unchanged.  The contiguous typemap must
leave lampi_msg_send_pack's ring, and T1 / T2 the ring of today's sequence over the reference's own pieces
(lampi_chain_csum_batch_strided, then lampi_header_csum_batch_strided).
"""
import ctypes

import numpy as np
import pytest

import tmap_model as tmm
from test_gpu_send_pack import CRC, DCSUM, GM, HCSUM, HDR, IB, NONE, SUM, WORDS, _first_diff, _msg_want

pytestmark = pytest.mark.gpu

FILL = dict(frag_seq0=2**64 - 2, frag_seq_step=3, desc_ptr0=0x00007F0012345000, desc_ptr_stride=0x1A8,
            seq_offset0=0x0000000100000010)
NFRAG = {100: 300, 1976: 61, 4096: 37, 65456: 5}
INVALID = 1  # hipErrorInvalidValue


def _dv():
    from lampi_amd import device as dv

    return dv


def _stride(frag_len):
    return (HDR + frag_len + 8 + 7) // 8 * 8  # room past the longest payload, 8-byte aligned


class _Send:
    """`count` elements of `tm` in a device buffer of random bytes (origin inside it), a ring of sentinel bytes."""

    def __init__(self, cuda, tm, count, frag_len, nslots, seed):
        import torch

        dv = _dv()
        self.tm, self.count, self.L, self.stride = tm, count, frag_len, _stride(frag_len)
        self.hbuf, self.origin = tmm.host_buffer(tm, count, seed)
        self.buf = torch.from_numpy(self.hbuf).to(cuda)
        self.dtm = dv.make_tmap(tm.pairs(), tm.extent, count, cuda)
        self.ring = torch.empty(nslots * self.stride, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.ring, seed=seed + 1)
        self.before_t = self.ring.clone()
        self.before = self.ring.cpu().numpy()
        self.tmpl = np.random.default_rng(seed + 2).integers(0, 256, size=HDR, dtype=np.uint8)

    def send(self, kind, mode, pack_off, pack_len, stream=None):
        self.ring.copy_(self.before_t)
        return _dv().tmap_send_pack(self.buf, self.dtm, self.L, self.ring, self.stride, self.tmpl, kind=kind, mode=mode,
                                    pack_off=pack_off, pack_len=pack_len, base_offset=self.origin, stream=stream, **FILL)

    def want(self, oracle, kind, mode, pack_off, pack_len):
        w = self.before.copy()
        m = tmm.packed(self.tm, self.hbuf, self.origin, pack_off, pack_len)
        _msg_want(oracle, w, m, kind, self.L, self.stride, pack_len, self.tmpl, FILL, mode)
        return w

    def check(self, oracle, kind, mode, pack_off, pack_len, what):
        import torch

        self.send(kind, mode, pack_off, pack_len)
        torch.cuda.synchronize()
        got, want = self.ring.cpu().numpy(), self.want(oracle, kind, mode, pack_off, pack_len)
        if not np.array_equal(got, want):
            i = int(np.nonzero(got != want)[0][0])
            pytest.fail(f"{what}: slot {i // self.stride}, byte {i % self.stride}: {got[i]} != {want[i]}")
        assert np.array_equal(self.buf.cpu().numpy(), self.hbuf), (what, "source changed")


@pytest.mark.parametrize("kind", [GM, IB], ids=["gm", "ib"])
@pytest.mark.parametrize("frag_len", tmm.FRAG_LENS)
@pytest.mark.parametrize("tm", tmm.TYPEMAPS, ids=[t.name for t in tmm.TYPEMAPS])
def test_ring_byte_for_byte(cuda, oracle, tm, frag_len, kind):
    """Every mode; the window's start (0, 7 bytes into a pair, an element boundary) and its last fragment (1, 15, 17
    bytes, a whole one) in turn."""
    nf = NFRAG[frag_len]
    offs = tmm.pack_offsets(tm)
    count = tmm.count_for(tm, max(offs) + nf * frag_len) + 1
    s = _Send(cuda, tm, count, frag_len, nf, seed=900 + frag_len % 97)
    turn = tmm.TYPEMAPS.index(tm) + tmm.FRAG_LENS.index(frag_len) + kind
    for mode in (CRC, SUM, NONE):
        for w in range(2):
            pack_off = offs[(turn + mode + w) % 3]
            last = tmm.LAST_LENS[(turn + 2 * mode + w) % 4]
            s.check(oracle, kind, mode, pack_off, tmm.window_len(frag_len, nf - w, last),
                    f"mode {mode} pack_off {pack_off} last {last}")


@pytest.mark.parametrize("kind,mode", [(k, m) for k in (GM, IB) for m in (CRC, SUM, NONE)])
def test_every_window_start_and_last_fragment(cuda, oracle, kind, mode):
    """T2 (chunks straddle pairs and elements) at IB's 1,976 bytes: all twelve (pack_off, last fragment) pairs."""
    tm, L, nf = tmm.T2, 1976, 9
    offs = tmm.pack_offsets(tm)
    s = _Send(cuda, tm, tmm.count_for(tm, max(offs) + nf * L) + 1, L, nf, seed=931)
    for pack_off in offs:
        for last in tmm.LAST_LENS:
            s.check(oracle, kind, mode, pack_off, tmm.window_len(L, nf, last), f"pack_off {pack_off} last {last}")


@pytest.mark.parametrize("kind,mode", [(k, m) for k in (GM, IB) for m in (CRC, SUM, NONE)])
def test_contiguous_typemap_equals_msg_send_pack(cuda, oracle, kind, mode):
    import torch

    dv = _dv()
    for L, nf, last in ((65456, 5, 17), (1976, 61, None), (100, 300, 1)):
        plen = tmm.window_len(L, nf, last)
        s = _Send(cuda, tmm.T5, tmm.count_for(tmm.T5, plen), L, nf, seed=940)
        s.send(kind, mode, 0, plen)
        ours = s.ring.clone()
        s.ring.copy_(s.before_t)
        dv.msg_send_pack(s.buf[s.origin:], L, s.ring, s.stride, s.tmpl, kind=kind, mode=mode, msg_len=plen, **FILL)
        torch.cuda.synchronize()
        assert torch.equal(ours, s.ring), (L, _first_diff(ours, s.ring, s.stride))
        assert np.array_equal(ours.cpu().numpy(), s.want(oracle, kind, mode, 0, plen))


@pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
@pytest.mark.parametrize("tm", [tmm.T1, tmm.T2], ids=["T1", "T2"])
def test_equals_todays_sequence(cuda, oracle, tm, mode):
    """GM: the pieces of the reference's walk through lampi_chain_csum_batch_strided (dataChecksum @64), then
    lampi_header_csum_batch_strided(68, 18), on headers prefilled the same way: identical rings."""
    import torch

    dv = _dv()
    L, nf = 1976, 40
    pack_off = tmm.pack_offsets(tm)[1]
    plen = tmm.window_len(L, nf, 15)
    count = tmm.count_for(tm, pack_off + plen) + 1
    s = _Send(cuda, tm, count, L, nf, seed=950)
    s.send(GM, mode, pack_off, plen)
    ours = s.ring.clone()
    want = s.want(oracle, GM, mode, pack_off, plen)
    assert np.array_equal(ours.cpu().numpy(), want)
    # today's sequence: the headers' bytes [0, 64) as the call builds them, the word @68 zero
    pre = s.before.copy().reshape(nf, s.stride)
    pre[:, :DCSUM] = want.reshape(nf, s.stride)[:, :DCSUM]
    pre[:, HCSUM:HDR] = 0
    s.ring.copy_(torch.from_numpy(pre.reshape(-1)).to(cuda))
    so, do, ln, first = [], [], [], [0]
    for j, (off, n) in enumerate(tmm.fragments(pack_off, plen, L)):
        at = 0
        for a, c in tmm.send_pieces(tm, off, n, count * tm.packed_size):
            so.append(s.origin + a)
            do.append(j * s.stride + HDR + at)
            ln.append(c)
            at += c
        first.append(len(ln))
    pieces = dv.make_copy_descs(s.buf, so, s.ring, do, ln, ln)
    first_t = torch.from_numpy(np.asarray(first, np.int32)).to(cuda)
    dv.chain_csum_batch_strided(pieces, first_t, s.ring, s.stride, offset=DCSUM, mode=mode)
    dv.header_csum_batch_strided(s.ring, nf, s.stride, HDR - 4, WORDS, s.ring, s.stride, offset=HCSUM, mode=mode)
    torch.cuda.synchronize()
    assert torch.equal(ours, s.ring), _first_diff(ours, s.ring, s.stride)


@pytest.mark.parametrize("kind,mode", [(k, m) for k in (GM, IB) for m in (CRC, SUM, NONE)])
def test_empty_message(cuda, oracle, kind, mode):
    """pack_len == 0: one empty fragment, its header written (at the window's start and in the middle of a pair)."""
    for L in (1976, 65456):
        s = _Send(cuda, tmm.T2, 4, L, 1, seed=960)
        for pack_off in (0, 72, 4 * tmm.T2.packed_size):
            s.check(oracle, kind, mode, pack_off, 0, f"L {L} pack_off {pack_off}")


@pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
def test_window_beyond_4_gib(cuda, oracle, mode):
    """Packed positions past 2^32: 2^40 elements of extent 0 (every element reads the same bytes, so the buffer
    stays small) and a window that starts 8 GiB into the message, in the middle of a pair."""
    tm = tmm.Typemap("T2x0", tmm.T2.size, tmm.T2.offset, 0, overlap_ok=True)
    s = _Send(cuda, tm, 1 << 40, 1976, 10, seed=980)
    pack_off = (1 << 33) // tm.packed_size * tm.packed_size + 3 * tm.packed_size + 8
    s.check(oracle, GM, mode, pack_off, tmm.window_len(1976, 10, 15), "8 GiB in")


def test_refusals_write_nothing(cuda):
    """Every refusal of the validation list returns hipErrorInvalidValue and leaves the ring untouched."""
    import torch

    from lampi_amd import lib
    from lampi_amd._lib import Tmap

    dv = _dv()
    tm = tmm.T2
    s = _Send(cuda, tm, 40, 500, 6, seed=970)
    f = lib().lampi_tmap_send_pack
    total = 40 * tm.packed_size
    fill = np.zeros(112, np.uint8)
    b, r, fp = s.buf.data_ptr() + s.origin, s.ring.data_ptr(), fill.ctypes.data

    def tmap(**kw):
        t = Tmap()
        ctypes.memmove(ctypes.addressof(t), ctypes.addressof(s.dtm.struct), ctypes.sizeof(Tmap))
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    good = tmap()
    tp = ctypes.addressof(good)

    def call(base=b, t=tp, off=0, plen=2000, L=500, ring=r, stride=s.stride, fl=fp, kind=GM, mode=CRC):
        return f(base, t, off, plen, L, ring, stride, fl, kind, mode, None)

    bad = [tmap(d_pairs=None), tmap(num_pairs=0), tmap(packed_size=0), tmap(count=(1 << 63) // tm.packed_size + 1),
           tmap(reserved=1)]
    for t in bad:
        assert call(t=ctypes.addressof(t)) == INVALID
    assert call(t=None) == INVALID
    assert call(off=total - 1999) == INVALID                    # pack_off + pack_len > count * packed_size
    assert call(off=total + 1, plen=0) == INVALID
    assert call(off=2**64 - 8, plen=16) == INVALID              # ... with the sum wrapping
    huge = tmap(count=(1 << 40))
    assert call(t=ctypes.addressof(huge), plen=(1 << 32) * 8, L=8, stride=80) == INVALID  # 2^32 fragments
    for mode in (3, -1, CRC | 0x100, SUM | (4 << 16)):           # no BY_BYTES, no hint bits
        assert call(mode=mode) == INVALID
    for kind in (2, 3, -1):                                      # Quadrics (3) is refused
        assert call(kind=kind) == INVALID
    assert call(L=0) == INVALID
    assert call(L=1 << 32) == INVALID
    assert call(stride=500 + HDR - 4) == INVALID                 # slot_stride < 72 + frag_len
    assert call(stride=s.stride + 4) == INVALID                  # not 8-byte aligned
    assert call(ring=r + 4) == INVALID
    assert call(ring=None) == INVALID
    assert call(fl=None) == INVALID
    assert call(base=None) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(s.ring, s.before_t)
    assert call() == 0                                           # the same arguments unaltered pass
    with pytest.raises(ValueError):                              # the binding checks what the pieces reach
        dv.tmap_send_pack(s.buf, s.dtm, 500, s.ring, s.stride, s.tmpl, base_offset=0)
    with pytest.raises(ValueError):
        dv.tmap_send_pack(s.buf, s.dtm, 500, s.ring[:s.stride], s.stride, s.tmpl, base_offset=s.origin)
    torch.cuda.synchronize()
