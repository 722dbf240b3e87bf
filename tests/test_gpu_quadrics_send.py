"""GPU parity of the Quadrics kind of the one-call send step (lampi_send_pack_batch, lampi_msg_send_pack with
LAMPI_SEND_HDR_QUADRICS) against tests/quadrics_model.py: whole rings and header tensors, prefilled with the
synthetic stream, so every byte the calls must not touch is checked too.
"""
import numpy as np
import pytest

import quadrics_model as qm
from quadrics_model import CRC, DATA, DCSUM, ELAN, HCSUM, HDR, INLINE, NONE, QUADRICS, SUM

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("mode", [CRC, SUM, NONE], ids=["crc", "sum", "none"])
SUMS = pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
SPAN = 65536 + 16


def _dv():
    from lampi_amd import device as dv

    return dv


def _first_diff(got_t, want_t, unit):
    d = (got_t != want_t).nonzero()
    if d.numel() == 0:
        return None
    i = int(d[0].item())
    return i // unit, i % unit, int(d.numel())


class QRing:
    """n slots of `slot` bytes -- header i at i*slot (hdr=(stride, offset): in a tensor of their own), destination i
    at i*slot + 128 + i % 16 -- and a source buffer with fragment i at i*SPAN + (i + 5) % 16, all prefilled."""

    def __init__(self, cuda, n, seed, hdr=None, room=65536):
        import torch

        dv = _dv()
        self.n, self.slot = n, HDR + room + 16
        self.ring = torch.empty(n * self.slot, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.ring, seed=seed)
        self.src = torch.empty(n * SPAN + 64, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.src, seed=seed + 1)
        self.host = self.src.cpu().numpy()
        self.hdr_t, self.hdr_stride, self.hdr_off = self.ring, self.slot, 0
        if hdr is not None:
            self.hdr_stride, self.hdr_off = hdr
            self.hdr_t = torch.empty(self.hdr_off + n * self.hdr_stride + 8, dtype=torch.uint8, device=cuda)
            dv.fill_stream(self.hdr_t, seed=seed + 2)
        k = np.arange(n, dtype=np.uint64)
        self.soffs = k * np.uint64(SPAN) + (k + np.uint64(5)) % np.uint64(16)
        self.doffs = k * np.uint64(self.slot) + np.uint64(HDR) + k % np.uint64(16)
        self.hat = self.hdr_off + np.arange(n, dtype=np.int64) * self.hdr_stride
        self.tensors = [self.ring] + ([self.hdr_t] if hdr is not None else [])
        self.before = [t.clone() for t in self.tensors]

    def batch(self, oracle, rng, copylens, csumlens, mode, fresh=False):
        """(descriptors, the expected tensors) for these lengths over the source bytes as they are; random starting
        registers in CRC mode (fresh: CRC_INITIAL_REGISTER, what a receiver verifies against)."""
        import torch

        dv = _dv()
        cl, ln = np.asarray(copylens, np.uint64), np.asarray(csumlens, np.uint64)
        parts = np.full(self.n, qm.M32, np.uint64) if fresh else rng.integers(0, 2**32, size=self.n, dtype=np.uint64)
        descs = dv.make_copy_descs(self.src, self.soffs, self.ring, self.doffs, cl, ln, parts if mode == CRC else None)
        want = [t.cpu().numpy() for t in self.before]
        qm.send_expect(oracle, self.host, self.soffs, cl, ln, parts, want[-1], self.hat, want[0], self.doffs, mode)
        return descs, [torch.from_numpy(w).to(self.ring.device) for w in want]

    def reset(self):
        for t, b in zip(self.tensors, self.before):
            t.copy_(b)

    def send(self, descs, mode, **kw):
        return _dv().send_pack_batch(descs, self.hdr_t, self.hdr_stride, offset=self.hdr_off, kind=QUADRICS, mode=mode,
                                     **kw)

    def check(self, want, what=""):
        import torch

        for t, w, unit in zip(self.tensors, want, (self.slot, self.hdr_stride)):
            assert torch.equal(t, w), (what, "ring" if t is self.ring else "hdrs", _first_diff(t, w, unit))


def _classes(rng, ln):
    """copylens for csumlens `ln`: a third copied whole, a third checksum-only, a third with copylen != csumlen
    (fewer bytes copied than checksummed, or -- every other one -- more)."""
    n = len(ln)
    cl, ln = ln.copy(), ln.copy()
    k = np.arange(n) % 3
    cl[k == 1] = 0
    for i in np.nonzero(k == 2)[0]:
        cut = min(int(ln[i]), int(rng.integers(1, 24)))
        if (i // 3) % 2 == 0:
            cl[i] = ln[i] - cut
        else:
            ln[i] = ln[i] - cut
    return cl, ln


@MODES
@pytest.mark.parametrize("hdr", [None, (160, 8)], ids=["in-slot", "hdrs-apart"])
def test_descriptor_form_byte_for_byte(cuda, oracle, hdr, mode):
    import torch

    rng = np.random.default_rng(900 + mode + (10 if hdr else 0))
    n = 601
    r = QRing(cuda, n, seed=910 + mode, hdr=hdr)
    cl, ln = _classes(rng, qm.mixed_lengths(rng, n))
    mx = np.maximum(cl, ln)
    assert ((cl > 0) & (cl < ln) & (ln <= INLINE)).any() and ((cl == 0) & (ln > INLINE)).any()
    assert ((cl == ln) & (ln > 0) & (ln <= INLINE)).any() and (mx == 0).any() and ((cl > ln) & (mx > INLINE)).any()
    descs, want = r.batch(oracle, rng, cl, ln, mode)
    r.send(descs, mode)
    torch.cuda.synchronize()
    r.check(want)


@SUMS
def test_equals_the_generic_sequence(cuda, oracle, mode):
    """frag_bcopy_batch_strided into the word @64 (the inline fragments given dst = header + 72), then
    header_csum_batch_strided(124, 32) into the word @124 (zeroed first): the same bytes as the one call.  (No empty fragment:
    the generic copy stores its checksum of nothing where the Quadrics sender leaves the word alone.)"""
    import torch

    dv = _dv()
    rng = np.random.default_rng(920 + mode)
    n = 601
    r = QRing(cuda, n, seed=925)
    ln = qm.mixed_lengths(rng, n)
    ln[ln == 0] = 7
    cl, ln = _classes(rng, ln)
    ln = np.maximum(ln, 1)
    descs, want = r.batch(oracle, rng, cl, ln, mode)
    r.send(descs, mode)
    torch.cuda.synchronize()
    r.check(want)
    one_call = r.ring.clone()
    r.reset()
    inline = np.maximum(cl, ln) <= INLINE
    k = np.arange(n, dtype=np.uint64)
    doffs = np.where(inline, k * np.uint64(r.slot) + np.uint64(DATA), r.doffs)
    d = descs.cpu().numpy().view(np.uint64).reshape(n, 4).copy()
    d[:, 1] = np.uint64(r.ring.data_ptr()) + doffs
    descs2 = torch.from_numpy(d.view(np.int64)).to(cuda)
    r.ring.view(n, r.slot)[:, HCSUM:HDR] = 0  # (the sender zeroes the word first, sendFrag.h:768: SUM adds 32 words)
    dv.frag_bcopy_batch_strided(descs2, r.ring, r.slot, offset=DCSUM, mode=mode)
    dv.header_csum_batch_strided(r.ring, n, r.slot, HCSUM, 32, r.ring, r.slot, offset=HCSUM, mode=mode)
    torch.cuda.synchronize()
    assert torch.equal(r.ring, one_call), _first_diff(r.ring, one_call, r.slot)


@MODES
def test_learned_shapes_20_calls(cuda, oracle, mode):
    """Twenty calls of fragments of at most 2 KiB on one descriptor array and stream until the census has landed
    (CRC: two fragments to a wave), then four batches of 2,049..65,536 bytes in the same array under the stale
    shape, then the first again; every call compared whole."""
    import torch

    rng = np.random.default_rng(930 + mode)
    n = 601
    r = QRing(cuda, n, seed=935)
    small = rng.integers(0, 2049, size=n).astype(np.uint64)
    small[:8] = [0, 1, 51, 52, 53, 2047, 2048, 64]
    big = rng.integers(2049, 65537, size=n).astype(np.uint64)
    prepared = {"small": r.batch(oracle, rng, *_classes(rng, small), mode),
                "big": r.batch(oracle, rng, *_classes(rng, big), mode)}
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        descs = torch.empty_like(prepared["small"][0])
        for i, key in enumerate(["small"] * 20 + ["big"] * 4 + ["small"] * 4):
            batch, want = prepared[key]
            descs.copy_(batch)
            r.reset()
            r.send(descs, mode, stream=stream)
            stream.synchronize()
            r.check(want, (i, key))


@MODES
def test_row_groups(cuda, oracle, mode):
    """LAMPI_CSUM_ROWS_HINT(16) over 300 fragments of 65,536 bytes with a few short, inline and empty ones among
    them: the copies run as row groups joined by a second launch, then the stamp."""
    import torch

    rng = np.random.default_rng(950 + mode)
    n = 300
    r = QRing(cuda, n, seed=955)
    ln = np.full(n, 65536, np.uint64)
    ln[[0, 7, 100, 150, 201, 299]] = [52, 0, 4097, 1, 65535, 53]
    descs, want = r.batch(oracle, rng, *_classes(rng, ln), mode)
    r.send(descs, mode, rows_hint=16)
    torch.cuda.synchronize()
    r.check(want)


TMPL = (np.arange(72, dtype=np.uint16) * 7 + 3).astype(np.uint8)
MSG_CASES = {
    # frag_len, slot_stride, message lengths
    "inline52": (52, 184, [52 * 300, 52 * 299 + 1, 52 * 299 + 51, 7]),
    "packed53": (53, 184, [53 * 300, 53 * 299 + 1, 53 * 299 + 52]),
    "packed2048": (2048, 2176, [2048 * 300, 2048 * 299 + 52, 2048 * 299 + 1, 2048 * 299 + 53, 2048 * 2 + 2047, 30]),
    "bare2048": (2048, 128, [2048 * 300, 2048 * 299 + 52, 2048 * 299 + 53, 40, 2048 * 515]),
}


@MODES
@pytest.mark.parametrize("case", list(MSG_CASES))
def test_message_form(cuda, oracle, case, mode):
    import torch

    dv = _dv()
    L, stride, lengths = MSG_CASES[case]
    assert stride == HDR or stride == (HDR + L + 7) // 8 * 8
    nmax = max((m + L - 1) // L for m in lengths)
    ring = torch.empty((nmax + 2) * stride, dtype=torch.uint8, device=cuda)
    dv.fill_stream(ring, seed=940)
    before = ring.clone()
    hbefore = before.cpu().numpy()
    msg = torch.empty(max(lengths) + 8, dtype=torch.uint8, device=cuda)
    dv.fill_stream(msg, seed=941)
    hm = msg.cpu().numpy()
    args = dict(frag_seq0=(1 << 40) + 5, frag_seq_step=3, desc_ptr0=0x7F0000001000, desc_ptr_stride=256,
                seq_offset0=(1 << 33) + 11)
    e0 = int(qm.u32(TMPL[None, ELAN:ELAN + 4])[0])
    for off, mlen in enumerate(lengths + [0]):  # (the last one: an empty message)
        off = off % 8  # the message at byte offsets 0..4
        m = hm[off:off + mlen]
        want = hbefore.copy()
        n = qm.msg_send_expect(oracle, m, L, want, stride, TMPL, args["frag_seq0"], 3, args["desc_ptr0"], 256,
                               args["seq_offset0"], mode)
        ring.copy_(before)
        dv.msg_send_pack(msg[off:], L, ring, stride, TMPL, kind=QUADRICS, mode=mode, msg_len=mlen, **args)
        torch.cuda.synchronize()
        got = ring.cpu().numpy()
        assert np.array_equal(got, want), (mlen, _first_diff(ring, torch.from_numpy(want).to(cuda), stride))
        # the envelopes field by field
        S = got[:n * stride].reshape(n, stride)
        lens = qm.u32(S[:, 20:24]).astype(np.int64)
        k = np.arange(n, dtype=np.int64)
        assert np.array_equal(lens, np.minimum(L, mlen - k * L) if mlen else np.zeros(1, np.int64))
        assert np.array_equal(qm.u32(S[:, ELAN:ELAN + 4]), ((e0 + k * L) & qm.M32).astype(np.uint32))
        assert np.array_equal(np.ascontiguousarray(S[:, 56:64]).view("<u8").reshape(n),
                              (args["seq_offset0"] + k * L).astype(np.uint64))
        for i in range(n):
            c = int(lens[i]) if lens[i] <= INLINE else 0
            assert not S[i, DATA + c:HCSUM].any(), i          # zero padding in data[]
            assert np.array_equal(S[i, DATA:DATA + c], m[i * L:i * L + c]), i
        if stride == HDR:  # a bare envelope queue: nothing but envelopes, nothing after the last one
            assert np.array_equal(got[n * stride:], hbefore[n * stride:])
        if mlen and (mlen % L) and (mlen % L) <= INLINE and L > INLINE and n > 1:
            assert lens[-1] <= INLINE < lens[0]  # the last fragment inline, the others not
            if stride > HDR:
                assert np.array_equal(S[-1, HDR:], hbefore[(n - 1) * stride + HDR:n * stride])
