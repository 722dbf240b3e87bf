"""GPU parity of the one-call receive step (lampi_recv_unpack_batch, lampi_msg_recv_unpack).

The reference receives a fragment in one place: the header test (ref src/path/gm/path.cc:364-393,
src/path/ib/path.cc:652-680), a fragment with a bad header back to the pool and never delivered (gm/path.cc:453-,
ib/path.cc:702-717), otherwise RecvDesc_t::CopyToApp (src/path/common/BaseDesc.cc:288-342) to the offset the
header's dataSeqOffset gives, checked against its dataChecksum.  Every expectation comes from the oracle alone
(tests/recv_unpack_model.py); each test prefills the application buffer with the synthetic stream and compares it
whole, so a dropped fragment's untouched range is checked, along with copied, csum, both masks and both counts.
"""
import numpy as np
import pytest

from recv_unpack_model import (HDR_FAULTS, LEN_AT, RecvRing, check, expect_ring, fault_classes, flip_bit,
                               pack_slots)
from test_gpu_send_pack import (CRC, DCSUM, EDGE_LENGTHS, GM, HCSUM, HDR, IB, MSG_CASES, NONE, SUM, WORDS, _fill,
                                _first_diff, _ib_lengths, _Msg)

pytestmark = pytest.mark.gpu

KINDS = pytest.mark.parametrize("kind", [GM, IB], ids=["gm", "ib"])
MODES = pytest.mark.parametrize("mode", [CRC, SUM, NONE], ids=["crc", "sum", "none"])
SUMS = pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])


def _dv():
    from lampi_amd import device as dv

    return dv


def _assert_classes(b, mode):
    """Each planted class is there, and reads as the model says: with checksumming on a header fault drops the
    fragment whatever its payload (the header wins: -2, data bit clear)."""
    cls, (copied, _, hbad, dbad) = b["cls"], b["want"]
    for c in (0, 1, 2, 3):
        assert (cls == c).any(), c
    if mode == NONE:
        assert not hbad.any() and not dbad.any() and (copied >= 0).all()
        return
    hdr = (cls == 1) | (cls == 3)
    assert np.array_equal(hbad, hdr) and (copied[hdr] == -2).all() and not dbad[hdr].any()
    assert (copied[cls == 2] == -1).any() and not dbad[cls == 0].any() and (copied[cls == 0] >= 0).all()


@KINDS
@MODES
def test_ring_byte_for_byte(cuda, oracle, kind, mode):
    """601 fragments of 0..65,456 bytes, the four fault classes, every end of the batch with every kind of fault
    (three passes: fragment 0 empty with a bad header and a corrupt last fragment; the reverse with a full first
    fragment; both faults at both ends)."""
    rng = np.random.default_rng(900 + 3 * kind + mode)
    n, slot = 601, 70016
    r = RecvRing(cuda, n, slot, seed=910 + mode)
    for p, (ends, first) in enumerate([((1, 2), 0), ((2, 1), 65456), ((3, 3), 1976)]):
        lens = rng.integers(0, 65457, size=n).astype(np.uint64)
        lens[rng.choice(np.arange(3, n - 1), size=len(EDGE_LENGTHS), replace=False)] = EDGE_LENGTHS
        lens[:3] = [first, 65456, 1976]
        lens[n - 1] = 4097
        b = r.batch(oracle, rng, lens, kind, mode, fault_classes(rng, n, ends), roomy=(0, n - 1))
        _assert_classes(b, mode)
        if mode != NONE:  # (an empty fragment is DataOK whatever its header's dataChecksum says)
            code = {1: -2, 2: -1, 3: -2}
            assert [int(b["want"][0][0]), int(b["want"][0][n - 1])] == [code[ends[0]] if first or ends[0] != 2 else 0,
                                                                         code[ends[1]]]
        al = b["descs"].cpu().numpy()[:, 2]
        assert (al <= 0).any() and ((al > 0) & (al < lens.astype(np.int64))).any() and (al > lens.astype(np.int64)).any()
        for hdrs in [True, False] if mode == NONE else [True]:  # (checksumming off: d_hdrs = None is accepted)
            r.load(b)
            r.check(r.recv(b["descs"], kind, mode, hdrs=hdrs), b, (p, hdrs))


@KINDS
@SUMS
def test_equals_the_three_call_sequence(cuda, oracle, kind, mode):
    """header_check_batch / header_compare_batch + copy_to_app_batch on the same ring: the header mask is the
    check's mask, and every fragment with a good header has the same copied, csum and data bit."""
    import torch

    dv = _dv()
    rng = np.random.default_rng(920 + 3 * kind + mode)
    n, slot = 601, 70016
    r = RecvRing(cuda, n, slot, seed=921)
    lens = rng.integers(0, 65457, size=n).astype(np.uint64)
    lens[:len(EDGE_LENGTHS)] = EDGE_LENGTHS
    b = r.batch(oracle, rng, lens, kind, mode, fault_classes(rng, n, (0, 1)))
    r.load(b)
    if kind == GM:
        m3, n3 = dv.header_check_batch(r.ring, n, slot, HDR, WORDS, HCSUM, mode=mode)
    else:
        m3, n3 = dv.header_compare_batch(r.ring, n, slot, HDR - 4, HCSUM, mode=mode)
    c3, s3, d3, nd3 = dv.copy_to_app_batch(b["descs"], r.ring, expected_stride=slot, expected_offset=DCSUM, mode=mode)
    torch.cuda.synchronize()
    c3, s3, bad3, d3 = c3.cpu().numpy(), dv.as_u32(s3), dv.mask_bits(m3, n), dv.mask_bits(d3, n)
    r.load(b)
    got = r.recv(b["descs"], kind, mode)
    r.check(got, b)
    copied, csum, hmask, dmask, nbad = got
    hb = dv.mask_bits(hmask, n)
    assert np.array_equal(hb, bad3) and int(nbad[0].item()) == int(n3.item())
    good = ~hb
    assert np.array_equal(copied.cpu().numpy()[good], c3[good])
    assert np.array_equal(dv.as_u32(csum)[good], s3[good])
    assert np.array_equal(dv.mask_bits(dmask, n)[good], d3[good])


def _sequence(cuda, r, prepared, order, kind, mode, **kw):
    """The batches of `order` through one descriptor array on a stream of its own (the learned shape is kept per
    stream and descriptor array), every call checked in full."""
    import torch

    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        descs = torch.empty_like(prepared[order[0]]["descs"])
        for i, k in enumerate(order):
            b = prepared[k]
            descs.copy_(b["descs"])
            r.load(b)
            r.check(r.recv(descs, kind, mode, stream=stream, **kw), b, (i, k))


@KINDS
@MODES
def test_learned_schedules(cuda, oracle, kind, mode):
    """IB-sized batches until the census picks the pair kernel (CRC, behind the pre-pass) / a wave per fragment
    (SUM, off), then batches of 2,049-70,000 bytes in the same descriptor array on the same stream under the stale
    shape, then IB again.  Header-bad fragments sit at indices the census samples and at indices it does not."""
    rng = np.random.default_rng(930 + 3 * kind + mode)
    n, slot = 601, 70096
    r = RecvRing(cuda, n, slot, seed=931)
    sampled = sorted(set(int(x) for x in np.arange(64) * n // 64))
    prepared = {}
    for name, lens in (("ib", _ib_lengths(rng, n, True)), ("big", rng.integers(2049, 70001, size=n))):
        cls = fault_classes(rng, n, (1, 2))
        cls[sampled[3:40:6]] = 1
        cls[[x + 1 for x in sampled[5:40:6]]] = 1
        cls[sampled[4:40:6]] = 2
        prepared[name] = r.batch(oracle, rng, lens, kind, mode, cls,
                                 app_lens=np.asarray(lens, np.int64) + np.where(np.arange(n) % 5 == 0, -3, 11))
    _sequence(cuda, r, prepared, ["ib"] * 20 + ["big"] * 4 + ["ib"] * 4, kind, mode)


def _row_group_batch(r, oracle, rng, n, length, kind, mode):
    """A fragment with fewer rows than the hint, one of length 0, one of length 1, an app_len that cuts a copy inside
    a row group, a header-bad fragment, a data-bad fragment whose flipped byte is in its last row group."""
    lens = np.full(n, length, np.uint64)
    lens[n // 2] = length - 4097
    lens[1] = 0
    lens[n - 2] = 1
    al = lens.astype(np.int64) + 7
    al[0] = length // 2 + 5
    cls = np.zeros(n, np.int64)
    cls[n - 1] = 1
    cls[2] = 2
    if n > 8:
        cls[5], cls[6] = 3, 1
    return r.batch(oracle, rng, lens, kind, mode, cls, app_lens=al, last_byte=(2,))


@KINDS
@MODES
@pytest.mark.parametrize("n,length,hint", [(300, 65456, 16), (5, (1 << 20) + 3, 0), (5, (1 << 20) + 3, 64),
                                           (40, 12000, 3)], ids=["gm16", "1m", "1m_hint64", "12k_hint3"])
def test_row_groups(cuda, oracle, n, length, hint, kind, mode):
    rng = np.random.default_rng(940 + mode)
    slot = (HDR + length + 15 + 63) // 64 * 64
    r = RecvRing(cuda, n, slot, seed=941)
    b = _row_group_batch(r, oracle, rng, n, length, kind, mode)
    if mode != NONE:
        assert list(b["want"][0][[2, n - 1]]) == [-1, -2]
    r.load(b)
    r.check(r.recv(b["descs"], kind, mode, rows_hint=hint), b)


@KINDS
@MODES
def test_learned_row_groups(cuda, oracle, kind, mode):
    """Equal 65,456-byte batches with no hint until the census learns 16 rows: 20 calls, each checked in full."""
    rng = np.random.default_rng(945 + mode)
    n, length = 300, 65456
    slot = (HDR + length + 15 + 63) // 64 * 64
    r = RecvRing(cuda, n, slot, seed=946)
    _sequence(cuda, r, {"rows": _row_group_batch(r, oracle, rng, n, length, kind, mode)}, ["rows"] * 20, kind, mode)


@KINDS
@MODES
@pytest.mark.parametrize("hdr", [(72, 0), (76, 4)], ids=["stride72", "stride76_off4"])
def test_headers_apart(cuda, oracle, hdr, kind, mode):
    """The headers in a tensor of their own (stride 72, and stride 76 from byte 4: 4-byte aligned only); the ring,
    the header tensor and the application buffer are compared in full."""
    import torch

    rng = np.random.default_rng(950 + 3 * kind + mode)
    n, slot = 601, 70016
    r = RecvRing(cuda, n, slot, seed=951 + mode, hdr=hdr)
    lens = rng.integers(0, 65457, size=n).astype(np.uint64)
    lens[rng.choice(n, size=len(EDGE_LENGTHS), replace=False)] = EDGE_LENGTHS
    b = r.batch(oracle, rng, lens, kind, mode, fault_classes(rng, n, (3, 1)))
    r.load(b)
    r.check(r.recv(b["descs"], kind, mode), b)
    assert torch.equal(r.ring, b["ring"]), ("ring", _first_diff(r.ring, b["ring"], slot))
    assert torch.equal(r.hdr_t, b["hdrs"]), ("headers", _first_diff(r.hdr_t, b["hdrs"], hdr[0]))


RING_CASES = {  # name: (frag_len, slot_stride, msg_len, seq_offset0)
    "gm": (65456, 65536, 36 * 65456 + 12345, 0x0000000100000010),
    "ib": (1976, 2048, 1976 * 700 + 55, 0x0000000100000010),
    "small": (256, 328, 256 * 1200 + 100, 0),
    "row": (4096, 4168, 4096 * 300, 0),
    "rows4": (16384, 16456, 16384 * 40, 0),
    "1m": (1 << 20, (1 << 20) + 72, 3 * (1 << 20) + 16400, 0),
    "odd": (1001, 1080, 1001 * 500 + 7, 0x123456789),
    "empty": (1976, 2048, 0, 77),
}


class _Slots:
    """A message packed into a ring of slots on the host, an application buffer prefilled with the stream."""

    def __init__(self, cuda, oracle, case, kind, mode, seed):
        import torch

        dv = _dv()
        self.L, self.stride, self.mlen, self.seq0 = RING_CASES[case]
        self.kind, self.mode, self.cuda, self.oracle = kind, mode, cuda, oracle
        self.n = (self.mlen + self.L - 1) // self.L if self.mlen else 1
        msg = torch.empty(self.mlen + 16, dtype=torch.uint8, device=cuda)
        dv.fill_stream(msg, seed=seed)
        self.m = msg.cpu().numpy()[:self.mlen]
        self.ring = torch.empty(self.n * self.stride, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.ring, seed=seed + 1)
        self.hring0 = self.ring.cpu().numpy()
        self.app = torch.empty(self.mlen + 64, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.app, seed=seed + 2)
        self.app_before = self.app.clone()
        self.happ0 = self.app.cpu().numpy()

    def run(self, rng, what, seq0=None, order=None, app_len=None, edit=None):
        import torch

        seq0 = self.seq0 if seq0 is None else seq0
        hring = self.hring0.copy()
        pack_slots(self.oracle, rng, hring, self.m, self.L, self.stride, seq0, self.kind, self.mode, order)
        if edit is not None:
            edit(hring)
        alen = self.mlen + 64 if app_len is None else app_len
        app = self.happ0.copy()
        want = expect_ring(self.oracle, hring, self.n, self.stride, app, alen, seq0, self.kind, self.mode)
        self.ring.copy_(torch.from_numpy(hring).to(self.cuda))
        self.app.copy_(self.app_before)
        got = _dv().msg_recv_unpack(self.ring, self.n, self.stride, self.app, kind=self.kind, mode=self.mode,
                                    seq_offset0=seq0, app_len=alen)
        check(got, want, self.n, self.app, app, self.L, what)
        return want


@KINDS
@MODES
@pytest.mark.parametrize("case", list(RING_CASES))
def test_ring_form(cuda, oracle, case, kind, mode):
    """Slots packed on the host from the oracle, four ways: permuted (with one bad header and one corrupt payload);
    app_len shorter than the message (one fragment cut, the later ones to the bit bucket, DataOK); a seq_offset0
    that wraps the field; one slot whose dataLength is one more than the slot holds (malformed: dropped, in every
    mode, its valid checksums notwithstanding)."""
    rng = np.random.default_rng(960 + 3 * kind + mode)
    x = _Slots(cuda, oracle, case, kind, mode, seed=961)
    n, L, stride = x.n, x.L, x.stride

    def faults(hring):
        if n < 4:
            return
        flip_bit(hring, 1 * stride, rng, *HDR_FAULTS[2])
        hring[(n - 2) * stride + HDR + 3] ^= np.uint8(0x10)

    want = x.run(rng, "permuted", order=rng.permutation(n), edit=faults)
    if n >= 4 and mode != NONE:
        assert sorted(want[0][[1, n - 2]]) == [-2, -1]
    if x.mlen:
        cut = x.mlen - (x.mlen // 3)
        want = x.run(rng, "short app", app_len=cut)
        assert (want[0] == 0).any() or n < 3
    x.run(rng, "wrapping offset", seq0=2**64 - L - 5)

    def malformed(hring):  # a header otherwise valid: dataLength set before the checksums are computed
        k = n // 2
        h = hring[k * stride:k * stride + HDR].copy()
        h[LEN_AT:LEN_AT + 4] = np.array([stride - 71], "<u4").view(np.uint8)
        if mode != NONE:
            from test_gpu_send_pack import _stamp

            dc, hc = _stamp(oracle, h[:DCSUM], int(np.ascontiguousarray(h[DCSUM:HCSUM]).view("<u4")[0]), False, kind,
                            mode)
            h[DCSUM:HCSUM] = np.array([dc], "<u4").view(np.uint8)
            h[HCSUM:] = np.array([hc], "<u4").view(np.uint8)
        hring[k * stride:k * stride + HDR] = h

    want = x.run(rng, "malformed", edit=malformed)
    assert want[0][n // 2] == -2 and int(want[2].sum()) == 1


@SUMS
@pytest.mark.parametrize("case", ["gm", "ib"])
def test_round_trip(cuda, oracle, case, mode):
    """msg_send_pack -> msg_recv_unpack: the message is delivered and both counts are 0; one flipped payload byte makes
    that slot alone -1 with its bytes still delivered; one flipped header byte makes that slot alone -2 with its
    range of the application buffer left as it was."""
    import torch

    dv = _dv()
    kind, L, stride, mlen, _ = MSG_CASES[case]
    fill = _fill(case)
    x = _Msg(cuda, oracle, MSG_CASES[case], fill, mode)
    x.send()
    n, lens = x.n, x.lens.astype(np.int64)

    def recv():
        app = torch.full((mlen + 32,), 0xA5, dtype=torch.uint8, device=cuda)
        out = dv.msg_recv_unpack(x.ring, n, stride, app, kind=kind, mode=mode, seq_offset0=fill["seq_offset0"],
                                 app_len=mlen)
        torch.cuda.synchronize()
        return app.cpu().numpy(), out[0].cpu().numpy(), dv.mask_bits(out[2], n), dv.mask_bits(out[3], n), \
            [int(v) for v in out[4].cpu().numpy()]

    clean = np.full(mlen + 32, 0xA5, np.uint8)
    clean[:mlen] = x.m
    app, copied, hb, db, nbad = recv()
    assert nbad == [0, 0] and np.array_equal(copied, lens) and np.array_equal(app, clean)
    victim = n // 3
    at = victim * stride + HDR + int(lens[victim]) // 2
    x.ring[at] ^= 0x10
    app, copied, hb, db, nbad = recv()
    want = clean.copy()
    want[victim * L + int(lens[victim]) // 2] ^= 0x10
    wc = lens.copy()
    wc[victim] = -1
    assert nbad == [0, 1] and list(np.nonzero(db)[0]) == [victim] and not hb.any()
    assert np.array_equal(copied, wc) and np.array_equal(app, want)
    x.ring[at] ^= 0x10
    x.ring[victim * stride + 40] ^= 0x04
    app, copied, hb, db, nbad = recv()
    want = clean.copy()
    want[victim * L:victim * L + int(lens[victim])] = 0xA5
    wc[victim] = -2
    assert nbad == [1, 0] and list(np.nonzero(hb)[0]) == [victim] and not db.any()
    assert np.array_equal(copied, wc) and np.array_equal(app, want)


def test_argument_checks(cuda):
    """Every rejection returns nonzero and leaves the sentinel-filled outputs and the application buffer untouched;
    an empty batch zeroes the two counts."""
    import torch

    from lampi_amd import lib

    dv = _dv()
    L = lib()
    ring = torch.zeros(4 * 4096, dtype=torch.uint8, device=cuda)
    app = torch.full((8192,), 0x5A, dtype=torch.uint8, device=cuda)
    descs = dv.make_recv_descs(ring, [HDR, 4096 + HDR], app, [0, 4096], [500, 700], [500, 700])
    outs = [torch.full((4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=cuda) for _ in range(5)]
    c, s, hm, dm, nb = [t.data_ptr() for t in outs]
    d, h, a = descs.data_ptr(), ring.data_ptr(), app.data_ptr()
    f = L.lampi_recv_unpack_batch
    bad = [
        f(d, 2, h, 4096, 2, c, s, hm, dm, nb, CRC, None), f(d, 2, h, 4096, -1, c, s, hm, dm, nb, CRC, None),  # kind
        f(d, 2, h, 4096, GM, c, s, hm, dm, nb, 3, None),                 # a bad mode
        f(d, 2, h, 4096, GM, c, s, hm, dm, nb, CRC | 0x100, None),       # LAMPI_CSUM_BY_BYTES
        f(d, 2, h, 4098, GM, c, s, hm, dm, nb, CRC, None),               # a misaligned stride
        f(d, 2, h + 2, 4096, GM, c, s, hm, dm, nb, CRC, None),           # misaligned headers
        f(d, 2, h, 68, GM, c, s, hm, dm, nb, CRC, None),                 # a stride that cannot hold a header
        f(d, 2, None, 4096, GM, c, s, hm, dm, nb, CRC, None),            # no headers with checksumming on
        f(d, 2, None, 4096, IB, c, s, hm, dm, nb, SUM, None),
        f(None, 2, h, 4096, GM, c, s, hm, dm, nb, CRC, None),            # no descriptors
        f(d, 2, h, 4096, GM, None, s, hm, dm, nb, CRC, None), f(d, 2, h, 4096, GM, c, None, hm, dm, nb, CRC, None),
        f(d, 2, h, 4096, GM, c, s, None, dm, nb, CRC, None), f(d, 2, h, 4096, GM, c, s, hm, None, nb, CRC, None),
        f(d, 2, h, 4096, GM, c, s, hm, dm, None, CRC, None), f(d, 0, h, 4096, GM, c, s, hm, dm, None, CRC, None),
        f(d, 1 << 32, h, 4096, GM, c, s, hm, dm, nb, CRC, None),         # 2^32 fragments
    ]
    g = L.lampi_msg_recv_unpack
    bad += [
        g(h, 2, 4096, 2, a, 8192, 0, c, s, hm, dm, nb, CRC, None), g(h, 2, 4096, GM, a, 8192, 0, c, s, hm, dm, nb, 3, None),
        g(h, 2, 4096, GM, a, 8192, 0, c, s, hm, dm, nb, CRC | 0x100, None),
        g(h, 2, 4092, GM, a, 8192, 0, c, s, hm, dm, nb, CRC, None),      # slot_stride not 8-byte aligned
        g(h + 4, 2, 4096, GM, a, 8192, 0, c, s, hm, dm, nb, CRC, None),  # ring not 8-byte aligned
        g(h, 2, 64, GM, a, 8192, 0, c, s, hm, dm, nb, CRC, None),        # a slot that cannot hold a header
        g(None, 2, 4096, GM, a, 8192, 0, c, s, hm, dm, nb, CRC, None),   # no ring
        g(h, 2, 4096, GM, None, 8192, 0, c, s, hm, dm, nb, CRC, None),   # no application buffer
        g(h, 2, 4096, GM, a, 8192, 0, None, s, hm, dm, nb, CRC, None), g(h, 2, 4096, GM, a, 8192, 0, c, None, hm, dm, nb, CRC, None),
        g(h, 2, 4096, GM, a, 8192, 0, c, s, None, dm, nb, CRC, None), g(h, 2, 4096, GM, a, 8192, 0, c, s, hm, None, nb, CRC, None),
        g(h, 2, 4096, GM, a, 8192, 0, c, s, hm, dm, None, CRC, None),
        g(h, 1 << 32, 4096, GM, a, 8192, 0, c, s, hm, dm, nb, CRC, None),
    ]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    assert all(bool((t == 0x5A5A5A5A5A5A5A5A).all()) for t in outs) and bool((app == 0x5A).all())
    assert f(d, 0, h, 4096, GM, c, s, hm, dm, nb, CRC, None) == 0
    torch.cuda.synchronize()
    assert outs[4].cpu().numpy().view(np.uint32)[:3].tolist() == [0, 0, 0x5A5A5A5A]
    outs[4].fill_(0x5A5A5A5A5A5A5A5A)
    assert g(None, 0, 4096, IB, None, 0, 0, None, None, None, None, nb, SUM, None) == 0
    torch.cuda.synchronize()
    assert outs[4].cpu().numpy().view(np.uint32)[:3].tolist() == [0, 0, 0x5A5A5A5A]
    assert all(bool((t == 0x5A5A5A5A5A5A5A5A).all()) for t in outs[:4]) and bool((app == 0x5A).all())
    with pytest.raises(ValueError):
        dv.recv_unpack_batch(descs, None, 4096, kind=GM, mode=CRC)
    with pytest.raises(ValueError):
        dv.recv_unpack_batch(descs, ring[:4096 + 64], 4096, kind=GM, mode=CRC)
    with pytest.raises(ValueError):
        dv.msg_recv_unpack(ring, 5, 4096, app)
