"""GPU parity of the Quadrics kind of the one-call receive step (lampi_recv_unpack_batch, lampi_msg_recv_unpack with
LAMPI_SEND_HDR_QUADRICS) against tests/quadrics_model.py: verdicts, checksums, masks and counts, and the application
buffer -- prefilled -- compared whole.
"""
import numpy as np
import pytest

import quadrics_model as qm
from quadrics_model import CRC, DATA, DCSUM, ELAN, HCSUM, HDR, INLINE, LEN_AT, NONE, QUADRICS, SEQOFF_AT, SUM
from recv_unpack_model import check, fault_classes, flip_bit

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("mode", [CRC, SUM, NONE], ids=["crc", "sum", "none"])
SUMS = pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
# a bit in bytes [0, 64), in the word @64, in [68, 124) -- dataElanAddr and data[] --, in the word @124
HDR_FAULTS = [(0, DCSUM), (DCSUM, ELAN), (ELAN, HCSUM), (HCSUM, HDR)]


def _dv():
    from lampi_amd import device as dv

    return dv


class QRecvRing:
    """n slots of `slot` bytes -- header i at i*slot (hdr=(stride, offset): in a tensor of their own), a payload of
    more than 52 bytes at i*slot + 128 + i % 16, a shorter one in its header at +72 -- and an application buffer
    with a region of `slot` bytes per fragment, destination i at i*slot + (i + 5) % 16; all prefilled."""

    def __init__(self, cuda, n, seed, hdr=None, room=65536):
        import torch

        dv = _dv()
        self.n, self.slot, self.cuda = n, HDR + room + 16, cuda
        self.ring = torch.empty(n * self.slot, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.ring, seed=seed)
        self.hring0 = self.ring.cpu().numpy()
        self.app = torch.empty(n * self.slot + 64, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.app, seed=seed + 1)
        self.app_before = self.app.clone()
        self.happ0 = self.app.cpu().numpy()
        self.hdr_stride, self.hdr_off, self.hdr_t, self.hhdr0 = self.slot, 0, self.ring, None
        if hdr is not None:
            self.hdr_stride, self.hdr_off = hdr
            self.hdr_t = torch.empty(self.hdr_off + n * self.hdr_stride + 8, dtype=torch.uint8, device=cuda)
            dv.fill_stream(self.hdr_t, seed=seed + 2)
            self.hhdr0 = self.hdr_t.cpu().numpy()
        k = np.arange(n, dtype=np.uint64)
        self.poffs = k * np.uint64(self.slot) + np.uint64(HDR) + k % np.uint64(16)
        self.aoffs = k * np.uint64(self.slot) + (k + np.uint64(5)) % np.uint64(16)
        self.hat = self.hdr_off + np.arange(n, dtype=np.int64) * self.hdr_stride

    def batch(self, oracle, rng, lens, mode, cls, app_lens=None, roomy=(), data_flip=()):
        """Fragments of `lens` bytes with valid headers, then faults by class (cls[i]: 0 clean; 1 header bad -- one
        bit flipped in [0, 64), the word @64, [68, 124) or the word @124 in turn; 2 data bad -- a payload byte
        flipped or, for every other one and for every inline fragment (whose payload the header checksum covers), a
        header re-stamped around a wrong dataChecksum; 3 both).  data_flip: inline fragments given a flipped data[]
        byte inside their payload.  app_lens: default three classes in turn -- <= 0, < length, > length (roomy:
        fragments given > length).  Returns a dict as recv_unpack_model.RecvRing.batch."""
        import torch

        dv = _dv()
        n = self.n
        ln = np.asarray(lens, np.uint64)
        hring = self.hring0.copy()
        apart = self.hhdr0 is not None
        hh = self.hhdr0.copy() if apart else hring
        if app_lens is None:
            k = np.arange(n) % 3
            al = np.where(k == 0, -(np.arange(n) % 7), np.where(k == 1, (ln // 2).astype(np.int64),
                                                               ln.astype(np.int64) + 9)).astype(np.int64)
            al[ln == 0] = np.where(k[ln == 0] == 0, 0, 5)
            al[list(roomy)] = ln[list(roomy)].astype(np.int64) + 9
        else:
            al = np.asarray(app_lens, np.int64)
        cls = np.asarray(cls)
        inline = ln <= INLINE
        # every payload as an offset into one array: the ring, then (when apart) the header tensor
        hbase = len(hring) if apart else 0

        def joined():
            return np.concatenate([hring, hh]) if apart else hring

        poffs = np.where(inline, (hbase + self.hat + DATA).astype(np.uint64), self.poffs)
        wrong = np.zeros(0, np.int64)
        if mode != NONE:
            vals = oracle.desc_batch(joined(), poffs, ln.astype(np.uint32), np.full(n, qm.M32, np.uint32)
                                     if mode == CRC else None, mode)
            data_bad = ((cls == 2) | (cls == 3)) & (ln > 0)
            wrong = np.nonzero(data_bad & (inline | (np.arange(n) % 2 == 1)))[0]
            vals2 = vals.copy()
            vals2[wrong] ^= (np.uint32(1) << rng.integers(0, 32, size=wrong.size).astype(np.uint32))
            idx = self.hat[:, None] + np.arange(HDR)
            H = hh[idx]
            qm.stamp_headers(oracle, H, vals2, mode)
            hh[idx] = H
        nh = 0
        skip = set(int(x) for x in wrong)
        for i in np.nonzero(cls != 0)[0]:
            i = int(i)
            if cls[i] in (1, 3):
                lo, hi = HDR_FAULTS[nh % 4]
                nh += 1
                flip_bit(hh, int(self.hat[i]), rng, lo, hi)
            if cls[i] in (2, 3) and i not in skip and ln[i] > 0:
                hring[int(self.poffs[i]) + int(rng.integers(0, int(ln[i])))] ^= np.uint8(0x10)
        for i in data_flip:
            assert 0 < ln[i] <= INLINE
            hh[int(self.hat[i]) + DATA + int(rng.integers(0, int(ln[i])))] ^= np.uint8(0x04)
        app = self.happ0.copy()
        want = qm.recv_expect(oracle, joined(), poffs, ln, hh[self.hat[:, None] + np.arange(HDR)], np.ones(n, bool),
                              app, self.aoffs, al, mode)
        descs = dv.make_recv_descs(self.ring, self.poffs, self.app, self.aoffs, ln, al)
        return dict(descs=descs, ring=torch.from_numpy(hring).to(self.cuda),
                    hdrs=torch.from_numpy(hh).to(self.cuda) if apart else None, want=want,
                    app=torch.from_numpy(app).to(self.cuda), cls=cls, lens=ln, app_lens=al)

    def load(self, b):
        self.ring.copy_(b["ring"])
        if b["hdrs"] is not None:
            self.hdr_t.copy_(b["hdrs"])
        self.app.copy_(self.app_before)

    def recv(self, descs, mode, **kw):
        return _dv().recv_unpack_batch(descs, self.hdr_t, self.hdr_stride, offset=self.hdr_off, kind=QUADRICS,
                                       mode=mode, **kw)

    def check(self, got, b, what=""):
        check(got, b["want"], self.n, self.app, b["app"], self.slot, what)


@MODES
@pytest.mark.parametrize("hdr", [None, (160, 8)], ids=["in-slot", "hdrs-apart"])
def test_descriptor_form(cuda, oracle, hdr, mode):
    rng = np.random.default_rng(1000 + mode + (10 if hdr else 0))
    n = 601
    r = QRecvRing(cuda, n, seed=1010 + mode, hdr=hdr)
    ln = qm.mixed_lengths(rng, n)
    ln[n - 1] = 3000
    cls = fault_classes(rng, n, (1, 2))
    inl = [int(i) for i in np.nonzero((ln > 0) & (ln <= INLINE) & (np.arange(n) % 3 != 0))[0]]
    flipped = [i for i in inl if cls[i] == 0][:3]
    cls[inl[-1]] = 2  # (an inline fragment with a wrong dataChecksum: DATA_BAD)
    b = r.batch(oracle, rng, ln, mode, cls, roomy=(n - 1, inl[-1]), data_flip=flipped)
    for c in (1, 2, 3):
        assert (cls == c).any()
    al = b["app_lens"]
    for sel in (al <= 0, (al > 0) & (al < ln.astype(np.int64)), al > ln.astype(np.int64)):
        assert sel.any()
    copied, csum, hbad, dbad = b["want"]
    if mode != NONE:
        assert hbad[0] and dbad[n - 1] and hbad.sum() > 40 and dbad.sum() > 10
        assert len(flipped) == 3 and all(copied[i] == -2 and not dbad[i] for i in flipped)
        assert copied[inl[-1]] == -1
    else:
        assert not hbad.any() and not dbad.any()
    r.load(b)
    r.check(r.recv(b["descs"], mode), b)


@MODES
def test_learned_shapes_20_calls(cuda, oracle, mode):
    """Twenty batches of fragments of at most 2 KiB on one descriptor array and stream until the census has landed,
    four of 2,049..65,536 bytes under the stale shape, then the first again."""
    import torch

    rng = np.random.default_rng(1020 + mode)
    n = 601
    r = QRecvRing(cuda, n, seed=1025)
    small = rng.integers(0, 2049, size=n).astype(np.uint64)
    small[:8] = [0, 1, 51, 52, 53, 2047, 2048, 64]
    big = rng.integers(2049, 65537, size=n).astype(np.uint64)
    prepared = {"small": r.batch(oracle, rng, small, mode, fault_classes(rng, n, (1, 2))),
                "big": r.batch(oracle, rng, big, mode, fault_classes(rng, n, (2, 1)))}
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        descs = torch.empty_like(prepared["small"]["descs"])
        for i, key in enumerate(["small"] * 20 + ["big"] * 4 + ["small"] * 4):
            b = prepared[key]
            descs.copy_(b["descs"])
            r.load(b)
            got = r.recv(descs, mode, stream=stream)
            stream.synchronize()
            r.check(got, b, (i, key))


@MODES
def test_row_groups(cuda, oracle, mode):
    """LAMPI_CSUM_ROWS_HINT(16) over 300 fragments of 65,536 bytes with a few short, inline and empty ones among
    them and faults at both ends: the first launch of the row groups zeroes the verdicts, the join gives them."""
    rng = np.random.default_rng(1030 + mode)
    n = 300
    r = QRecvRing(cuda, n, seed=1035)
    ln = np.full(n, 65536, np.uint64)
    ln[[3, 7, 100, 150, 201, 298]] = [52, 0, 4097, 1, 65535, 53]
    b = r.batch(oracle, rng, ln, mode, fault_classes(rng, n, (1, 2)), roomy=(n - 1,))
    r.load(b)
    r.check(r.recv(b["descs"], mode, rows_hint=16), b)


def _slots(oracle, rng, hring, lens, seqoffs, stride, order, mode):
    """Envelope + payload slots written into hring: fragment k (lens[k] random bytes, dataSeqOffset seqoffs[k]) in
    slot order[k], inline when it fits, else at slot + 128; valid words @64 / @124.  Returns the payloads."""
    n = len(lens)
    H = rng.integers(0, 256, size=(n, HDR), dtype=np.uint8)
    H[:, LEN_AT:LEN_AT + 4] = qm.le(lens)
    H[:, SEQOFF_AT:SEQOFF_AT + 8] = np.array([int(x) & qm.M64 for x in seqoffs], "<u8").view(np.uint8).reshape(n, 8)
    pay = [rng.integers(0, 256, size=int(c), dtype=np.uint8) for c in lens]
    for k in range(n):
        if 0 < lens[k] <= INLINE:
            H[k, DATA:DATA + int(lens[k])] = pay[k]
    if mode != NONE:
        flat = np.concatenate(pay + [np.zeros(1, np.uint8)])
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        vals = oracle.desc_batch(flat, offs, np.asarray(lens, np.uint32), np.full(n, qm.M32, np.uint32)
                                 if mode == CRC else None, mode)
        qm.stamp_headers(oracle, H, vals, mode)
    for k in range(n):
        s, c = int(order[k]) * stride, int(lens[k])
        hring[s:s + HDR] = H[k]
        if c > INLINE and s + HDR + c <= s + stride:
            hring[s + HDR:s + HDR + c] = pay[k]
    return pay


@MODES
@pytest.mark.parametrize("stride", [2176, 128], ids=["slots2176", "bare128"])
def test_ring_form(cuda, oracle, stride, mode):
    """Permuted slots, inline and +128 payloads mixed, a ring cut short by app_len, failed headers, corrupt
    payloads, and malformed lengths: 2,049 in a 2,176-byte slot; 53 in a 128-byte slot."""
    import torch

    dv = _dv()
    rng = np.random.default_rng(1040 + mode + stride)
    n, seq0 = 300, (1 << 63) + 77
    room = stride - HDR
    lens = np.where(rng.random(n) < 0.4, rng.integers(0, INLINE + 1, size=n), rng.integers(53, 2049, size=n))
    lens[:6] = [0, 1, 52, 53, 2048, 51]
    lens[30], lens[60] = 1000, 20  # (the corrupt payloads below: one at +128, one inside data[])
    if room == 0:
        lens = np.minimum(lens, INLINE)
    lens = lens.astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    total = int(lens.sum())
    order = rng.permutation(n)
    ring = torch.empty(n * stride, dtype=torch.uint8, device=cuda)
    dv.fill_stream(ring, seed=1041)
    hring = ring.cpu().numpy()
    _slots(oracle, rng, hring, lens, [seq0 + int(o) for o in offs], stride, order, mode)
    bad_len = 2049 if room else 53
    mal = [int(order[7]), int(order[200])]
    for s in mal:  # malformed: valid headers claiming more than the slot holds
        H = hring[s * stride:s * stride + HDR].reshape(1, HDR).copy()
        H[:, LEN_AT:LEN_AT + 4] = qm.le([bad_len])
        qm.stamp_headers(oracle, H, qm.u32(H[:, DCSUM:ELAN]), mode)
        hring[s * stride:s * stride + HDR] = H[0]
    for j, s in enumerate([int(order[0]), int(order[50]), int(order[120]), int(order[n - 1])]):
        flip_bit(hring, s * stride, rng, *HDR_FAULTS[j % 4])
    for k in (30, 60, 90):  # corrupt payloads: a byte at +128, or inside data[] (that one fails the header)
        s, c = int(order[k]) * stride, int(lens[k])
        if c:
            hring[s + (DATA if c <= INLINE else HDR) + c // 2] ^= np.uint8(0x20)
    app = torch.empty(total + 64, dtype=torch.uint8, device=cuda)
    dv.fill_stream(app, seed=1042)
    app_len = total - int(lens[-3:].sum()) - 5  # cut: the last fragments fall off the posted buffer
    want_app = app.cpu().numpy()
    want = qm.ring_recv_expect(oracle, hring, n, stride, want_app, app_len, seq0, mode)
    assert all(want[0][s] == -2 for s in mal)
    if mode != NONE:
        assert want[2].sum() >= 6
        assert room == 0 or want[3].any()
    ring.copy_(torch.from_numpy(hring).to(cuda))
    got = dv.msg_recv_unpack(ring, n, stride, app, kind=QUADRICS, mode=mode, seq_offset0=seq0, app_len=app_len)
    check(got, want, n, app, want_app, 4096)


TMPL = (np.arange(72, dtype=np.uint16) * 5 + 1).astype(np.uint8)


@SUMS
@pytest.mark.parametrize("L,stride", [(52, 184), (2048, 2176)], ids=["inline52", "packed2048"])
def test_round_trip_message(cuda, oracle, L, stride, mode):
    import torch

    dv = _dv()
    mlen = L * 299 + 37
    n = 300
    msg = torch.empty(mlen, dtype=torch.uint8, device=cuda)
    dv.fill_stream(msg, seed=1050)
    ring = torch.empty(n * stride, dtype=torch.uint8, device=cuda)
    dv.fill_stream(ring, seed=1051)
    app = torch.zeros(mlen + 16, dtype=torch.uint8, device=cuda)
    dv.msg_send_pack(msg, L, ring, stride, TMPL, seq_offset0=4096, kind=QUADRICS, mode=mode)
    copied, csum, hmask, dmask, nbad = dv.msg_recv_unpack(ring, n, stride, app, kind=QUADRICS, mode=mode,
                                                          seq_offset0=4096, app_len=mlen)
    torch.cuda.synchronize()
    assert [int(x) for x in nbad.cpu().numpy()] == [0, 0]
    assert np.array_equal(copied.cpu().numpy(), np.minimum(L, mlen - np.arange(n) * L))
    assert torch.equal(app[:mlen], msg) and not bool(app[mlen:].any())
    want = oracle.desc_batch(msg.cpu().numpy(), np.arange(n, dtype=np.uint64) * np.uint64(L),
                             np.minimum(L, mlen - np.arange(n) * L).astype(np.uint32),
                             np.full(n, qm.M32, np.uint32) if mode == CRC else None, mode)
    assert np.array_equal(dv.as_u32(csum), want)


@SUMS
def test_round_trip_checksum_only(cuda, oracle, mode):
    """send_pack_batch of fragments that are not copied (copylen 0: Elan-addressable memory) -- the inline ones are
    -- then recv_unpack_batch with frag = the source address: the receiver finds every payload where the sender
    left it."""
    import torch

    dv = _dv()
    rng = np.random.default_rng(1060 + mode)
    n = 400
    ln = rng.integers(1, 9000, size=n).astype(np.uint64)
    ln[:40] = rng.integers(1, INLINE + 1, size=40).astype(np.uint64)
    ln[40:44] = [53, 2048, 4097, 65536]
    span = 65536 + 16
    src = torch.empty(n * span, dtype=torch.uint8, device=cuda)
    dv.fill_stream(src, seed=1061)
    hdrs = torch.empty(n * 136, dtype=torch.uint8, device=cuda)
    dv.fill_stream(hdrs, seed=1062)
    app = torch.zeros(n * span, dtype=torch.uint8, device=cuda)
    k = np.arange(n, dtype=np.uint64)
    soffs = k * np.uint64(span) + k % np.uint64(16)
    cl = np.where(ln <= INLINE, ln, 0)
    sdescs = dv.make_copy_descs(src, soffs, app, k * np.uint64(span), cl, ln)
    dv.send_pack_batch(sdescs, hdrs, 136, kind=QUADRICS, mode=mode)
    torch.cuda.synchronize()
    assert not bool(app.any())  # nothing was copied outside the headers
    rdescs = dv.make_recv_descs(src, soffs, app, k * np.uint64(span), ln, np.full(n, 1 << 20, np.int64))
    copied, csum, hmask, dmask, nbad = dv.recv_unpack_batch(rdescs, hdrs, 136, kind=QUADRICS, mode=mode)
    torch.cuda.synchronize()
    assert [int(x) for x in nbad.cpu().numpy()] == [0, 0]
    assert np.array_equal(copied.cpu().numpy(), ln.astype(np.int64))
    hs, ha = src.cpu().numpy(), app.cpu().numpy()
    for i in range(n):
        assert np.array_equal(ha[i * span:i * span + int(ln[i])], hs[int(soffs[i]):int(soffs[i]) + int(ln[i])]), i


def test_argument_checks(cuda):
    """Every rejection returns nonzero and leaves sentinel-filled outputs untouched; the value 2 is still no kind."""
    import torch

    from lampi_amd import lib

    dv = _dv()
    L = lib()
    Q = QUADRICS
    src = torch.empty(8192, dtype=torch.uint8, device=cuda)
    dv.fill_stream(src, seed=9)
    ring = torch.full((8 * 4096,), 0x5A, dtype=torch.uint8, device=cuda)
    app = torch.full((8192,), 0x5A, dtype=torch.uint8, device=cuda)
    outs = [torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device=cuda) for _ in range(4)]
    copied = torch.full((8,), 0x5A5A, dtype=torch.int64, device=cuda)
    sd = dv.make_copy_descs(src, [0, 100], ring, [HDR, 4096 + HDR], [500, 40], [500, 40])
    rd = dv.make_recv_descs(ring, [HDR, 4096 + HDR], app, [0, 4096], [500, 40], [600, 600])
    h = ring.data_ptr()
    fill = torch.zeros(112, dtype=torch.uint8).numpy()
    fp = fill.ctypes.data
    send, msend = L.lampi_send_pack_batch, L.lampi_msg_send_pack
    recv, mrecv = L.lampi_recv_unpack_batch, L.lampi_msg_recv_unpack
    o = [copied.data_ptr()] + [t.data_ptr() for t in outs]
    for mode in (CRC, SUM, NONE):
        assert send(sd.data_ptr(), 2, h, 124, Q, mode, None) != 0           # hdr_stride 124
        assert send(sd.data_ptr(), 2, None, 4096, Q, mode, None) != 0       # no headers, in each mode
        assert recv(rd.data_ptr(), 2, h, 124, Q, *o, mode, None) != 0
        assert recv(rd.data_ptr(), 2, None, 4096, Q, *o, mode, None) != 0
        assert msend(src.data_ptr(), 8192, 2048, h, 120, fp, Q, mode, None) != 0   # slot_stride 120
        assert msend(src.data_ptr(), 8192, 2048, h, 136, fp, Q, mode, None) != 0   # neither bare nor roomy
        assert msend(src.data_ptr(), 8192, 40, h, 120, fp, Q, mode, None) != 0
        assert mrecv(h, 4, 120, Q, app.data_ptr(), 8192, 0, *o, mode, None) != 0
        # the value 2 is no kind, on all four entry points
        assert send(sd.data_ptr(), 2, h, 4096, 2, mode, None) != 0
        assert recv(rd.data_ptr(), 2, h, 4096, 2, *o, mode, None) != 0
        assert msend(src.data_ptr(), 8192, 2048, h, 4096, fp, 2, mode, None) != 0
        assert mrecv(h, 4, 4096, 2, app.data_ptr(), 8192, 0, *o, mode, None) != 0
    torch.cuda.synchronize()
    assert bool((ring == 0x5A).all()) and bool((app == 0x5A).all()) and bool((copied == 0x5A5A).all())
    assert all(bool((t == 0x5A5A5A5A).all()) for t in outs)
    # what the checks let through: an envelope-only queue and inline fragments in 128-byte slots
    assert msend(src.data_ptr(), 8192, 2048, h, 128, fp, Q, CRC, None) == 0
    assert msend(src.data_ptr(), 400, 40, h, 128, fp, Q, NONE, None) == 0
    torch.cuda.synchronize()
    assert bool((ring[4 * 128 + 6 * 128:] == 0x5A).all())
    with pytest.raises(ValueError):
        dv.recv_unpack_batch(rd, None, 4096, kind=Q, mode=NONE)
    with pytest.raises(ValueError):
        dv.send_pack_batch(sd, ring[:4096 + 72], 4096, kind=Q, mode=CRC)
    with pytest.raises(ValueError):
        dv.msg_send_pack(src, 2048, ring, 136, TMPL, kind=Q)
