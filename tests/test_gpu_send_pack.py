"""GPU parity of the one-call send step (lampi_send_pack_batch, lampi_msg_send_pack).

The reference packs a fragment in one place (gmSendFragDesc::init, ref src/path/gm/sendFrag.cc:143-226;
ibSendFragDesc::pack_buffer / init, ref src/path/ib/sendFrag.cc:119-138, :289-320): the payload is copied into the
NIC buffer with the checksum fused, that value goes into dataChecksum @64 of the 72-byte header, then the 68 header
bytes holding it are checksummed into `checksum` @68:

  GM  CRC / SUM   @64 = v; @68 = BasePath_t::headerChecksum(H, 68, 18), the word @68 taken as 0 (:134)
      off         payload copied, neither word written
  IB  CRC / SUM   @64 = v, 0 for a fragment of length 0 (:306); @68 = uicrc(H, 68) / uicsum(H, 68), not swapped
      off         payload copied, both words 0 (:313)

Everything is compared bit for bit with the oracle (the pinned restatement's uicrc, uicsum, header_checksum): whole
rings, so every byte the calls must not touch is checked too.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HDR, DCSUM, HCSUM, WORDS = 72, 64, 68, 18
GM, IB = 0, 1
CRC, SUM, NONE = 0, 1, 2
KINDS = pytest.mark.parametrize("kind", [GM, IB], ids=["gm", "ib"])
MODES = pytest.mark.parametrize("mode", [CRC, SUM, NONE], ids=["crc", "sum", "none"])
SUMS = pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
# (tests that once ran one kind only keep that kind's ids bare)
GM_FIRST = pytest.mark.parametrize("kind,mode", [(k, m) for k in (GM, IB) for m in (CRC, SUM, NONE)],
                                   ids=["crc", "sum", "none", "ib-crc", "ib-sum", "ib-none"])
IB_FIRST = pytest.mark.parametrize("kind,mode", [(k, m) for k in (IB, GM) for m in (CRC, SUM, NONE)],
                                   ids=["crc", "sum", "none", "gm-crc", "gm-sum", "gm-none"])
EDGE_LENGTHS = [0, 1, 3, 15, 16, 17, 1975, 1976, 2047, 2048, 2049, 4095, 4096, 4097, 65455, 65456]


def _dv():
    from lampi_amd import device as dv

    return dv


def _le(x):
    return np.array([x & 0xFFFFFFFF], "<u4").view(np.uint8)


def _stamp(oracle, head, v, empty, kind, mode):
    """The flavour table: (word @64, word @68) for a header whose first 64 bytes are `head`, or None when neither
    is written."""
    if mode == NONE:
        return (0, 0) if kind == IB else None
    dc = 0 if (kind == IB and empty) else int(v)
    h = np.concatenate([head, _le(dc), np.zeros(4, np.uint8)])
    if kind == GM:
        return dc, oracle.header_checksum(h, HDR - 4, WORDS, mode == CRC)
    return dc, (oracle.uicrc(h, HDR - 4) if mode == CRC else oracle.uicsum(h, HDR - 4)[0])


def _ib_lengths(rng, n, odd):
    """IB-sized fragments (16..2048 bytes, the half-frame edges among them); `odd`: a few fragments the pair
    kernel cannot take at indices the census does not sample (tests/test_gpu_shapes.py)."""
    edge = np.array([16, 17, 31, 32, 33, 1024, 1975, 1976, 2031, 2032, 2047, 2048], np.uint64)
    ln = np.where(rng.random(n) < 0.6, 1976, np.where(rng.random(n) < 0.5, rng.choice(edge, size=n),
                                                      rng.integers(16, 2049, size=n))).astype(np.uint64)
    if odd:
        sampled = set(int(x) for x in np.arange(64) * n // 64)
        free = [i for i in range(n) if i not in sampled]
        pick = rng.choice(free, size=12, replace=False)
        ln[pick] = rng.choice(np.array([0, 5, 15, 2049, 4096, 65456], np.uint64), size=12)
    return ln


def _stamp_all(oracle, heads, vals, empty, kind, mode):
    """_stamp for n headers at once (heads: n x 64 bytes): the words @64 and @68 as two uint32 arrays, or None.
    uicrc / uicsum of the 68 bytes holding the word @64 come from one oracle.desc_batch call -- the flavour table:
    GM swaps the CRC, GM's sum of words 0..16 is uicsum(H, 68) --, and a spread of headers is checked against the
    scalar _stamp (oracle.header_checksum)."""
    n = len(heads)
    if mode == NONE:
        return (np.zeros(n, np.uint32), np.zeros(n, np.uint32)) if kind == IB else None
    dc = np.where(np.asarray(empty, bool) & (kind == IB), 0, np.asarray(vals, np.uint32)).astype(np.uint32)
    h = np.empty((n, HDR - 4), np.uint8)
    h[:, :DCSUM] = heads
    h[:, DCSUM:] = dc.astype("<u4").view(np.uint8).reshape(n, 4)
    hc = oracle.desc_batch(h.reshape(-1), np.arange(n, dtype=np.uint64) * np.uint64(HDR - 4),
                           np.full(n, HDR - 4, np.uint32), None, mode)
    if kind == GM and mode == CRC:
        hc = hc.byteswap()
    for i in sorted(set(int(x) for x in np.arange(32) * n // 32)):
        assert (int(dc[i]), int(hc[i])) == _stamp(oracle, heads[i], vals[i], bool(empty[i]), kind, mode), i
    return dc, hc


def _put_words(buf, at, w):
    """uint32 w[i] stored little-endian at byte at[i] of buf."""
    idx = np.asarray(at, np.int64)[:, None] + np.arange(4)
    buf[idx] = np.asarray(w, np.uint32).astype("<u4").view(np.uint8).reshape(-1, 4)


class _Ring:
    """A ring of n slots of `slot` bytes (header + payload room) filled with the synthetic stream -- the word @68
    left as garbage --, a source buffer with one region of `span` bytes per slot, and the host copies of both.
    hdr=(stride, offset): the headers in a tensor of their own instead, header i at offset + i*stride; pay=True:
    the payloads in a third tensor, fragment i's at i*span + i % 16 (every residue mod 16); the ring is then
    untouched."""

    def __init__(self, cuda, n, slot, seed, span=None, hdr=None, pay=False):
        import torch

        dv = _dv()
        self.n, self.slot, self.span = n, slot, span or slot
        self.ring = torch.empty(n * slot, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.ring, seed=seed)
        self.src = torch.empty(n * self.span + 64, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.src, seed=seed + 1)
        self.host = self.src.cpu().numpy()
        k = np.arange(n, dtype=np.uint64)
        self.hdr_t, self.hdr_stride, self.hdr_off = self.ring, slot, 0
        if hdr is not None:
            self.hdr_stride, self.hdr_off = hdr
            self.hdr_t = torch.empty(self.hdr_off + n * self.hdr_stride + 8, dtype=torch.uint8, device=cuda)
            dv.fill_stream(self.hdr_t, seed=seed + 2)
        self.pay_t, self.doffs, self.room = self.ring, k * np.uint64(slot) + np.uint64(HDR), slot - HDR
        if pay:
            self.pay_t = torch.empty(n * self.span + 16, dtype=torch.uint8, device=cuda)
            dv.fill_stream(self.pay_t, seed=seed + 3)
            self.doffs, self.room = k * np.uint64(self.span) + k % np.uint64(16), self.span - 15
        self.tensors = [self.ring] + ([self.hdr_t] if hdr is not None else []) + ([self.pay_t] if pay else [])
        self.before_ts = [t.clone() for t in self.tensors]

    @property
    def before_t(self):
        return self.before_ts[0]

    def rebase(self):
        """The tensors as they are now become what reset() restores and what batch() models."""
        self.before_ts = [t.clone() for t in self.tensors]

    def batch(self, oracle, rng, lens, kind, mode, ragged=True, copylens=None):
        """Descriptors of csumlen `lens` and copylen `copylens` (default: csumlen, a fifth fewer bytes when ragged),
        sources at offsets % 16 in 0..15, random registers in CRC mode.  The model: copylen bytes copied, the
        checksum over max(copylen, csumlen) source bytes, a fragment empty when that max is 0; with checksumming off
        only the copylen bytes count (MEMCOPY_FUNC).  Returns (descs, the expected ring as a device tensor -- with
        headers or payloads apart the list of expected tensors, self.tensors' order)."""
        dv = _dv()
        n = self.n
        ln = np.asarray(lens, np.uint64)
        cl = ln.copy() if copylens is None else np.asarray(copylens, np.uint64)
        if ragged and copylens is None:
            cut = rng.random(n) < 0.2
            cl[cut] -= np.minimum(ln[cut], rng.integers(1, 24, size=int(cut.sum())).astype(np.uint64))
        mx = np.maximum(cl, ln)
        assert int(mx.max()) + 15 <= self.span and int(cl.max()) <= self.room
        offs = np.arange(n, dtype=np.uint64) * np.uint64(self.span) + (np.arange(n, dtype=np.uint64) + 5) % 16
        parts = rng.integers(0, 2**32, size=n, dtype=np.uint64)
        descs = dv.make_copy_descs(self.src, offs, self.pay_t, self.doffs, cl, ln, parts if mode == CRC else None)
        self.last = (offs, cl, ln, parts)
        return descs, self.expected(oracle, kind, mode)

    def refill(self, seed):
        """New source bytes in place (the descriptors made so far still point at them)."""
        _dv().fill_stream(self.src, seed=seed)
        self.host = self.src.cpu().numpy()

    def expected(self, oracle, kind, mode):
        """The model's tensors for the last batch() made, over the source bytes as they are now."""
        import torch

        offs, cl, ln, parts = self.last
        n, mx = self.n, np.maximum(cl, ln)
        vals = np.zeros(n, np.uint32)
        if mode != NONE:
            vals = oracle.desc_batch(self.host, offs, mx.astype(np.uint32),
                                     parts.astype(np.uint32) if mode == CRC else None, mode)
        want = [t.cpu().numpy() for t in self.before_ts]
        wh = want[1 if self.hdr_t is not self.ring else 0]
        wp = want[-1] if self.pay_t is not self.ring else want[0]
        for i in range(n):
            a, c, t = int(offs[i]), int(cl[i]), int(self.doffs[i])
            wp[t:t + c] = self.host[a:a + c]
        at = self.hdr_off + np.arange(n, dtype=np.int64) * self.hdr_stride
        w = _stamp_all(oracle, wh[at[:, None] + np.arange(DCSUM)], vals, mx == 0, kind, mode)
        if w is not None:
            _put_words(wh, at + DCSUM, w[0])
            _put_words(wh, at + HCSUM, w[1])
        want = [torch.from_numpy(x).to(self.ring.device) for x in want]
        return want[0] if len(want) == 1 else want

    def send(self, descs, kind, mode, hdrs=True, **kw):
        """send_pack_batch on this ring's headers (hdrs=False: none passed, GM with checksumming off)."""
        return _dv().send_pack_batch(descs, self.hdr_t if hdrs else None, self.hdr_stride, offset=self.hdr_off,
                                     kind=kind, mode=mode, **kw)

    def reset(self):
        for t, b in zip(self.tensors, self.before_ts):
            t.copy_(b)


def _first_diff(got_t, want_t, slot):
    d = (got_t != want_t).nonzero()
    if d.numel() == 0:
        return None
    i = int(d[0].item())
    return i // slot, i % slot, int(d.numel())


@KINDS
@MODES
def test_descriptor_form_ring_byte_for_byte(cuda, oracle, kind, mode):
    import torch

    dv = _dv()
    rng = np.random.default_rng(700 + 3 * kind + mode)
    n, slot = 601, 70016
    r = _Ring(cuda, n, slot, seed=710 + mode)
    lens = rng.integers(0, 65457, size=n).astype(np.uint64)
    pos = rng.choice(n, size=len(EDGE_LENGTHS), replace=False)
    lens[pos] = EDGE_LENGTHS
    lens[:3] = [0, 65456, 1976]  # (an empty first fragment: IB's zero dataChecksum)
    descs, want = r.batch(oracle, rng, lens, kind, mode)
    dv.send_pack_batch(descs, r.ring, slot, kind=kind, mode=mode)
    torch.cuda.synchronize()
    assert np.array_equal(r.ring.cpu().numpy(), want.cpu().numpy()), _first_diff(r.ring, want, slot)


def _learned_sequence(cuda, r, prepared, order, kind, mode):
    """The batches of `order` through one descriptor array on a stream of its own -- the learned shape is kept per
    (stream, descriptor array), so a batch of another shape written over the array runs under the stale one until
    the next census (every 16th call) --, every call checked byte for byte."""
    import torch

    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        descs = torch.empty_like(prepared[order[0]][0])
        for i, k in enumerate(order):
            batch, want = prepared[k]
            descs.copy_(batch)
            r.reset()
            r.send(descs, kind, mode, stream=stream)
            assert torch.equal(r.ring, want), (i, k, _first_diff(r.ring, want, r.slot))


@IB_FIRST
def test_learned_schedules(cuda, oracle, kind, mode):
    """IB-sized batches until the census picks the pair kernel (CRC: the pair copy into pooled values, then
    send_stamp_kernel<false>) / a wave per fragment (SUM: SendSource, off: SendCopyOnlySource on
    sum_copy_waves_kernel, kShapeSendPackNone), then batches of 2,049-70,000 bytes in the same descriptor array
    on the same stream -- all four under the stale shape, every wave's fragments left to the leftover launch --
    then IB again; every call checked byte for byte."""
    rng = np.random.default_rng(720 + mode)
    n, slot = 601, 70080  # (72 + 70,000 bytes fit a slot)
    r = _Ring(cuda, n, slot, seed=722)
    prepared = {"ib": r.batch(oracle, rng, _ib_lengths(rng, n, True), kind, mode),
                "big": r.batch(oracle, rng, rng.integers(2049, 70001, size=n), kind, mode)}
    _learned_sequence(cuda, r, prepared, ["ib"] * 20 + ["big"] * 4 + ["ib"] * 4, kind, mode)


@KINDS
@MODES
def test_learned_row_groups(cuda, oracle, kind, mode):
    """Equal 65,456-byte batches with no hint until the census learns 16 rows (CRC: launch_crc_light_frag_copy of
    CopySource with row groups, then send_stamp_kernel<false>; SUM / off: GroupSource<SendSource> /
    GroupSource<SendCopyOnlySource> and sum_group_join_kernel's emit, out == nullptr), then the same batch with
    twelve fragments the census does not sample made 0-4,097 bytes -- four calls under the stale shape -- then
    the first batch again."""
    rng = np.random.default_rng(725 + mode)
    n, length = 300, 65456
    slot = (HDR + length + 63) // 64 * 64
    r = _Ring(cuda, n, slot, seed=726)
    lens = np.full(n, length, np.uint64)
    odd = lens.copy()
    sampled = set(int(x) for x in np.arange(64) * n // 64)
    pick = rng.choice([i for i in range(n) if i not in sampled], size=12, replace=False)
    odd[pick] = np.tile(np.array([0, 5, 15, 1976, 4096, 4097], np.uint64), 2)
    prepared = {"rows": r.batch(oracle, rng, lens, kind, mode), "odd": r.batch(oracle, rng, odd, kind, mode)}
    _learned_sequence(cuda, r, prepared, ["rows"] * 20 + ["odd"] * 4 + ["rows"] * 4, kind, mode)


@GM_FIRST
@pytest.mark.parametrize("n,length,hint", [(300, 65456, 16), (5, (1 << 20) + 3, 0), (5, (1 << 20) + 3, 64),
                                           (40, 12000, 3)], ids=["gm16", "1m", "1m_hint64", "12k_hint3"])
def test_row_groups(cuda, oracle, n, length, hint, kind, mode):
    """Row groups (LAMPI_CSUM_ROWS_HINT).  CRC: launch_crc_light_frag_copy of CopySource into pooled values, then
    send_stamp_kernel<false> (its own test for an empty fragment); SUM: GroupSource<SendSource> and
    sum_group_join_kernel, whose emit stamps through get_join and the lazy prefix; off: GroupSource<
    SendCopyOnlySource> and the join with out == nullptr (IB's two zeros; GM writes no header, with the ring passed
    and with none).  Each batch has a fragment with fewer rows than the hint says, one of length 0, one of
    length 1, and copies cut short inside a row group."""
    import torch

    rng = np.random.default_rng(730 + mode)
    slot = (HDR + length + 63) // 64 * 64
    r = _Ring(cuda, n, slot, seed=731)
    lens = np.full(n, length, np.uint64)
    lens[n // 2] = length - 4097  # one fragment with fewer rows than the hint says
    lens[1] = 0
    lens[n - 2] = 1
    descs, want = r.batch(oracle, rng, lens, kind, mode, ragged=True)
    for hdrs in [True, False] if (kind, mode) == (GM, NONE) else [True]:
        r.reset()
        r.send(descs, kind, mode, hdrs=hdrs, rows_hint=hint)
        torch.cuda.synchronize()
        assert torch.equal(r.ring, want), (hdrs, _first_diff(r.ring, want, slot))


def _four_way_lengths(rng, n):
    """(copylens, csumlens) of 0..65,456 bytes with EDGE_LENGTHS planted, descriptor i of class i % 4:
    copylen < csumlen; copylen > csumlen (every third of these csumlen == 0); copylen == 0 < csumlen; both 0."""
    a = rng.integers(0, 65457, size=n).astype(np.uint64)
    a[rng.choice(n, size=len(EDGE_LENGTHS), replace=False)] = EDGE_LENGTHS
    a = np.maximum(a, 1)  # the longer of the two
    less = np.minimum((a * rng.random(n)).astype(np.uint64), a - 1)  # the shorter: 0 .. a - 1,
    near = rng.random(n) < 0.3
    less[near] = a[near] - np.minimum(a[near], rng.integers(1, 24, size=int(near.sum())).astype(np.uint64))  # or just under
    k = np.arange(n) % 4
    cl = np.where(k == 0, less, np.where(k == 1, a, 0)).astype(np.uint64)
    sl = np.where(k == 1, less, np.where(k == 3, 0, a)).astype(np.uint64)
    sl[(k == 1) & (np.arange(n) % 3 == 0)] = 0
    return cl, sl


@KINDS
@MODES
def test_copy_and_checksum_lengths(cuda, oracle, kind, mode):
    """bcopy semantics per descriptor: copylen bytes copied (none for copylen == 0: the destination untouched), the
    checksum over max(copylen, csumlen), IB's empty rule on that max -- csumlen == 0 < copylen is not empty."""
    import torch

    rng = np.random.default_rng(760 + 3 * kind + mode)
    n, slot = 601, 70016
    r = _Ring(cuda, n, slot, seed=761 + mode)
    cl, sl = _four_way_lengths(rng, n)
    k = np.arange(n)
    assert (cl[k % 4 == 0] < sl[k % 4 == 0]).all() and (cl[k % 4 == 1] > sl[k % 4 == 1]).all()
    assert (sl[k % 4 == 1] == 0).any() and (sl[k % 4 == 1] > 0).any()
    assert (cl[k % 4 == 2] == 0).all() and (sl[k % 4 == 2] > 0).all() and not (cl[k % 4 == 3] | sl[k % 4 == 3]).any()
    descs, want = r.batch(oracle, rng, sl, kind, mode, copylens=cl)
    r.send(descs, kind, mode)
    torch.cuda.synchronize()
    assert torch.equal(r.ring, want), _first_diff(r.ring, want, slot)


@KINDS
@MODES
@pytest.mark.parametrize("hdr", [(72, 0), (76, 4)], ids=["stride72", "stride76_off4"])
def test_headers_apart_and_odd_destinations(cuda, oracle, hdr, kind, mode):
    """Headers packed in a tensor of their own (stride 72, and stride 76 from byte 4: 4-byte aligned only, the gap
    bytes compared too), payload destinations in a third tensor at every residue mod 16; the ring itself, the header
    tensor and the payload tensor are compared in full."""
    import torch

    rng = np.random.default_rng(770 + 3 * kind + mode)
    n, slot = 601, 70016
    r = _Ring(cuda, n, slot, seed=771 + mode, hdr=hdr, pay=True)
    lens = rng.integers(0, 65457, size=n).astype(np.uint64)
    pos = rng.choice(n, size=len(EDGE_LENGTHS), replace=False)
    lens[pos] = EDGE_LENGTHS
    lens[:3] = [0, 65456, 1976]
    descs, want = r.batch(oracle, rng, lens, kind, mode)
    r.send(descs, kind, mode)
    torch.cuda.synchronize()
    for name, got, exp, unit in zip(["ring", "headers", "payloads"], r.tensors, want, [slot, hdr[0], slot]):
        assert torch.equal(got, exp), (name, _first_diff(got, exp, unit))


@SUMS
def test_equals_the_two_call_sequence(cuda, oracle, mode):
    """A GM ring (checksum word zeroed, a fresh header) packed by frag_bcopy_batch_strided + header_csum_batch_strided
    and by send_pack_batch: identical rings."""
    import torch

    dv = _dv()
    rng = np.random.default_rng(740 + mode)
    n, slot = 601, 70016
    r = _Ring(cuda, n, slot, seed=741)
    r.ring.view(n, slot)[:, HCSUM:HCSUM + 4] = 0
    r.rebase()
    lens = rng.integers(0, 65457, size=n).astype(np.uint64)
    lens[:len(EDGE_LENGTHS)] = EDGE_LENGTHS
    descs, want = r.batch(oracle, rng, lens, GM, mode)
    dv.frag_bcopy_batch_strided(descs, r.ring, slot, offset=DCSUM, mode=mode)
    dv.header_csum_batch_strided(r.ring, n, slot, HDR - 4, WORDS, r.ring, slot, offset=HCSUM, mode=mode)
    two = r.ring.clone()
    r.reset()
    dv.send_pack_batch(descs, r.ring, slot, kind=GM, mode=mode)
    torch.cuda.synchronize()
    assert torch.equal(r.ring, two), _first_diff(r.ring, two, slot)
    assert torch.equal(r.ring, want), _first_diff(r.ring, want, slot)


MSG_CASES = {  # name: (kind, frag_len, slot_stride, msg_len, source offset)
    "gm": (GM, 65456, 65536, 36 * 65456 + 12345, 3),
    "ib": (IB, 1976, 2048, 1976 * 700 + 55, 0),
    "small": (IB, 256, 328, 4096 * 300 + 100, 0),
    "empty_gm": (GM, 65456, 65536, 0, 0),
    "empty_ib": (IB, 1976, 2048, 0, 0),
    # the launcher each reaches, read from launch_msg_bcopy (checksumming off runs the SUM schedule):
    # CRC crc_light_copy_kernel, R = 16, and crc_light_join_kernel a thread per fragment; SUM the memset of the
    # pooled values and sum_copy_row_kernel's atomic row sums
    "gm_aligned": (GM, 65456, 65536, 40 * 65456, 0),
    # ... the rows past a short last fragment (4,112 bytes) empty
    "gm_aligned_short_last": (GM, 65456, 65536, 40 * 65456 + 4096 + 16, 0),
    # R == 1: CRC crc_light_copy_kernel straight into the values, no join; SUM sum_copy_row_kernel, no memset
    "row": (IB, 4096, 4168, 4096 * 300, 0),
    # CRC R = 4, the join's thread-per-fragment branch; SUM launch_sum_copy_groups(MsgCopySource), W = 4, G = 4
    "rows4": (GM, 16384, 16456, 16384 * 40, 0),
    # CRC R = 40 > kJoinThreadRows, a wave per fragment in the join; SUM W = 40, G = 64; a short last fragment
    "rows40": (GM, 163840, 163912, 163840 * 6 + 8192 + 16, 0),
    # CRC R = 256 in the join's wave branch; SUM W = 256, G = 64
    "1m": (GM, 1 << 20, (1 << 20) + 72, 3 * (1 << 20) + 16400, 0),
    # sum_row4k_copy_kernel<4> (CRC: then launch_crc_msg's packed rows), the 40-byte tail through the recursion: CRC
    # launch_crc_light_frag_copy(MsgCopySource), SUM a workgroup per fragment
    "pow2_64": (IB, 64, 136, 4096 * 256 + 40, 0),
    # sum_row4k_copy_kernel<64>, a tail of four fragments
    "pow2_1k": (IB, 1024, 1096, 4096 * 256 + 3 * 1024 + 5, 0),
    # an odd frag_len from an odd address: CRC launch_crc_light_frag_copy(MsgCopySource), SUM a workgroup per fragment
    "odd": (IB, 1001, 1080, 1001 * 500 + 7, 1),
    # a message shorter than one fragment: CRC launch_crc_light_frag_copy, SUM MsgRowCopySource's row items
    "short_only": (GM, 65456, 65536, 100, 0),
}
FILL = dict(frag_seq0=0x1122334455667788, frag_seq_step=3, desc_ptr0=0x00007F0012345000, desc_ptr_stride=0x1A8,
            seq_offset0=0x0000000100000010)
OLD_CASES = ["gm", "ib", "small", "empty_gm", "empty_ib"]


def _fill(case):
    """The header fields' start values: the later cases wrap all three 64-bit fields within the first fragments."""
    if case in OLD_CASES:
        return FILL
    return dict(frag_seq0=2**64 - 2, frag_seq_step=3, desc_ptr0=2**64 - 0x100, desc_ptr_stride=0x1A8,
                seq_offset0=2**64 - MSG_CASES[case][1] - 5)


def _msg_want(oracle, want, m, kind, L, stride, mlen, tmpl, fill, mode):
    """The model of msg_send_pack written into `want` (the ring before the call, numpy); returns (n, lengths)."""
    n = (mlen + L - 1) // L if mlen else 1
    k = np.arange(n, dtype=np.uint64)
    lens = np.minimum(L, mlen - np.arange(n, dtype=np.int64) * L).astype(np.uint64)
    vals = np.zeros(n, np.uint32)
    if mode != NONE:
        vals = oracle.desc_batch(m if mlen else np.zeros(1, np.uint8), k * np.uint64(L), lens.astype(np.uint32),
                                 np.full(n, 0xFFFFFFFF, np.uint32) if mode == CRC else None, mode)
    m64 = (1 << 64) - 1
    h = np.tile(np.asarray(tmpl, np.uint8), (n, 1))
    h[:, 20:24] = lens.astype("<u4").view(np.uint8).reshape(n, 4)
    for at, x0, step in [(32, fill["frag_seq0"], fill["frag_seq_step"]),
                         (48, fill["desc_ptr0"], fill["desc_ptr_stride"]), (56, fill["seq_offset0"], L)]:
        h[:, at:at + 8] = np.array([(x0 + i * step) & m64 for i in range(n)], "<u8").view(np.uint8).reshape(n, 8)
    w = _stamp_all(oracle, h[:, :DCSUM], vals, lens == 0, kind, mode)
    if w is None:  # GM with checksumming off: the template's word @64, 0 @68
        h[:, HCSUM:] = 0
    else:
        h[:, DCSUM:HCSUM] = w[0].astype("<u4").view(np.uint8).reshape(n, 4)
        h[:, HCSUM:] = w[1].astype("<u4").view(np.uint8).reshape(n, 4)
    for i in range(n):
        s, c = i * stride, int(lens[i])
        want[s:s + HDR] = h[i]
        want[s + HDR:s + HDR + c] = m[i * L:i * L + c]
    return n, lens


class _Msg:
    """A message of `shape` (a MSG_CASES tuple), its ring before the call and the expected ring (numpy)."""

    def __init__(self, cuda, oracle, shape, fill, mode, seed=751):
        import torch

        dv = _dv()
        self.kind, self.L, self.stride, self.mlen, soff = shape
        self.fill, self.mode = fill, mode
        rng = np.random.default_rng(seed - 1 + mode)
        n = (self.mlen + self.L - 1) // self.L if self.mlen else 1
        buf = torch.empty(self.mlen + soff + 16, dtype=torch.uint8, device=cuda)
        dv.fill_stream(buf, seed=seed)
        self.msg = buf[soff:soff + self.mlen]
        self.ring = torch.empty(n * self.stride, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.ring, seed=seed + 1)
        self.before_t = self.ring.clone()
        self.tmpl = rng.integers(0, 256, size=HDR, dtype=np.uint8)
        self.buf = buf
        self.model(oracle)

    def model(self, oracle):
        self.m = self.msg.cpu().numpy()
        self.want = self.before_t.cpu().numpy().copy()
        self.n, self.lens = _msg_want(oracle, self.want, self.m, self.kind, self.L, self.stride, self.mlen, self.tmpl,
                                      self.fill, self.mode)

    def refill(self, oracle, seed):
        """New message bytes in place, and the model over them."""
        _dv().fill_stream(self.buf, seed=seed)
        self.model(oracle)

    def send(self, stream=None):
        _dv().msg_send_pack(self.msg, self.L, self.ring, self.stride, self.tmpl, kind=self.kind, mode=self.mode,
                            msg_len=self.mlen, stream=stream, **self.fill)

    def reset(self):
        self.ring.copy_(self.before_t)


def _msg_pack(cuda, oracle, case, mode):
    """Runs msg_send_pack on a fresh ring; returns (ring tensor, expected ring (numpy), message bytes, n, lengths)."""
    x = _Msg(cuda, oracle, MSG_CASES[case], _fill(case), mode)
    x.send()
    return x.ring, x.want, x.m, x.n, x.lens


@MODES
@pytest.mark.parametrize("case", list(MSG_CASES))
def test_message_form(cuda, oracle, case, mode):
    """The whole header built on the device field by field, every payload byte, and every byte between a
    payload's end and the next slot unchanged."""
    ring, want, _, n, _ = _msg_pack(cuda, oracle, case, mode)
    got = ring.cpu().numpy()
    stride = MSG_CASES[case][2]
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        pytest.fail(f"slot {i // stride} of {n}, byte {i % stride}: {got[i]} != {want[i]}")


@SUMS
@pytest.mark.parametrize("case", ["gm", "ib"])
def test_round_trip(cuda, oracle, case, mode):
    """What the send step packed passes the receive step: the receiver's header test, CopyToApp against the ring's
    own dataChecksum words, the delivered bytes; one flipped payload byte is reported for its slot alone."""
    import torch

    dv = _dv()
    kind, L, stride, mlen, _ = MSG_CASES[case]
    ring, want, m, n, lens = _msg_pack(cuda, oracle, case, mode)
    assert np.array_equal(ring.cpu().numpy(), want)
    if kind == GM:
        mask, nbad = dv.header_check_batch(ring, n, stride, HDR, WORDS, HCSUM, mode=mode)
    else:
        mask, nbad = dv.header_compare_batch(ring, n, stride, HDR - 4, HCSUM, mode=mode)
    assert int(nbad.item()) == 0
    app = torch.zeros(mlen, dtype=torch.uint8, device=cuda)
    k = np.arange(n, dtype=np.uint64)
    descs = dv.make_recv_descs(ring, k * np.uint64(stride) + np.uint64(HDR), app, k * np.uint64(L), lens,
                               lens.astype(np.int64))
    copied, _, mask, nbad = dv.copy_to_app_batch(descs, ring, expected_stride=stride, expected_offset=DCSUM, mode=mode)
    assert int(nbad.item()) == 0
    assert np.array_equal(copied.cpu().numpy(), lens.astype(np.int64))
    assert np.array_equal(app.cpu().numpy(), m)
    victim = n // 3
    ring[victim * stride + HDR + int(lens[victim]) // 2] ^= 0x10
    copied, _, mask, nbad = dv.copy_to_app_batch(descs, ring, expected_stride=stride, expected_offset=DCSUM, mode=mode)
    bad = dv.mask_bits(mask, n)
    assert int(nbad.item()) == 1 and list(np.nonzero(bad)[0]) == [victim]
    assert int(copied[victim].item()) == -1


def test_argument_checks(cuda):
    """Every rejection returns nonzero and writes nothing; n == 0 is a no-op; GM with checksumming off takes no
    headers."""
    import torch

    from lampi_amd import lib

    dv = _dv()
    L = lib()
    src = torch.empty(4096, dtype=torch.uint8, device=cuda)
    dv.fill_stream(src, seed=9)
    ring = torch.full((4 * 4096,), 0x5A, dtype=torch.uint8, device=cuda)
    descs = dv.make_copy_descs(src, [0, 100], ring, [HDR, 4096 + HDR], [500, 700], [500, 700])
    d, h = descs.data_ptr(), ring.data_ptr()
    f = L.lampi_send_pack_batch
    assert f(d, 2, h, 4096, 2, CRC, None) != 0          # a bad kind
    assert f(d, 2, h, 4096, -1, CRC, None) != 0
    assert f(d, 2, h, 4096, GM, 3, None) != 0           # a bad mode
    assert f(d, 2, h, 4096, GM, 0x100, None) != 0       # (BY_BYTES is not a send mode)
    assert f(d, 2, h, 4098, GM, CRC, None) != 0         # a misaligned stride
    assert f(d, 2, h + 2, 4096, GM, CRC, None) != 0     # misaligned headers
    assert f(d, 2, h, 68, GM, CRC, None) != 0           # a stride that cannot hold a header
    assert f(d, 2, None, 4096, GM, CRC, None) != 0      # no headers
    assert f(d, 2, None, 4096, GM, SUM, None) != 0
    assert f(d, 2, None, 4096, IB, NONE, None) != 0     # (IB writes zeros with checksumming off)
    assert f(None, 2, h, 4096, GM, CRC, None) != 0      # no descriptors
    assert f(d, 1 << 32, h, 4096, GM, CRC, None) != 0   # more than 2^32 - 1 fragments
    assert f(d, 0, h, 4096, GM, CRC, None) == 0         # an empty batch
    assert f(None, 0, None, 4096, IB, SUM, None) == 0
    torch.cuda.synchronize()
    assert bool((ring == 0x5A).all())
    fill = torch.zeros(112, dtype=torch.uint8).numpy()
    g = L.lampi_msg_send_pack
    s, fp = src.data_ptr(), fill.ctypes.data
    assert g(s, 1000, 0, h, 4096, fp, GM, CRC, None) != 0        # frag_len 0
    assert g(s, 1000, 500, h, 568, fp, GM, CRC, None) != 0       # slot_stride < 72 + frag_len
    assert g(s, 1000, 500, h, 4092, fp, GM, CRC, None) != 0      # slot_stride not 8-byte aligned
    assert g(s, 1000, 500, h + 4, 4096, fp, GM, CRC, None) != 0  # ring not 8-byte aligned
    assert g(s, 1000, 500, h, 4096, None, GM, CRC, None) != 0    # no fill
    assert g(s, 1000, 500, h, 4096, fp, 2, CRC, None) != 0
    assert g(s, 1000, 500, h, 4096, fp, GM, 3, None) != 0
    assert g(None, 1000, 500, h, 4096, fp, GM, CRC, None) != 0
    torch.cuda.synchronize()
    assert bool((ring == 0x5A).all())
    # GM with checksumming off: the copies alone, no header pointer needed
    assert f(d, 2, None, 4096, GM, NONE, None) == 0
    torch.cuda.synchronize()
    want = np.full(ring.numel(), 0x5A, np.uint8)
    hs = src.cpu().numpy()
    want[HDR:HDR + 500] = hs[:500]
    want[4096 + HDR:4096 + HDR + 700] = hs[100:800]
    assert np.array_equal(ring.cpu().numpy(), want)
    with pytest.raises(ValueError):
        dv.send_pack_batch(descs, None, 4096, kind=IB, mode=NONE)
    with pytest.raises(ValueError):
        dv.send_pack_batch(descs, ring[:4096 + 64], 4096, kind=GM, mode=CRC)
    with pytest.raises(ValueError):
        dv.msg_send_pack(src, 500, ring[:4096], 4096, np.zeros(HDR, np.uint8))
