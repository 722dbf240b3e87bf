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


class _Ring:
    """A ring of n slots of `slot` bytes (header + payload room) filled with the synthetic stream -- the word @68
    left as garbage --, a source buffer with one region per slot, and the host copies of both."""

    def __init__(self, cuda, n, slot, seed, span=None):
        import torch

        dv = _dv()
        self.n, self.slot, self.span = n, slot, span or slot
        self.ring = torch.empty(n * slot, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.ring, seed=seed)
        self.before_t = self.ring.clone()
        self.before = self.before_t.cpu().numpy()
        self.src = torch.empty(n * self.span + 64, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.src, seed=seed + 1)
        self.host = self.src.cpu().numpy()

    def batch(self, oracle, rng, lens, kind, mode, ragged=True):
        """Descriptors for payload lengths `lens` (csumlen; a fifth copy fewer bytes when ragged), sources at
        offsets % 16 in 0..15, random registers in CRC mode; returns (descs, the expected ring as a device tensor)."""
        import torch

        dv = _dv()
        n = self.n
        ln = np.asarray(lens, np.uint64)
        cl = ln.copy()
        if ragged:
            cut = rng.random(n) < 0.2
            cl[cut] -= np.minimum(ln[cut], rng.integers(1, 24, size=int(cut.sum())).astype(np.uint64))
        offs = np.arange(n, dtype=np.uint64) * np.uint64(self.span) + (np.arange(n, dtype=np.uint64) + 5) % 16
        doffs = np.arange(n, dtype=np.uint64) * np.uint64(self.slot) + np.uint64(HDR)
        parts = rng.integers(0, 2**32, size=n, dtype=np.uint64)
        descs = dv.make_copy_descs(self.src, offs, self.ring, doffs, cl, ln, parts if mode == CRC else None)
        vals = None
        if mode != NONE:
            vals = oracle.desc_batch(self.host, offs, ln.astype(np.uint32),
                                     parts.astype(np.uint32) if mode == CRC else None, mode)
        want = self.before.copy()
        for i in range(n):
            s = i * self.slot
            a, c = int(offs[i]), int(cl[i])
            want[s + HDR:s + HDR + c] = self.host[a:a + c]
            # (checksumming off: only the copylen bytes count, as MEMCOPY_FUNC; the length is still the fragment's)
            w = _stamp(oracle, want[s:s + DCSUM], 0 if vals is None else vals[i], int(ln[i]) == 0, kind, mode)
            if w is not None:
                want[s + DCSUM:s + DCSUM + 4] = _le(w[0])
                want[s + HCSUM:s + HCSUM + 4] = _le(w[1])
        return descs, torch.from_numpy(want).to(self.ring.device)

    def reset(self):
        self.ring.copy_(self.before_t)


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


@SUMS
def test_learned_schedules(cuda, oracle, mode):
    """IB-sized batches until the census picks the pair kernel (CRC) / a wave per fragment (SUM), then batches of
    2,049-70,000 bytes on the same stream -- the first of them under the stale shape, every wave's fragments left
    to the leftover launch -- then IB again; every call checked byte for byte."""
    import torch

    dv = _dv()
    rng = np.random.default_rng(720 + mode)
    n, slot = 601, 70080  # (72 + 70,000 bytes fit a slot)
    r = _Ring(cuda, n, slot, seed=722)
    prepared = {"ib": r.batch(oracle, rng, _ib_lengths(rng, n, True), IB, mode),
                "big": r.batch(oracle, rng, rng.integers(2049, 70001, size=n), IB, mode)}
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        for i, k in enumerate(["ib"] * 20 + ["big"] * 4 + ["ib"] * 4):
            descs, want = prepared[k]
            r.reset()
            dv.send_pack_batch(descs, r.ring, slot, kind=IB, mode=mode, stream=stream)
            assert torch.equal(r.ring, want), (i, k, _first_diff(r.ring, want, slot))


@SUMS
@pytest.mark.parametrize("n,length,hint", [(300, 65456, 16), (5, (1 << 20) + 3, 0), (5, (1 << 20) + 3, 64)],
                         ids=["gm16", "1m", "1m_hint64"])
def test_row_groups(cuda, oracle, n, length, hint, mode):
    """Row groups (LAMPI_CSUM_ROWS_HINT): the join kernels' emit stamps the headers."""
    import torch

    dv = _dv()
    rng = np.random.default_rng(730 + mode)
    slot = (HDR + length + 63) // 64 * 64
    r = _Ring(cuda, n, slot, seed=731)
    lens = np.full(n, length, np.uint64)
    lens[n // 2] = length - 4097  # one fragment with fewer rows than the hint says
    descs, want = r.batch(oracle, rng, lens, GM, mode, ragged=False)
    dv.send_pack_batch(descs, r.ring, slot, kind=GM, mode=mode, rows_hint=hint)
    torch.cuda.synchronize()
    assert torch.equal(r.ring, want), _first_diff(r.ring, want, slot)


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
    r.before_t = r.ring.clone()
    r.before = r.before_t.cpu().numpy()
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
}
FILL = dict(frag_seq0=0x1122334455667788, frag_seq_step=3, desc_ptr0=0x00007F0012345000, desc_ptr_stride=0x1A8,
            seq_offset0=0x0000000100000010)


def _msg_pack(cuda, oracle, case, mode):
    """Runs msg_send_pack on a fresh ring; returns (ring tensor, expected ring (numpy), message bytes, n, lengths)."""
    import torch

    dv = _dv()
    kind, L, stride, mlen, soff = MSG_CASES[case]
    rng = np.random.default_rng(750 + mode)
    n = (mlen + L - 1) // L if mlen else 1
    buf = torch.empty(mlen + soff + 16, dtype=torch.uint8, device=cuda)
    dv.fill_stream(buf, seed=751)
    msg = buf[soff:soff + mlen]
    m = msg.cpu().numpy()
    ring = torch.empty(n * stride, dtype=torch.uint8, device=cuda)
    dv.fill_stream(ring, seed=752)
    want = ring.cpu().numpy().copy()
    tmpl = rng.integers(0, 256, size=HDR, dtype=np.uint8)
    dv.msg_send_pack(msg, L, ring, stride, tmpl, kind=kind, mode=mode, msg_len=mlen, **FILL)
    lens = np.array([min(L, mlen - k * L) for k in range(n)], np.uint64)
    vals = None
    if mode != NONE:
        vals = oracle.desc_batch(m if mlen else np.zeros(1, np.uint8), np.arange(n, dtype=np.uint64) * np.uint64(L),
                                 lens.astype(np.uint32), np.full(n, 0xFFFFFFFF, np.uint32) if mode == CRC else None,
                                 mode)
    m64 = (1 << 64) - 1
    for k in range(n):
        s, c = k * stride, int(lens[k])
        h = tmpl.copy()
        h[20:24] = _le(c)
        h[32:40] = np.array([(FILL["frag_seq0"] + k * FILL["frag_seq_step"]) & m64], "<u8").view(np.uint8)
        h[48:56] = np.array([(FILL["desc_ptr0"] + k * FILL["desc_ptr_stride"]) & m64], "<u8").view(np.uint8)
        h[56:64] = np.array([(FILL["seq_offset0"] + k * L) & m64], "<u8").view(np.uint8)
        w = _stamp(oracle, h[:DCSUM], 0 if vals is None else vals[k], c == 0, kind, mode)
        if w is None:  # GM with checksumming off: the template's word @64, 0 @68
            h[HCSUM:HCSUM + 4] = 0
        else:
            h[DCSUM:DCSUM + 4] = _le(w[0])
            h[HCSUM:HCSUM + 4] = _le(w[1])
        want[s:s + HDR] = h
        want[s + HDR:s + HDR + c] = m[k * L:k * L + c]
    return ring, want, m, n, lens


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
