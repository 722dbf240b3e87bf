"""CPU: the Quadrics model (tests/quadrics_model.py) agrees with itself and, where oracle/_ref is built, with the
compiled reference: a header packed by the send model passes the receive model's test, one flipped bit anywhere in
it fails, and the dataChecksum / header checksum values equal the reference's own uicrc / uicsum / bcopy_* results.
"""
import numpy as np
import pytest

import quadrics_model as qm
from quadrics_model import CRC, DATA, DCSUM, ELAN, HCSUM, HDR, INLINE, NONE, SUM

LENGTHS = [0, 1, 51, 52, 53, 2048]
SUMS = pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
REGIONS = [(0, DCSUM), (DCSUM, ELAN), (ELAN, HCSUM), (HCSUM, HDR)]


def _pack(oracle, rng, mode, copy):
    """One fragment per length (copied, or checksum-only), random headers; returns (headers n x 128 before, after,
    src, soffs, dst before, after, doffs, parts, vals)."""
    n = len(LENGTHS)
    ln = np.array(LENGTHS, np.uint64)
    cl = ln.copy() if copy else np.zeros(n, np.uint64)
    src = rng.integers(0, 256, size=n * 2064, dtype=np.uint8)
    soffs = np.arange(n, dtype=np.uint64) * np.uint64(2064) + np.arange(n, dtype=np.uint64) % 16
    parts = rng.integers(0, 2**32, size=n, dtype=np.uint64)
    hdrs0 = rng.integers(0, 256, size=n * HDR, dtype=np.uint8)
    dst0 = rng.integers(0, 256, size=n * 2064, dtype=np.uint8)
    hdrs, dst = hdrs0.copy(), dst0.copy()
    hat = np.arange(n, dtype=np.int64) * HDR
    doffs = np.arange(n, dtype=np.uint64) * np.uint64(2064) + np.uint64(3)
    vals = qm.send_expect(oracle, src, soffs, cl, ln, parts, hdrs, hat, dst, doffs, mode)
    return hdrs0.reshape(n, HDR), hdrs.reshape(n, HDR), src, soffs, dst0, dst, doffs, parts, vals, cl, ln


@SUMS
@pytest.mark.parametrize("copy", [True, False], ids=["copied", "csum-only"])
def test_packed_header_passes_and_any_flipped_bit_fails(oracle, mode, copy):
    rng = np.random.default_rng(31 + mode + 2 * copy)
    H0, H, src, soffs, dst0, dst, doffs, parts, vals, cl, ln = _pack(oracle, rng, mode, copy)
    assert qm.header_ok(oracle, H, mode).all()
    for i, L in enumerate(LENGTHS):
        a, c = int(soffs[i]), int(cl[i])
        # exactly the table's bytes changed
        want = H0[i].copy()
        if L and L <= INLINE:
            want[DATA:DATA + c] = src[a:a + c]
        if L:
            want[DCSUM:ELAN] = qm.le([vals[i]])[0]
        assert np.array_equal(H[i, :HCSUM], want[:HCSUM]), L
        t = int(doffs[i])
        moved = dst[t:t + 2064 - 3]
        if L > INLINE and c:
            assert np.array_equal(moved[:c], src[a:a + c]) and np.array_equal(moved[c:], dst0[t + c:t + 2064 - 3])
        else:
            assert np.array_equal(moved, dst0[t:t + 2064 - 3]), L
        for lo, hi in REGIONS:
            for _ in range(4):
                B = H[i:i + 1].copy()
                B[0, int(rng.integers(lo, hi))] ^= np.uint8(1 << int(rng.integers(0, 8)))
                assert not qm.header_ok(oracle, B, mode)[0], (L, lo)


def test_checksumming_off(oracle):
    rng = np.random.default_rng(37)
    for copy in (True, False):
        H0, H, src, soffs, dst0, dst, doffs, parts, vals, cl, ln = _pack(oracle, rng, NONE, copy)
        assert qm.header_ok(oracle, H, NONE).all() and not vals.any()
        for i, L in enumerate(LENGTHS):
            want = H0[i].copy()
            c = int(cl[i])
            if L and L <= INLINE:
                want[DATA:DATA + c] = src[int(soffs[i]):int(soffs[i]) + c]
            if c:
                want[DCSUM:ELAN] = 0
            want[HCSUM:] = 0
            assert np.array_equal(H[i], want), (copy, L)


@SUMS
def test_receive_model_delivers_what_was_packed(oracle, mode):
    rng = np.random.default_rng(41 + mode)
    H0, H, src, soffs, dst0, dst, doffs, parts, vals, cl, ln = _pack(oracle, rng, mode, True)
    # the sender's register is the receiver's only from CRC_INITIAL_REGISTER: restamp with those values
    n = len(LENGTHS)
    fresh = oracle.desc_batch(src, soffs, ln.astype(np.uint32), np.full(n, qm.M32, np.uint32) if mode == CRC else None,
                              mode)
    keep = H[:, DCSUM:ELAN].copy()
    qm.stamp_headers(oracle, H, fresh, mode)
    H[0, DCSUM:ELAN] = keep[0]  # (the empty fragment's word is the caller's)
    H[:, HCSUM:] = qm.le(qm.header_csums(oracle, H, mode))
    base = np.concatenate([dst, H.reshape(-1)])
    poffs = np.where(ln <= INLINE, len(dst) + np.arange(n) * HDR + DATA, doffs.astype(np.int64)).astype(np.uint64)
    app = np.zeros(n * 2064, np.uint8)
    aoffs = np.arange(n, dtype=np.uint64) * np.uint64(2064)
    copied, csum, hbad, dbad = qm.recv_expect(oracle, base, poffs, ln, H, np.ones(n, bool), app, aoffs,
                                               np.full(n, 4096, np.int64), mode)
    assert not hbad.any() and not dbad.any()
    assert [int(x) for x in copied] == LENGTHS
    for i, L in enumerate(LENGTHS):
        assert np.array_equal(app[i * 2064:i * 2064 + L], src[int(soffs[i]):int(soffs[i]) + L]), L
    # a flipped payload byte inside the header is a header failure, outside it a data failure
    i52, i53 = LENGTHS.index(52), LENGTHS.index(53)
    base[len(dst) + i52 * HDR + DATA + 7] ^= np.uint8(4)
    H2 = base[len(dst):].reshape(n, HDR)
    base[int(doffs[i53]) + 9] ^= np.uint8(4)
    copied, csum, hbad, dbad = qm.recv_expect(oracle, base, poffs, ln, H2, np.ones(n, bool), app, aoffs,
                                               np.full(n, 4096, np.int64), mode)
    assert copied[i52] == -2 and hbad[i52] and not dbad[i52]
    assert copied[i53] == -1 and dbad[i53] and not hbad[i53]


@SUMS
def test_values_equal_the_compiled_reference(oracle, reference, mode):
    rng = np.random.default_rng(43 + mode)
    for copy in (True, False):
        H0, H, src, soffs, dst0, dst, doffs, parts, vals, cl, ln = _pack(oracle, rng, mode, copy)
        for i, L in enumerate(LENGTHS):
            if L == 0:
                continue
            a = int(soffs[i])
            v = qm.frag_value(reference, src[a:a + L], int(cl[i]), L, int(parts[i]), mode)
            assert v == int(vals[i]) == int(qm.u32(H[i:i + 1, DCSUM:ELAN])[0]), (copy, L)
        for i in range(len(LENGTHS)):
            h = np.ascontiguousarray(H[i])
            stored = int(qm.u32(H[i:i + 1, HCSUM:])[0])
            if mode == CRC:
                c = reference.uicrc(h, HCSUM)
                assert int.from_bytes(c.to_bytes(4, "little"), "big") == stored
                assert reference.uicrc(h, HDR) == 0
            else:
                assert reference.uicsum(h, HCSUM)[0] == stored
                assert reference.uicsum(h, HDR)[0] == (2 * stored) & qm.M32
