"""The model of the Quadrics flavour of the one-call send and receive steps (LAMPI_SEND_HDR_QUADRICS), from the
oracle alone, and the fixtures tests/test_quadrics_model.py and tests/test_gpu_quadrics_*.py share.

quadricsCtlHdr_t's MESSAGE_DATA header (ref src/path/quadrics/header.h:71-87, :164-179) is 128 bytes: dataLength
@20, frag_seq @32, sendFragDescPtr @48, dataSeqOffset @56, dataChecksum @64, dataElanAddr @68, data[52] @72,
checksum @124.

  send (ref src/path/quadrics/sendFrag.h:766-880, :970-986), len = max(copylen, csumlen):
    len == 0              nothing copied, the word @64 left alone
    0 < len <= 52         copylen bytes to header + 72; @64 = bcopy_uicrc / bcopy_uicsum (off: 0 when copylen > 0)
    len > 52, copylen > 0 copied to dst; @64 = the same value (off: 0)
    len > 52, copylen = 0 nothing copied; @64 = uicrc / uicsum of the source (off: untouched, nothing read)
    then                  @124 = header_checksum(H, 124, 32, usecrc), that word taken as 0 (off: 0)
  receive (ref src/path/quadrics/path.cc:839-900, recvFrag.h:54-126, recvFrag.cc:150-160):
    CRC uicrc(H, 128) == 0, SUM the 32 words' sum == 2 x the word @124; a failed header drops the fragment;
    the payload is at header + 72 when length <= 52; then copy_to_app / copy_to_app_nochecksum against the word @64.

Bulk values come from oracle.desc_batch; a spread of fragments is re-checked call by call with oracle.uicrc, uicsum,
bcopy_uicrc, bcopy_uicsum, header_checksum, copy_to_app and copy_to_app_nochecksum.
"""
import numpy as np

HDR, DCSUM, ELAN, DATA, INLINE, HCSUM, WORDS = 128, 64, 68, 72, 52, 124, 32
LEN_AT, SEQ_AT, PTR_AT, SEQOFF_AT = 20, 32, 48, 56
QUADRICS = 3
CRC, SUM, NONE = 0, 1, 2
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
EDGE_LENGTHS = [0, 1, 3, 51, 52, 53, 64, 2047, 2048, 2049, 4096, 4097, 65535, 65536]


def u32(rows):
    """n x 4 bytes -> n little-endian words."""
    return np.ascontiguousarray(rows).view("<u4").reshape(len(rows))


def le(words):
    """n words -> n x 4 bytes, little-endian."""
    return np.asarray(words, np.uint32).astype("<u4").view(np.uint8).reshape(-1, 4)


def _spread(n, k=24):
    return sorted(set(int(x) for x in np.arange(k) * n // k)) if n else []


def header_csums(oracle, H, mode):
    """The word @124 of n headers (H: n x 128 bytes, whatever their word @124 holds) as the sender computes it:
    header_checksum(H, 124, 32, usecrc) with that word taken as 0 -- bswap32(uicrc(H, 124)) or the sum of words
    0..30, in bulk; a spread re-checked with oracle.header_checksum."""
    n = len(H)
    if mode == NONE:
        return np.zeros(n, np.uint32)
    flat = np.ascontiguousarray(H).reshape(-1)
    v = oracle.desc_batch(flat, np.arange(n, dtype=np.uint64) * np.uint64(HDR), np.full(n, HCSUM, np.uint32),
                          np.full(n, M32, np.uint32) if mode == CRC else None, mode)
    if mode == CRC:
        v = v.byteswap()
    for i in _spread(n, 32):
        z = np.array(H[i], np.uint8)
        z[HCSUM:] = 0
        assert oracle.header_checksum(z, HCSUM, WORDS, mode == CRC) == int(v[i]), i
    return v


def header_ok(oracle, H, mode):
    """The receiver's verdict on n headers (n x 128 bytes): True = passes."""
    n = len(H)
    if mode == NONE or n == 0:
        return np.ones(n, bool)
    H = np.ascontiguousarray(H)
    flat = H.reshape(-1)
    v = oracle.desc_batch(flat, np.arange(n, dtype=np.uint64) * np.uint64(HDR), np.full(n, HDR, np.uint32),
                          np.full(n, M32, np.uint32) if mode == CRC else None, mode)
    w31 = u32(H[:, HCSUM:HDR])
    ok = v == 0 if mode == CRC else v == ((w31.astype(np.uint64) * 2) & M32).astype(np.uint32)
    for i in _spread(n, 32):
        if mode == CRC:
            s = oracle.uicrc(H[i], HDR) == 0
        else:
            s = oracle.uicsum(H[i], HDR)[0] == (2 * int(w31[i])) & M32
        assert bool(s) == bool(ok[i]), i
    return ok


def frag_value(oracle, src, copylen, csumlen, partial, mode):
    """One fragment's dataChecksum call by call: bcopy_uicrc / bcopy_uicsum where bytes are copied, uicrc / uicsum
    where none are (the Elan-addressable send)."""
    mx = max(copylen, csumlen)
    s = np.ascontiguousarray(src[:mx]) if mx else np.zeros(1, np.uint8)
    if copylen == 0:
        return oracle.uicrc(s, mx, partial) if mode == CRC else oracle.uicsum(s, mx)[0]
    dst = np.zeros(max(copylen, 1), np.uint8)
    if mode == CRC:
        v = oracle.bcopy_uicrc(s, dst, copylen, csumlen, partial)
    else:
        v = oracle.bcopy_uicsum(s, dst, copylen, csumlen)[0]
    assert np.array_equal(dst[:copylen], s[:copylen])
    return v


def send_expect(oracle, src, soffs, copylens, csumlens, parts, hdrs, hat, dst, doffs, mode):
    """The descriptor form's model.  Fragment i = src[soffs[i]:], its header the 128 bytes at hdrs[hat[i]:], its
    destination dst[doffs[i]:] (ignored when inline).  hdrs and dst (numpy; they may be one array) are changed in
    place to what the call must leave.  Returns the dataChecksum values (0 where none is computed)."""
    n = len(soffs)
    cl, ln = np.asarray(copylens, np.uint64), np.asarray(csumlens, np.uint64)
    mx = np.maximum(cl, ln)
    on = mode != NONE
    vals = np.zeros(n, np.uint32)
    if on:
        vals = oracle.desc_batch(src, np.asarray(soffs, np.uint64), mx.astype(np.uint32),
                                 np.asarray(parts, np.uint64).astype(np.uint32) if mode == CRC else None, mode)
        for i in _spread(n):
            a = int(soffs[i])
            assert frag_value(oracle, src[a:a + int(mx[i])], int(cl[i]), int(ln[i]), int(parts[i]), mode) == \
                int(vals[i]), i
    for i in range(n):
        a, c, m, h = int(soffs[i]), int(cl[i]), int(mx[i]), int(hat[i])
        if m == 0:
            continue
        if m <= INLINE:
            hdrs[h + DATA:h + DATA + c] = src[a:a + c]
        elif c:
            t = int(doffs[i])
            dst[t:t + c] = src[a:a + c]
        if on:
            hdrs[h + DCSUM:h + DCSUM + 4] = le([vals[i]])[0]
        elif c:
            hdrs[h + DCSUM:h + DCSUM + 4] = 0
    idx = np.asarray(hat, np.int64)[:, None] + np.arange(HDR)
    hc = header_csums(oracle, hdrs[idx], mode)
    hdrs[np.asarray(hat, np.int64)[:, None] + HCSUM + np.arange(4)] = le(hc)
    return vals


def msg_send_expect(oracle, m, L, ring, stride, tmpl, seq0, seq_step, ptr0, ptr_stride, so0, mode):
    """The message form's model: the ring (numpy, in place) as lampi_msg_send_pack must leave it.  Returns the
    number of slots written."""
    mlen = len(m)
    n = (mlen + L - 1) // L if mlen else 1
    bare = stride == HDR
    lens = np.minimum(L, mlen - np.arange(n, dtype=np.int64) * L).astype(np.int64) if mlen else np.zeros(1, np.int64)
    on = mode != NONE
    vals = np.zeros(n, np.uint32)
    if on:
        vals = oracle.desc_batch(m if mlen else np.zeros(1, np.uint8), np.arange(n, dtype=np.uint64) * np.uint64(L),
                                 lens.astype(np.uint32), np.full(n, M32, np.uint32) if mode == CRC else None, mode)
        for k in _spread(n):
            c = int(lens[k])
            cp = 0 if (bare and c > INLINE) else c
            assert frag_value(oracle, m[k * L:k * L + c], cp, c, M32, mode) == int(vals[k]), k
    t = np.asarray(tmpl, np.uint8)
    H = np.zeros((n, HDR), np.uint8)
    H[:, :DATA] = t
    k = np.arange(n, dtype=np.uint64)
    H[:, LEN_AT:LEN_AT + 4] = le(lens)
    H[:, SEQ_AT:SEQ_AT + 8] = np.array([(seq0 + int(i) * seq_step) & M64 for i in k], "<u8").view(np.uint8).reshape(n, 8)
    H[:, PTR_AT:PTR_AT + 8] = np.array([(ptr0 + int(i) * ptr_stride) & M64 for i in k], "<u8").view(np.uint8).reshape(n, 8)
    H[:, SEQOFF_AT:SEQOFF_AT + 8] = np.array([(so0 + int(i) * L) & M64 for i in k], "<u8").view(np.uint8).reshape(n, 8)
    e0 = int(u32(t[None, ELAN:ELAN + 4])[0])
    H[:, ELAN:ELAN + 4] = le([(e0 + int(i) * L) & M32 for i in k])
    for i in range(n):
        c, s = int(lens[i]), i * stride
        if c == 0:
            continue
        if c <= INLINE:
            H[i, DATA:DATA + c] = m[i * L:i * L + c]
        elif not bare:
            ring[s + HDR:s + HDR + c] = m[i * L:i * L + c]
        if on:
            H[i, DCSUM:DCSUM + 4] = le([vals[i]])[0]
        elif c <= INLINE or not bare:
            H[i, DCSUM:DCSUM + 4] = 0
    H[:, HCSUM:] = le(header_csums(oracle, H, mode))
    for i in range(n):
        ring[i * stride:i * stride + HDR] = H[i]
    return n


def recv_expect(oracle, base, poffs, lens, H, ok_extra, app, aoffs, alens, mode):
    """The receive model over the bytes as they are: fragment i = lens[i] bytes at base[poffs[i]] (the caller has
    already pointed an inline fragment at its header's data[]), header H[i] (n x 128), delivered to app[aoffs[i]]
    with alens[i] bytes of room.  ok_extra: False drops the fragment whatever its checksum says (malformed).  Writes
    the deliveries into app (numpy, in place); returns (copied int64, csum uint32, hdr bad bool, data bad bool)."""
    from oracle.oracle import copy_to_app, copy_to_app_nochecksum

    n = len(lens)
    ok = header_ok(oracle, H, mode) & np.asarray(ok_extra, bool)
    exp = u32(np.ascontiguousarray(H)[:, DCSUM:DCSUM + 4])
    crc = mode == CRC
    ln = np.where(ok, np.asarray(lens, np.uint64), 0).astype(np.uint32)
    vals = np.zeros(n, np.uint32)
    if mode != NONE:
        vals = oracle.desc_batch(base, np.where(ok, np.asarray(poffs, np.uint64), 0).astype(np.uint64), ln,
                                 np.full(n, M32, np.uint32) if crc else None, mode)
    copied = np.empty(n, np.int64)
    csum = np.zeros(n, np.uint32)
    empty = 0 if mode == NONE else (M32 if crc else 0)
    spread = set(_spread(n))
    for i in range(n):
        if not ok[i]:
            copied[i] = -2
            continue
        a, L, room = int(poffs[i]), int(ln[i]), int(alens[i])
        c = 0 if room <= 0 else min(L, room)
        if c == 0:
            copied[i], csum[i] = 0, empty
        else:
            t = int(aoffs[i])
            app[t:t + c] = base[a:a + c]
            if mode == NONE:
                copied[i] = c
            else:
                csum[i] = vals[i]
                copied[i] = c if vals[i] == exp[i] else -1
        if i in spread:
            frag = base[a:a + L]
            r = (copy_to_app_nochecksum(frag, L, room) if mode == NONE else
                 copy_to_app(oracle, frag if L else np.zeros(1, np.uint8), L, room, int(exp[i]), crc))
            assert (int(r[0]), int(r[1])) == (int(copied[i]), int(csum[i])), (i, r[:2], copied[i], csum[i])
            assert np.array_equal(r[2], base[a:a + c]), i
    return copied, csum, ~ok, copied == -1


def ring_recv_expect(oracle, hring, nslots, stride, app, app_len, seq0, mode):
    """The ring form's model over the ring bytes as they are: every field from the 128-byte envelopes, the payload at
    slot + 72 (dataLength <= 52) or slot + 128; a longer dataLength than the slot holds is malformed."""
    S = hring[:nslots * stride].reshape(nslots, stride)
    H = S[:, :HDR]
    lens = u32(H[:, LEN_AT:LEN_AT + 4]).astype(np.uint64)
    well = (lens <= INLINE) | (lens <= stride - HDR)
    so = np.ascontiguousarray(H[:, SEQOFF_AT:SEQOFF_AT + 8]).view("<u8").reshape(nslots)
    off = [(int(x) - seq0) & M64 for x in so]
    room = np.array([0 if o >= app_len else app_len - o for o in off], np.int64)
    aoffs = np.array([o if r > 0 else 0 for o, r in zip(off, room)], np.uint64)
    poffs = np.arange(nslots, dtype=np.uint64) * np.uint64(stride) + np.where(lens <= INLINE, DATA, HDR).astype(np.uint64)
    return recv_expect(oracle, hring, poffs, np.where(well, lens, 0), H, well, app, aoffs, room, mode)


def stamp_headers(oracle, H, vals, mode):
    """n x 128 headers given the dataChecksum values `vals` and a valid word @124 (checksumming on), in place."""
    if mode == NONE:
        return H
    H[:, DCSUM:DCSUM + 4] = le(vals)
    H[:, HCSUM:] = le(header_csums(oracle, H, mode))
    return H


def mixed_lengths(rng, n):
    """The lengths of the descriptor-form tests: every edge, then 36 more inline fragments (1..52 bytes -- uniform
    lengths would hold next to none), the rest random in 0..65,536; shuffled but for fragments 0 and n - 1, which
    stay an edge (0) and a random length."""
    ln = rng.integers(0, 65537, size=n).astype(np.uint64)
    e = len(EDGE_LENGTHS)
    ln[:e] = EDGE_LENGTHS
    ln[e:e + 36] = rng.integers(1, INLINE + 1, size=36).astype(np.uint64)
    mid = ln[1:n - 1].copy()
    rng.shuffle(mid)
    ln[1:n - 1] = mid
    return ln
