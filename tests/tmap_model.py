"""The model of the typemap forms of the one-call steps (lampi_tmap_send_pack, lampi_tmap_recv_unpack), from the
oracle alone, and the typemaps and fixtures tests/test_tmap_model.py and tests/test_gpu_tmap_*.py share.

  (a) index_map      the address rule as a vectorised index map: packed byte p lives at
                     (p // packed_size) * extent + offset[i] + (r - seq_offset[i]), r = p % packed_size, i the last
                     pair with seq_offset <= r (relative to the datatype's origin; may be negative)
  (b) send_pieces    the reference's own walk restated: gmSendFragDesc::init's non-contiguous branch
      recv_pieces    (ref src/path/gm/sendFrag.cc:165-214: init_cnt, the first-pair formula, the ti loop) and
                     non_contiguous_copy (ref src/path/common/BaseDesc.cc:93-160), each yielding a fragment's pieces
  (c) classes        the geometry classes of a call -- the frame and address rules of tmap_kernels.h's header comment
                     restated --, and SEND_SWEEP / RECV_SWEEP, the cases tests/test_gpu_tmap_sweep.py runs and
                     tests/test_tmap_classes.py proves to reach every required class
"""
import numpy as np


class Typemap:
    """A datatype: pairs (size, offset) in packed order, seq_offset their running sum, and its extent."""

    def __init__(self, name, sizes, offsets, extent, overlap_ok=False):
        self.name = name
        self.size = np.asarray(sizes, np.int64)
        self.offset = np.asarray(offsets, np.int64)
        self.seq = np.concatenate(([0], np.cumsum(self.size[:-1]))).astype(np.int64)
        self.extent = int(extent)
        self.packed_size = int(self.size.sum())
        self.num_pairs = len(self.size)
        assert self.num_pairs >= 1 and int(self.size.min()) >= 1
        # the pieces of one element and of neighbouring elements do not overlap
        lo, hi = self.offset, self.offset + self.size
        order = np.argsort(lo)
        assert np.all(hi[order][:-1] <= lo[order][1:]), name
        assert overlap_ok or int(hi.max()) - int(lo.min()) <= self.extent, name  # (a send may read elements that overlap)

    def pairs(self):
        return np.stack([self.size, self.offset], axis=1)

    def span(self, count):
        """[lo, hi) relative to the origin that `count` elements' pieces lie in."""
        return int(self.offset.min()), (count - 1) * self.extent + int((self.offset + self.size).max())


def _scattered(name, n, seed):
    """n pairs of random sizes 1..40 at shuffled non-overlapping offsets with gaps of 0..7 bytes."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 41, size=n)
    offsets = np.empty(n, np.int64)
    cur = 0
    for j in rng.permutation(n):
        offsets[j] = cur + int(rng.integers(0, 8))
        cur = int(offsets[j] + sizes[j])
    return Typemap(name, sizes, offsets, cur + 5)


T1 = Typemap("T1", [8], [3], 24)                              # a vector of 8-byte blocks
T2 = Typemap("T2", [1, 13, 51], [70, -16, 0], 128)            # a struct: packed_size 65, a negative offset
T3 = Typemap("T3", [5000, 3001], [5, 6001], 12288)            # pieces longer than a row
T4A = _scattered("T4a", 64, 41)                               # staged in LDS
T4B = _scattered("T4b", 5000, 42)                             # 120 KB of pairs: read through L2
T5 = Typemap("T5", [48], [0], 48)                             # contiguous
TYPEMAPS = [T1, T2, T3, T4A, T4B, T5]
FRAG_LENS = [100, 1976, 4096, 65456]
LAST_LENS = [1, 15, 17, None]                                 # the last fragment's bytes (None: a whole fragment)


def _struct15(name, seed):
    """15 pairs of sizes 1..15 in packed order at shuffled non-overlapping offsets with gaps of 0..3 bytes."""
    rng = np.random.default_rng(seed)
    sizes = np.arange(1, 16)
    offsets = np.empty(15, np.int64)
    cur = 0
    for j in rng.permutation(15):
        offsets[j] = cur + int(rng.integers(0, 4))
        cur = int(offsets[j] + sizes[j])
    return Typemap(name, sizes, offsets, cur + 2)


# The sweep's typemaps (tests/test_tmap_classes.py, tests/test_gpu_tmap_sweep.py): elements shorter than a chunk,
# pieces either side of 16 bytes, elements either side of locate's 8 KiB cut and of a row plus a chunk, pair counts
# either side of the LDS cut.
S1 = Typemap("S1", [1], [0], 3)
S2 = Typemap("S2", [1, 1], [2, 0], 5)
S3 = Typemap("S3", [2, 1], [0, 5], 7)
S7 = Typemap("S7", [3, 4], [9, 1], 13)
S15 = Typemap("S15", [15], [1], 17)
S16 = Typemap("S16", [16], [3], 21)
S17 = Typemap("S17", [17], [0], 18)
S120 = _struct15("S120", 43)
S8192 = Typemap("S8192", [4096, 4096], [7, 4200], 8400)
S8193 = Typemap("S8193", [4096, 4097], [1, 4100], 8300)
S4111 = Typemap("S4111", [4111], [5], 4200)
S63 = Typemap("S63", [2] * 63, [3 * j for j in range(63)], 190)
S65 = Typemap("S65", [1] * 65, [2 * (64 - j) for j in range(65)], 131)
SWEEP_TYPEMAPS = [S1, S2, S3, S7, S15, S16, S17, S120, S8192, S8193, S4111, S63, S65]
SWEEP_LONG = [S8192, S8193, S4111]                            # elements longer than a row


def index_map(tm, p):
    """(a): the byte index, relative to the origin, of each packed byte in p."""
    p = np.asarray(p, np.int64)
    e, r = p // tm.packed_size, p % tm.packed_size
    i = np.searchsorted(tm.seq, r, side="right") - 1
    return e * tm.extent + tm.offset[i] + (r - tm.seq[i])


def first_pair(tm, seq_off):
    """The starting typemap index of BaseDesc.cc:93-105 (the path layer computes tmapIndex_m the same way)."""
    init_cnt = seq_off // tm.packed_size
    t = tm.num_pairs - 1
    for i in range(tm.num_pairs):
        s = init_cnt * tm.packed_size + int(tm.seq[i])
        if s == seq_off:
            return i
        if s > seq_off:
            return i - 1
    return t


def send_pieces(tm, seq_off, length, msg_len):
    """(b), send: the pieces (source index relative to the origin, bytes) gmSendFragDesc::init copies to
    payloadp + len_copied for the fragment of `length` bytes at seqOffset_m = seq_off of a message of msg_len
    packed bytes; zero-length calls left out."""
    ps, ext = tm.packed_size, tm.extent
    tm_init = first_pair(tm, seq_off)
    init_cnt, tot_cnt = seq_off // ps, msg_len // ps
    start = init_cnt * ext
    out = []
    src = start + int(tm.offset[tm_init]) - init_cnt * ps - int(tm.seq[tm_init]) + seq_off
    n = int(tm.size[tm_init]) + init_cnt * ps + int(tm.seq[tm_init]) - seq_off
    n = min(n, length)
    if n:
        out.append((src, n))
    copied = n
    tm_init += 1
    for _ in range(init_cnt, tot_cnt):
        for ti in range(tm_init, tm.num_pairs):
            n = min(int(tm.size[ti]), length - copied)
            if n == 0:
                break
            out.append((start + int(tm.offset[ti]), n))
            copied += n
        if copied == length:
            break  # (the reference's loops run on making zero-length tests; nothing more is copied)
        tm_init = 0
        start += ext
    return out


def recv_pieces(tm, seq_off, frag_len, msg_len):
    """(b), receive: the pieces (destination index relative to the origin, offset in the payload, bytes) of
    non_contiguous_copy for a fragment of frag_len bytes at frag_seq_off = seq_off."""
    ps, ext = tm.packed_size, tm.extent
    init_cnt, tot_cnt = seq_off // ps, msg_len // ps
    t0 = first_pair(tm, seq_off)
    out = []
    dest = init_cnt * ext + int(tm.offset[t0]) - init_cnt * ps - int(tm.seq[t0]) + seq_off
    n = 0 if frag_len == 0 else min(int(tm.size[t0]) + init_cnt * ps + int(tm.seq[t0]) - seq_off, frag_len)
    if n:
        out.append((dest, 0, n))
    copied = n
    if frag_len - copied:
        t0 += 1
        for cnt in range(init_cnt, tot_cnt):
            for ti in range(t0, tm.num_pairs):
                n = min(int(tm.size[ti]), frag_len - copied)
                if n == 0:
                    return out
                out.append((cnt * ext + int(tm.offset[ti]), copied, n))
                copied += n
            t0 = 0
    return out


def fragments(pack_off, pack_len, frag_len):
    """[(packed offset, bytes)] of a window's fragments; one empty fragment for an empty window."""
    n = (pack_len + frag_len - 1) // frag_len if pack_len else 1
    return [(pack_off + j * frag_len, min(frag_len, pack_len - j * frag_len)) for j in range(n)]


def pack_offsets(tm):
    """The three window starts: 0, 7 bytes into a pair (the first pair of at least 8 bytes, in element 1), an
    element boundary."""
    i = int(np.nonzero(tm.size >= 8)[0][0])
    return [0, tm.packed_size + int(tm.seq[i]) + 7, 2 * tm.packed_size]


def window_len(frag_len, nfrag, last):
    """A window of nfrag fragments whose last one holds `last` bytes (None: a whole fragment)."""
    return nfrag * frag_len if last is None else (nfrag - 1) * frag_len + last


def count_for(tm, nbytes):
    """Elements that hold at least nbytes packed bytes."""
    return (nbytes + tm.packed_size - 1) // tm.packed_size


def host_buffer(tm, count, seed, pad=32):
    """(buffer of random bytes, the origin's byte offset in it) around `count` elements, `pad` bytes of margin."""
    lo, hi = tm.span(count)
    origin = pad - min(lo, 0)
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=origin + max(hi, 0) + pad, dtype=np.uint8), origin


def packed(tm, buf, origin, pack_off, pack_len):
    """The packed bytes [pack_off, pack_off + pack_len) of the message at buf[origin], by (a)."""
    return buf[origin + index_map(tm, pack_off + np.arange(pack_len, dtype=np.int64))]


# ---- the geometry classes of a call (the ledger tests/test_tmap_classes.py keeps) ---------------------------------
#
# The frame rules restated from the header comment of lampi_amd/csrc/tmap_kernels.h (Frames / Addresses):
#   R = max(1, ceil(room / 4096)) rows, room = frag_len (send) or slot_stride - 72 (receive);
#   CRC: the fragment's L bytes at frame offsets [P, P + L), P = 4096 R - L, the register's four bytes at Q = P, or
#        Q = P - 4 when L < 4;  SUM / off: P = 0;
#   chunks of 16 bytes at frame offsets 1024 q + 16 lane of each row, i.e. at every multiple of 16;
#   packed byte p lives in element p // packed_size, pair = the last with seq_offset <= p % packed_size; a row divides
#   once for its first fragment byte, a chunk adds its distance d: in the same element, one subtraction
#   (packed_size > 8192) or a division with quotient q.
CRC, SUM, NONE = 0, 1, 2                                      # lampi_csum_mode
ROW, CHUNK, HDR_BYTES = 4096, 16, 72


def frame_rows(room):
    return max(1, (room + ROW - 1) // ROW)


def _fragment_classes(tm, p0, L, ncopy, R, mode, recv, out):
    """The tags of one fragment: L bytes from packed byte p0 in a frame of R rows, the first ncopy of them moved on
    the typemap side (ncopy < L: a receive cut by app_len)."""
    P = ROW * R - L if mode == CRC else 0
    if mode == CRC:
        Q = P - 4 if L < 4 else P
        if L < 4:
            out.add(("tiny", L))
        for x in range((Q - 15 + CHUNK - 1) // CHUNK * CHUNK, Q + 4, CHUNK):  # chunks with -4 < Q - x < 16
            if 0 <= x < ROW * R:
                out.add(("dl", Q - x))
        if Q // ROW != (Q + 3) // ROW:
            out.add(("dl_rows",))
    if L == 0:
        return
    f = np.arange(P, P + L, dtype=np.int64)                   # frame offsets of the fragment's bytes
    p = p0 + (f - P)
    e, r = p // tm.packed_size, p % tm.packed_size
    i = np.searchsorted(tm.seq, r, side="right") - 1
    avail = tm.size[i] - (r - tm.seq[i])                      # bytes of the piece from this byte on
    ch, k = f // CHUNK, f % CHUNK
    first = np.concatenate(([True], ch[1:] != ch[:-1]))       # the chunk's first / last byte inside the fragment
    last = np.concatenate((first[1:], [True]))
    for kk in k[first & (k != 0)]:
        out.update([("cut", int(kk)), ("cut", int(kk), "first")])
    for kk in k[last & (k != CHUNK - 1)] + 1:
        out.update([("cut", int(kk)), ("cut", int(kk), "last")])
    # the typemap side: the moved bytes of each chunk as runs from one piece
    if recv and ncopy < L:
        c = P + ncopy - 1                                     # the last delivered byte's frame offset
        sel = (ch == c // CHUNK) & (f <= c)
        pieces = len(set(zip(e[sel].tolist(), i[sel].tolist())))
        out.add(("clip", int((c + 1) % CHUNK), pieces > 1))
    n = min(ncopy, L)
    if n == 0:
        return
    e, i, avail, ch, k, first = e[:n], i[:n], avail[:n], ch[:n], k[:n], first[:n]
    start = first | np.concatenate(([False], (e[1:] != e[:-1]) | (i[1:] != i[:-1])))
    s = np.flatnonzero(start)
    run_len = np.diff(np.concatenate((s, [n])))
    # locate: the distance of a chunk's first byte from its row's first fragment byte
    fa = np.maximum(f[:n][first] // ROW * ROW, P)
    rr = (p0 + fa - P) % tm.packed_size + (f[:n][first] - fa)
    q = rr // tm.packed_size
    if np.any(q == 0):
        out.add(("locate", "in"))
    if np.any(q > 0):
        if tm.packed_size > 8192:
            out.add(("locate", "sub"))
        else:
            out.update(("locate", "div", int(v)) for v in np.unique(np.minimum(q[q > 0], 3)))
    cs = np.flatnonzero(first)                                # per chunk: its first byte, bytes and runs
    nbytes = np.diff(np.concatenate((cs, [n])))
    nruns = np.add.reduceat(start.astype(np.int64), cs)
    whole = (k[cs] == 0) & (nbytes == CHUNK)
    for a in (16, 17):
        if np.any(whole & (avail[cs] == a)):
            out.add(("fast", a))
    if np.any(whole & (avail[cs] == 15)):
        out.add(("near", 15))
    one_access = np.repeat(whole & (nruns == 1), nruns)       # per run: its chunk moves as one 16-byte access
    spans = np.unique(np.stack([k[s], run_len])[:, ~one_access], axis=1)
    out.update(("span", int(a), int(b)) for a, b in spans.T)
    wrap = np.concatenate(([False], e[1:] != e[:-1])) & ~first
    w = np.add.reduceat(wrap.astype(np.int64), cs)
    out.update(("wraps", int(v)) for v in np.unique(np.minimum(w[w > 0], 16)))


def classes(tm, pack_off, pack_len, frag_len, mode, recv_room=None, app_len=None, frags=None):
    """The set of geometry tags of one call.  Send: the window's fragments (fragments()) in frames of frag_len.
    Receive (recv_room = slot_stride - 72): the same fragments, or frags = [(packed offset, bytes)] one per slot,
    every header good, delivered into app_len packed bytes (default: everything fits).

      ("dl", d)             CRC: a chunk starts d bytes before the register's four bytes, -4 < d < 16
      ("dl_rows",)          CRC: those four bytes lie in two rows
      ("tiny", L)           CRC: a fragment of L < 4 bytes (receive: only where something is delivered)
      ("span", k, n)        bytes [k, k + n) of a chunk come from one piece and the chunk does not move as one
                            16-byte access (it holds a piece boundary or is cut by the fragment or by app_len)
      ("fast", a)           a whole chunk from a piece with exactly a = 16 or 17 bytes left
      ("near", 15)          a whole chunk whose first piece has exactly 15 bytes left
      ("wraps", w)          the walk passes w times from an element's last pair to the next element's first inside
                            one chunk (capped at 16; 16 one-byte elements in a chunk are 15 wraps)
      ("locate", ...)       "in": the chunk's first byte lies in the element of its row's first byte; "sub":
                            beyond, packed_size > 8192; ("div", q): beyond, q elements on (capped at 3)
      ("R", R), ("join", "thread" | "wave" | "wave2")   rows; with a checksum and R > 1, the join by R <= 32,
                            33..64, > 64
      ("tailwaves", n R % 4), ("staged", num_pairs <= 64)
      ("cut", k), ("cut", k, "first" | "last")   a chunk's first byte inside the fragment is its byte k != 0, or
                            its last one byte k - 1 != 15
      ("clip", c, b)        receive: app_len cuts a fragment inside or at the end of a chunk, c = bytes of that chunk
                            before the cut mod 16; b: the chunk's delivered bytes come from more than one piece
                            (the cut itself always ends an element: app_len is a whole number of them)
    """
    recv = recv_room is not None
    R = frame_rows(recv_room if recv else frag_len)
    fr = list(frags) if frags is not None else fragments(pack_off, pack_len, frag_len)
    out = {("R", R), ("tailwaves", len(fr) * R % 4), ("staged", tm.num_pairs <= 64)}
    if mode != NONE and R > 1:
        out.add(("join", "thread" if R <= 32 else "wave" if R <= 64 else "wave2"))
    for off, n in fr:
        ncopy = n
        if recv:
            assert n <= recv_room
            if app_len is not None:
                ncopy = min(n, max(app_len - off, 0))
            if ncopy == 0:
                continue                                      # nothing delivered: the rows do not run
        _fragment_classes(tm, off, ncopy if mode == NONE else n, ncopy, R, mode, recv, out)
    return out


# ---- the sweep's cases ---------------------------------------------------------------------------------------------
#
# Send: (typemap, pack_off, pack_len, frag_len).  Receive: (typemap, count, slot_stride, [(packed offset, bytes)]
# per slot in message order) -- the slots tile [0, sum of bytes) back to back; app_len = count * packed_size.

FRAME_LENS = list(range(1, 81)) + list(range(4090, 4103)) + list(range(8189, 8196))
FRAME_TYPEMAPS = [T2, S3]


def _send_frames():
    """Every frame length: two whole fragments and a last one of 0..3 or frag_len - 1 bytes in turn; the window
    starts at a different byte each time."""
    out = []
    for tm in FRAME_TYPEMAPS:
        for j, L in enumerate(FRAME_LENS):
            last = min([0, 1, 2, 3, L - 1][j % 5], L - 1)
            out.append((tm, 7 * j % (3 * tm.packed_size), 2 * L + last, L))
    return out


def phase_frag_lens(tm):
    """Fragment lengths coprime to packed_size -- fragment j starts at phase (pack_off + j frag_len) mod packed_size,
    so packed_size fragments visit every phase --: the first, the middle and the last of the candidates."""
    if tm in SWEEP_LONG:
        return [17, 4097]
    c = [L for L in (1, 2, 3, 5, 15, 17, 31, 33, 47) if np.gcd(L, tm.packed_size) == 1]
    return [c[0], c[len(c) // 2], c[-1]]


def _send_phases():
    out = []
    for tm in SWEEP_TYPEMAPS:
        for L in phase_frag_lens(tm):
            if tm in SWEEP_LONG:  # from 40 bytes before an element's end, over it
                nf = 8 if L == 17 else 5
                out += [(tm, (1 + w) * tm.packed_size - 40 - w, window_len(L, nf, 3 + w), L) for w in range(2)]
            else:
                nf = min(tm.packed_size, 130) + 1
                out += [(tm, w, window_len(L, nf, 1 + w), L) for w in range(2)]
    return out


ROW_LENS = [33 * ROW - 5, 70 * ROW - 1]
ROW_TYPEMAPS = [T2, S3, S120]


def _send_rows():
    """R = 33 and 70 (the join's wave branch, once and twice round): three fragments and a short last one; one, two
    and three fragments at R = 1 and R = 2 (one to three live waves in the last workgroup); the empty window."""
    out = []
    for w, tm in enumerate(ROW_TYPEMAPS):
        out += [(tm, 5 + w, window_len(L, 4, 2 + 5 * w), L) for L in ROW_LENS]
        out += [(tm, w, window_len(L, nf, L - 3 * w), L) for L in (100, 5000) for nf in (1, 2, 3)]
        out += [(tm, 3 + w, 0, L) for L in (100, 5000) + tuple(ROW_LENS)]  # the empty window: its last row alone
    return out


SEND_FRAMES, SEND_PHASES, SEND_ROWS = _send_frames(), _send_phases(), _send_rows()
SEND_SWEEP = SEND_FRAMES + SEND_PHASES + SEND_ROWS

RECV_LEN_TYPEMAPS = [T2, S1, S120]
RECV_CLIP_TYPEMAPS = [S120, S1]
EDGE_4K, EDGE_8K = list(range(4090, 4103)), list(range(8189, 8196))


def tile(lens):
    """[(packed offset, bytes)] of fragments of `lens` bytes back to back from packed byte 0."""
    offs = np.concatenate(([0], np.cumsum(lens[:-1]))) if len(lens) else []
    return [(int(o), int(n)) for o, n in zip(offs, lens)]


def _recv_lengths():
    """Slots of 0..95 bytes in a shuffled order of the message, in slots of one, two and three rows -- with the
    row-edge lengths that fit beside them."""
    out = []
    for w, tm in enumerate(RECV_LEN_TYPEMAPS):
        for R in (1, 2, 3):
            lens = list(range(96)) + ([x for x in EDGE_4K + EDGE_8K if x <= R * ROW] if R > 1 else [])
            lens = np.random.default_rng(50 + 3 * w + R).permutation(lens)
            out.append((tm, count_for(tm, int(lens.sum())) + 1, HDR_BYTES + R * ROW, tile(lens)))
    return out


def _recv_clips():
    """app_len = count * packed_size cuts the third of five fragments after c = 0..33 bytes; the fourth and fifth
    lie wholly beyond it."""
    out = []
    for tm in RECV_CLIP_TYPEMAPS:
        for c in range(34):
            count = (150 + c + tm.packed_size - 1) // tm.packed_size + 1
            cut_at = count * tm.packed_size - c
            lens = [40 + c % 7, cut_at - (40 + c % 7), c + 1 + 5 * c % 23, 33, 1]
            out.append((tm, count, HDR_BYTES + 400 + (c % 3) * ROW, tile(lens)))
    return out


def _recv_rows():
    """Slots of 33 and of 70 rows, the lengths spread over the rows; seven slots (3 and 2 live waves in the last
    workgroup)."""
    out = []
    for w, tm in enumerate(ROW_TYPEMAPS):
        for R in (33, 70):
            lens = [R * ROW - 5, 0, 5 * ROW + 3, 1, (R - 1) * ROW + 1 + w, ROW - 1 - w, R * ROW]
            out.append((tm, count_for(tm, sum(lens)) + 1, HDR_BYTES + R * ROW, tile(lens)))
    return out


def _recv_phases():
    """Every sweep typemap on the scattering side: equal fragments of its middle coprime length over every phase."""
    out = []
    for w, tm in enumerate(SWEEP_TYPEMAPS):
        L = phase_frag_lens(tm)[1]
        nf = 5 if tm in SWEEP_LONG else min(tm.packed_size, 130) + 1
        off = tm.packed_size - 40 if tm in SWEEP_LONG else 0  # (from 40 bytes before an element's end)
        mlen = window_len(L, nf, 1 + w % 3)
        out.append((tm, count_for(tm, off + mlen), HDR_BYTES + frame_rows(L) * ROW, fragments(off, mlen, L)))
    return out


RECV_LENGTHS, RECV_CLIPS, RECV_ROWS, RECV_PHASES = _recv_lengths(), _recv_clips(), _recv_rows(), _recv_phases()
RECV_SWEEP = RECV_LENGTHS + RECV_CLIPS + RECV_ROWS + RECV_PHASES


def send_classes(case, mode):
    tm, pack_off, pack_len, frag_len = case
    return classes(tm, pack_off, pack_len, frag_len, mode)


def recv_classes(case, mode):
    tm, count, stride, frags = case
    return classes(tm, 0, 0, 0, mode, recv_room=stride - HDR_BYTES, app_len=count * tm.packed_size, frags=frags)
