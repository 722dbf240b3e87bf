"""The model of the typemap forms of the one-call steps (lampi_tmap_send_pack, lampi_tmap_recv_unpack), from the
oracle alone, and the typemaps and fixtures tests/test_tmap_model.py and tests/test_gpu_tmap_*.py share.

  (a) index_map      the address rule as a vectorised index map: packed byte p lives at
                     (p // packed_size) * extent + offset[i] + (r - seq_offset[i]), r = p % packed_size, i the last
                     pair with seq_offset <= r (relative to the datatype's origin; may be negative)
  (b) send_pieces    the reference's own walk restated: gmSendFragDesc::init's non-contiguous branch
      recv_pieces    (ref src/path/gm/sendFrag.cc:165-214: init_cnt, the first-pair formula, the ti loop) and
                     non_contiguous_copy (ref src/path/common/BaseDesc.cc:93-160), each yielding a fragment's pieces
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
