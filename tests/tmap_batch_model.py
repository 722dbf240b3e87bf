"""The model of the descriptor forms of the typemap steps (lampi_tmap_send_pack_batch,
lampi_tmap_recv_unpack_batch) and the batches tests/test_tmap_batch_model.py and tests/test_gpu_tmap_batch_*.py share.

Nothing here comes from the library: the receive side is tests/recv_unpack_model.py's descriptor-form model
(expect: the header test, the drop, CopyToApp against the word @64, from the oracle) run over the concatenated packed
views of the batch's messages and mapped back per message through tests/tmap_model.py's address rule (index_map); the
send side is the address rule (packed) for the payloads and tests/test_gpu_send_pack.py's flavour table (_stamp_all)
for the words @64 / @68.  An invalid record (include/lampi_csum.h) is skipped on send and dropped as a failed header
on receive.
"""
import numpy as np

import tmap_model as tmm
from recv_unpack_model import expect, flip_bit
from test_gpu_send_pack import CRC, DCSUM, HCSUM, HDR, NONE, _put_words, _stamp_all

BATCH_TYPEMAPS = [tmm.T1, tmm.T2, tmm.T3, tmm.S63, tmm.S65, tmm.T4B, tmm.T5]
BASE_LENS = [0, 1, 3, 15, 17, 100, 1976, 4096, 4097]
MAX_LENS = [4096, 9000, 65456, 140000]     # R = 1 (no join), 3, 16 (thread join), 35 (wave join)
LONG_MSGS = (1, 4)                         # the messages that hold a max_len fragment in the 140,000 class
HDR_STRIDE, HDR_OFF = 76, 4                # headers in a tensor of their own, 4-byte aligned only


class Message:
    """`count` elements of `tm` in a host buffer of random bytes around the origin."""

    def __init__(self, tm, count, seed):
        self.tm, self.count = tm, count
        self.total = count * tm.packed_size
        self.hbuf, self.origin = tmm.host_buffer(tm, count, seed)
        self.idx = self.origin + tmm.index_map(tm, np.arange(self.total, dtype=np.int64))


class Batch:
    """Records (msg, pack_off, length, payload offset) over a list of Message; valid[i]: the record is valid."""

    def __init__(self, msgs, msg, pack_off, length, max_len, poffs=None, nmsgs=None):
        self.msgs, self.max_len = msgs, max_len
        self.nmsgs = len(msgs) if nmsgs is None else nmsgs
        self.msg = np.asarray(msg, np.int64)
        self.pack_off = np.asarray(pack_off, np.int64)
        self.length = np.asarray(length, np.int64)
        self.n = len(self.msg)
        if poffs is None:  # payloads one after another at every residue mod 16, eight bytes of gap
            poffs, cur = np.empty(self.n, np.int64), 16
            for i in range(self.n):
                poffs[i] = cur + i % 16
                cur = int(poffs[i] + self.length[i]) + 8
        self.poffs = np.asarray(poffs, np.int64)
        self.pay_size = int((self.poffs + self.length).max()) + max_len + 64 if self.n else 64
        self.hat = HDR_OFF + np.arange(self.n, dtype=np.int64) * HDR_STRIDE
        self.valid = np.ones(self.n, bool)

    def permuted(self, order):
        """The same fragments at the same payload offsets, the records in another order."""
        b = Batch(self.msgs, self.msg[order], self.pack_off[order], self.length[order], self.max_len,
                  self.poffs[order], self.nmsgs)
        b.valid = self.valid[order]
        return b


def message_lens(max_len, k, rng):
    """About 12 lengths for message k: every base length that fits, max_len itself (in the 140,000 class in two
    messages only: one or two long fragments among short ones), shuffled."""
    lens = [x for x in BASE_LENS if x <= max_len]
    lens += [max_len if (max_len <= 65456 or k in LONG_MSGS) else 4097, min(max_len, 1976)]
    while len(lens) < 12:
        lens.append((17, 100, 1976)[len(lens) % 3])
    return [int(x) for x in rng.permutation(lens)]


CLIPPED_MSGS = (1, 3)                      # receive: the messages posted short (T2, S63)


def window_starts(tm):
    """tmm.pack_offsets -- 0, 7 bytes into a pair, an element boundary --; a typemap without a pair of 8 bytes
    (S63, S65) starts 7 bytes into element 1 instead (inside a pair where the pairs are longer than a byte)."""
    if np.any(tm.size >= 8):
        return tmm.pack_offsets(tm)
    return [0, tm.packed_size + 7, 2 * tm.packed_size]


def plan(max_len, order, recv, seed):
    """One batch over BATCH_TYPEMAPS: message k's fragments tile its packed bytes from window_starts(tm)[k % 3] on
    (0, 7 bytes into a pair, an element boundary).  recv: the messages of CLIPPED_MSGS are posted short -- count
    elements end inside one of its fragments, so that one is clipped and the later ones lie at pack_off >= app_len.
    order: "grouped" (by message) or "robin" (round-robin across the messages)."""
    rng = np.random.default_rng(seed)
    msgs, recs = [], []
    for k, tm in enumerate(BATCH_TYPEMAPS):
        lens = message_lens(max_len, k, rng)
        start = window_starts(tm)[k % 3]
        offs = start + np.concatenate(([0], np.cumsum(lens[:-1])))
        end = int(offs[-1] + lens[-1])
        count = tmm.count_for(tm, end) + 1
        if recv and k in CLIPPED_MSGS:
            j = len(lens) - 4
            count = max(1, int(offs[j] + max(lens[j], 2) // 2) // tm.packed_size)
        msgs.append(Message(tm, count, seed + 10 + k))
        recs += [(j, k, int(o), n) for j, (o, n) in enumerate(zip(offs, lens))]
    if order == "robin":
        recs.sort(key=lambda r: (r[0], r[1]))
    return Batch(msgs, [r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs], max_len)


def _init(n, mode):
    return np.full(n, 0xFFFFFFFF, np.uint32) if mode == CRC else None


def _vals(oracle, pay, b, mode):
    ok = b.valid
    return oracle.desc_batch(pay, np.where(ok, b.poffs, 0).astype(np.uint64),
                             np.where(ok, b.length, 0).astype(np.uint32), _init(b.n, mode), mode)


def send_want(oracle, b, pay, hdr, hat, kind, mode):
    """The send step's model, in place: every valid record's packed bytes at its payload offset of `pay`, the words
    @64 / @68 of its header (at hat[i] of `hdr`, bytes [0, 64) as they are) by the flavour table."""
    for i in np.nonzero(b.valid)[0]:
        m, c = b.msgs[b.msg[i]], int(b.length[i])
        pay[b.poffs[i]:b.poffs[i] + c] = tmm.packed(m.tm, m.hbuf, m.origin, int(b.pack_off[i]), c)
    vals = np.zeros(b.n, np.uint32) if mode == NONE else _vals(oracle, pay, b, mode)
    w = _stamp_all(oracle, hdr[np.asarray(hat)[:, None] + np.arange(DCSUM)], vals, b.length == 0, kind, mode)
    if w is not None:
        ok = b.valid
        _put_words(hdr, np.asarray(hat)[ok] + DCSUM, w[0][ok])
        _put_words(hdr, np.asarray(hat)[ok] + HCSUM, w[1][ok])


def recv_fill(oracle, rng, b, pay, hdr, hat, kind, mode, faults=True):
    """A drained batch, in place: random sender bytes at every record's payload offset, its header random bytes
    with the valid words @64 / @68; then the faults by record index i % 10 -- 1, 7: a header bit, in bytes [0, 64),
    the word @64, the word @68 in turn; 3, 7: a payload byte, every other time the last one; 5: a consistent header
    with a wrong dataChecksum."""
    hat = np.asarray(hat)
    for i in range(b.n):
        pay[b.poffs[i]:b.poffs[i] + b.length[i]] = rng.integers(0, 256, size=int(b.length[i]), dtype=np.uint8)
        hdr[hat[i]:hat[i] + DCSUM] = rng.integers(0, 256, size=DCSUM, dtype=np.uint8)
    cls = np.arange(b.n) % 10 if faults else np.zeros(b.n, np.int64)
    if mode != NONE:
        vals = _vals(oracle, pay, b, mode)
        wrong = np.nonzero(cls == 5)[0]
        vals[wrong] ^= np.uint32(1) << rng.integers(0, 32, size=wrong.size).astype(np.uint32)
        w = _stamp_all(oracle, hdr[hat[:, None] + np.arange(DCSUM)], vals, b.length == 0, kind, mode)
        _put_words(hdr, hat + DCSUM, w[0])
        _put_words(hdr, hat + HCSUM, w[1])
    ranges = [(0, DCSUM), (DCSUM, HCSUM), (HCSUM, HDR)]
    nh = 0
    for i in np.nonzero(np.isin(cls, (1, 3, 7)))[0]:
        c = int(b.length[i])
        if cls[i] in (1, 7):
            flip_bit(hdr, int(hat[i]), rng, *ranges[nh % 3])
            nh += 1
        if cls[i] in (3, 7) and c:
            pay[b.poffs[i] + (c - 1 if i % 20 == 3 else int(rng.integers(0, c)))] ^= np.uint8(0x10)


def recv_want(oracle, b, pay, hdr, hat, kind, mode):
    """The receive step's model over the bytes as they are: expect() on the concatenated packed views of the
    messages' buffers, mapped back per message.  Returns (expect()'s tuple, [the expected buffer of each message])."""
    starts = np.concatenate(([0], np.cumsum([m.total for m in b.msgs]))).astype(np.int64)
    app = np.concatenate([m.hbuf[m.idx] for m in b.msgs] + [np.zeros(1, np.uint8)])
    aoffs, alens = np.zeros(b.n, np.uint64), np.zeros(b.n, np.int64)
    for i in np.nonzero(b.valid)[0]:
        m = b.msgs[b.msg[i]]
        room = m.total - int(b.pack_off[i])
        if room > 0:
            aoffs[i], alens[i] = starts[b.msg[i]] + int(b.pack_off[i]), room
    H = hdr[np.asarray(hat)[:, None] + np.arange(HDR)]
    want = expect(oracle, pay, b.poffs.astype(np.uint64), b.length.astype(np.uint64), H, b.valid, app, aoffs, alens,
                  kind, mode)
    bufs = []
    for k, m in enumerate(b.msgs):
        w = m.hbuf.copy()
        w[m.idx] = app[starts[k]:starts[k + 1]]
        bufs.append(w)
    return want, bufs
