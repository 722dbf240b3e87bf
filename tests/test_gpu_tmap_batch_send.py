"""GPU parity of the descriptor form of the typemap send step (lampi_tmap_send_pack_batch) against
tests/tmap_batch_model.py.

One batch holds the fragments of seven messages -- T1, T2 (a negative offset), T3 (pieces longer than a row), S63 and
S65 (either side of the LDS cut), T4b (5,000 pairs, read through L2), T5 (contiguous) --, about twelve each, of 0 to
max_len bytes, as records grouped by message (a workgroup's four items on one typemap: the staged path) and
round-robin across the messages (four typemaps in every workgroup).  The payload tensor and the header tensor are
compared whole: payloads, the words @64 / @68, and the sentinel bytes everywhere else; the sources must be unchanged.
"""
import numpy as np
import pytest

import tmap_batch_model as tbm
import tmap_model as tmm
from test_gpu_send_pack import CRC, DCSUM, GM, HDR, IB, NONE, SUM

pytestmark = pytest.mark.gpu

KIND_MODE = pytest.mark.parametrize("kind,mode", [(k, m) for k in (GM, IB) for m in (CRC, SUM, NONE)])
INVALID = 1  # hipErrorInvalidValue
FILL = dict(frag_seq0=2**64 - 2, frag_seq_step=3, desc_ptr0=0x00007F0012345000, desc_ptr_stride=0x1A8,
            seq_offset0=0x0000000100000010)


def _dv():
    from lampi_amd import device as dv

    return dv


class Device:
    """A batch on the device: the messages' buffers, the message table, the payload and header tensors (sentinel
    bytes: the synthetic stream) and the records."""

    def __init__(self, cuda, b, seed, extra_entries=()):
        import torch

        dv = _dv()
        self.b, self.cuda = b, cuda
        self.bufs = [torch.from_numpy(m.hbuf).to(cuda) for m in b.msgs]
        self.tmaps = [dv.make_tmap(m.tm.pairs(), m.tm.extent, m.count, cuda) for m in b.msgs]
        self.msgs = dv.make_tmap_msgs([(t, buf, m.origin) for t, buf, m in zip(self.tmaps, self.bufs, b.msgs)], cuda)
        if extra_entries:  # copies of entry 0 with fields changed: (column of the int64 [nmsgs, 8] table, value)
            rows = [self.msgs.table[0].clone() for _ in extra_entries]
            for row, (col, val, mask) in zip(rows, extra_entries):
                row[col] = (int(row[col]) & mask) | val
            self.msgs.table = torch.cat([self.msgs.table] + [r[None] for r in rows])
        self.pay = torch.empty(b.pay_size, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.pay, seed=seed)
        self.hdr = torch.empty(tbm.HDR_OFF + b.n * tbm.HDR_STRIDE + 8, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.hdr, seed=seed + 1)
        self.pay0, self.hdr0 = self.pay.cpu().numpy(), self.hdr.cpu().numpy()
        self.frags = dv.make_tmap_frags(self.pay.data_ptr() + b.poffs, b.pack_off, b.length, b.msg, cuda)

    def load(self, pay, hdr):
        import torch

        self.pay.copy_(torch.from_numpy(pay).to(self.cuda))
        self.hdr.copy_(torch.from_numpy(hdr).to(self.cuda))

    def sources_unchanged(self):
        return all(np.array_equal(t.cpu().numpy(), m.hbuf) for t, m in zip(self.bufs, self.b.msgs))


def _first(got, want):
    i = int(np.nonzero(got != want)[0][0])
    return i, int(got[i]), int(want[i])


def check_send(oracle, d, kind, mode, what):
    import torch

    b = d.b
    d.load(d.pay0, d.hdr0)
    _dv().tmap_send_pack_batch(d.frags, d.msgs, b.max_len, d.hdr, tbm.HDR_STRIDE, offset=tbm.HDR_OFF, kind=kind,
                               mode=mode)
    torch.cuda.synchronize()
    pay, hdr = d.pay0.copy(), d.hdr0.copy()
    tbm.send_want(oracle, b, pay, hdr, b.hat, kind, mode)
    got_p, got_h = d.pay.cpu().numpy(), d.hdr.cpu().numpy()
    if not np.array_equal(got_h, hdr):
        i, g, w = _first(got_h, hdr)
        pytest.fail(f"{what}: header {(i - tbm.HDR_OFF) // tbm.HDR_STRIDE} byte {(i - tbm.HDR_OFF) % tbm.HDR_STRIDE}: "
                    f"{g} != {w}")
    if not np.array_equal(got_p, pay):
        i, g, w = _first(got_p, pay)
        f = int(np.searchsorted(np.sort(b.poffs), i, side="right")) - 1
        pytest.fail(f"{what}: payload byte {i} (record at sorted position {f}): {g} != {w}")
    assert d.sources_unchanged(), (what, "source changed")


@KIND_MODE
@pytest.mark.parametrize("order", ["grouped", "robin"])
@pytest.mark.parametrize("max_len", tbm.MAX_LENS)
def test_payloads_and_headers_byte_for_byte(cuda, oracle, max_len, order, kind, mode):
    b = tbm.plan(max_len, order, False, seed=3000 + max_len % 89)
    check_send(oracle, Device(cuda, b, seed=3100), kind, mode, f"max_len {max_len} {order}")


@KIND_MODE
def test_invalid_records_are_skipped(cuda, oracle, kind, mode):
    """One record of each invalid kind in an otherwise good round-robin batch: msg == nmsgs, length == max_len + 1,
    an entry with packed_size == 0, one with num_pairs == 0, a window one byte past its message.  Their payload
    addresses and their entries' bases point inside the test's tensors; nothing of theirs is written."""
    max_len = 9000
    g = tbm.plan(max_len, "robin", False, seed=3200)
    n0, nm = g.n, len(g.msgs)
    m0 = g.msgs[0]
    bad = [(nm + 2, 0, 100), (0, 0, max_len + 1), (nm, 0, 100), (nm + 1, 0, 100), (0, m0.total - 99, 100)]
    at = [1, 6, 11, 16, n0 + 4]                                    # positions in the new batch
    msg, off, ln, valid = list(g.msg), list(g.pack_off), list(g.length), [True] * n0
    for p, (m, o, c) in zip(at, bad):
        msg.insert(p, m), off.insert(p, o), ln.insert(p, c), valid.insert(p, False)
    b = tbm.Batch(g.msgs, msg, off, ln, max_len, nmsgs=nm + 2)
    b.valid = np.array(valid)
    # entry nm: packed_size (word 2) zero; entry nm + 1: num_pairs (the low half of word 4) zero
    d = Device(cuda, b, seed=3300, extra_entries=[(2, 0, 0), (4, 0, ~0xFFFFFFFF)])
    assert len(d.msgs) == nm + 2
    check_send(oracle, d, kind, mode, "invalid records")


@KIND_MODE
def test_single_message_equals_tmap_send_pack(cuda, oracle, kind, mode):
    """One message, consecutive fragments: the ring lampi_tmap_send_pack leaves, byte for byte -- bytes [0, 64) of
    each header taken from that ring (GM with checksumming off: the whole header, the batch form writes no word of
    it there)."""
    import torch

    dv = _dv()
    for tm, L, nf, last in ((tmm.T2, 1976, 23, 17), (tmm.T3, 65456, 4, 1), (tmm.T4B, 4096, 9, None)):
        stride = (HDR + L + 15) // 8 * 8
        pack_off = tmm.pack_offsets(tm)[1]
        plen = tmm.window_len(L, nf, last)
        m = tbm.Message(tm, tmm.count_for(tm, pack_off + plen) + 1, 3400)
        k = np.arange(nf, dtype=np.int64)
        b = tbm.Batch([m], np.zeros(nf, np.int64), pack_off + k * L, np.minimum(L, plen - k * L), L,
                      poffs=k * stride + HDR)
        buf = torch.from_numpy(m.hbuf).to(cuda)
        dtm = dv.make_tmap(tm.pairs(), tm.extent, m.count, cuda)
        ring = torch.empty(nf * stride, dtype=torch.uint8, device=cuda)
        dv.fill_stream(ring, seed=3401)
        before = ring.clone()
        tmpl = np.random.default_rng(3402).integers(0, 256, size=HDR, dtype=np.uint8)
        dv.tmap_send_pack(buf, dtm, L, ring, stride, tmpl, kind=kind, mode=mode, pack_off=pack_off, pack_len=plen,
                          base_offset=m.origin, **FILL)
        theirs = ring.clone()
        keep = HDR if (kind == GM and mode == NONE) else DCSUM
        ring.copy_(before)
        ring.view(nf, stride)[:, :keep] = theirs.view(nf, stride)[:, :keep]
        msgs = dv.make_tmap_msgs([(dtm, buf, m.origin)], cuda)
        frags = dv.make_tmap_frags(ring.data_ptr() + b.poffs, b.pack_off, b.length, b.msg, cuda)
        dv.tmap_send_pack_batch(frags, msgs, L, ring, stride, kind=kind, mode=mode)
        torch.cuda.synchronize()
        assert torch.equal(ring, theirs), (tm.name, L)


def test_refusals_write_nothing(cuda, oracle):
    """Every host-checked refusal returns hipErrorInvalidValue and leaves the payloads and headers at their sentinel;
    n == 0 returns 0."""
    import torch

    from lampi_amd import lib

    b = tbm.plan(4096, "grouped", False, seed=3500)
    d = Device(cuda, b, seed=3501)
    f = lib().lampi_tmap_send_pack_batch
    hp = d.hdr.data_ptr() + tbm.HDR_OFF

    def call(frags=d.frags.data_ptr(), n=b.n, msgs=d.msgs.table.data_ptr(), nmsgs=len(d.msgs), max_len=4096, hdrs=hp,
             stride=tbm.HDR_STRIDE, kind=GM, mode=CRC):
        return f(frags, n, msgs, nmsgs, max_len, hdrs, stride, kind, mode, None)

    assert call(frags=None) == INVALID
    assert call(msgs=None) == INVALID
    assert call(nmsgs=0) == INVALID
    assert call(nmsgs=1 << 32) == INVALID
    assert call(n=1 << 32) == INVALID
    for kind in (2, 3, -1):                                        # Quadrics (3) is refused
        assert call(kind=kind) == INVALID
    for mode in (3, -1, CRC | 0x100, SUM | (4 << 16)):             # no BY_BYTES, no hint bits
        assert call(mode=mode) == INVALID
    assert call(stride=68) == INVALID
    assert call(stride=tbm.HDR_STRIDE + 2) == INVALID
    assert call(hdrs=hp + 2) == INVALID
    assert call(hdrs=None) == INVALID
    assert call(hdrs=None, mode=NONE, kind=IB) == INVALID          # only GM with checksumming off needs no headers
    torch.cuda.synchronize()
    assert np.array_equal(d.pay.cpu().numpy(), d.pay0) and np.array_equal(d.hdr.cpu().numpy(), d.hdr0)
    assert call(n=0) == 0
    assert call(n=0, frags=None, msgs=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.pay.cpu().numpy(), d.pay0) and np.array_equal(d.hdr.cpu().numpy(), d.hdr0)
    # GM with checksumming off: no header word is written, the headers may be absent
    _dv().tmap_send_pack_batch(d.frags, d.msgs, 4096, None, tbm.HDR_STRIDE, kind=GM, mode=NONE)
    torch.cuda.synchronize()
    pay, hdr = d.pay0.copy(), d.hdr0.copy()
    tbm.send_want(oracle, b, pay, hdr, b.hat, GM, NONE)
    assert np.array_equal(d.pay.cpu().numpy(), pay) and np.array_equal(d.hdr.cpu().numpy(), d.hdr0)
    with pytest.raises(ValueError):                                # the binding checks what the pieces reach
        _dv().make_tmap_msgs([(d.tmaps[1], d.bufs[1], 0)], cuda)
