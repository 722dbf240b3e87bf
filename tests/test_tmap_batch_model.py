"""CPU: the batch model of the descriptor forms of the typemap steps (tests/tmap_batch_model.py) against the
per-message compositions the typemap forms' tests already use.

Run on one message with consecutive fragments it must give what tests/test_gpu_tmap_recv.py composes -- expect_ring
over the packed view of the buffer, mapped back through the address rule -- and, on the send side, the ring
tests/test_gpu_tmap_send.py composes from tmm.packed and the flavour table (_msg_want, _stamp_all).  The batches the
GPU tests run are checked for the shapes they promise.
"""
import numpy as np
import pytest

import tmap_batch_model as tbm
import tmap_model as tmm
from recv_unpack_model import expect_ring, flip_bit, pack_slots
from test_gpu_send_pack import CRC, DCSUM, GM, HCSUM, HDR, IB, NONE, SUM, _msg_want

FILL = dict(frag_seq0=2**64 - 2, frag_seq_step=3, desc_ptr0=0x00007F0012345000, desc_ptr_stride=0x1A8,
            seq_offset0=0x0000000100000010)
CASES = [(tmm.T2, 1976, 23), (tmm.T3, 4096, 9), (tmm.T4A, 100, 60)]


@pytest.mark.parametrize("kind,mode", [(k, m) for k in (GM, IB) for m in (CRC, SUM, NONE)])
@pytest.mark.parametrize("tm,L,nf", CASES, ids=[c[0].name for c in CASES])
def test_receive_equals_the_ring_composition(oracle, tm, L, nf, kind, mode):
    rng = np.random.default_rng(2100 + mode)
    stride = (HDR + L + 15) // 8 * 8
    mlen = (nf - 1) * L + 17
    # posted short: app_len ends inside a fragment that carries no fault below, later fragments lie beyond it
    count = max(c for c in range(1, (nf - 2) * L // tm.packed_size + 1)
                if c * tm.packed_size % L and c * tm.packed_size // L % 5 in (0, 2, 4))
    msg = tbm.Message(tm, count, 2110)
    hring = rng.integers(0, 256, size=nf * stride, dtype=np.uint8)
    sender = rng.integers(0, 256, size=mlen, dtype=np.uint8)
    seq0 = 2**64 - 4096 * 3 - 5
    n, _ = pack_slots(oracle, rng, hring, sender, L, stride, seq0, kind, mode)
    assert n == nf
    for k in range(n):                                             # faults: a header bit, a payload byte
        if k % 5 == 1:
            flip_bit(hring, k * stride, rng, 0, 20)                  # (not the length: the records carry it)
        if k % 5 == 3:
            hring[k * stride + HDR + (k % 17)] ^= np.uint8(4)
    # the existing composition: the ring form over the packed view, mapped back through the address rule
    app = msg.hbuf[msg.idx]
    want_ring = expect_ring(oracle, hring, n, stride, app, msg.total, seq0, kind, mode)
    want_buf = msg.hbuf.copy()
    want_buf[msg.idx] = app
    # the batch model: the same fragments as records
    k = np.arange(n, dtype=np.int64)
    lens = np.minimum(L, mlen - k * L)
    b = tbm.Batch([msg], np.zeros(n, np.int64), k * L, lens, L, poffs=k * stride + HDR)
    want, bufs = tbm.recv_want(oracle, b, hring, hring, k * stride, kind, mode)
    for a, c in zip(want, want_ring):
        assert np.array_equal(a, c)
    assert np.array_equal(bufs[0], want_buf)
    copied = want[0]
    assert np.any((copied > 0) & (copied < lens)) and np.any((copied == 0) & (lens > 0))
    if mode != NONE:
        assert np.any(copied == -2) and np.any(copied == -1)


@pytest.mark.parametrize("kind,mode", [(k, m) for k in (GM, IB) for m in (CRC, SUM, NONE)])
@pytest.mark.parametrize("tm,L,nf", CASES, ids=[c[0].name for c in CASES])
def test_send_equals_the_ring_composition(oracle, tm, L, nf, kind, mode):
    rng = np.random.default_rng(2200 + mode)
    stride = (HDR + L + 15) // 8 * 8
    pack_off = tmm.pack_offsets(tm)[1]
    plen = (nf - 1) * L + 15
    msg = tbm.Message(tm, tmm.count_for(tm, pack_off + plen) + 1, 2210)
    before = rng.integers(0, 256, size=nf * stride, dtype=np.uint8)
    tmpl = rng.integers(0, 256, size=HDR, dtype=np.uint8)
    ring = before.copy()                                            # tests/test_gpu_tmap_send.py: _Send.want
    _msg_want(oracle, ring, tmm.packed(tm, msg.hbuf, msg.origin, pack_off, plen), kind, L, stride, plen, tmpl, FILL, mode)
    k = np.arange(nf, dtype=np.int64)
    lens = np.minimum(L, plen - k * L)
    mine = before.copy().reshape(nf, stride)
    # the caller's part: bytes [0, 64) of every header (GM with checksumming off writes no header word at all, so
    # there the whole header is the caller's)
    keep = HDR if (kind == GM and mode == NONE) else DCSUM
    mine[:, :keep] = ring.reshape(nf, stride)[:, :keep]
    mine = mine.reshape(-1)
    b = tbm.Batch([msg], np.zeros(nf, np.int64), pack_off + k * L, lens, L, poffs=k * stride + HDR)
    tbm.send_want(oracle, b, mine, mine, k * stride, kind, mode)
    assert np.array_equal(mine, ring)


@pytest.mark.parametrize("recv", [False, True], ids=["send", "recv"])
@pytest.mark.parametrize("max_len", tbm.MAX_LENS)
def test_planned_batches_have_the_promised_shapes(max_len, recv):
    g, r = tbm.plan(max_len, "grouped", recv, 7), tbm.plan(max_len, "robin", recv, 7)
    assert g.n == r.n == 12 * len(tbm.BATCH_TYPEMAPS)
    assert int(g.length.max()) == max_len and set(tbm.BASE_LENS) & set(g.length.tolist()) >= \
        {x for x in tbm.BASE_LENS if x <= max_len}
    assert sorted(zip(g.msg, g.pack_off, g.length)) == sorted(zip(r.msg, r.pack_off, r.length))
    # grouped: the four items of a workgroup name one message wherever R >= 4 or the message's run is long enough;
    # round-robin: four consecutive records always name four messages
    assert all(len(set(r.msg[i:i + 4])) == 4 for i in range(0, r.n - 3))
    assert all(len(set(g.msg[i:i + 12])) == 1 for i in range(0, g.n, 12))
    if max_len > 65456:                                            # one or two long fragments among short ones
        assert int((g.length == max_len).sum()) == 2
    for k, m in enumerate(g.msgs):
        sel = g.msg == k
        ends = g.pack_off[sel] + g.length[sel]
        assert int(g.pack_off[sel].min()) == tbm.window_starts(m.tm)[k % 3]
        if recv and k in tbm.CLIPPED_MSGS:
            assert np.any((g.pack_off[sel] < m.total) & (ends > m.total)) or np.any(g.pack_off[sel] >= m.total)
        else:
            assert int(ends.max()) <= m.total
        o = np.argsort(g.pack_off[sel], kind="stable")
        assert np.all(ends[o][:-1] <= g.pack_off[sel][o][1:])     # no two fragments overlap
