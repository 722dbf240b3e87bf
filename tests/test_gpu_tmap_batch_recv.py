"""GPU parity of the descriptor form of the typemap receive step (lampi_tmap_recv_unpack_batch) against
tests/tmap_batch_model.py.

The batches are tests/test_gpu_tmap_batch_send.py's -- seven messages, records grouped by message and round-robin
across them, the four max_len classes -- as drained fragments with faults of every class of
tests/test_gpu_tmap_recv.py: header bits in [0, 64), in the word @64 and in the word @68; payload bytes, the last one
included; a consistent header with a wrong dataChecksum; a delivery clipped by app_len; pack_off >= app_len.
d_copied, d_csum, both masks (no stray bits) and both counts must be exact and every message's buffer is compared
whole: the gaps between the pieces and the pieces of dropped fragments keep their sentinel.  The header and payload
tensors must be unchanged.
"""
import numpy as np
import pytest

import tmap_batch_model as tbm
import tmap_model as tmm
from recv_unpack_model import check
from test_gpu_send_pack import CRC, GM, HDR, IB, NONE, SUM
from test_gpu_tmap_batch_send import INVALID, KIND_MODE, Device

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A


def _dv():
    from lampi_amd import device as dv

    return dv


def run_recv(oracle, d, kind, mode, rng, what, hdrs=True):
    """Fill the batch's payloads and headers with faults, run the call, compare everything with the model."""
    import torch

    b = d.b
    pay, hdr = d.pay0.copy(), d.hdr0.copy()
    tbm.recv_fill(oracle, rng, b, pay, hdr, b.hat, kind, mode)
    d.load(pay, hdr)
    for t, m in zip(d.bufs, b.msgs):
        t.copy_(torch.from_numpy(m.hbuf).to(d.cuda))
    want, bufs = tbm.recv_want(oracle, b, pay, hdr, b.hat, kind, mode)
    got = _dv().tmap_recv_unpack_batch(d.frags, d.msgs, b.max_len, d.hdr if hdrs else None, tbm.HDR_STRIDE,
                                       offset=tbm.HDR_OFF, kind=kind, mode=mode)
    check(got, want, b.n, d.bufs[0], bufs[0], b.msgs[0].tm.extent, what)
    for k in range(1, len(bufs)):
        assert np.array_equal(d.bufs[k].cpu().numpy(), bufs[k]), (what, "buffer", k)
    assert np.array_equal(d.pay.cpu().numpy(), pay), (what, "payloads changed")
    assert np.array_equal(d.hdr.cpu().numpy(), hdr), (what, "headers changed")
    return want


@KIND_MODE
@pytest.mark.parametrize("order", ["grouped", "robin"])
@pytest.mark.parametrize("max_len", tbm.MAX_LENS)
def test_outputs_and_buffers(cuda, oracle, max_len, order, kind, mode):
    b = tbm.plan(max_len, order, True, seed=4000 + max_len % 89)
    d = Device(cuda, b, seed=4100)
    copied, _, hbad, dbad = run_recv(oracle, d, kind, mode, np.random.default_rng(4200 + mode), f"{max_len} {order}")
    # the model's verdicts hold every class
    assert int(hbad.sum()) >= (0 if mode == NONE else 3)          # (one per place of the flipped header bit)
    assert int(dbad.sum()) >= (0 if mode == NONE else 2)          # (a payload byte; a wrong dataChecksum)
    assert np.any((copied > 0) & (copied < b.length))             # clipped by app_len
    assert np.any((copied == 0) & (b.length > 0))                 # pack_off >= app_len
    assert np.any(copied == b.length)


@pytest.mark.parametrize("kind", [GM, IB], ids=["gm", "ib"])
def test_checksumming_off_reads_no_header(cuda, oracle, kind):
    b = tbm.plan(9000, "robin", True, seed=4300)
    run_recv(oracle, Device(cuda, b, seed=4301), kind, NONE, np.random.default_rng(4302), "no headers", hdrs=False)


@KIND_MODE
def test_invalid_records_are_dropped(cuda, oracle, kind, mode):
    """One record of each invalid kind in an otherwise good round-robin batch (msg == nmsgs, length == max_len + 1,
    an entry with packed_size == 0, one with num_pairs == 0): dropped as a failed header in every mode, nothing of
    theirs read or delivered; every other fragment exact."""
    max_len = 9000
    g = tbm.plan(max_len, "robin", True, seed=4400)
    n0, nm = g.n, len(g.msgs)
    bad = [(nm + 2, 0, 100), (0, 0, max_len + 1), (nm, 0, 100), (nm + 1, 0, 100)]
    at = [1, 6, 11, n0 + 3]
    msg, off, ln, valid = list(g.msg), list(g.pack_off), list(g.length), [True] * n0
    for p, (m, o, c) in zip(at, bad):
        msg.insert(p, m), off.insert(p, o), ln.insert(p, c), valid.insert(p, False)
    b = tbm.Batch(g.msgs, msg, off, ln, max_len, nmsgs=nm + 2)
    b.valid = np.array(valid)
    d = Device(cuda, b, seed=4401, extra_entries=[(2, 0, 0), (4, 0, ~0xFFFFFFFF)])
    copied, csum, hbad, _ = run_recv(oracle, d, kind, mode, np.random.default_rng(4402), "invalid records")
    assert np.all(copied[~b.valid] == -2) and np.all(csum[~b.valid] == 0) and np.all(hbad[~b.valid])


@KIND_MODE
def test_single_message_equals_tmap_recv_unpack(cuda, oracle, kind, mode):
    """On the ring lampi_tmap_send_pack wrote (one message, consecutive fragments, two payload bytes then flipped),
    the batch form gives lampi_tmap_recv_unpack's outputs and buffer."""
    import torch

    dv = _dv()
    for tm, L, nf, last in ((tmm.T2, 1976, 23, 17), (tmm.T3, 65456, 4, 1), (tmm.T4B, 4096, 9, None)):
        stride = (HDR + L + 15) // 8 * 8
        plen = tmm.window_len(L, nf, last)
        src = tbm.Message(tm, tmm.count_for(tm, plen), 4500)
        sbuf = torch.from_numpy(src.hbuf).to(cuda)
        dtm = dv.make_tmap(tm.pairs(), tm.extent, src.count, cuda)
        ring = torch.empty(nf * stride, dtype=torch.uint8, device=cuda)
        dv.fill_stream(ring, seed=4501)
        tmpl = np.random.default_rng(4502).integers(0, 256, size=HDR, dtype=np.uint8)
        seq0 = 0x0000000100000010
        dv.tmap_send_pack(sbuf, dtm, L, ring, stride, tmpl, kind=kind, mode=mode, pack_len=plen, base_offset=src.origin,
                          seq_offset0=seq0)
        ring[HDR + 5] ^= 0x20
        ring[(nf - 1) * stride + HDR + (last or L) - 1] ^= 0x01
        # posted short by two elements: the last fragment is clipped or beyond
        dst = tbm.Message(tm, max(1, src.count - 2), 4503)
        rtm = dv.make_tmap(tm.pairs(), tm.extent, dst.count, cuda)
        dbuf = torch.from_numpy(dst.hbuf).to(cuda)
        theirs = dv.tmap_recv_unpack(ring, nf, stride, dbuf, rtm, kind=kind, mode=mode, seq_offset0=seq0,
                                     base_offset=dst.origin)
        their_buf = dbuf.clone()
        dbuf.copy_(torch.from_numpy(dst.hbuf).to(cuda))
        k = np.arange(nf, dtype=np.int64)
        frags = dv.make_tmap_frags(ring.data_ptr() + k * stride + HDR, k * L, np.minimum(L, plen - k * L),
                                   np.zeros(nf, np.int64), cuda)
        msgs = dv.make_tmap_msgs([(rtm, dbuf, dst.origin)], cuda)
        mine = dv.tmap_recv_unpack_batch(frags, msgs, L, ring, stride, kind=kind, mode=mode)
        torch.cuda.synchronize()
        for a, c in zip(mine, theirs):
            assert torch.equal(a, c), (tm.name, L)
        assert torch.equal(dbuf, their_buf), (tm.name, L)
        if mode != NONE:
            assert int(theirs[4][1]) >= 1                          # (the flipped payload bytes were noticed)


def test_refusals_write_nothing(cuda, oracle):
    """Every host-checked refusal returns hipErrorInvalidValue and leaves the outputs, headers and buffers at their
    sentinel; n == 0 returns 0 with both counts zeroed."""
    import torch

    from lampi_amd import lib

    b = tbm.plan(4096, "grouped", True, seed=4600)
    d = Device(cuda, b, seed=4601)
    pay, hdr = d.pay0.copy(), d.hdr0.copy()
    tbm.recv_fill(oracle, np.random.default_rng(4602), b, pay, hdr, b.hat, GM, CRC, faults=False)
    d.load(pay, hdr)
    f = lib().lampi_tmap_recv_unpack_batch
    outs = [torch.full((2 * b.n,), SENT, dtype=torch.int32, device=cuda) for _ in range(5)]
    copied, csum, hm, dm, nbad = [o.data_ptr() for o in outs]
    hp = d.hdr.data_ptr() + tbm.HDR_OFF

    def call(frags=d.frags.data_ptr(), n=b.n, msgs=d.msgs.table.data_ptr(), nmsgs=len(d.msgs), max_len=4096, hdrs=hp,
             stride=tbm.HDR_STRIDE, kind=GM, cp=copied, cs=csum, h=hm, dd=dm, nb=nbad, mode=CRC):
        return f(frags, n, msgs, nmsgs, max_len, hdrs, stride, kind, cp, cs, h, dd, nb, mode, None)

    assert call(frags=None) == INVALID
    assert call(msgs=None) == INVALID
    assert call(nmsgs=0) == INVALID
    assert call(nmsgs=1 << 32) == INVALID
    assert call(n=1 << 32) == INVALID
    for kind in (2, 3, -1):                                        # Quadrics (3) is refused
        assert call(kind=kind) == INVALID
    for mode in (3, -1, CRC | 0x100, SUM | (4 << 16)):
        assert call(mode=mode) == INVALID
    assert call(stride=68) == INVALID
    assert call(stride=tbm.HDR_STRIDE + 2) == INVALID
    assert call(hdrs=hp + 2) == INVALID
    assert call(hdrs=None) == INVALID
    assert call(hdrs=None, mode=SUM) == INVALID
    for kw in (dict(cp=None), dict(cs=None), dict(h=None), dict(dd=None), dict(nb=None)):
        assert call(**kw) == INVALID
    torch.cuda.synchronize()

    def untouched():
        return (all(np.array_equal(t.cpu().numpy(), m.hbuf) for t, m in zip(d.bufs, b.msgs))
                and np.array_equal(d.pay.cpu().numpy(), pay) and np.array_equal(d.hdr.cpu().numpy(), hdr))

    assert untouched()
    for o in outs:
        assert bool((o == SENT).all())
    assert call(n=0) == 0                                          # no fragments: both counts zeroed, nothing else
    torch.cuda.synchronize()
    assert [int(x) for x in outs[4][:2].cpu()] == [0, 0] and bool((outs[4][2:] == SENT).all())
    for o in outs[:4]:
        assert bool((o == SENT).all())
    assert untouched()
    assert call() == 0                                             # the same arguments unaltered pass
    torch.cuda.synchronize()
    assert [int(x) for x in outs[4][:2].cpu()] == [0, 0]
