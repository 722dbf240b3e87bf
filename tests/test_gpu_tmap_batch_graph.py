"""The descriptor forms of the typemap steps in a captured graph: two round trips between datatypes of equal packed
length (T2 x 8,001 -> T3 x 65 and T3 x 65 -> T2 x 8,001, as tests/test_gpu_tmap_graph.py), their fragments as records
in round-robin order, sent by one lampi_tmap_send_pack_batch and received by one lampi_tmap_recv_unpack_batch on one
stream.  While a stream is being captured a call's scratch is a buffer of its own, so a replay must not depend on a
pooled buffer a later eager call replaced, and it must read the sources as they are at replay time.  Expectations
come from tests/tmap_batch_model.py alone."""
import numpy as np
import pytest

import tmap_batch_model as tbm
import tmap_model as tmm
from test_gpu_send_pack import CRC, DCSUM, GM, HDR, IB, SUM

pytestmark = pytest.mark.gpu

COUNT2, COUNT3 = tmm.T3.packed_size, tmm.T2.packed_size  # 520,065 packed bytes either way
TOTAL = COUNT2 * tmm.T2.packed_size
L = 65456
STRIDE = (HDR + L + 15) // 8 * 8


class _Trips:
    def __init__(self, cuda, seed):
        import torch

        from lampi_amd import device as dv

        self.cuda = cuda
        nf = (TOTAL + L - 1) // L
        j = np.repeat(np.arange(nf, dtype=np.int64), 2)
        msg = np.tile(np.array([0, 1], np.int64), nf)               # round-robin: A, B, A, B, ...
        self.n = 2 * nf
        self.rec = (msg, j * L, np.minimum(L, TOTAL - j * L), np.arange(self.n, dtype=np.int64) * STRIDE + HDR)
        self.hat = np.arange(self.n, dtype=np.int64) * STRIDE
        self.src = [tbm.Message(tmm.T2, COUNT2, seed), tbm.Message(tmm.T3, COUNT3, seed + 1)]
        self.dst = [tbm.Message(tmm.T3, COUNT3, seed + 2), tbm.Message(tmm.T2, COUNT2, seed + 3)]
        self.ring = torch.empty(self.n * STRIDE, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.ring, seed=seed + 4)
        self.ring0 = self.ring.cpu().numpy()
        self.ring0_t = self.ring.clone()
        self.sbuf = [torch.from_numpy(m.hbuf).to(cuda) for m in self.src]
        self.dbuf = [torch.from_numpy(m.hbuf).to(cuda) for m in self.dst]
        self.tmaps = [dv.make_tmap(m.tm.pairs(), m.tm.extent, m.count, cuda) for m in self.src + self.dst]
        self.smsgs = dv.make_tmap_msgs([(self.tmaps[k], self.sbuf[k], self.src[k].origin) for k in range(2)], cuda)
        self.dmsgs = dv.make_tmap_msgs([(self.tmaps[2 + k], self.dbuf[k], self.dst[k].origin) for k in range(2)], cuda)
        self.frags = dv.make_tmap_frags(self.ring.data_ptr() + self.rec[3], self.rec[1], self.rec[2], msg, cuda)

    def batch(self, msgs):
        return tbm.Batch(msgs, self.rec[0], self.rec[1], self.rec[2], L, poffs=self.rec[3])

    def run(self, kind, mode):
        from lampi_amd import device as dv

        dv.tmap_send_pack_batch(self.frags, self.smsgs, L, self.ring, STRIDE, kind=kind, mode=mode)
        return dv.tmap_recv_unpack_batch(self.frags, self.dmsgs, L, self.ring, STRIDE, kind=kind, mode=mode)

    def new_source(self, seed):
        import torch

        self.src = [tbm.Message(m.tm, m.count, seed + k) for k, m in enumerate(self.src)]
        for t, m in zip(self.sbuf, self.src):
            t.copy_(torch.from_numpy(m.hbuf).to(self.cuda))

    def reset(self):
        import torch

        self.ring.copy_(self.ring0_t)
        for t, m in zip(self.dbuf, self.dst):
            t.copy_(torch.from_numpy(m.hbuf).to(self.cuda))

    def check(self, oracle, got, kind, mode, what):
        import torch

        from lampi_amd import device as dv

        torch.cuda.synchronize()
        copied, csum, hmask, dmask, nbad = got
        ring = self.ring0.copy()
        tbm.send_want(oracle, self.batch(self.src), ring, ring, self.hat, kind, mode)
        assert np.array_equal(self.ring.cpu().numpy(), ring), (what, "ring")
        want, bufs = tbm.recv_want(oracle, self.batch(self.dst), ring, ring, self.hat, kind, mode)
        assert [int(x) for x in nbad.cpu()] == [0, 0], what
        assert not dv.mask_bits(hmask, self.n).any() and not dv.mask_bits(dmask, self.n).any(), what
        assert np.array_equal(copied.cpu().numpy(), want[0]) and np.array_equal(want[0], self.rec[2]), what
        assert np.array_equal(dv.as_u32(csum), want[1]), (what, "csum")
        stored = ring.reshape(self.n, STRIDE)[:, DCSUM:DCSUM + 4].copy().view("<u4").reshape(self.n)
        assert np.array_equal(want[1], stored), (what, "model")
        for k in range(2):
            assert np.array_equal(self.dbuf[k].cpu().numpy(), bufs[k]), (what, "destination", k)
            assert np.array_equal(self.sbuf[k].cpu().numpy(), self.src[k].hbuf), (what, "source", k)


@pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
def test_graph_replay_results(cuda, oracle, mode):
    """Both calls captured into one graph on one stream after a warm-up on a side stream; then eager calls of another
    shape on the default stream that regrow both pooled buffers; then new source bytes in place and two replays, each
    compared with the models."""
    import torch

    from lampi_amd import device as dv

    t = _Trips(cuda, seed=5000 + mode)
    out = {}

    def run():
        out["recv"] = t.run(GM, mode)

    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    t.check(oracle, out["recv"], GM, mode, "warm-up")
    t.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    # eager, another shape: 7,000 records of 100 bytes in frames of 40 rows both ways -- 21,000 words of records and
    # values (more than the 64 KiB the second pooled buffer starts with) and 280,000 row words (more than the first
    # one's 1 MiB)
    n2, max2 = 7000, 160000
    m = tbm.Message(tmm.T1, tmm.count_for(tmm.T1, n2 * 100), 5100)
    k = np.arange(n2, dtype=np.int64)
    b = tbm.Batch([m], np.zeros(n2, np.int64), k * 100, np.full(n2, 100), max2, poffs=k * 176 + HDR)
    ring2 = torch.empty(n2 * 176, dtype=torch.uint8, device=cuda)
    dv.fill_stream(ring2, seed=5101)
    want2 = ring2.cpu().numpy()
    buf2 = torch.from_numpy(m.hbuf).to(cuda)
    tm2 = dv.make_tmap(m.tm.pairs(), m.tm.extent, m.count, cuda)
    msgs2 = dv.make_tmap_msgs([(tm2, buf2, m.origin)], cuda)
    frags2 = dv.make_tmap_frags(ring2.data_ptr() + b.poffs, b.pack_off, b.length, b.msg, cuda)
    dv.tmap_send_pack_batch(frags2, msgs2, max2, ring2, 176, kind=IB, mode=mode)
    got2 = dv.tmap_recv_unpack_batch(frags2, msgs2, max2, ring2, 176, kind=IB, mode=mode)
    torch.cuda.synchronize()
    tbm.send_want(oracle, b, want2, want2, k * 176, IB, mode)
    assert np.array_equal(ring2.cpu().numpy(), want2), "eager send"
    assert [int(x) for x in got2[4].cpu()] == [0, 0] and bool((got2[0] == 100).all())
    assert np.array_equal(buf2.cpu().numpy(), m.hbuf)              # (delivered onto itself: unchanged)
    for i in range(2):
        t.new_source(5200 + 10 * i)
        t.reset()
        for x in out["recv"]:
            x.fill_(0x5A)
        g.replay()
        t.check(oracle, out["recv"], GM, mode, (i, "replay"))
