"""The typemap send and receive steps together: a round trip between two datatypes of equal packed length, and what
a replayed graph of both calls gives.  While a stream is being captured a call's scratch (row values, fragment
values, header records) is a buffer of its own instead of the stream's pooled ones, so a replay must not depend on a
pooled buffer that a later eager call replaced, and it must read the source as it is at replay time.  Expectations
come from the oracle and tests/tmap_model.py alone."""
import numpy as np
import pytest

import tmap_model as tmm
from test_gpu_send_pack import CRC, GM, IB, SUM
from test_gpu_tmap_send import FILL, _Send

pytestmark = pytest.mark.gpu

# T2 (packed_size 65) x 8,001 elements and T3 (8,001) x 65 elements: 520,065 packed bytes each
COUNT2, COUNT3 = tmm.T3.packed_size, tmm.T2.packed_size
TOTAL = COUNT2 * tmm.T2.packed_size


class _Trip:
    """tmap_send_pack of T2 into a ring, tmap_recv_unpack of that ring through T3 into a second buffer."""

    def __init__(self, cuda, kind, frag_len, seed):
        import torch

        from lampi_amd import device as dv

        self.kind, self.L = kind, frag_len
        self.n = (TOTAL + frag_len - 1) // frag_len
        self.s = _Send(cuda, tmm.T2, COUNT2, frag_len, self.n, seed)
        self.hdst, self.dorigin = tmm.host_buffer(tmm.T3, COUNT3, seed + 5)
        self.dst = torch.from_numpy(self.hdst).to(cuda)
        self.dst_before = self.dst.clone()
        self.dtm3 = dv.make_tmap(tmm.T3.pairs(), tmm.T3.extent, COUNT3, cuda)
        self.idx3 = self.dorigin + tmm.index_map(tmm.T3, np.arange(TOTAL, dtype=np.int64))
        self.cuda = cuda

    def run(self, mode):
        from lampi_amd import device as dv

        s = self.s
        dv.tmap_send_pack(s.buf, s.dtm, s.L, s.ring, s.stride, s.tmpl, kind=self.kind, mode=mode,
                          base_offset=s.origin, **FILL)
        return dv.tmap_recv_unpack(s.ring, self.n, s.stride, self.dst, self.dtm3, kind=self.kind, mode=mode,
                                   seq_offset0=FILL["seq_offset0"], base_offset=self.dorigin)

    def new_source(self, seed):
        import torch

        s = self.s
        s.hbuf = np.random.default_rng(seed).integers(0, 256, size=s.hbuf.size, dtype=np.uint8)
        s.buf.copy_(torch.from_numpy(s.hbuf).to(self.cuda))

    def reset(self):
        self.s.ring.copy_(self.s.before_t)
        self.dst.copy_(self.dst_before)

    def check(self, oracle, got, mode, what):
        import torch

        from lampi_amd import device as dv

        torch.cuda.synchronize()
        s = self.s
        copied, csum, hmask, dmask, nbad = got
        assert [int(x) for x in nbad.cpu()] == [0, 0], what
        assert not dv.mask_bits(hmask, self.n).any() and not dv.mask_bits(dmask, self.n).any(), what
        lens = np.minimum(self.L, TOTAL - np.arange(self.n, dtype=np.int64) * self.L)
        assert np.array_equal(copied.cpu().numpy(), lens), what
        ring_want = s.want(oracle, self.kind, mode, 0, TOTAL)
        assert np.array_equal(s.ring.cpu().numpy(), ring_want), (what, "ring")
        stored = ring_want.reshape(self.n, s.stride)[:, 64:68].copy().view("<u4").reshape(self.n)
        assert np.array_equal(dv.as_u32(csum), stored), (what, "csum")
        want = self.hdst.copy()
        want[self.idx3] = tmm.packed(tmm.T2, s.hbuf, s.origin, 0, TOTAL)  # the pieces equal, the gaps their sentinel
        assert np.array_equal(self.dst.cpu().numpy(), want), (what, "destination")


@pytest.mark.parametrize("kind,frag_len", [(GM, 65456), (IB, 1976)], ids=["gm", "ib"])
@pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
def test_round_trip_between_two_datatypes(cuda, oracle, mode, kind, frag_len):
    t = _Trip(cuda, kind, frag_len, seed=1400 + mode)
    t.check(oracle, t.run(mode), mode, "round trip")


@pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
def test_graph_replay_results(cuda, oracle, mode):
    """Both calls captured into one graph on one stream after a warm-up on a side stream; then eager calls of another
    shape on the default stream that regrow both pooled buffers; then new source bytes in place and two replays, each
    compared with the models."""
    import torch

    from lampi_amd import device as dv

    t = _Trip(cuda, GM, 65456, seed=1450 + mode)
    out = {}

    def run():
        out["recv"] = t.run(mode)

    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    t.check(oracle, out["recv"], mode, "warm-up")
    t.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    # eager, another shape: 7,000 fragments of 100 bytes both ways (21,000 words of records and values: more than the
    # 64 KiB the second pooled buffer starts with), then 40,000 descriptors with rows_hint=8 (1.28 MB of row-group
    # values: more than the first one's 1 MiB)
    small = _Send(cuda, tmm.T1, tmm.count_for(tmm.T1, 700000), 100, 7000, seed=1460)
    small.check(oracle, IB, mode, 0, 700000, "eager send")
    dst2 = torch.zeros_like(small.buf)
    got = dv.tmap_recv_unpack(small.ring, 7000, small.stride, dst2, small.dtm, kind=IB, mode=mode,
                              seq_offset0=FILL["seq_offset0"], base_offset=small.origin)
    torch.cuda.synchronize()
    assert [int(x) for x in got[4].cpu()] == [0, 0]
    assert torch.equal(dst2[small.origin + 3:small.origin + 11], small.buf[small.origin + 3:small.origin + 11])
    k = np.arange(40000, dtype=np.uint64) * np.uint64(200)
    src8, dst8 = torch.zeros(40000 * 200, dtype=torch.uint8, device=cuda), torch.empty(40000 * 200, dtype=torch.uint8,
                                                                                       device=cuda)
    dv.frag_bcopy_batch(dv.make_copy_descs(src8, k, dst8, k, np.full(40000, 200), np.full(40000, 200)), mode=mode,
                        rows_hint=8)
    torch.cuda.synchronize()
    for i in range(2):
        t.new_source(1470 + i)
        t.reset()
        for x in out["recv"]:
            x.fill_(0x5A)
        g.replay()
        t.check(oracle, out["recv"], mode, (i, "replay"))
