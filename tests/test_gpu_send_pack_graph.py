"""What a replayed graph of send-step calls writes.  While a stream is being captured a call's scratch is a buffer
of its own instead of the stream's pooled ones (stream_buffer), so a replay must not depend on a pooled buffer that
a later eager call replaced, and it must read the sources as they are at replay time.  Expected rings come from the
oracle alone (tests/test_gpu_send_pack.py's model)."""
import numpy as np
import pytest

from test_gpu_send_pack import GM, MSG_CASES, SUMS, _fill, _first_diff, _Msg, _Ring

pytestmark = pytest.mark.gpu


@SUMS
def test_graph_replay_results(cuda, oracle, mode):
    """A linear capture -- msg_send_pack of the gm_aligned shape, then send_pack_batch with rows_hint=16 on 300
    fragments of 65,456 bytes -- after a warm-up on a side stream; then eager calls on the default stream that regrow
    both pooled buffers (40,000 fragments with rows_hint=8: 1.28 MB of row-group scratch, and in CRC mode 160 KB of
    values; a message of 30,000 fragments for the values in SUM mode), new source bytes in place, and two replays,
    each compared with the oracle's rings for the new bytes."""
    import torch

    rng = np.random.default_rng(850 + mode)
    x = _Msg(cuda, oracle, MSG_CASES["gm_aligned"], _fill("gm_aligned"), mode, seed=851)
    n, length = 300, 65456
    slot = (72 + length + 63) // 64 * 64
    r = _Ring(cuda, n, slot, seed=855)
    descs, _ = r.batch(oracle, rng, np.full(n, length, np.uint64), GM, mode)
    big = _Ring(cuda, 40000, 272, seed=860)
    bdescs, bwant = big.batch(oracle, rng, rng.integers(64, 201, size=40000), GM, mode)
    y = _Msg(cuda, oracle, (GM, 64, 136, 64 * 30000, 0), _fill("gm_aligned"), mode, seed=865)

    def run():
        x.send()
        r.send(descs, GM, mode, rows_hint=16)

    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    big.send(bdescs, GM, mode, rows_hint=8)
    y.send()
    torch.cuda.synchronize()
    assert torch.equal(big.ring, bwant), _first_diff(big.ring, bwant, 272)
    ywant = torch.from_numpy(y.want).to(cuda)
    assert torch.equal(y.ring, ywant), _first_diff(y.ring, ywant, y.stride)
    x.refill(oracle, seed=870)
    r.refill(seed=871)
    xwant, rwant = torch.from_numpy(x.want).to(cuda), r.expected(oracle, GM, mode)
    for i in range(2):
        x.reset()
        r.reset()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(x.ring, xwant), (i, "message", _first_diff(x.ring, xwant, x.stride))
        assert torch.equal(r.ring, rwant), (i, "batch", _first_diff(r.ring, rwant, slot))
