"""What a replayed graph of receive-step calls gives.  While a stream is being captured a call's scratch (the header
pre-pass's records, the row groups' values) is a buffer of its own instead of the stream's pooled ones, so a replay
must not depend on a pooled buffer that a later eager call replaced, and it must read the ring as it is at replay
time.  Expectations come from the oracle alone (tests/recv_unpack_model.py)."""
import numpy as np
import pytest

from recv_unpack_model import RecvRing, check, expect_ring, flip_bit, pack_slots, HDR_FAULTS
from test_gpu_send_pack import CRC, GM, SUM

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", [CRC, SUM], ids=["crc", "sum"])
def test_graph_replay_results(cuda, oracle, mode):
    """A linear capture -- msg_recv_unpack of 40 aligned GM slots, then recv_unpack_batch with rows_hint=16 on 300
    fragments of 65,456 bytes -- after a warm-up on a side stream; then eager calls on the default stream that regrow
    both pooled buffers (40,000 fragments with rows_hint=8: 1.28 MB of row-group scratch and 320 KB of header
    records); then new ring bytes in place with a different set of bad headers, and two replays, each compared with
    the oracle."""
    import torch

    from lampi_amd import device as dv

    rng = np.random.default_rng(980 + mode)
    L, stride, nslots = 65456, 65536, 40
    msg = torch.empty(nslots * L, dtype=torch.uint8, device=cuda)
    ring = torch.empty(nslots * stride, dtype=torch.uint8, device=cuda)
    app = torch.empty(nslots * L + 64, dtype=torch.uint8, device=cuda)
    dv.fill_stream(ring, seed=981)
    dv.fill_stream(app, seed=982)
    app_before, hring0, happ0 = app.clone(), ring.cpu().numpy(), app.cpu().numpy()

    def slots(seed, bad):
        """The ring's bytes for a new message with the headers of `bad` failing, and the model's outputs."""
        dv.fill_stream(msg, seed=seed)
        hring = hring0.copy()
        pack_slots(oracle, rng, hring, msg.cpu().numpy(), L, stride, 16, GM, mode)
        for j, k in enumerate(bad):
            flip_bit(hring, k * stride, rng, *HDR_FAULTS[j % 3])
        want_app = happ0.copy()
        want = expect_ring(oracle, hring, nslots, stride, want_app, nslots * L, 16, GM, mode)
        assert list(np.nonzero(want[2])[0]) == sorted(bad)
        return torch.from_numpy(hring).to(cuda), want, want_app

    n, length = 300, 65456
    slot = (72 + length + 15 + 63) // 64 * 64
    r = RecvRing(cuda, n, slot, seed=985)

    def batch(bad):
        cls = np.zeros(n, np.int64)
        cls[list(bad)] = 1
        cls[7] = 2
        return r.batch(oracle, rng, np.full(n, length, np.uint64), GM, mode, cls,
                       app_lens=np.full(n, length + 3, np.int64))

    b0 = batch([0, 150])
    s0 = slots(983, [3])
    big = RecvRing(cuda, 40000, 288, seed=990)
    bcls = np.zeros(40000, np.int64)
    bcls[[5, 39999]] = 1
    bb = big.batch(oracle, rng, rng.integers(64, 201, size=40000), GM, mode, bcls,
                   app_lens=np.full(40000, 300, np.int64))
    out = {}

    def run():
        out["msg"] = dv.msg_recv_unpack(ring, nslots, stride, app, kind=GM, mode=mode, seq_offset0=16,
                                        app_len=nslots * L)
        out["batch"] = r.recv(b0["descs"], GM, mode, rows_hint=16)

    ring.copy_(s0[0])
    r.load(b0)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    check(out["msg"], s0[1], nslots, app, s0[2], L, "warm-up message")
    r.check(out["batch"], b0, "warm-up batch")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    big.load(bb)
    big.check(big.recv(bb["descs"], GM, mode, rows_hint=8), bb, "eager")
    s1 = slots(987, [0, 17, 39])
    b1 = batch([1, 299])
    b1["descs"] = b0["descs"]  # (the captured call reads the descriptors it was given: the same fragments)
    for i in range(2):
        ring.copy_(s1[0])
        app.copy_(app_before)
        r.load(b1)
        for t in out["msg"] + out["batch"]:
            t.fill_(0x5A)
        g.replay()
        check(out["msg"], s1[1], nslots, app, s1[2], L, (i, "message"))
        r.check(out["batch"], b1, (i, "batch"))
