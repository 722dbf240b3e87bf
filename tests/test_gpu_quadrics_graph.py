"""What a replayed graph of the Quadrics send and receive steps gives.  While a stream is being captured both calls
take buffers of their own for the values between their launches (the checksums ahead of the stamp, the header
pre-pass's records), so a replay must not depend on a pooled buffer that a later, larger eager call replaced, and
it must read the source bytes as they are at replay time.  Expectations come from tests/quadrics_model.py."""
import numpy as np
import pytest

import quadrics_model as qm
from quadrics_model import CRC, DATA, HDR, INLINE, QUADRICS
from recv_unpack_model import check
from test_gpu_quadrics_send import QRing

pytestmark = pytest.mark.gpu


def test_graph_replay_send_then_receive(cuda, oracle):
    """One linear capture (no parallel branches) in CRC mode: send_pack_batch of 300 fragments of 0..8,192 bytes
    into a ring -- the inline ones into their envelopes --, then recv_unpack_batch out of that ring into an
    application buffer.  After the capture an eager send and receive of 40,000 fragments regrow both pooled
    buffers; then the source is refilled and the graph replayed twice, each replay compared with the model."""
    import torch

    from lampi_amd import device as dv

    mode = CRC
    rng = np.random.default_rng(1100)
    n = 300
    r = QRing(cuda, n, seed=1101, room=8192)
    ln = rng.integers(0, 8193, size=n).astype(np.uint64)
    edges = [0, 1, 3, 51, 52, 53, 64, 2047, 2048, 2049, 4096, 4097, 8191, 8192]
    ln[:len(edges)] = edges
    ln[20:40] = rng.integers(1, INLINE + 1, size=20).astype(np.uint64)
    descs, _ = r.batch(oracle, rng, ln, ln, mode, fresh=True)
    app = torch.empty(n * r.slot, dtype=torch.uint8, device=cuda)
    dv.fill_stream(app, seed=1102)
    app_before, happ0 = app.clone(), app.cpu().numpy()
    k = np.arange(n, dtype=np.uint64)
    aoffs = k * np.uint64(r.slot) + k % np.uint64(8)
    room = np.full(n, 1 << 20, np.int64)
    rdescs = dv.make_recv_descs(r.ring, r.doffs, app, aoffs, ln, room)
    poffs = np.where(ln <= INLINE, (r.hat + DATA).astype(np.uint64), r.doffs)

    def model():
        """The ring after the send and the receive's outputs, over the source bytes as they are now."""
        want_ring = r.before[0].cpu().numpy()
        parts = np.full(n, qm.M32, np.uint64)
        qm.send_expect(oracle, r.host, r.soffs, ln, ln, parts, want_ring, r.hat, want_ring, r.doffs, mode)
        want_app = happ0.copy()
        want = qm.recv_expect(oracle, want_ring, poffs, ln, want_ring[r.hat[:, None] + np.arange(HDR)],
                              np.ones(n, bool), want_app, aoffs, room, mode)
        assert not want[2].any() and not want[3].any()
        return torch.from_numpy(want_ring).to(cuda), want, want_app

    out = {}

    def run():
        r.send(descs, mode)
        out["recv"] = dv.recv_unpack_batch(rdescs, r.ring, r.slot, kind=QUADRICS, mode=mode)

    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    w0 = model()
    assert torch.equal(r.ring, w0[0])
    check(out["recv"], w0[1], n, app, w0[2], r.slot, "warm-up")
    r.reset()
    app.copy_(app_before)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    # larger eager calls on the default stream: 160 KB of values, 320 KB of header records
    big = 40000
    bsrc = torch.empty(big * 64, dtype=torch.uint8, device=cuda)
    dv.fill_stream(bsrc, seed=1103)
    bring = torch.zeros(big * 192, dtype=torch.uint8, device=cuda)
    bk = np.arange(big, dtype=np.uint64)
    bl = np.full(big, 60, np.uint64)
    bd = dv.make_copy_descs(bsrc, bk * np.uint64(64), bring, bk * np.uint64(192) + np.uint64(HDR), bl, bl)
    dv.send_pack_batch(bd, bring, 192, kind=QUADRICS, mode=mode)
    bapp = torch.zeros(big * 64, dtype=torch.uint8, device=cuda)
    brd = dv.make_recv_descs(bring, bk * np.uint64(192) + np.uint64(HDR), bapp, bk * np.uint64(64), bl,
                             np.full(big, 64, np.int64))
    bc = dv.recv_unpack_batch(brd, bring, 192, kind=QUADRICS, mode=mode)
    torch.cuda.synchronize()
    assert [int(x) for x in bc[4].cpu().numpy()] == [0, 0] and bool((bc[0] == 60).all())
    assert torch.equal(bapp.view(big, 64)[:, :60], bsrc.view(big, 64)[:, :60])
    # new source bytes, two replays
    dv.fill_stream(r.src, seed=1104)
    r.host = r.src.cpu().numpy()
    w1 = model()
    for i in range(2):
        r.reset()
        app.copy_(app_before)
        for t in out["recv"]:
            t.fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(r.ring, w1[0]), i
        check(out["recv"], w1[1], n, app, w1[2], r.slot, (i, "replay"))
