"""The send step's state across calls: the two pooled buffers of a (thread, device, stream) slot -- stream_scratch,
taken by the copy launchers, and stream_vals, taken by the stamp's callers -- across a regrowth with calls queued
back to back, and the device entry points called from several threads at once.  Expected rings come from the
oracle alone (tests/test_gpu_send_pack.py's model)."""
import threading

import numpy as np
import pytest

from test_gpu_send_pack import GM, SUMS, _first_diff, _Msg, _Ring

pytestmark = pytest.mark.gpu

FILL = dict(frag_seq0=2**64 - 2, frag_seq_step=3, desc_ptr0=2**64 - 0x100, desc_ptr_stride=0x1A8)


def _msg(cuda, oracle, frag_len, nfrag, mode, seed):
    shape = (GM, frag_len, frag_len + 72, frag_len * nfrag, 0)
    return _Msg(cuda, oracle, shape, dict(FILL, seq_offset0=2**64 - frag_len - 5), mode, seed=seed)


@SUMS
def test_pool_regrowth(cuda, oracle, mode):
    """stream_vals starts at 64 KiB (16,384 words) and regrows with synchronize + hipFree + hipMalloc: batches of
    64, 20,000, 64 and 40,000 fragments with rows_hint=2 (CRC: the two-launch route, values pooled) and messages of
    30,000 and 100 64-byte fragments between them, one stream, no host synchronisation until the end; every call
    has a ring of its own.  The pools only grow: a second and a third pass leave lampi_device_scratch_bytes()
    where the first left it."""
    import torch

    from lampi_amd import lib

    rng = np.random.default_rng(780 + mode)
    steps = []  # (what to launch, ring tensor, expected ring, bytes per slot, what to reset)
    for i, n in enumerate([64, 20000, None, 64, 40000, None]):
        if n is None:
            x = _msg(cuda, oracle, 64, 30000 if i == 2 else 100, mode, seed=790 + 3 * i)
            steps.append((x.send, x.ring, torch.from_numpy(x.want).to(cuda), x.stride, x.reset))
            continue
        r = _Ring(cuda, n, 272, seed=781 + 4 * i)
        descs, want = r.batch(oracle, rng, rng.integers(64, 201, size=n), GM, mode)
        steps.append((lambda stream, r=r, descs=descs: r.send(descs, GM, mode, stream=stream, rows_hint=2), r.ring,
                      want, 272, r.reset))
    stream = torch.cuda.Stream(device=cuda)
    held = []
    with torch.cuda.stream(stream):
        for _ in range(3):
            for _, _, _, _, reset in steps:
                reset()
            for send, _, _, _, _ in steps:
                send(stream)
            stream.synchronize()
            held.append(int(lib().lampi_device_scratch_bytes()))
            for i, (_, ring, want, slot, _) in enumerate(steps):
                assert torch.equal(ring, want), (i, _first_diff(ring, want, slot))
    assert held[1] == held[0] and held[2] == held[0], held


@SUMS
def test_threads_share_streams(cuda, oracle, mode):
    """Four threads in the device entry points at once, two of them on torch's default stream (the scratch table is
    keyed by thread as well, so they never share a pooled buffer) and two on streams of their own: twelve rounds each
    of a rows_hint=2 batch of 300 fragments of 4,097-8,000 bytes and a message of 16 KiB fragments -- the routes
    that take both pooled buffers --, every ring compared."""
    import torch

    nthreads, rounds, n, slot = 4, 12, 300, 8128
    work = []
    for t in range(nthreads):
        rng = np.random.default_rng(800 + 10 * mode + t)
        r = _Ring(cuda, n, slot, seed=810 + 4 * t)
        descs, want = r.batch(oracle, rng, rng.integers(4097, 8001, size=n), GM, mode)
        x = _msg(cuda, oracle, 16384, 40, mode, seed=830 + 3 * t)
        work.append((r, descs, want, x, torch.from_numpy(x.want).to(cuda),
                     torch.cuda.Stream(device=cuda) if t >= 2 else None))
    torch.cuda.synchronize()
    barrier = threading.Barrier(nthreads)
    errors = [None] * nthreads

    def run(t):
        r, descs, want, x, xwant, stream = work[t]
        try:
            with torch.cuda.stream(stream):
                barrier.wait(timeout=60)
                for i in range(rounds):
                    r.reset()
                    r.send(descs, GM, mode, stream=stream, rows_hint=2)
                    assert torch.equal(r.ring, want), (t, i, "batch", _first_diff(r.ring, want, slot))
                    x.reset()
                    x.send(stream)
                    assert torch.equal(x.ring, xwant), (t, i, "message", _first_diff(x.ring, xwant, x.stride))
        except BaseException as e:  # re-raised in the main thread
            errors[t] = e

    threads = [threading.Thread(target=run, args=(t,), daemon=True) for t in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads), "a thread is still running"
    for e in errors:
        if e is not None:
            raise e
