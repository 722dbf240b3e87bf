"""GPU: the host-memory one-call steps from a native C++ caller (tests/native_host_pack/host_pack_caller.cc).

lampi_host_msg_send_pack and lampi_host_recv_unpack_batch in GM, IB and Quadrics shapes (64 KiB buffers, 2 KiB
buffers, 128-byte envelopes with 2,048-byte and inline payloads, an empty message), CRC / SUM / checksumming off,
pinned and pageable rings, on two threads at once and then on the main thread after lampi_host_release().  Each
message is packed in three gated calls and every ring byte is compared with the slot rebuilt from the oracle inside
the program; then headers and payloads are corrupted, the ring is drained in one call and every verdict, count,
checksum and application byte is compared.  Invalid arguments write nothing; after the last release no pinned
memory and no device scratch is held.  The binary is built on the CPU by __graft_entry__.build().
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_native_host_pack_caller_matches_oracle(cuda):
    exe = os.path.join(HERE, "native_host_pack", "host_pack_caller")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} not built: run __graft_entry__.build() (make -C tests/native_host_pack)")
    r = subprocess.run([exe, "2"], capture_output=True, text=True, timeout=600)
    out = r.stdout
    assert r.returncode == 0, out[-4000:] + r.stderr[-2000:]
    assert out.strip().endswith("bad 0 done"), out[-2000:]
    lines = [ln for ln in out.splitlines() if ln.startswith(("send ", "recv ", "invalid", "empty"))]
    assert lines and all(ln.endswith(" ok") for ln in lines)
    # 5 shapes x 3 modes x 2 rings x (send + recv) on 2 threads + main, + 2 edge lines
    assert len(lines) == 5 * 3 * 2 * 2 * (2 + 1) + 2
    # the drained rings really held dropped and corrupt fragments
    assert any(ln.startswith("recv ") and " hdr_bad 0 " not in ln for ln in lines)
    assert any(ln.startswith("recv ") and " data_bad 0 " not in ln for ln in lines)
    assert "pinned_after_release 0 scratch_after_release 0" in out
