"""CPU: the DMA plan of the host receive step (lampi_amd/csrc/host_pack_items.h on host_plan.h), executed on the CPU.

tests/native_host_pack/unpack_plan_check.cc presents random batches of lampi_host_recv_slot records to the planner
exactly as lampi_host_recv_unpack_batch does -- GM / IB / Quadrics headers, payloads behind their headers and apart,
inline Quadrics payloads, fragments with nothing to deliver, ring order and shuffled, chunk sizes from 4 KiB to
32 MiB -- and runs every planned transfer as a memcpy: no transfer may leave the ring or the staging sizes the
planner announced, every header and payload must arrive where the descriptors will point, the application arena must
receive exactly the deliveries, and a batch several times the chunk size must be cut into chunks (the item a chunk
may start at always carries bytes: the planner passes over empty items before it looks for a boundary).  No GPU and
no library involved.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_unpack_plan_executes_exactly():
    exe = os.path.join(HERE, "native_host_pack", "unpack_plan_check")
    assert os.path.exists(exe), "run __graft_entry__.build() (make -C tests/native_host_pack)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "bad 0 done"
    assert all(ln.endswith(" ok") for ln in lines[:-1]) and len(lines) == 8 * 2 * 4 * 3 + 1
    # 400 fragments at a 4 KiB chunk size are many chunks
    small = [ln for ln in lines if " n 400 cap 4096 " in ln]
    assert len(small) == 16 and all(int(ln.split(" chunks ")[1].split()[0]) >= 3 for ln in small), small
    # slots at a constant pitch with wide gaps still move up as one 2D copy per chunk, headers included
    wide = [ln for ln in lines if ln.startswith("gm_4k_in_64k ring_order n 400 cap 33554432 ")]
    assert len(wide) == 1 and " chunks 1 h2d 1 " in wide[0], wide
