"""CPU: the DMA plans of the host typemap steps (lampi_amd/csrc/host_tmap_plan.h), executed on the CPU.

tests/native_host_tmap/tmap_plan_check.cc plans windows of T1, T2, T3, T5, S1, S65, T4a, a type of touching pairs,
extent 0, extent < size and a negative extent exactly as lampi_host_tmap_send_pack and
lampi_host_tmap_recv_unpack_batch do -- the three window starts of tmap_model.pack_offsets, last fragments of 1, 15,
17 bytes and a whole one, chunk caps from 4 KiB to 32 MiB, both directions, receive runs with fragments dropped at
the start, middle and end -- and runs every planned transfer as a memcpy against the header's address rule applied
byte by byte: the pieces route reads and writes exactly the pieces' bytes, the span route reads only bytes on pages
that a piece of the window's elements touches, and no transfer leaves the staging sizes that were announced.  One
type either side of each span rule, built from the header's own constants, must take the route the rule says.  No
GPU and no library involved.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tmap_plans_execute_exactly():
    exe = os.path.join(HERE, "native_host_tmap", "tmap_plan_check")
    assert os.path.exists(exe), "run __graft_entry__.build() (make -C tests/native_host_tmap)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "bad 0 done"
    assert all(ln.endswith(" ok") for ln in lines[:-1]) and len(lines) > 400
    for name in ("T1", "T2", "T3", "T5", "S1", "S65", "T4a", "touching", "extent0", "extent<size", "negative"):
        send = [ln for ln in lines if ln.startswith(f"send {name} ")]
        # windows x last fragments x (any route, pieces alone), and the empty window
        assert len(send) >= 3 * 4 * 2 + 1, (name, len(send))
        if name not in ("extent0", "extent<size"):  # (overlapping elements: deliveries are unspecified)
            assert len([ln for ln in lines if ln.startswith(f"recv {name} ")]) >= 12, name
    # both routes ran, and the pieces route also where the span route would have been taken
    assert any(" span=0 " not in ln for ln in lines if ln.startswith("send T1 ") and "pieces alone" not in ln)
    assert all(" span=0 " in ln for ln in lines if "pieces alone" in ln)
    # either side of each span rule
    for rule, route in (("gap-in-footprint<G", "span=1 pieces=0"), ("gap-in-footprint=G", "span=0 pieces=1"),
                        ("gap-between<G", "span=1 pieces=0"), ("gap-between=G", "span=0 pieces=1"),
                        ("rowbytes=RB", "span=1 pieces=0"), ("rowbytes>RB", "span=0 pieces=1"),
                        ("ratio=R", "span=1 pieces=0"), ("ratio>R", "span=0 pieces=1")):
        hit = [ln for ln in lines if ln.startswith(f"send {rule} ")]
        assert len(hit) == 1 and route in hit[0], hit
    # whole elements: one pitched transfer per typemap pair
    assert "whole elements of T1: 1 2D transfers ok" in lines
    assert "whole elements of T2: 3 2D transfers ok" in lines
    assert "whole elements of touching: 1 2D transfers ok" in lines
    assert len([ln for ln in lines if ln.startswith("inconsistent: ")]) == 5
