"""The host-memory one-call steps, A/B: what the parent commit can do for a host message and a host NIC ring against
lampi_host_msg_send_pack and lampi_host_recv_unpack_batch.  Whole calls (they are synchronous), wall clock, 2
warm-ups and 5 reps per figure, 256 MiB page-locked buffers (lampi_host_register).

  GM  4,096 x 65,456-byte fragments in 64 KiB slots        IB  131,072 x 1,976 bytes in 2 KiB slots
  modes CRC, SUM and NONE

  send  A   lampi_host_msg_bcopy alone, into ring + 72 (the parent commit's library, --lib-a PATH loaded through
            LAMPI_CSUM_LIB).  It does LESS than B: no header is written and none is checksummed -- it is all the
            parent can do on this path.
        B   lampi_host_msg_send_pack from this tree's library: headers, payloads, both checksum words.
        bar: B no further behind A than A's spread (max - min of its five), plus the share of extra bytes B must
            write, 72 of 65,528 (GM) and 72 of 2,048 (IB) -- from the layout, not measured.
  recv  A   lampi_host_header_check_batch (GM) / lampi_host_header_compare_batch (IB), then
            lampi_host_copy_to_app_batch with the expected values prepared beforehand and NO host filtering between
            the two calls, which favours A; with checksumming off the copy alone.
        B   lampi_host_recv_unpack_batch.
        bar: B no further behind A than A's spread.

The ring both receive lines drain is packed by the device form lampi_msg_send_pack (both libraries have it) and
downloaded.  Every line checks its result (the ring's payloads / the application buffer against the message).  Every
line runs in a fresh child process under its own time limit; the lines alternate five times and a child that fails
or runs out of time stops the rest.  The table (median of the five, GiB/s of payload, A's spread, * = behind the bar)
goes to --out (default profiles/r12/host_pack_ab.txt).

python tools/microbench/host_pack_ab.py --lib-a /path/to/parent/liblampi_csum.so [--out FILE] [--rounds 5]
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)

HDR = 72
SHAPES = {"gm": (4096, 65456, 65536, 0), "ib": (131072, 1976, 2048, 1)}  # n, payload, slot, header kind
EXTRA = {"gm": 72 / 65528, "ib": 72 / 2048}  # the header bytes B's send writes on top of A's, per slot byte written
MODES = (("crc", 0), ("sum", 1), ("none", 2))
CHILD_LIMIT = 300  # seconds per child
NEW = ("lampi_host_msg_send_pack", "lampi_host_recv_unpack_batch")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(line):
    import numpy as np
    import torch

    from lampi_amd import _lib

    if line == "A":  # the parent commit's library has no host one-call symbols
        for k in NEW:
            _lib.PROTOTYPES.pop(k, None)
    from lampi_amd import device as dv

    L_ = _lib.lib()

    def timed(run, reps=5):
        for _ in range(2):
            run()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t)

    def pinned(nbytes):
        a = np.zeros(nbytes, np.uint8)
        assert L_.lampi_host_register(a.ctypes.data, a.nbytes) == 0
        return a

    tmpl = np.arange(HDR, dtype=np.uint8)
    fill = _lib.SendHdrFill()
    fill.tmpl[:] = tmpl.tolist()
    fill.frag_seq0, fill.frag_seq_step, fill.desc_ptr0, fill.desc_ptr_stride, fill.seq_offset0 = 1, 1, 4096, 256, 0
    for shape, (n, L, slot, kind) in SHAPES.items():
        mlen, rbytes = n * L, n * slot
        dmsg = torch.empty(mlen, dtype=torch.uint8, device="cuda")
        dv.fill_stream(dmsg, seed=13)
        msg, ring, app = pinned(mlen), pinned(rbytes), pinned(mlen)
        msg[:] = dmsg.cpu().numpy()
        k = np.arange(n, dtype=np.uint64)
        out = np.zeros(n, np.uint32)
        copied, csum = np.zeros(n, np.int64), np.zeros(n, np.uint32)
        hmask, dmask, nbad = np.zeros(n // 32 + 1, np.uint32), np.zeros(n // 32 + 1, np.uint32), np.zeros(2, np.uint32)
        hoffs = k * np.uint64(slot)
        m, r, a = msg.ctypes.data, ring.ctypes.data, app.ctypes.data
        payloads = lambda: ring.reshape(n, slot)[:, HDR:HDR + L].reshape(-1)
        for mname, mode in MODES:
            # ---- send
            ring[:] = 0
            if line == "A":
                send = lambda: L_.lampi_host_msg_bcopy(m, mlen, L, 0, n, r + HDR, slot, 0xFFFFFFFF, out.ctypes.data, mode)
            else:
                send = lambda: L_.lampi_host_msg_send_pack(m, mlen, L, 0, n, r, slot, ctypes.addressof(fill), kind, mode)
            assert send() == 0
            ms = timed(send)
            if not np.array_equal(payloads(), msg):
                raise SystemExit(f"{line} {shape} send {mname}: wrong payloads")
            print(json.dumps({"line": line, "shape": shape, "step": "send", "mode": mname, "ms": ms, "bytes": mlen}),
                  flush=True)
            # ---- receive: the ring as the device form packs it
            dring = torch.zeros(rbytes, dtype=torch.uint8, device="cuda")
            dv.msg_send_pack(dmsg, L, dring, slot, tmpl, frag_seq0=1, frag_seq_step=1, desc_ptr0=4096,
                             desc_ptr_stride=256, seq_offset0=0, kind=kind, mode=mode)
            torch.cuda.synchronize()
            ring[:] = dring.cpu().numpy()
            del dring
            if line == "A":
                frags = np.zeros(n, dtype=np.dtype([("frag_off", "<u8"), ("app", "<u8"), ("app_len", "<i8"),
                                                    ("length", "<u4"), ("expected", "<u4")]))
                frags["frag_off"], frags["app"] = hoffs + np.uint64(HDR), np.uint64(a) + k * np.uint64(L)
                frags["app_len"], frags["length"] = L, L
                frags["expected"] = ring.reshape(n, slot)[:, 64:68].copy().view("<u4").reshape(n)

                def recv():
                    if mode != 2:
                        if kind == 0:
                            rc = L_.lampi_host_header_check_batch(r, rbytes, hoffs.ctypes.data, n, HDR, 18, 68,
                                                                  hmask.ctypes.data, nbad.ctypes.data, mode)
                        else:
                            rc = L_.lampi_host_header_compare_batch(r, rbytes, hoffs.ctypes.data, n, HDR - 4, 68,
                                                                    hmask.ctypes.data, nbad.ctypes.data, mode)
                        assert rc == 0
                    return L_.lampi_host_copy_to_app_batch(r, rbytes, frags.ctypes.data, n, copied.ctypes.data,
                                                           csum.ctypes.data, dmask.ctypes.data, nbad.ctypes.data + 4, mode)
            else:
                slots = np.zeros(n, dtype=np.dtype([("hdr_off", "<u8"), ("frag_off", "<u8"), ("app", "<u8"),
                                                    ("app_len", "<i8"), ("length", "<u4"), ("reserved", "<u4")]))
                slots["hdr_off"], slots["frag_off"] = hoffs, hoffs + np.uint64(HDR)
                slots["app"], slots["app_len"], slots["length"] = np.uint64(a) + k * np.uint64(L), L, L

                def recv():
                    return L_.lampi_host_recv_unpack_batch(r, rbytes, slots.ctypes.data, n, kind, copied.ctypes.data,
                                                           csum.ctypes.data, hmask.ctypes.data, dmask.ctypes.data,
                                                           nbad.ctypes.data, mode)
            app[:] = 0
            nbad[:] = 0
            assert recv() == 0
            ms = timed(recv)
            if [int(x) for x in nbad] != [0, 0] or not np.array_equal(app, msg) or not (copied == L).all():
                raise SystemExit(f"{line} {shape} recv {mname}: wrong result (nbad {nbad})")
            print(json.dumps({"line": line, "shape": shape, "step": "recv", "mode": mname, "ms": ms, "bytes": mlen}),
                  flush=True)
        for x in (msg, ring, app):
            L_.lampi_host_unregister(x.ctypes.data)
        del dmsg
        torch.cuda.synchronize()


def drive():
    lib_a = arg("--lib-a")
    if not lib_a or not os.path.exists(lib_a):
        sys.exit("--lib-a: the parent commit's liblampi_csum.so is required for line A")
    out = arg("--out", os.path.join(ROOT, "profiles", "r12", "host_pack_ab.txt"))
    rounds = int(arg("--rounds", "5"))
    envs = {"A": {"LAMPI_CSUM_LIB": os.path.abspath(lib_a)}, "B": {}}
    times = {}  # (shape, step, mode) -> line -> [(ms, bytes)]
    failed = None
    for r in range(rounds):
        for line in ("A", "B"):
            env = {k: v for k, v in os.environ.items() if k != "LAMPI_CSUM_LIB"}
            env.update(envs[line])
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", line], env=env,
                                   capture_output=True, text=True, timeout=CHILD_LIMIT)
            except subprocess.TimeoutExpired:
                failed = f"round {r} line {line}: no result within {CHILD_LIMIT} s"
                break
            if p.returncode != 0:
                failed = f"round {r} line {line}: exit {p.returncode}\n{p.stdout[-500:]}\n{p.stderr[-2000:]}"
                break
            for row in p.stdout.splitlines():
                if row.startswith("{"):
                    x = json.loads(row)
                    times.setdefault((x["shape"], x["step"], x["mode"]), {}).setdefault(line, []).append(
                        (x["ms"], x["bytes"]))
            print(f"round {r} line {line} done", flush=True)
        if failed:
            break
    rows = ["host one-call steps A/B: median ms of %d fresh processes per line (GiB/s of payload); 256 MiB page-locked "
            "buffers" % rounds,
            "send: A = host_msg_bcopy alone (parent commit's library; writes no header), B = host_msg_send_pack; bar = A + "
            "A's spread + A x 72/65528 (gm) or 72/2048 (ib)",
            "recv: A = host_header_check/compare_batch + host_copy_to_app_batch (no host filtering), B = "
            "host_recv_unpack_batch; bar = A + A's spread;  * = B behind its bar",
            f"{'shape':5s} {'step':4s} {'mode':4s} {'A':>18s} {'B':>19s} {'A spread':>9s} {'bar':>9s}"]
    for key in sorted(times):
        t = times[key]
        if "A" not in t or "B" not in t:
            continue
        a, b = (statistics.median(m for m, _ in t[x]) for x in ("A", "B"))
        spread = max(m for m, _ in t["A"]) - min(m for m, _ in t["A"])
        bar = a + spread + (a * EXTRA[key[0]] if key[1] == "send" else 0.0)
        gib = lambda ms: t["A"][0][1] / (ms * 1e-3) / 2**30
        rows.append(f"{key[0]:5s} {key[1]:4s} {key[2]:4s} {a:9.3f} ({gib(a):6.2f}) {b:9.3f} ({gib(b):6.2f})"
                    f"{'*' if b > bar else ' '} {spread:9.3f} {bar:9.3f}")
    for key in sorted(times):
        for line in ("A", "B"):
            if line in times[key]:
                rows.append(f"raw {key[0]} {key[1]} {key[2]} {line}: " + " ".join(f"{m:.3f}" for m, _ in times[key][line]))
    if failed:
        rows.append("STOPPED: " + failed)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(rows) + "\n")
    print("\n".join(rows))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child"))
    else:
        drive()
