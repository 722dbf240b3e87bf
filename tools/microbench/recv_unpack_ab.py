"""The receive step, A/B: the three-call sequence against the one-call forms (lampi_recv_unpack_batch,
lampi_msg_recv_unpack), whole rings on one stream, device events, 5 warm-ups and 20 reps per figure.

  GM ring  16,384 x 65,456-byte payloads in 64 KiB slots        IB ring  262,144 x 1,976 bytes in 2 KiB slots
  modes CRC, SUM and NONE; every header valid, every payload intact (the rings are packed by lampi_msg_send_pack)
  bytes counted: payload read + payload written + 72 header bytes per slot

  A   lampi_header_check_batch (GM) / lampi_header_compare_batch (IB), then lampi_copy_to_app_batch reading the
      expected values out of the same headers -- no host read-back of the mask in between, which favours A -- from a
      library built from the parent commit (--lib-a PATH, loaded through LAMPI_CSUM_LIB); with checksumming off
      the copy alone
  B   lampi_recv_unpack_batch (form desc) and lampi_msg_recv_unpack (form msg) from this tree's library

All lines call the C ABI with outputs allocated once.  Every line runs in a fresh child process under its own time
limit; the lines alternate five times and a child that fails or runs out of time stops the rest.  The table (median
of the five, A's spread = max - min of its five, shares of 8 TB/s) goes to --out (default
profiles/r08/recv_unpack_ab.txt).

python tools/microbench/recv_unpack_ab.py --lib-a /path/to/parent/liblampi_csum.so [--out FILE] [--rounds 5]
                                          [--lines A,B]
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)

HDR = 72
SHAPES = {"gm": (16384, 65456, 65536, 0), "ib": (262144, 1976, 2048, 1)}  # n, payload, slot, header kind
MODES = (("crc", 0), ("sum", 1), ("none", 2))
CHILD_LIMIT = 240  # seconds per child
NEW = ("lampi_recv_unpack_batch", "lampi_msg_recv_unpack")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(line):
    import numpy as np
    import torch

    from lampi_amd import _lib

    if line == "A":  # the parent commit's library has no receive-step symbols
        for k in NEW:
            _lib.PROTOTYPES.pop(k, None)
    from lampi_amd import device as dv

    L_ = _lib.lib()

    def timed(run, reps=20):
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    tmpl = np.arange(HDR, dtype=np.uint8)
    for shape, (n, L, slot, kind) in SHAPES.items():
        msg = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        dv.fill_stream(msg, seed=13)
        ring = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
        dv.fill_stream(ring, seed=14)
        app = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        k = np.arange(n, dtype=np.uint64)
        lens = np.full(n, L, np.uint64)
        descs = dv.make_recv_descs(ring, k * np.uint64(slot) + np.uint64(HDR), app, k * np.uint64(L), lens,
                                   lens.astype(np.int64))
        words = (n + 31) // 32
        copied = torch.empty(n, dtype=torch.int64, device="cuda")
        csum = torch.empty(n, dtype=torch.int32, device="cuda")
        hmask, dmask = (torch.empty(words, dtype=torch.int32, device="cuda") for _ in range(2))
        nbad = torch.empty(2, dtype=torch.int32, device="cuda")
        d, r, a = descs.data_ptr(), ring.data_ptr(), app.data_ptr()
        c, s, hm, dm, nb = (t.data_ptr() for t in (copied, csum, hmask, dmask, nbad))
        stream = int(torch.cuda.current_stream().cuda_stream)
        for mname, mode in MODES:
            dv.msg_send_pack(msg, L, ring, slot, tmpl, frag_seq0=1, frag_seq_step=1, desc_ptr0=4096,
                             desc_ptr_stride=256, seq_offset0=0, kind=kind, mode=mode)
            torch.cuda.synchronize()
            if line == "A":
                def a_desc():
                    if mode != 2:
                        if kind == 0:
                            rc = L_.lampi_header_check_batch(r, n, slot, HDR, 18, 68, hm, nb, mode, stream)
                        else:
                            rc = L_.lampi_header_compare_batch(r, n, slot, HDR - 4, 68, hm, nb, mode, stream)
                        assert rc == 0
                    assert L_.lampi_copy_to_app_batch(d, n, r + 64, slot, c, s, dm, nb + 4, mode, stream) == 0

                runs = {"desc": a_desc}
            else:
                runs = {"desc": lambda: L_.lampi_recv_unpack_batch(d, n, r, slot, kind, c, s, hm, dm, nb, mode, stream),
                        "msg": lambda: L_.lampi_msg_recv_unpack(r, n, slot, kind, a, n * L, 0, c, s, hm, dm, nb, mode,
                                                                stream)}
            for form, run in runs.items():
                app.zero_()
                nbad.zero_()
                ms = timed(run)
                bad = [int(x) for x in nbad.cpu().numpy()]
                ok = bad == [0, 0] and bool(torch.equal(app, msg)) and bool((copied == L).all())
                if not ok:
                    raise SystemExit(f"{line} {shape} {form} {mname}: wrong result (nbad {bad})")
                print(json.dumps({"line": line, "shape": shape, "form": form, "mode": mname, "ms": ms,
                                  "bytes": n * (2 * L + HDR)}), flush=True)
        del msg, ring, app, descs
        torch.cuda.synchronize()


def drive():
    lib_a = arg("--lib-a")
    if not lib_a or not os.path.exists(lib_a):
        sys.exit("--lib-a: the parent commit's liblampi_csum.so is required for line A")
    lines = arg("--lines", "A,B").split(",")
    out = arg("--out", os.path.join(ROOT, "profiles", "r08", "recv_unpack_ab.txt"))
    rounds = int(arg("--rounds", "5"))
    envs = {"A": {"LAMPI_CSUM_LIB": os.path.abspath(lib_a)}, "B": {}}
    times = {}  # (shape, mode) -> column -> [(ms, bytes)]
    failed = None
    for r in range(rounds):
        for line in lines:
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
                    col = "A" if line == "A" else f"{line} {x['form']}"
                    times.setdefault((x["shape"], x["mode"]), {}).setdefault(col, []).append((x["ms"], x["bytes"]))
            print(f"round {r} line {line} done", flush=True)
        if failed:
            break
    cols = ["A"] + [f"{ln} {form}" for ln in lines if ln != "A" for form in ("desc", "msg")]
    rows = ["receive step A/B: median ms of %d fresh processes per line (share of 8 TB/s; bytes = payload read + written "
            "+ 72 per slot)" % rounds,
            "A = header check / compare + copy_to_app_batch (parent commit's library, no host read-back); B = "
            "recv_unpack_batch (desc) / msg_recv_unpack (msg); "
            "spread = max - min of A's repeats; * = behind A by more than that",
            f"{'shape':5s} {'mode':4s} " + " ".join(f"{c:>17s}" for c in cols) + f" {'A spread':>9s}"]
    for key in sorted(times):
        t = times[key]
        a = statistics.median(m for m, _ in t["A"]) if "A" in t else None
        spread = max(m for m, _ in t["A"]) - min(m for m, _ in t["A"]) if "A" in t else 0.0
        cells = []
        for col in cols:
            if col not in t:
                cells.append(f"{'-':>17s}")
                continue
            med = statistics.median(m for m, _ in t[col])
            late = "*" if a is not None and col != "A" and med > a + spread else " "
            cells.append(f"{med:8.4f} ({t[col][0][1] / (med * 1e-3) / 8e12:5.3f}){late}")
        rows.append(f"{key[0]:5s} {key[1]:4s} " + " ".join(cells) + f" {spread:9.4f}")
    for key in sorted(times):
        for col in cols:
            if col in times[key]:
                rows.append(f"raw {key[0]} {key[1]} {col}: " + " ".join(f"{m:.4f}" for m, _ in times[key][col]))
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
