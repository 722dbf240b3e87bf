"""The send step, A/B: today's two-call sequence against the one-call forms (lampi_send_pack_batch,
lampi_msg_send_pack), whole rings on one stream, device events, 5 warm-ups and 20 reps per figure.

  GM ring  16,384 x 65,456-byte payloads in 64 KiB slots        IB ring  262,144 x 1,976 bytes in 2 KiB slots
  modes CRC, SUM and NONE; the message form and the descriptor form
  bytes counted: payload read + payload written + 72 header bytes per slot

  A   msg_bcopy_strided / frag_bcopy_batch_strided, then header_csum_batch_strided -- from a library built from the
      parent commit (--lib-a PATH, loaded through LAMPI_CSUM_LIB)
  B   msg_send_pack / send_pack_batch from this tree's library

Every line runs in a fresh child process under its own time limit; the lines alternate A, B five times and a
child that fails or runs out of time stops the rest.  The table (median of the five, A's spread = max - min of its
five, shares of 8 TB/s) goes to --out (default profiles/r07/send_pack_ab.txt).

python tools/microbench/send_pack_ab.py --lib-a /path/to/parent/liblampi_csum.so [--out FILE] [--rounds 5]
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


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(line):
    import numpy as np
    import torch

    from lampi_amd import _lib

    if line == "A":  # the parent commit's library has no send-pack symbols
        for k in ("lampi_send_pack_batch", "lampi_msg_send_pack"):
            _lib.PROTOTYPES.pop(k, None)
    from lampi_amd import device as dv

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
        k = np.arange(n, dtype=np.uint64)
        lens = np.full(n, L, np.uint64)
        descs = dv.make_copy_descs(msg, k * np.uint64(L), ring, k * np.uint64(slot) + np.uint64(HDR), lens, lens)
        for mname, mode in MODES:
            runs = {}
            if line == "A":
                def a_msg():
                    dv.msg_bcopy_strided(msg, L, ring[HDR:], slot, ring, slot, out_offset=64, mode=mode)
                    dv.header_csum_batch_strided(ring, n, slot, HDR - 4, 18, ring, slot, offset=68, mode=mode)

                def a_desc():
                    dv.frag_bcopy_batch_strided(descs, ring, slot, offset=64, mode=mode)
                    dv.header_csum_batch_strided(ring, n, slot, HDR - 4, 18, ring, slot, offset=68, mode=mode)

                runs = {"msg": a_msg, "desc": a_desc}
            else:
                runs = {"msg": lambda: dv.msg_send_pack(msg, L, ring, slot, tmpl, frag_seq0=1, frag_seq_step=1,
                                                        desc_ptr0=4096, desc_ptr_stride=256, kind=kind, mode=mode),
                        "desc": lambda: dv.send_pack_batch(descs, ring, slot, kind=kind, mode=mode)}
            for form, run in runs.items():
                ms = timed(run)
                print(json.dumps({"line": line, "shape": shape, "form": form, "mode": mname, "ms": ms,
                                  "bytes": n * (2 * L + HDR)}), flush=True)
        del msg, ring, descs
        torch.cuda.synchronize()


def drive():
    lib_a = arg("--lib-a")
    if not lib_a or not os.path.exists(lib_a):
        sys.exit("--lib-a: the parent commit's liblampi_csum.so is required for line A")
    out = arg("--out", os.path.join(ROOT, "profiles", "r07", "send_pack_ab.txt"))
    rounds = int(arg("--rounds", "5"))
    envs = {"A": {"LAMPI_CSUM_LIB": os.path.abspath(lib_a)}, "B": {}}
    times = {}  # (shape, form, mode) -> line -> [ms]
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
                failed = f"round {r} line {line}: exit {p.returncode}\n{p.stderr[-2000:]}"
                break
            for row in p.stdout.splitlines():
                if row.startswith("{"):
                    x = json.loads(row)
                    times.setdefault((x["shape"], x["form"], x["mode"]), {}).setdefault(line, []).append(
                        (x["ms"], x["bytes"]))
            print(f"round {r} line {line} done", flush=True)
        if failed:
            break
    rows = ["send step A/B: median ms of %d fresh processes per line (share of 8 TB/s; bytes = payload read + written "
            "+ 72 per slot)" % rounds,
            "A = bcopy_strided + header_csum_batch_strided (parent commit's library), B = the one-call form; "
            "spread = max - min of A's repeats",
            f"{'shape':5s} {'form':4s} {'mode':4s} {'A ms':>16s} {'A spread':>9s} {'B ms':>16s}  verdict"]
    for key in sorted(times):
        t = times[key]

        def cell(line):
            if line not in t:
                return None, f"{'-':>16s}"
            med = statistics.median(m for m, _ in t[line])
            return med, f"{med:8.4f} ({t[line][0][1] / (med * 1e-3) / 8e12:5.3f})"

        a, ca = cell("A")
        b, cb = cell("B")
        spread = max(m for m, _ in t["A"]) - min(m for m, _ in t["A"]) if "A" in t else 0.0
        verdict = ""
        if a is not None and b is not None:
            verdict = "B meets" if b <= a + spread else "B misses"
        rows.append(f"{key[0]:5s} {key[1]:4s} {key[2]:4s} {ca} {spread:9.4f} {cb}  {verdict}")
    for key in sorted(times):
        for line in ("A", "B"):
            if line in times[key]:
                rows.append(f"raw {key[0]} {key[1]} {key[2]} {line}: " + " ".join(f"{m:.4f}" for m, _ in times[key][line]))
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
