"""The descriptor forms of the typemap steps (lampi_tmap_send_pack_batch, lampi_tmap_recv_unpack_batch), A/B: one
typemap call per message against one batch call for all of them, and the price of the per-fragment records on a
single message.  Whole rings on one stream through the C ABI with every argument and output prebuilt (no binding
work inside the timed region), device events, 3 warm-ups and 10 reps per figure.

  case M   many messages, four fragments each, the datatypes T1, T2 and T4a of tests/tmap_model.py in rotation:
           ib  256 messages x 4 x 1,976 bytes in 2 KiB slots      gm  64 messages x 4 x 65,456 bytes in 64 KiB slots
           A   one lampi_tmap_send_pack / lampi_tmap_recv_unpack per message, from a library built from the parent
               commit (--lib-a PATH, loaded through LAMPI_CSUM_LIB)
           B   one lampi_tmap_send_pack_batch / lampi_tmap_recv_unpack_batch over the same slots, records grouped by
               message, from this tree's library
  case U   one message: 1,024 x 65,456 bytes of T1 in 64 KiB slots, this tree's library both times:
           ring     lampi_tmap_send_pack / lampi_tmap_recv_unpack
           records  the same fragments handed over as records
  modes    CRC and SUM; send and receive

Every line runs in a fresh child process under its own time limit; the lines alternate A, B five times and a child
that fails or runs out of time stops the rest.  The table (medians of the five, A's spread = max - min of its five)
goes to --out (default profiles/r11/tmap_batch_ab.txt).

python tools/microbench/tmap_batch_ab.py --lib-a /path/to/parent/liblampi_csum.so [--out FILE] [--rounds 5]
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HDR = 72
CASES_M = {"ib": (256, 1976, 2048, 1), "gm": (64, 65456, 65536, 0)}  # messages, payload, slot, header kind
FRAGS = 4
CASE_U = (1024, 65456, 65536, 0)
MODES = (("crc", 0), ("sum", 1))
CHILD_LIMIT = 420  # seconds per child
SEQ0 = 4096
NEW = ("lampi_tmap_send_pack_batch", "lampi_tmap_recv_unpack_batch")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(line):
    import numpy as np
    import torch

    import tmap_model as tmm
    from lampi_amd import _lib

    if line == "A":  # the parent commit's library has no descriptor forms
        for k in NEW:
            _lib.PROTOTYPES.pop(k, None)
    from lampi_amd import device as dv

    lib = _lib.lib()
    stream = None

    def timed(run, reps=10):
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def fill_of(tmpl):
        f = _lib.SendHdrFill()
        f.tmpl[:] = tmpl.tolist()
        f.frag_seq0, f.frag_seq_step, f.desc_ptr0, f.desc_ptr_stride, f.seq_offset0 = 1, 1, 4096, 256, SEQ0
        return f

    def outputs(n):
        return [torch.empty(max(n, 1), dtype=torch.int64, device="cuda"),
                torch.empty(max(n, 1), dtype=torch.int32, device="cuda"),
                torch.empty(max(n, 1), dtype=torch.int32, device="cuda"),  # (a mask word per message in case M's A)
                torch.empty(max(n, 1), dtype=torch.int32, device="cuda"),
                torch.empty(2, dtype=torch.int32, device="cuda")]

    def message(tm, nbytes, seed):
        count = tmm.count_for(tm, nbytes)
        lo, hi = tm.span(count)
        origin = 32 - min(lo, 0)
        buf = torch.empty(origin + hi + 32, dtype=torch.uint8, device="cuda")
        dv.fill_stream(buf, seed=seed)
        return dv.make_tmap(tm.pairs(), tm.extent, count, "cuda"), buf, origin

    def emit(case, ring, d, mname, ms, nbytes):
        print(json.dumps({"line": line, "case": case, "ring": ring, "dir": d, "mode": mname, "ms": ms,
                          "bytes": nbytes}), flush=True)

    def ring_calls(msgs, ring, L, slot, kind, mode, fill, outs):
        """One typemap call per message: message k's fragments in slots [k nf, (k + 1) nf)."""
        o = [x.data_ptr() for x in outs]
        sends, recvs = [], []
        for k, (tm, buf, origin, nf) in enumerate(msgs):
            rp, bp = ring.data_ptr() + k * FRAGS * slot if nf == FRAGS else ring.data_ptr(), buf.data_ptr() + origin
            tp, fp = ctypes.addressof(tm.struct), ctypes.addressof(fill)
            sends.append((bp, tp, 0, nf * L, L, rp, slot, fp, kind, mode, stream))
            recvs.append((rp, nf, slot, kind, bp, tp, SEQ0, o[0] + 8 * k * FRAGS, o[1] + 4 * k * FRAGS, o[2] + 4 * k,
                          o[3] + 4 * k, o[4], mode, stream))

        def send():
            for a in sends:
                if lib.lampi_tmap_send_pack(*a):
                    sys.exit("lampi_tmap_send_pack failed")

        def recv():
            for a in recvs:
                if lib.lampi_tmap_recv_unpack(*a):
                    sys.exit("lampi_tmap_recv_unpack failed")

        return send, recv

    def batch_calls(msgs, ring, L, slot, kind, mode, outs):
        """One batch call: the same slots as records grouped by message."""
        table = dv.make_tmap_msgs([(tm, buf, origin) for tm, buf, origin, _ in msgs], "cuda")
        msg = np.concatenate([np.full(nf, k, np.int64) for k, (_, _, _, nf) in enumerate(msgs)])
        j = np.concatenate([np.arange(nf, dtype=np.int64) for _, _, _, nf in msgs])
        n = len(msg)
        frags = dv.make_tmap_frags(ring.data_ptr() + np.arange(n, dtype=np.int64) * slot + HDR, j * L,
                                   np.full(n, L), msg, "cuda")
        o = [x.data_ptr() for x in outs]
        sa = (frags.data_ptr(), n, table.table.data_ptr(), len(table), L, ring.data_ptr(), slot, kind, mode, stream)
        ra = sa[:8] + tuple(o) + (mode, stream)

        def send():
            if lib.lampi_tmap_send_pack_batch(*sa):
                sys.exit("lampi_tmap_send_pack_batch failed")

        def recv():
            if lib.lampi_tmap_recv_unpack_batch(*ra):
                sys.exit("lampi_tmap_recv_unpack_batch failed")

        return send, recv, (table, frags)

    def measure(case, rname, variants, build, outs, nbytes, mname):
        build()  # a valid ring for the receive figures
        for vname, (send, recv) in variants:
            recv()
            torch.cuda.synchronize()
            if int(outs[4].cpu().numpy().sum()) != 0:
                sys.exit(f"{line} {case} {rname} {vname} {mname}: the receive step reported failures on a valid ring")
            for d, run in (("recv", recv), ("send", send)):
                emit(case + vname, rname, d, mname, timed(run), nbytes)

    tmpl = np.arange(HDR, dtype=np.uint8)
    fill = fill_of(tmpl)
    rotation = (tmm.T1, tmm.T2, tmm.T4A)
    for rname, (nmsg, L, slot, kind) in CASES_M.items():
        msgs = [message(rotation[k % 3], FRAGS * L, 20 + k) + (FRAGS,) for k in range(nmsg)]
        ring = torch.empty(nmsg * FRAGS * slot, dtype=torch.uint8, device="cuda")
        dv.fill_stream(ring, seed=19)
        outs = outputs(nmsg * FRAGS)
        for mname, mode in MODES:
            send, recv = ring_calls(msgs, ring, L, slot, kind, mode, fill, outs)
            variants = [("", (send, recv))]
            if line == "B":
                bs, br, keep = batch_calls(msgs, ring, L, slot, kind, mode, outs)
                variants = [("", (bs, br))]
            measure("M", rname, variants, send, outs, nmsg * FRAGS * (2 * L + HDR), mname)
        del msgs, ring
        torch.cuda.synchronize()
    if line == "B":
        n, L, slot, kind = CASE_U
        one = [message(tmm.T1, n * L, 18) + (n,)]
        ring = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
        dv.fill_stream(ring, seed=17)
        outs = outputs(n)
        for mname, mode in MODES:
            send, recv = ring_calls(one, ring, L, slot, kind, mode, fill, outs)
            bs, br, keep = batch_calls(one, ring, L, slot, kind, mode, outs)
            measure("U", "gm", [("-ring", (send, recv)), ("-records", (bs, br))], send, outs, n * (2 * L + HDR), mname)


def drive():
    lib_a = arg("--lib-a")
    if not lib_a or not os.path.exists(lib_a):
        sys.exit("--lib-a: the parent commit's liblampi_csum.so is required for line A")
    out = arg("--out", os.path.join(ROOT, "profiles", "r11", "tmap_batch_ab.txt"))
    rounds = int(arg("--rounds", "5"))
    envs = {"A": {"LAMPI_CSUM_LIB": os.path.abspath(lib_a)}, "B": {}}
    times = {}  # (case, ring, dir, mode) -> line -> [(ms, bytes)]
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
                    times.setdefault((x["case"], x["ring"], x["dir"], x["mode"]), {}).setdefault(line, []).append(
                        (x["ms"], x["bytes"]))
            print(f"round {r} line {line} done", flush=True)
        if failed:
            break

    def med(runs):
        return statistics.median(m for m, _ in runs)

    def cell(runs):
        m = med(runs)
        return f"{m:9.4f} ({runs[0][1] / (m * 1e-3) / 1e9:5.0f})"

    rows = ["typemap descriptor forms A/B: median ms of %d fresh processes per line (GB/s; bytes = packed bytes read + "
            "written + 72 per slot)" % rounds,
            "case M: A = one typemap call per message (parent commit's library), B = one batch call; spread = max - "
            "min of A's repeats; B is ahead when A - B exceeds that spread",
            f"{'dir':4s} {'ring':4s} {'mode':4s} {'A ms':>17s} {'A spread':>9s} {'B ms':>17s} {'A/B':>7s}  verdict"]
    not_ahead = []
    for key in sorted(k for k in times if k[0] == "M"):
        t = times[key]
        if "A" not in t or "B" not in t:
            continue
        a, b = med(t["A"]), med(t["B"])
        spread = max(m for m, _ in t["A"]) - min(m for m, _ in t["A"])
        ahead = a - b > spread
        if not ahead:
            not_ahead.append(" ".join(key[1:]))
        rows.append(f"{key[2]:4s} {key[1]:4s} {key[3]:4s} {cell(t['A'])} {spread:9.4f} {cell(t['B'])} {a / b:7.2f}  "
                    f"{'B ahead' if ahead else 'B not ahead'}")
    rows.append("not ahead: " + (", ".join(not_ahead) if not_ahead else "none"))
    rows += ["case U: one message of 1,024 x 65,456 bytes of T1, this tree's library: the ring form against the same "
             "fragments as records; ratio = records / ring",
             f"{'dir':4s} {'mode':4s} {'ring ms':>17s} {'records ms':>17s} {'ratio':>6s}"]
    for key in sorted(k for k in times if k[0] == "U-ring"):
        rec = times.get(("U-records",) + key[1:], {}).get("B")
        ring = times[key].get("B")
        if rec and ring:
            rows.append(f"{key[2]:4s} {key[3]:4s} {cell(ring)} {cell(rec)} {med(rec) / med(ring):6.3f}")
    for key in sorted(times):
        for line in ("A", "B"):
            if line in times[key]:
                rows.append(f"raw {' '.join(key)} {line}: " + " ".join(f"{m:.4f}" for m, _ in times[key][line]))
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
