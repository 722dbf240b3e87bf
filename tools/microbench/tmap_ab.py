"""The typemap send and receive steps, A/B/C: today's per-piece sequence against the one-call typemap forms
(lampi_tmap_send_pack, lampi_tmap_recv_unpack) and against the contiguous ring forms as the ceiling; whole rings on
one stream, device events, 3 warm-ups and 10 reps per figure.

  typemaps  v8     8-byte blocks at stride 24            v512   512-byte blocks at stride 1,024
            s64    a struct of (4, 8, 52) with extent 96  v64k   64 KiB blocks at stride 128 KiB
  rings     gm     1,024 x 65,456-byte payloads in 64 KiB slots   ib   32,768 x 1,976 bytes in 2 KiB slots
  modes     CRC, SUM and NONE; send and receive
  bytes counted: packed bytes read + written + 72 header bytes per slot; A's descriptor bytes are listed apart

  A   send: chain_csum_batch_strided over the typemap's pieces (prebuilt, resident on the device), then
      header_csum_batch_strided; receive: header_check_batch (IB: header_compare_batch), then
      chain_copy_to_app_batch -- from a library built from the parent commit (--lib-a PATH, loaded through
      LAMPI_CSUM_LIB)
  B   tmap_send_pack / tmap_recv_unpack from this tree's library
  C   msg_send_pack / msg_recv_unpack of the same packed bytes from / into a contiguous buffer: the ceiling

Every line runs in a fresh child process under its own time limit; the lines alternate A, B, C five times and a
child that fails or runs out of time stops the rest.  The table (median of the five, A's spread = max - min of its
five, B's share of C) goes to --out (default profiles/r10/tmap_ab.txt).

python tools/microbench/tmap_ab.py --lib-a /path/to/parent/liblampi_csum.so [--out FILE] [--rounds 5]
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)

HDR = 72
TYPEMAPS = {  # name: (sizes, offsets, extent)
    "v8": ([8], [0], 24), "v512": ([512], [0], 1024), "s64": ([4, 8, 52], [0, 8, 40], 96),
    "v64k": ([65536], [0], 131072)}
RINGS = {"gm": (1024, 65456, 65536, 0), "ib": (32768, 1976, 2048, 1)}  # n, payload, slot, header kind
MODES = (("crc", 0), ("sum", 1), ("none", 2))
CHILD_LIMIT = 420  # seconds per child
SEQ0 = 4096


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def pieces_of(np, sizes, offsets, extent, total, L, slot):
    """The typemap pieces of every fragment, cut as the reference's walk cuts them (at pair and at fragment
    boundaries): (byte index in the typemap buffer, byte index in the ring, bytes, first piece of each fragment)."""
    sizes, offsets = np.asarray(sizes, np.int64), np.asarray(offsets, np.int64)
    seq = np.concatenate(([0], np.cumsum(sizes[:-1])))
    ps = int(sizes.sum())
    count = (total + ps - 1) // ps
    starts = (np.arange(count, dtype=np.int64)[:, None] * ps + seq[None, :]).reshape(-1)
    starts = np.union1d(starts[starts < total], np.arange(0, total, L, dtype=np.int64))
    lens = np.diff(np.append(starts, total))
    e, r = starts // ps, starts % ps
    i = np.searchsorted(seq, r, side="right") - 1
    src = e * extent + offsets[i] + (r - seq[i])
    dst = (starts // L) * slot + HDR + starts % L
    first = np.searchsorted(starts, np.arange((total + L - 1) // L + 1, dtype=np.int64) * L)
    return src, dst, lens, first.astype(np.int32)


def child(line):
    import numpy as np
    import torch

    from lampi_amd import _lib

    if line == "A":  # the parent commit's library has no typemap symbols
        for k in ("lampi_tmap_send_pack", "lampi_tmap_recv_unpack"):
            _lib.PROTOTYPES.pop(k, None)
    from lampi_amd import device as dv

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

    tmpl = np.arange(HDR, dtype=np.uint8)
    for rname, (n, L, slot, kind) in RINGS.items():
        total = n * L
        msg = torch.empty(total, dtype=torch.uint8, device="cuda")  # the packed bytes (C's message, the rings' payloads)
        dv.fill_stream(msg, seed=13)
        ring = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
        for tname, (sizes, offsets, extent) in TYPEMAPS.items():
            if line == "C" and tname != "v8":
                continue  # (the ceiling does not depend on the typemap: measured once per ring)
            ps = sum(sizes)
            count = (total + ps - 1) // ps
            buf = None
            if line != "C":
                buf = torch.empty(count * extent, dtype=torch.uint8, device="cuda")
                dv.fill_stream(buf, seed=14)
            desc_bytes = 0
            if line == "A":
                src, dst, lens, first = pieces_of(np, sizes, offsets, extent, total, L, slot)
                send_pieces = dv.make_copy_descs(buf, src, ring, dst, lens, lens)
                recv_pieces = dv.make_copy_descs(ring, dst, buf, src, lens, lens)
                first_t = torch.from_numpy(first).to("cuda")
                desc_bytes = 32 * len(lens)
                del src, dst, lens
            elif line == "B":
                tm = dv.make_tmap(np.stack([sizes, offsets], axis=1), extent, count, "cuda")
            for mname, mode in MODES:
                if line == "A":
                    def send():
                        dv.chain_csum_batch_strided(send_pieces, first_t, ring, slot, offset=64, mode=mode)
                        dv.header_csum_batch_strided(ring, n, slot, HDR - 4, 18, ring, slot, offset=68, mode=mode)

                    def recv():
                        if mode != 2:
                            if kind == 0:
                                dv.header_check_batch(ring, n, slot, HDR, 18, 68, mode=mode)
                            else:
                                dv.header_compare_batch(ring, n, slot, HDR - 4, 68, mode=mode)
                        return dv.chain_copy_to_app_batch(recv_pieces, first_t, None if mode == 2 else ring[64:], slot,
                                                          mode=mode)[3]
                elif line == "B":
                    def send():
                        dv.tmap_send_pack(buf, tm, L, ring, slot, tmpl, frag_seq0=1, frag_seq_step=1, desc_ptr0=4096,
                                          desc_ptr_stride=256, seq_offset0=SEQ0, kind=kind, mode=mode, pack_len=total)

                    def recv():
                        return dv.tmap_recv_unpack(ring, n, slot, buf, tm, kind=kind, mode=mode, seq_offset0=SEQ0)[4]
                else:
                    app = torch.empty(total, dtype=torch.uint8, device="cuda")

                    def send():
                        dv.msg_send_pack(msg, L, ring, slot, tmpl, frag_seq0=1, frag_seq_step=1, desc_ptr0=4096,
                                         desc_ptr_stride=256, seq_offset0=SEQ0, kind=kind, mode=mode)

                    def recv():
                        return dv.msg_recv_unpack(ring, n, slot, app, kind=kind, mode=mode, seq_offset0=SEQ0)[4]
                # a valid ring of the packed bytes for the receive figures, built the same way in every line
                dv.msg_send_pack(msg, L, ring, slot, tmpl, frag_seq0=1, frag_seq_step=1, desc_ptr0=4096,
                                 desc_ptr_stride=256, seq_offset0=SEQ0, kind=kind, mode=mode)
                nbad = recv()
                torch.cuda.synchronize()
                if int(nbad.cpu().numpy().sum()) != 0:
                    sys.exit(f"{line} {rname} {tname} {mname}: the receive step reported failures on a valid ring")
                for d, run in (("recv", recv), ("send", send)):
                    ms = timed(run)
                    print(json.dumps({"line": line, "ring": rname, "tmap": tname, "dir": d, "mode": mname, "ms": ms,
                                      "bytes": n * (2 * L + HDR), "desc_bytes": desc_bytes}), flush=True)
            if line == "A":
                del send_pieces, recv_pieces, first_t
            del buf
            torch.cuda.synchronize()
        del msg, ring
        torch.cuda.synchronize()


def drive():
    lib_a = arg("--lib-a")
    if not lib_a or not os.path.exists(lib_a):
        sys.exit("--lib-a: the parent commit's liblampi_csum.so is required for line A")
    out = arg("--out", os.path.join(ROOT, "profiles", "r10", "tmap_ab.txt"))
    rounds = int(arg("--rounds", "5"))
    envs = {"A": {"LAMPI_CSUM_LIB": os.path.abspath(lib_a)}, "B": {}, "C": {}}
    times = {}  # (dir, ring, tmap, mode) -> line -> [(ms, bytes, desc_bytes)]
    failed = None
    for r in range(rounds):
        for line in ("A", "B", "C"):
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
                    times.setdefault((x["dir"], x["ring"], x["tmap"], x["mode"]), {}).setdefault(line, []).append(
                        (x["ms"], x["bytes"], x["desc_bytes"]))
            print(f"round {r} line {line} done", flush=True)
        if failed:
            break
    rows = ["typemap steps A/B/C: median ms of %d fresh processes per line (GB/s; bytes = packed bytes read + written "
            "+ 72 per slot)" % rounds,
            "A = today's per-piece sequence (parent commit's library; its descriptor bytes listed, not counted), "
            "B = the one-call typemap form, C = the contiguous ring form (the ceiling); spread = max - min of A's repeats",
            f"{'dir':4s} {'ring':4s} {'tmap':5s} {'mode':4s} {'A ms':>17s} {'A spread':>9s} {'A desc MB':>9s} "
            f"{'B ms':>17s} {'C ms':>17s} {'B/C':>5s}  verdict"]
    behind = []
    for key in sorted(times):
        t = times[key]
        c_t = times.get((key[0], key[1], "v8", key[3]), {})

        def cell(runs):
            if not runs:
                return None, f"{'-':>17s}"
            med = statistics.median(m for m, _, _ in runs)
            return med, f"{med:9.4f} ({runs[0][1] / (med * 1e-3) / 1e9:5.0f})"

        a, ca = cell(t.get("A"))
        b, cb = cell(t.get("B"))
        c, cc = cell(c_t.get("C"))
        spread = max(m for m, _, _ in t["A"]) - min(m for m, _, _ in t["A"]) if "A" in t else 0.0
        desc = t["A"][0][2] / 1e6 if "A" in t else 0.0
        verdict = ""
        if a is not None and b is not None:
            verdict = "B meets" if b <= a + spread else "B behind"
            if b > a + spread:
                behind.append(" ".join(key))
        share = f"{c / b:5.2f}" if b and c else f"{'-':>5s}"
        rows.append(f"{key[0]:4s} {key[1]:4s} {key[2]:5s} {key[3]:4s} {ca} {spread:9.4f} {desc:9.1f} {cb} {cc} {share}  "
                    f"{verdict}")
    rows.append("behind: " + (", ".join(behind) if behind else "none"))
    for key in sorted(times):
        for line in ("A", "B", "C"):
            if line in times[key]:
                rows.append(f"raw {' '.join(key)} {line}: " + " ".join(f"{m:.4f}" for m, _, _ in times[key][line]))
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
