"""The Quadrics flavour of the send and receive steps, A/B: the generic sequence of the parent commit against the
one-call forms with LAMPI_SEND_HDR_QUADRICS, whole rings on one stream, device events, 5 warm-ups and 20 reps per
figure.

  packed small   262,144 x 2,048 bytes in 2,176-byte slots     descriptor and message forms, CRC, SUM and NONE
  packed large   16,384 x 65,536 bytes in 65,664-byte slots    descriptor and message forms, CRC and SUM
  inline         1,048,576 x 52 bytes in 128-byte envelopes    message form, CRC and SUM
  csum-only      the two packed shapes into a bare queue of 128-byte envelopes (send only): the message form, and
                 the descriptor form with copylen == 0
  bytes counted: payload read + payload written (none for csum-only) + 128 per envelope

  send  A  lampi_msg_bcopy_strided / lampi_frag_bcopy_batch_strided (csum-only: lampi_frag_csum_batch_strided over
           16-byte descriptors) with the checksum into the word @64, then lampi_header_csum_batch_strided into the
           word @124 -- crclen 124 and word_count 31: what (124, 32) gives over a zeroed word, without the zeroing
           a repeated call would need (which favours A)
        B  lampi_msg_send_pack / lampi_send_pack_batch
  recv  A  lampi_header_check_batch(128, 32, 124), then lampi_copy_to_app_batch reading the expected values out of
           the same headers (no host read-back of the mask in between, which favours A)
        B  lampi_msg_recv_unpack / lampi_recv_unpack_batch
  A runs a library built from the parent commit (--lib-a PATH, loaded through LAMPI_CSUM_LIB), B this tree's.

Every line runs in a fresh child process under its own time limit; A and B alternate five times and a child that
fails or runs out of time stops the rest.  Both lines check what they computed (every header passes
lampi_header_check_batch after a send; every byte delivered after a receive).  The table (median of the five, A's
spread = max - min of its five, shares of 8 TB/s) goes to --out (default profiles/r09/quadrics_ab.txt).

python tools/microbench/quadrics_ab.py --lib-a /path/to/parent/liblampi_csum.so [--out FILE] [--rounds 5]
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)

HDR, INLINE, Q = 128, 52, 3
# shape -> n, fragment length, slot, modes
SHAPES = {"small": (262144, 2048, 2176, ("crc", "sum", "none")), "large": (16384, 65536, 65664, ("crc", "sum")),
          "inline": (1048576, 52, 128, ("crc", "sum"))}
MODE = {"crc": 0, "sum": 1, "none": 2}
CHILD_LIMIT = 300  # seconds per child


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(line):
    import numpy as np
    import torch

    from lampi_amd import _lib
    from lampi_amd import device as dv

    L_ = _lib.lib()
    stream = int(torch.cuda.current_stream().cuda_stream)

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

    def report(step, shape, form, mname, ms, nbytes):
        print(json.dumps({"line": line, "step": step, "shape": shape, "form": form, "mode": mname, "ms": ms,
                          "bytes": nbytes}), flush=True)

    def ok(rc):
        assert rc == 0, rc

    tmpl = np.arange(72, dtype=np.uint8)
    fill = _lib.SendHdrFill()
    fill.tmpl[:] = tmpl.tolist()
    fill.frag_seq0, fill.frag_seq_step, fill.desc_ptr0, fill.desc_ptr_stride, fill.seq_offset0 = 1, 1, 4096, 256, 0
    import ctypes

    fp = ctypes.addressof(fill)
    for shape, (n, L, slot, modes) in SHAPES.items():
        inline = L <= INLINE
        pay = 72 if inline else HDR  # where slot k's payload lives
        msg = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        dv.fill_stream(msg, seed=13)
        ring = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
        app = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        k = np.arange(n, dtype=np.uint64)
        lens = np.full(n, L, np.uint64)
        # the envelopes' constant fields for line A (B's message form writes its own): dataLength, dataSeqOffset
        H = np.zeros((n, HDR), np.uint8)
        H[:, :72] = tmpl
        H[:, 20:24] = lens.astype("<u4").view(np.uint8).reshape(n, 4)
        H[:, 56:64] = (k * np.uint64(L)).astype("<u8").view(np.uint8).reshape(n, 8)
        H[:, 68:124] = 0
        Ht = torch.from_numpy(H).cuda()
        ring.view(n, slot)[:, :HDR] = Ht
        cdescs = dv.make_copy_descs(msg, k * np.uint64(L), ring, k * np.uint64(slot) + np.uint64(pay), lens, lens)
        rdescs = dv.make_recv_descs(ring, k * np.uint64(slot) + np.uint64(pay), app, k * np.uint64(L), lens,
                                    lens.astype(np.int64))
        words = (n + 31) // 32
        copied = torch.empty(n, dtype=torch.int64, device="cuda")
        csum = torch.empty(n, dtype=torch.int32, device="cuda")
        hmask, dmask = (torch.empty(words, dtype=torch.int32, device="cuda") for _ in range(2))
        nbad = torch.zeros(2, dtype=torch.int32, device="cuda")
        m, r, a = msg.data_ptr(), ring.data_ptr(), app.data_ptr()
        cd, rd = cdescs.data_ptr(), rdescs.data_ptr()
        c, s, hm, dm, nb = (t.data_ptr() for t in (copied, csum, hmask, dmask, nbad))
        for mname in modes:
            mode = MODE[mname]

            def hcsum(base=r, stride=slot):
                ok(L_.lampi_header_csum_batch_strided(base, n, stride, 124, 31, base + 124, stride, mode, stream))

            def a_send_msg():
                ok(L_.lampi_msg_bcopy_strided(m, n * L, L, r + pay, slot, 0xFFFFFFFF, r + 64, slot, mode, stream))
                hcsum()

            def a_send_desc():
                ok(L_.lampi_frag_bcopy_batch_strided(cd, n, r + 64, slot, mode, stream))
                hcsum()

            def a_recv():
                if mode != 2:
                    ok(L_.lampi_header_check_batch(r, n, slot, HDR, 32, 124, hm, nb, mode, stream))
                ok(L_.lampi_copy_to_app_batch(rd, n, r + 64, slot, c, s, dm, nb + 4, mode, stream))

            if line == "A":
                sends = {"msg": a_send_msg} if inline else {"msg": a_send_msg, "desc": a_send_desc}
                recvs = {"msg": a_recv} if inline else {"msg": a_recv, "desc": a_recv}
            else:
                sends = {"msg": lambda: ok(L_.lampi_msg_send_pack(m, n * L, L, r, slot, fp, Q, mode, stream))}
                recvs = {"msg": lambda: ok(L_.lampi_msg_recv_unpack(r, n, slot, Q, a, n * L, 0, c, s, hm, dm, nb, mode,
                                                                    stream))}
                if not inline:
                    sends["desc"] = lambda: ok(L_.lampi_send_pack_batch(cd, n, r, slot, Q, mode, stream))
                    recvs["desc"] = lambda: ok(L_.lampi_recv_unpack_batch(rd, n, r, slot, Q, c, s, hm, dm, nb, mode,
                                                                          stream))
            nbytes = n * (2 * L + HDR)
            for form, run in sends.items():
                ring.view(n, slot)[:, :HDR] = Ht
                ms = timed(run)
                if mode != 2:
                    nbad.zero_()
                    ok(L_.lampi_header_check_batch(r, n, slot, HDR, 32, 124, hm, nb, mode, stream))
                    if int(nbad[0].item()) != 0:
                        raise SystemExit(f"{line} send {shape} {form} {mname}: {int(nbad[0].item())} headers fail")
                report("send", shape, form, mname, ms, nbytes)
            for form, run in recvs.items():  # (over the ring the last send left)
                app.zero_()
                nbad.zero_()
                copied.zero_()
                ms = timed(run)
                bad = [int(x) for x in nbad.cpu().numpy()]
                if not (bad == [0, 0] and bool(torch.equal(app, msg)) and bool((copied == L).all())):
                    raise SystemExit(f"{line} recv {shape} {form} {mname}: wrong result (nbad {bad})")
                report("recv", shape, form, mname, ms, nbytes)
        # checksum-only sends into a bare envelope queue (send only)
        if not inline:
            queue = torch.zeros(n * HDR, dtype=torch.uint8, device="cuda")
            q = queue.data_ptr()
            queue.view(n, HDR)[:] = Ht
            fdescs = dv.make_descs(msg, k * np.uint64(L), lens)
            zdescs = dv.make_copy_descs(msg, k * np.uint64(L), ring, k * np.uint64(slot) + np.uint64(HDR),
                                        np.zeros(n, np.uint64), lens)
            fd, zd = fdescs.data_ptr(), zdescs.data_ptr()
            for mname in ("crc", "sum"):
                mode = MODE[mname]

                def a_csum():
                    ok(L_.lampi_frag_csum_batch_strided(fd, n, q + 64, HDR, mode, stream))
                    ok(L_.lampi_header_csum_batch_strided(q, n, HDR, 124, 31, q + 124, HDR, mode, stream))

                if line == "A":
                    runs = {"msg": a_csum, "desc": a_csum}
                else:
                    runs = {"msg": lambda: ok(L_.lampi_msg_send_pack(m, n * L, L, q, HDR, fp, Q, mode, stream)),
                            "desc": lambda: ok(L_.lampi_send_pack_batch(zd, n, q, HDR, Q, mode, stream))}
                for form, run in runs.items():
                    queue.view(n, HDR)[:] = Ht
                    ms = timed(run)
                    nbad.zero_()
                    ok(L_.lampi_header_check_batch(q, n, HDR, HDR, 32, 124, hm, nb, mode, stream))
                    if int(nbad[0].item()) != 0:
                        raise SystemExit(f"{line} csum-only {shape} {form} {mname}: headers fail")
                    report("send", shape + "-csum-only", form, mname, ms, n * (L + HDR))
            del queue, fdescs, zdescs
        del msg, ring, app, cdescs, rdescs, Ht
        torch.cuda.synchronize()


def drive():
    lib_a = arg("--lib-a")
    if not lib_a or not os.path.exists(lib_a):
        sys.exit("--lib-a: the parent commit's liblampi_csum.so is required for line A")
    out = arg("--out", os.path.join(ROOT, "profiles", "r09", "quadrics_ab.txt"))
    rounds = int(arg("--rounds", "5"))
    envs = {"A": {"LAMPI_CSUM_LIB": os.path.abspath(lib_a)}, "B": {}}
    times = {}  # (step, shape, form, mode) -> line -> [(ms, bytes)]
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
            for row in p.stdout.splitlines():
                if row.startswith("{"):
                    x = json.loads(row)
                    times.setdefault((x["step"], x["shape"], x["form"], x["mode"]), {}).setdefault(line, []).append(
                        (x["ms"], x["bytes"]))
            if p.returncode != 0:
                failed = f"round {r} line {line}: exit {p.returncode}\n{p.stdout[-500:]}\n{p.stderr[-2000:]}"
                break
            print(f"round {r} line {line} done", flush=True)
        if failed:
            break
    rows = ["Quadrics send and receive steps, A/B: median ms of %d fresh processes per line (share of 8 TB/s; bytes = "
            "payload read + written + 128 per envelope; csum-only: payload read + 128)" % rounds,
            "A = the generic sequence (parent commit's library), B = the one-call form with LAMPI_SEND_HDR_QUADRICS; "
            "spread = max - min of A's repeats; B meets when B <= A + spread",
            f"{'step':4s} {'shape':16s} {'form':4s} {'mode':4s} {'A ms':>16s} {'A spread':>9s} {'B ms':>16s}  verdict"]
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
        rows.append(f"{key[0]:4s} {key[1]:16s} {key[2]:4s} {key[3]:4s} {ca} {spread:9.4f} {cb}  {verdict}")
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
