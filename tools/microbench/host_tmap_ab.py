"""The host-memory typemap steps, A/B: what the parent commit can do for a non-contiguous datatype in host memory
against lampi_host_tmap_send_pack and lampi_host_tmap_recv_unpack_batch.  Whole calls (they are synchronous), wall
clock, 1 warm-up and 3 reps per figure (a call of over a second is timed once, cold), page-locked buffers (lampi_host_register), GM's 65,456-byte fragments in
64 KiB slots.

  typemaps (round 10's)  v8    8-byte blocks at stride 24           v512  512-byte blocks at stride 1,024
                         s64   a struct of (4, 8, 52), extent 96    v64k  64 KiB blocks at stride 128 KiB
  each over a 256 MiB host buffer (count = 256 MiB / extent), the ring as large as the packed message needs

  send  A   lampi_host_chain_csum_batch over the reference walk's pieces (prebuilt), into ring + 72 (the parent
            commit's library, --lib-a PATH loaded through LAMPI_CSUM_LIB).  It does LESS than B: no header is
            written and none is checksummed.
        B   lampi_host_tmap_send_pack from this tree's library.
  recv  A   lampi_host_chain_copy_to_app_batch over the same pieces the other way, the expected values gathered
            beforehand: no header is tested.
        B   lampi_host_tmap_recv_unpack_batch.
  bar: B no further behind A than A's spread (max - min of its five).

The ring both receive lines drain is packed by the device form lampi_tmap_send_pack (both libraries have it) and
downloaded.  Every line checks its result.  Every line runs in a fresh child process under its own time limit; the
lines alternate --rounds times (default 5); a child that fails or runs out of time stops the rest, and the figures it
printed before are kept.

--sweep: the span route's ratio.  B alone, send, CRC: 8- and 512-byte blocks at strides from 2 to 33 host bytes per
packed byte, every type once by the pieces route alone and once by the span route, one child each.  The two
routes are two builds of this tree's library, CXXFLAGS += -DLAMPI_TMAP_SPAN_RATIO=0 and += -DLAMPI_TMAP_SPAN_RATIO=1000000
-DLAMPI_TMAP_SPAN_ROW_BYTES=1000000000 (--lib-pieces, --lib-span; there is no run-time switch).  The stride at which
the two columns cross is kTmapSpanRowBytes (lampi_amd/csrc/host_tmap_plan.h).

The tables (median ms, GiB/s of packed bytes, A's spread, * = behind the bar) go to --out (default
profiles/r13/host_tmap_ab.txt; the sweep is appended to it).

python tools/microbench/host_tmap_ab.py --lib-a /path/to/parent/liblampi_csum.so [--out FILE] [--rounds 5]
                                        [--modes crc,sum,none]
python tools/microbench/host_tmap_ab.py --sweep --lib-pieces PATH --lib-span PATH [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HDR, L, SLOT = 72, 65456, 65536
BUF = 256 << 20
TYPEMAPS = {  # name: (sizes, offsets, extent)
    "v8": ([8], [0], 24), "v512": ([512], [0], 1024), "s64": ([4, 8, 52], [0, 8, 40], 96),
    "v64k": ([65536], [0], 131072)}
SWEEP = [("b8", 8, s) for s in (16, 24, 40, 72, 136, 264)] + [("b512", 512, s) for s in (768, 1024, 1536, 2560, 4096)]
MODES = {"crc": 0, "sum": 1, "none": 2}
CHILD_LIMIT = 400  # seconds per child
NEW = ("lampi_host_tmap_send_pack", "lampi_host_tmap_recv_unpack_batch")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(run, reps=3):
    """Median of `reps` calls after a warm-up -- or the first call's own time where that takes over a second (the
    parent's per-piece path on the fine-grained types runs for seconds to tens of seconds a call)."""
    t0 = time.perf_counter()
    rc = run()
    first = (time.perf_counter() - t0) * 1e3
    assert rc == 0, rc
    if first > 1000.0:
        return first
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rc = run()
        t.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, rc
    return statistics.median(t)


class Shape:
    """A typemap over a BUF-byte page-locked host buffer, its ring, and the checks of both steps."""

    def __init__(self, np, lib, sizes, offsets, extent):
        self.np, self.lib = np, lib
        self.sizes, self.offsets, self.extent = list(sizes), list(offsets), extent
        self.ps = sum(sizes)
        self.count = BUF // extent
        self.total = self.count * self.ps
        self.n = (self.total + L - 1) // L
        self.base = self.pinned(self.count * extent)
        self.ring = self.pinned(self.n * SLOT)
        rng = np.random.default_rng(13)
        self.base[:] = rng.integers(0, 256, size=self.base.size, dtype=np.uint8)

    def pinned(self, nbytes):
        a = self.np.zeros(nbytes, self.np.uint8)
        assert self.lib.lampi_host_register(a.ctypes.data, a.nbytes) == 0
        return a

    def release(self):
        for x in (self.base, self.ring):
            self.lib.lampi_host_unregister(x.ctypes.data)

    def packed_of(self, buf):
        """The packed message of a buffer: the pairs' columns of the element matrix, side by side."""
        m = buf.reshape(self.count, self.extent)
        return self.np.concatenate([m[:, o:o + s] for s, o in zip(self.sizes, self.offsets)], axis=1).reshape(-1)

    def ring_payloads(self):
        full = self.total // L
        p = self.ring[:full * SLOT].reshape(full, SLOT)[:, HDR:HDR + L].reshape(-1)
        tail = self.ring[full * SLOT + HDR:full * SLOT + HDR + self.total - full * L]
        return self.np.concatenate([p, tail])


def child(line, modes, only=None):
    import numpy as np
    import torch

    from lampi_amd import _lib

    if line == "A":  # the parent commit's library has no host typemap symbols
        for k in NEW:
            _lib.PROTOTYPES.pop(k, None)
    from lampi_amd import device as dv
    from tmap_ab import pieces_of

    lib = _lib.lib()
    tmpl = np.arange(HDR, dtype=np.uint8)
    fill = _lib.SendHdrFill()
    fill.tmpl[:] = tmpl.tolist()
    fill.frag_seq0, fill.frag_seq_step, fill.desc_ptr0, fill.desc_ptr_stride, fill.seq_offset0 = 1, 1, 4096, 256, 0
    shapes = TYPEMAPS if only is None else {only[0]: ([only[1]], [0], only[2])}
    for tname, (sizes, offsets, extent) in shapes.items():
        x = Shape(np, lib, sizes, offsets, extent)
        want = x.packed_of(x.base)
        n, total = x.n, x.total
        pairs = np.zeros(len(sizes), dtype=np.dtype([("size", "<u8"), ("offset", "<i8"), ("seq_offset", "<i8")]))
        pairs["size"], pairs["offset"] = sizes, offsets
        pairs["seq_offset"] = np.concatenate(([0], np.cumsum(sizes[:-1])))
        htm = _lib.HostTmap(pairs.ctypes.data, extent, x.ps, x.count, len(sizes), 0)
        b, r = x.base.ctypes.data, x.ring.ctypes.data
        k = np.arange(n, dtype=np.uint64)
        lens = np.minimum(L, total - np.arange(n, dtype=np.int64) * L).astype(np.uint32)
        out = np.zeros(n, np.uint32)
        copied, csum = np.zeros(n, np.int64), np.zeros(n, np.uint32)
        hmask, dmask, nbad = np.zeros(n // 32 + 1, np.uint32), np.zeros(n // 32 + 1, np.uint32), np.zeros(2, np.uint32)
        if line == "A":
            src, dst, plen, first = pieces_of(np, sizes, offsets, extent, total, L, SLOT)
            rec = np.dtype([("src", "<u8"), ("dst", "<u8"), ("copylen", "<u4"), ("csumlen", "<u4"),
                            ("partial", "<u4"), ("reserved", "<u4")])
            sp, rp = np.zeros(len(plen), rec), np.zeros(len(plen), rec)
            sp["src"], sp["dst"] = np.uint64(b) + src.astype(np.uint64), np.uint64(r) + dst.astype(np.uint64)
            rp["src"], rp["dst"] = sp["dst"], sp["src"]
            for p in (sp, rp):
                p["copylen"] = p["csumlen"] = plen
                p["partial"] = 0xFFFFFFFF
            first = np.ascontiguousarray(first, np.uint32)
        else:
            slots = np.zeros(n, dtype=np.dtype([("hdr_off", "<u8"), ("frag_off", "<u8"), ("pack_off", "<u8"),
                                                ("length", "<u4"), ("reserved", "<u4")]))
            slots["hdr_off"], slots["frag_off"] = k * np.uint64(SLOT), k * np.uint64(SLOT) + np.uint64(HDR)
            slots["pack_off"], slots["length"] = k * np.uint64(L), lens
        for mname in modes:
            mode = MODES[mname]
            # ---- send
            x.ring[:] = 0
            if line == "A":
                send = lambda: lib.lampi_host_chain_csum_batch(sp.ctypes.data, len(sp), first.ctypes.data, n,
                                                               out.ctypes.data, mode)
            else:
                send = lambda: lib.lampi_host_tmap_send_pack(b, ctypes.addressof(htm), 0, total, L, r, SLOT,
                                                             ctypes.addressof(fill), 0, mode)
            ms = timed(send)
            if not np.array_equal(x.ring_payloads(), want):
                raise SystemExit(f"{line} {tname} send {mname}: wrong payloads")
            print(json.dumps({"line": line, "shape": tname, "step": "send", "mode": mname, "ms": ms, "bytes": total}),
                  flush=True)
            if only is not None:
                continue
            # ---- receive: the ring as the device form packs it, into the same buffer zeroed
            dbase = torch.from_numpy(x.base).cuda()
            dring = torch.zeros(n * SLOT, dtype=torch.uint8, device="cuda")
            tm = dv.make_tmap(np.stack([sizes, offsets], axis=1), extent, x.count, "cuda")
            dv.tmap_send_pack(dbase, tm, L, dring, SLOT, tmpl, frag_seq0=1, frag_seq_step=1, desc_ptr0=4096,
                              desc_ptr_stride=256, seq_offset0=0, kind=0, mode=mode, pack_len=total)
            torch.cuda.synchronize()
            x.ring[:] = dring.cpu().numpy()
            del dring, dbase, tm
            keep = x.base.copy()
            x.base[:] = 0
            if line == "A":
                expected = np.ascontiguousarray(x.ring.reshape(n, SLOT)[:, 64:68]).view("<u4").reshape(n).copy()
                recv = lambda: lib.lampi_host_chain_copy_to_app_batch(rp.ctypes.data, len(rp), first.ctypes.data, n,
                                                                      expected.ctypes.data, copied.ctypes.data,
                                                                      csum.ctypes.data, dmask.ctypes.data,
                                                                      nbad.ctypes.data + 4, mode)
            else:
                recv = lambda: lib.lampi_host_tmap_recv_unpack_batch(r, x.ring.size, slots.ctypes.data, n, 0, b,
                                                                     ctypes.addressof(htm), copied.ctypes.data,
                                                                     csum.ctypes.data, hmask.ctypes.data,
                                                                     dmask.ctypes.data, nbad.ctypes.data, mode)
            nbad[:] = 0
            ms = timed(recv)
            if [int(v) for v in nbad] != [0, 0] or not np.array_equal(x.packed_of(x.base), want) or \
                    not (copied == lens).all():
                raise SystemExit(f"{line} {tname} recv {mname}: wrong result (nbad {nbad})")
            x.base[:] = keep
            print(json.dumps({"line": line, "shape": tname, "step": "recv", "mode": mname, "ms": ms, "bytes": total}),
                  flush=True)
        x.release()
        torch.cuda.synchronize()


def run_child(args, env_extra, times, key_of):
    env = {k: v for k, v in os.environ.items() if k != "LAMPI_CSUM_LIB"}
    env.update(env_extra)
    failed, stdout = None, ""
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, env=env,
                           capture_output=True, text=True, timeout=CHILD_LIMIT)
        stdout = p.stdout
        if p.returncode != 0:
            failed = f"{args}: exit {p.returncode}\n{p.stdout[-300:]}\n{p.stderr[-1500:]}"
    except subprocess.TimeoutExpired as e:
        stdout = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        failed = f"{args}: no result within {CHILD_LIMIT} s"
    for row in stdout.splitlines():
        if row.startswith("{"):
            x = json.loads(row)
            times.setdefault(key_of(x), []).append((x["ms"], x["bytes"]))
    return failed


def gib(ms, nbytes):
    return nbytes / (ms * 1e-3) / 2**30


def drive():
    lib_a = arg("--lib-a")
    out = arg("--out", os.path.join(ROOT, "profiles", "r13", "host_tmap_ab.txt"))
    rounds = int(arg("--rounds", "5"))
    modes = arg("--modes", "crc,sum,none")
    rows, failed = [], None
    if "--sweep" not in sys.argv:
        if not lib_a or not os.path.exists(lib_a):
            sys.exit("--lib-a: the parent commit's liblampi_csum.so is required for line A")
        times = {}  # (shape, step, mode, line) -> [(ms, bytes)]
        for r in range(rounds):
            for line, env in (("A", {"LAMPI_CSUM_LIB": os.path.abspath(lib_a)}), ("B", {})):
                failed = run_child([line, modes], env, times,
                                   lambda x: (x["shape"], x["step"], x["mode"], x["line"]))
                print(f"round {r} line {line} {'FAILED' if failed else 'done'}", flush=True)
                if failed:
                    break
            if failed:
                break
        rows += [f"host typemap steps A/B: median ms of {rounds} fresh processes per line (GiB/s of packed bytes); "
                 "256 MiB page-locked buffers, 65,456-byte fragments in 64 KiB slots",
                 "send: A = host_chain_csum_batch over the walk's pieces (parent commit's library; writes no header), "
                 "B = host_tmap_send_pack",
                 "recv: A = host_chain_copy_to_app_batch (tests no header), B = host_tmap_recv_unpack_batch; "
                 "bar = A + A's spread;  * = B behind its bar",
                 f"{'shape':5s} {'step':4s} {'mode':4s} {'A':>19s} {'B':>20s} {'A spread':>9s} {'bar':>10s} {'A/B':>6s}"]
        for key in sorted({k[:3] for k in times}):
            ta, tb = times.get(key + ("A",)), times.get(key + ("B",))
            if not ta or not tb:
                continue
            a, b = (statistics.median(m for m, _ in t) for t in (ta, tb))
            spread = max(m for m, _ in ta) - min(m for m, _ in ta)
            nb = ta[0][1]
            rows.append(f"{key[0]:5s} {key[1]:4s} {key[2]:4s} {a:10.3f} ({gib(a, nb):6.2f}) {b:10.3f} "
                        f"({gib(b, nb):6.2f}){'*' if b > a + spread else ' '} {spread:9.3f} {a + spread:10.3f} "
                        f"{a / b:6.2f}")
        for key in sorted(times):
            rows.append("raw " + " ".join(key) + ": " + " ".join(f"{m:.3f}" for m, _ in times[key]))
        mode = "w"
    else:
        libs = {"pieces": arg("--lib-pieces"), "span": arg("--lib-span")}
        if not all(v and os.path.exists(v) for v in libs.values()):
            sys.exit("--sweep: --lib-pieces and --lib-span (this tree built for one route each, see the header comment)")
        times = {}  # (shape, route) -> [(ms, bytes)]
        for name, size, stride in SWEEP:
            for route in ("pieces", "span"):
                failed = run_child(["B", "crc", name, str(size), str(stride)],
                                   {"LAMPI_CSUM_LIB": os.path.abspath(libs[route])},
                                   times, lambda x, route=route: (x["shape"], route))
                print(f"sweep {name} stride {stride} {route} {'FAILED' if failed else 'done'}", flush=True)
                if failed:
                    break
            if failed:
                break
        rows += ["", "span-ratio sweep: host_tmap_send_pack, GM, CRC, 256 MiB page-locked buffer, one fresh process per "
                 "figure; ms (GiB/s of packed bytes)",
                 f"{'blocks':>6s} {'stride':>6s} {'ratio':>6s} {'pieces route':>20s} {'span route':>20s}  faster"]
        for name, size, stride in SWEEP:
            p, s = times.get((f"{name}@{stride}", "pieces")), times.get((f"{name}@{stride}", "span"))
            if not p or not s:
                continue
            (pm, nb), (sm, _) = p[0], s[0]
            rows.append(f"{size:6d} {stride:6d} {stride / size:6.2f} {pm:10.3f} ({gib(pm, nb):6.2f}) {sm:10.3f} "
                        f"({gib(sm, nb):6.2f})  {'span' if sm < pm else 'pieces'}")
        mode = "a"
    if failed:
        rows.append("STOPPED: " + failed)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, mode) as f:
        f.write("\n".join(rows) + "\n")
    print("\n".join(rows))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    if "--child" in sys.argv:
        a = sys.argv[sys.argv.index("--child") + 1:]
        only = (f"{a[2]}@{a[4]}", int(a[3]), int(a[4])) if len(a) > 2 else None
        child(a[0], a[1].split(","), only)
    else:
        drive()
