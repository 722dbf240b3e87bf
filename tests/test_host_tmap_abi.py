"""CPU: the ABI of the host-memory typemap steps (lampi_host_tmap_send_pack, lampi_host_tmap_recv_unpack_batch).

The struct layouts, the prototypes, that both names are declared, exported and bound, and a table of what the two
entry points refuse, as tests/test_host_pack_abi.py keeps for the contiguous host forms: a row is a well-formed call
with one thing changed and the value it must return (1 = hipErrorInvalidValue, 0 = an empty call answered before the
device is asked for).  The table runs in one child process with the devices hidden, so a call that passes validation
returns hipErrorNoDevice instead of touching a GPU; the well-formed calls must get that far (neither 0 nor 1).  Every
buffer a call could write -- the ring, the datatype's buffer, the five outputs -- holds a guard pattern that must be
unchanged after every row.
"""
import ctypes
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lampi_host_tmap_send_pack", "lampi_host_tmap_recv_unpack_batch")

CRC, SUM, NONE = 0, 1, 2
BY_BYTES = 0x100
HINT = 16 << 16  # LAMPI_CSUM_ROWS_HINT(16)
GM, IB, QUADRICS = 0, 1, 3
GUARD = 0xA5
RING_BYTES = 8192
COUNT = 64  # elements of T2 (packed_size 65): 4,160 packed bytes


def test_struct_layouts():
    from lampi_amd import _lib

    T, S = _lib.HostTmap, _lib.HostTmapSlot
    assert ctypes.sizeof(T) == 40 and ctypes.sizeof(S) == 32
    assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, _ in T._fields_] == [
        ("h_pairs", 0, 8), ("extent", 8, 8), ("packed_size", 16, 8), ("count", 24, 8), ("num_pairs", 32, 4),
        ("reserved", 36, 4)]
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [
        ("hdr_off", 0, 8), ("frag_off", 8, 8), ("pack_off", 16, 8), ("length", 24, 4), ("reserved", 28, 4)]


def test_prototypes():
    from lampi_amd import _lib

    c_int, p, z, u64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    assert _lib.PROTOTYPES[NAMES[0]] == (c_int, [p, p, u64, u64, z, p, z, p, c_int, c_int])
    assert _lib.PROTOTYPES[NAMES[1]] == (c_int, [p, z, p, z, c_int, p, p, p, p, p, p, p, c_int])


def test_declared_exported_and_bound():
    import lampi_amd
    from lampi_amd import host

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lampi_csum.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", lampi_amd._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    lib = lampi_amd.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(lib, name) is not None
    for struct in ("lampi_host_tmap", "lampi_host_tmap_slot"):
        assert re.search(r"\}\s*%s\s*;" % struct, src), struct
    for fn in ("make_host_tmap", "make_tmap_slots", "host_tmap_send_pack", "host_tmap_recv_unpack_batch"):
        assert callable(getattr(host, fn)), fn


class _Buffers:
    """The host memory the rows point into, every byte GUARD but the fill, the typemaps and the slot records."""

    def __init__(self):
        from lampi_amd import _lib

        mk = lambda n: (ctypes.c_uint8 * n)(*([GUARD] * n))
        self.base = mk(COUNT * 128 + 64)
        self.ring = mk(RING_BYTES)
        self.outs = {k: mk(64) for k in ("h_copied", "h_csum", "h_hdr_mask", "h_data_mask", "h_nbad")}
        self.fill = ctypes.create_string_buffer(112)
        self.keep = []
        self.lib = _lib

    def origin(self):
        return ctypes.addressof(self.base) + 32

    def tmap(self, pairs=((1, 70, 0), (13, -16, 1), (51, 0, 14)), **change):
        """T2 of tests/tmap_model.py over COUNT elements; pairs: (size, offset, seq_offset); change: struct fields."""
        arr = (self.lib.TmapElt * max(len(pairs), 1))()
        for i, (size, off, seq) in enumerate(pairs):
            arr[i] = self.lib.TmapElt(size, off, seq)
        t = self.lib.HostTmap(ctypes.addressof(arr), 128, 65, COUNT, len(pairs), 0)
        for k, v in change.items():
            setattr(t, k, v)
        self.keep += [arr, t]
        return ctypes.addressof(t)

    def slots(self, n=4, **change):
        """n records in 1,024-byte slots, 500-byte payloads behind 72-byte headers; change: fields of record 1."""
        arr = (self.lib.HostTmapSlot * n)()
        for i in range(n):
            arr[i] = self.lib.HostTmapSlot(i * 1024, i * 1024 + 72, i * 500, 500, 0)
        for k, v in change.items():
            setattr(arr[1], k, v)
        self.keep.append(arr)
        return ctypes.addressof(arr)

    def intact(self, counts_zeroed=False):
        nbad = self.outs["h_nbad"]
        ok = True
        if counts_zeroed:
            ok = bytes(nbad[0:8]) == bytes(8)
            for i in range(8):
                nbad[i] = GUARD
        guards = [self.ring, self.base] + list(self.outs.values())
        return ok and all(bytes(g) == bytes([GUARD]) * len(g) for g in guards)


def _tables(b):
    a = ctypes.addressof
    send = dict(h_base=b.origin(), h_tmap=b.tmap(), pack_off=0, pack_len=4096, frag_len=512, h_ring=a(b.ring),
                slot_stride=1024, h_fill=a(b.fill), hdr_kind=GM, mode=CRC)
    recv = dict(h_ring=a(b.ring), ring_bytes=RING_BYTES, h_slots=b.slots(), n=4, hdr_kind=GM, h_base=b.origin(),
                h_tmap=b.tmap(), **{k: a(v) for k, v in b.outs.items()}, mode=CRC)
    # the typemap rules, shared by both calls
    tmap_rows = [
        ("tmap null", dict(h_tmap=0), 1),
        ("pairs null", dict(h_tmap=b.tmap(h_pairs=0)), 1),
        ("num_pairs 0", dict(h_tmap=b.tmap(num_pairs=0)), 1),
        ("packed_size 0", dict(h_tmap=b.tmap(packed_size=0)), 1),
        ("tmap reserved set", dict(h_tmap=b.tmap(reserved=1)), 1),
        ("count * packed_size = 2^63", dict(h_tmap=b.tmap(pairs=((1 << 32, 0, 0),), packed_size=1 << 32,
                                                          count=1 << 31)), 1),
        ("count * packed_size wraps", dict(h_tmap=b.tmap(count=(1 << 64) - 1)), 1),
        ("seq_offset[0] != 0", dict(h_tmap=b.tmap(pairs=((1, 70, 1), (13, -16, 2), (51, 0, 15)))), 1),
        ("seq_offset[2] != seq_offset[1] + size[1]", dict(h_tmap=b.tmap(pairs=((1, 70, 0), (13, -16, 1),
                                                                               (51, 0, 15)))), 1),
        ("a size of 0", dict(h_tmap=b.tmap(pairs=((1, 70, 0), (0, -16, 1), (64, 0, 1)))), 1),
        ("sizes short of packed_size", dict(h_tmap=b.tmap(pairs=((1, 70, 0), (13, -16, 1)))), 1),
        ("sizes past packed_size", dict(h_tmap=b.tmap(pairs=((1, 70, 0), (13, -16, 1), (52, 0, 14)))), 1),
        ("a size that wraps the sum", dict(h_tmap=b.tmap(pairs=((1, 70, 0), ((1 << 64) - 1, -16, 1),
                                                                (65, 0, 0)))), 1),
    ]
    send_rows = [
        ("well-formed", {}, None),
        ("well-formed, window inside a pair", dict(pack_off=65 + 8, pack_len=4000), None),
        ("well-formed, Quadrics", dict(hdr_kind=QUADRICS, slot_stride=640), None),
        ("well-formed, Quadrics bare queue", dict(hdr_kind=QUADRICS, slot_stride=128), None),
        ("well-formed, IB, SUM", dict(hdr_kind=IB, mode=SUM), None),
        ("well-formed, NONE", dict(mode=NONE), None),
        ("well-formed, unaligned ring and stride", dict(h_ring=a(b.ring) + 3, slot_stride=585), None),
        ("well-formed, empty window", dict(pack_len=0), None),
        ("well-formed, empty window at the end", dict(pack_off=COUNT * 65, pack_len=0), None),
        ("fill null", dict(h_fill=0), 1),
        ("ring null", dict(h_ring=0), 1),
        ("kind 2", dict(hdr_kind=2), 1),
        ("kind 4", dict(hdr_kind=4), 1),
        ("kind -1", dict(hdr_kind=-1), 1),
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("BY_BYTES", dict(mode=CRC | BY_BYTES), 1),
        ("frag_len 0", dict(frag_len=0), 1),
        ("frag_len over 1 GiB", dict(frag_len=(1 << 30) + 1, slot_stride=1 << 31), 1),
        ("slot stride below header + frag_len", dict(slot_stride=583), 1),
        ("slot stride below the header", dict(slot_stride=64), 1),
        ("Quadrics slot stride below 128 + frag_len", dict(hdr_kind=QUADRICS, slot_stride=639), 1),
        ("GM stride 128 is no bare queue", dict(slot_stride=128), 1),
        ("window ends past the message", dict(pack_off=100, pack_len=COUNT * 65 - 99), 1),
        ("window starts past the message", dict(pack_off=COUNT * 65 + 1, pack_len=0), 1),
        ("window wraps", dict(pack_off=(1 << 64) - 8, pack_len=16), 1),
        ("2^32 fragments", dict(h_tmap=b.tmap(pairs=((1 << 32, 0, 0),), packed_size=1 << 32, count=2),
                                frag_len=1, slot_stride=128, pack_len=1 << 32), 1),
    ] + tmap_rows
    recv_rows = [
        ("well-formed", {}, None),
        ("well-formed, NONE", dict(mode=NONE), None),
        ("well-formed, Quadrics, header at the ring's end", dict(hdr_kind=QUADRICS,
                                                                 h_slots=b.slots(hdr_off=RING_BYTES - 128)), None),
        ("well-formed, pack_off at the end, payload anywhere", dict(h_slots=b.slots(pack_off=COUNT * 65,
                                                                                    frag_off=1 << 40)), None),
        ("well-formed, pack_off past the end", dict(h_slots=b.slots(pack_off=1 << 62, frag_off=1 << 40)), None),
        ("well-formed, truncating fragment", dict(h_slots=b.slots(pack_off=COUNT * 65 - 100)), None),
        ("well-formed, Quadrics inline, payload offset ignored",
         dict(hdr_kind=QUADRICS, h_slots=b.slots(length=52, frag_off=1 << 40)), None),
        ("n == 0", dict(n=0), 0),
        ("n == 0, ring and records null", dict(n=0, h_ring=0, h_slots=0), 0),
        ("ring null", dict(h_ring=0), 1),
        ("records null", dict(h_slots=0), 1),
        ("kind 2", dict(hdr_kind=2), 1),
        ("kind 2, n == 0", dict(hdr_kind=2, n=0), 1),
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("BY_BYTES", dict(mode=SUM | BY_BYTES), 1),
        ("n over 2^32 - 1", dict(n=1 << 32), 1),
        ("reserved set", dict(h_slots=b.slots(reserved=1)), 1),
        ("header starts past the ring", dict(h_slots=b.slots(hdr_off=RING_BYTES + 1)), 1),
        ("header ends past the ring", dict(h_slots=b.slots(hdr_off=RING_BYTES - 71)), 1),
        ("Quadrics header ends past the ring", dict(hdr_kind=QUADRICS, h_slots=b.slots(hdr_off=RING_BYTES - 127)), 1),
        ("header offset wraps", dict(h_slots=b.slots(hdr_off=(1 << 64) - 8)), 1),
        ("payload starts past the ring", dict(h_slots=b.slots(frag_off=RING_BYTES + 1)), 1),
        ("payload ends past the ring", dict(h_slots=b.slots(frag_off=RING_BYTES - 499)), 1),
        ("payload ends past the ring, NONE", dict(mode=NONE, h_slots=b.slots(frag_off=RING_BYTES - 499)), 1),
        ("payload offset wraps", dict(h_slots=b.slots(frag_off=(1 << 64) - 8)), 1),
        ("length over 1 GiB", dict(h_slots=b.slots(length=(1 << 30) + 1)), 1),
        ("length over 1 GiB, nothing to copy", dict(h_slots=b.slots(length=(1 << 30) + 1, pack_off=COUNT * 65)), 1),
        ("n == 0, tmap null", dict(n=0, h_tmap=0), 1),
    ] + tmap_rows + [(f"{k} null", {k: 0}, 1) for k in b.outs] + [(f"{k} null, n == 0", {k: 0, "n": 0}, 1)
                                                                   for k in b.outs]
    out = []
    for name, base, rows in ((NAMES[0], send, send_rows), (NAMES[1], recv, recv_rows)):
        for what, change, want in rows:
            assert set(change) <= set(base), (name, what)
            out.append((name, what, tuple(dict(base, **change).values()), want))
    return out


def _child():
    sys.path.insert(0, ROOT)
    from lampi_amd import _lib

    lib = _lib.lib()
    b = _Buffers()
    got = []
    for name, what, args, want in _tables(b):
        rc = getattr(lib, name)(*args)
        got.append([name, what, want, rc, b.intact(counts_zeroed=want == 0 and "recv" in name)])
    print(json.dumps(got))


def test_refusals_and_empty_calls_without_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) >= 90
    assert {name for name, *_ in got} == set(NAMES)
    wrong = []
    for name, what, want, rc, intact in got:
        if want is None:
            if rc in (0, 1):  # the well-formed call must get as far as the device (hipErrorNoDevice there)
                wrong.append(f"{name}: {what}: returned {rc}")
        elif rc != want:
            wrong.append(f"{name}: {what}: returned {rc}, expected {want}")
        if not intact:
            wrong.append(f"{name}: {what}: a guard byte changed")
    assert not wrong, "\n".join(wrong)


if __name__ == "__main__":
    _child()
