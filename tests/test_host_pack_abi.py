"""CPU: the ABI of the host-memory one-call steps (lampi_host_msg_send_pack, lampi_host_recv_unpack_batch).

The record layout, and a table of what the two entry points refuse, as tests/test_abi_refusals.py keeps for the
device entry points: a row is a well-formed call with one thing changed and the value it must return (1 =
hipErrorInvalidValue, 0 = an empty call answered before the device is asked for).  The table runs in one child
process with the devices hidden, so a call that passes validation returns hipErrorNoDevice instead of touching a
GPU; the well-formed calls must get that far (neither 0 nor 1).  Every buffer a call could write -- the ring, the
application buffer, the five outputs -- holds a guard pattern that must be unchanged after every row.
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CRC, SUM, NONE = 0, 1, 2
BY_BYTES = 0x100
HINT = 16 << 16  # LAMPI_CSUM_ROWS_HINT(16)
GM, IB, QUADRICS = 0, 1, 3
GUARD = 0xA5
RING_BYTES = 8192


def test_slot_record_layout():
    from lampi_amd import _lib

    S = _lib.HostRecvSlot
    assert ctypes.sizeof(S) == 40
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [
        ("hdr_off", 0, 8), ("frag_off", 8, 8), ("app", 16, 8), ("app_len", 24, 8), ("length", 32, 4),
        ("reserved", 36, 4)]


def test_prototypes():
    from lampi_amd import _lib

    c_int, p, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.PROTOTYPES["lampi_host_msg_send_pack"] == (c_int, [p, z, z, z, z, p, z, p, c_int, c_int])
    assert _lib.PROTOTYPES["lampi_host_recv_unpack_batch"] == (c_int, [p, z, p, z, c_int, p, p, p, p, p, c_int])


class _Buffers:
    """The host memory the rows point into, every byte GUARD but the message, the fill and the slot records."""

    def __init__(self):
        from lampi_amd import _lib

        mk = lambda n: (ctypes.c_uint8 * n)(*([GUARD] * n))
        self.msg = mk(4096)
        self.ring = mk(RING_BYTES)
        self.app = mk(4096)
        self.outs = {k: mk(64) for k in ("h_copied", "h_csum", "h_hdr_mask", "h_data_mask", "h_nbad")}
        self.fill = ctypes.create_string_buffer(112)
        self.keep = []
        self.Slot = _lib.HostRecvSlot

    def slots(self, n=4, **change):
        """n records in 1,024-byte slots, 500-byte payloads behind 72-byte headers; change: fields of record 1."""
        arr = (self.Slot * n)()
        for i in range(n):
            arr[i] = self.Slot(i * 1024, i * 1024 + 72, ctypes.addressof(self.app) + i * 512, 500, 500, 0)
        for k, v in change.items():
            setattr(arr[1], k, v)
        self.keep.append(arr)
        return ctypes.addressof(arr)

    def intact(self, counts_zeroed=False):
        """Every guard byte as it was -- but for an empty receive's two counts, which must be 0 -- and the counts'
        guard put back."""
        nbad = self.outs["h_nbad"]
        ok = True
        if counts_zeroed:
            ok = bytes(nbad[0:8]) == bytes(8)
            for i in range(8):
                nbad[i] = GUARD
        guards = [self.ring, self.app] + list(self.outs.values())
        return ok and all(bytes(g) == bytes([GUARD]) * len(g) for g in guards)


def _tables(b):
    a = ctypes.addressof
    send = dict(h_msg=a(b.msg), msg_len=4096, frag_len=512, k_first=0, k_count=8, h_ring=a(b.ring), slot_stride=1024,
                h_fill=a(b.fill), hdr_kind=GM, mode=CRC)
    recv = dict(h_ring=a(b.ring), ring_bytes=RING_BYTES, h_slots=b.slots(), n=4, hdr_kind=GM,
                **{k: a(v) for k, v in b.outs.items()}, mode=CRC)
    send_rows = [
        ("well-formed", {}, None),
        ("well-formed, Quadrics bare queue", dict(hdr_kind=QUADRICS, slot_stride=128), None),
        ("well-formed, Quadrics inline at stride 128", dict(hdr_kind=QUADRICS, slot_stride=128, frag_len=52), None),
        ("well-formed, unaligned ring and stride", dict(h_ring=a(b.ring) + 3, slot_stride=585), None),
        ("k_count == 0", dict(k_count=0), 0),
        ("k_count == 0 at the end", dict(k_first=8, k_count=0), 0),
        ("k_count == 0, message null", dict(k_count=0, h_msg=0), 1),
        ("fill null", dict(h_fill=0), 1),
        ("fill null, k_count == 0", dict(h_fill=0, k_count=0), 1),
        ("ring null", dict(h_ring=0), 1),
        ("message null", dict(h_msg=0), 1),
        ("kind 2", dict(hdr_kind=2), 1),
        ("kind 4", dict(hdr_kind=4), 1),
        ("kind -1", dict(hdr_kind=-1), 1),
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("BY_BYTES", dict(mode=CRC | BY_BYTES), 1),
        ("frag_len 0", dict(frag_len=0), 1),
        ("frag_len over 1 GiB", dict(frag_len=(1 << 30) + 1, slot_stride=1 << 31, k_count=1), 1),
        ("range starts past the message", dict(k_first=9, k_count=0), 1),
        ("range ends past the message", dict(k_first=4, k_count=5), 1),
        ("empty message, two fragments", dict(msg_len=0, k_count=2), 1),
        ("slot stride below header + frag_len", dict(slot_stride=583), 1),
        ("slot stride below the header", dict(slot_stride=64), 1),
        ("Quadrics slot stride below 128 + frag_len", dict(hdr_kind=QUADRICS, slot_stride=639), 1),
        ("Quadrics slot stride below the envelope", dict(hdr_kind=QUADRICS, slot_stride=120, frag_len=8), 1),
        ("GM stride 128 is no bare queue", dict(slot_stride=128), 1),
    ]
    recv_rows = [
        ("well-formed", {}, None),
        ("well-formed, NONE", dict(mode=NONE), None),
        ("well-formed, Quadrics, header at the ring's end", dict(hdr_kind=QUADRICS,
                                                                 h_slots=b.slots(hdr_off=RING_BYTES - 128)), None),
        ("well-formed, nothing to copy, payload anywhere", dict(h_slots=b.slots(app_len=0, frag_off=1 << 40, app=0)),
         None),
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
        ("length over 1 GiB, nothing to copy", dict(h_slots=b.slots(length=(1 << 30) + 1, app_len=0)), 1),
        ("application address null", dict(h_slots=b.slots(app=0)), 1),
    ] + [(f"{k} null", {k: 0}, 1) for k in b.outs] + [(f"{k} null, n == 0", {k: 0, "n": 0}, 1) for k in b.outs]
    out = []
    for name, base, rows in (("lampi_host_msg_send_pack", send, send_rows),
                             ("lampi_host_recv_unpack_batch", recv, recv_rows)):
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
    assert len(got) >= 60
    assert {name for name, *_ in got} == {"lampi_host_msg_send_pack", "lampi_host_recv_unpack_batch"}
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
