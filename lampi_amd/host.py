"""The one-call send and receive steps over host memory (numpy arrays), through liblampi_csum.so.

``host_msg_send_pack`` packs fragments of a host message into a host NIC ring -- headers, payloads, dataChecksum
and the header checksum -- and ``host_recv_unpack_batch`` tests, delivers and verifies a drained batch of such
slots (include/lampi_csum.h: lampi_host_msg_send_pack, lampi_host_recv_unpack_batch).  The arrays may be
pageable or page-locked (``host_register``); the work is done on the GPU, the CPU touches no payload byte.
``host_tmap_send_pack`` and ``host_tmap_recv_unpack_batch`` are the same two steps for a non-contiguous datatype,
its typemap from ``make_host_tmap`` (lampi_host_tmap_send_pack, lampi_host_tmap_recv_unpack_batch).
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import CRC32, HDR_GM, HDR_QUADRICS, HostRecvSlot, HostTmap, HostTmapSlot, SendHdrFill, check, lib

SEND_HDR_BYTES = 72
QUADRICS_HDR_BYTES = 128
QUADRICS_INLINE_BYTES = 52


def _bytes(a: np.ndarray, what: str) -> np.ndarray:
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
        raise ValueError(f"{what} must be a contiguous 1-D uint8 array")
    return a


def make_fill(tmpl, frag_seq0: int = 0, frag_seq_step: int = 0, desc_ptr0: int = 0, desc_ptr_stride: int = 0,
              seq_offset0: int = 0) -> SendHdrFill:
    """A ``lampi_send_hdr_fill``: the 72 template bytes and the start and step of the per-fragment series."""
    t = np.ascontiguousarray(np.frombuffer(bytes(tmpl), dtype=np.uint8) if not isinstance(tmpl, np.ndarray)
                             else tmpl.view(np.uint8).reshape(-1))
    if t.size != SEND_HDR_BYTES:
        raise ValueError("tmpl must be 72 bytes")
    fill = SendHdrFill()
    fill.tmpl[:] = t.tolist()
    m64 = 2**64 - 1
    fill.frag_seq0, fill.frag_seq_step = frag_seq0 & m64, frag_seq_step & m64
    fill.desc_ptr0, fill.desc_ptr_stride = desc_ptr0 & m64, desc_ptr_stride & m64
    fill.seq_offset0 = seq_offset0 & m64
    return fill


def host_msg_send_pack(msg: np.ndarray, frag_len: int, ring: np.ndarray, slot_stride: int, fill: SendHdrFill,
                       kind: int = HDR_GM, mode: int = CRC32, k_first: int = 0, k_count: int | None = None,
                       ring_offset: int = 0) -> np.ndarray:
    """Fragments [k_first, k_first + k_count) of ``msg`` (default: all) packed into the slots at ``ring`` +
    ring_offset + i*slot_stride: each slot's header built from ``fill`` for its fragment of the whole message,
    its payload, dataChecksum and header checksum as ``kind`` and ``mode`` say.  Returns ``ring``."""
    _bytes(msg, "msg")
    _bytes(ring, "ring")
    if not ring.flags.writeable:
        raise ValueError("ring must be writeable")
    if frag_len < 1:
        raise ValueError("frag_len must be at least 1")
    nfr = (msg.size - 1) // frag_len + 1 if msg.size else 1
    if k_count is None:
        k_count = nfr - k_first
    if k_first < 0 or k_count < 0 or k_first + k_count > nfr:
        raise ValueError("fragment range outside the message")
    hb = QUADRICS_HDR_BYTES if kind == HDR_QUADRICS else SEND_HDR_BYTES
    bare = kind == HDR_QUADRICS and slot_stride == QUADRICS_HDR_BYTES
    if k_count:
        last = min(frag_len, msg.size - (k_first + k_count - 1) * frag_len) if msg.size else 0
        tail = hb if (bare or (kind == HDR_QUADRICS and last <= QUADRICS_INLINE_BYTES)) else hb + last
        if ring_offset < 0 or ring_offset + (k_count - 1) * slot_stride + tail > ring.size:
            raise ValueError("ring is too small")
    check(lib().lampi_host_msg_send_pack(msg.ctypes.data if msg.size else None, msg.size, frag_len, k_first, k_count,
                                         ring.ctypes.data + ring_offset, slot_stride, ctypes.addressof(fill), kind,
                                         mode), "lampi_host_msg_send_pack")
    return ring


def make_recv_slots(hdr_offs, frag_offs, app: np.ndarray, app_offs, lengths, app_lens):
    """An array of ``lampi_host_recv_slot``: fragment i = lengths[i] bytes at ring offset frag_offs[i] behind the
    header at hdr_offs[i], delivered to ``app`` + app_offs[i] with app_lens[i] bytes of room (may be <= 0)."""
    _bytes(app, "app")
    n = len(lengths)
    if not (len(hdr_offs) == len(frag_offs) == len(app_offs) == len(app_lens) == n):
        raise ValueError("slot fields differ in size")
    rec = np.zeros(n, dtype=np.dtype([("hdr_off", "<u8"), ("frag_off", "<u8"), ("app", "<u8"), ("app_len", "<i8"),
                                      ("length", "<u4"), ("reserved", "<u4")]))
    assert rec.dtype.itemsize == ctypes.sizeof(HostRecvSlot)
    rec["hdr_off"], rec["frag_off"] = np.asarray(hdr_offs, np.uint64), np.asarray(frag_offs, np.uint64)
    rec["app"] = np.uint64(app.ctypes.data) + np.asarray(app_offs, np.uint64)
    rec["app_len"], rec["length"] = np.asarray(app_lens, np.int64), np.asarray(lengths, np.uint32)
    copy = np.minimum(rec["length"].astype(np.int64), np.maximum(rec["app_len"], 0))
    if n and int((np.asarray(app_offs, np.int64) + copy).max()) > app.size:
        raise ValueError("a delivery extends past the end of app")
    return rec


def host_recv_unpack_batch(ring: np.ndarray, slots: np.ndarray, kind: int = HDR_GM, mode: int = CRC32):
    """The receive step over a host ring: returns (copied int64[n], csum uint32[n], hdr_mask uint32[ceil(n/32)],
    data_mask, nbad uint32[2]).  ``slots`` comes from ``make_recv_slots``, whose ``app`` array receives the
    deliveries and must stay alive and in place during the call."""
    _bytes(ring, "ring")
    n = len(slots)
    words = max(1, (n + 31) // 32)
    copied, csum = np.empty(max(n, 1), np.int64), np.empty(max(n, 1), np.uint32)
    hmask, dmask, nbad = np.zeros(words, np.uint32), np.zeros(words, np.uint32), np.empty(2, np.uint32)
    check(lib().lampi_host_recv_unpack_batch(ring.ctypes.data, ring.size, slots.ctypes.data if n else None, n, kind,
                                             copied.ctypes.data, csum.ctypes.data, hmask.ctypes.data,
                                             dmask.ctypes.data, nbad.ctypes.data, mode),
          "lampi_host_recv_unpack_batch")
    return copied[:n], csum[:n], hmask, dmask, nbad


class HostTmapHandle:
    """A ``lampi_host_tmap`` with the pair array it points to kept alive."""

    def __init__(self, pairs: np.ndarray, extent: int, packed_size: int, count: int):
        self.pairs = pairs
        self.tmap = HostTmap(pairs.ctypes.data, extent & (2**64 - 1), packed_size, count, len(pairs), 0)

    @property
    def total(self) -> int:
        return self.tmap.count * self.tmap.packed_size

    def addr(self) -> int:
        return ctypes.addressof(self.tmap)


def make_host_tmap(sizes, offsets, extent: int, count: int) -> HostTmapHandle:
    """A typemap in host memory: pairs (size, offset) in packed order, seq_offset their running sum
    (``ULMTypeMapElt_t`` as it is), the datatype's extent and the message's element count."""
    sizes, offsets = np.asarray(sizes, np.uint64), np.asarray(offsets, np.int64)
    if sizes.ndim != 1 or sizes.shape != offsets.shape or sizes.size == 0:
        raise ValueError("sizes and offsets must be equal-length, non-empty 1-D arrays")
    pairs = np.zeros(sizes.size, dtype=np.dtype([("size", "<u8"), ("offset", "<i8"), ("seq_offset", "<i8")]))
    pairs["size"], pairs["offset"] = sizes, offsets
    pairs["seq_offset"] = np.concatenate(([0], np.cumsum(sizes[:-1].astype(np.int64))))
    return HostTmapHandle(pairs, extent, int(sizes.sum()), count)


def host_tmap_send_pack(base: np.ndarray, origin: int, tmap: HostTmapHandle, pack_off: int, pack_len: int,
                        frag_len: int, ring: np.ndarray, slot_stride: int, fill: SendHdrFill, kind: int = HDR_GM,
                        mode: int = CRC32, ring_offset: int = 0) -> np.ndarray:
    """Packed bytes [pack_off, pack_off + pack_len) of the message whose datatype origin is ``base[origin]``, gathered
    through ``tmap`` and packed into the slots at ``ring`` + ring_offset + j*slot_stride as ``host_msg_send_pack``
    packs a contiguous message of those bytes.  Returns ``ring``."""
    _bytes(base, "base")
    _bytes(ring, "ring")
    if not ring.flags.writeable:
        raise ValueError("ring must be writeable")
    if frag_len < 1 or pack_off < 0 or pack_len < 0 or pack_off + pack_len > tmap.total:
        raise ValueError("window outside the message")
    hb = QUADRICS_HDR_BYTES if kind == HDR_QUADRICS else SEND_HDR_BYTES
    bare = kind == HDR_QUADRICS and slot_stride == QUADRICS_HDR_BYTES
    nfr = (pack_len - 1) // frag_len + 1 if pack_len else 1
    last = pack_len - (nfr - 1) * frag_len
    tail = hb if (bare or (kind == HDR_QUADRICS and last <= QUADRICS_INLINE_BYTES)) else hb + last
    if ring_offset < 0 or ring_offset + (nfr - 1) * slot_stride + tail > ring.size:
        raise ValueError("ring is too small")
    check(lib().lampi_host_tmap_send_pack(base.ctypes.data + origin, tmap.addr(), pack_off, pack_len, frag_len,
                                          ring.ctypes.data + ring_offset, slot_stride, ctypes.addressof(fill), kind,
                                          mode), "lampi_host_tmap_send_pack")
    return ring


def make_tmap_slots(hdr_offs, frag_offs, pack_offs, lengths) -> np.ndarray:
    """An array of ``lampi_host_tmap_slot``: fragment i = lengths[i] bytes at ring offset frag_offs[i] behind the
    header at hdr_offs[i], its first byte packed byte pack_offs[i] of the message."""
    n = len(lengths)
    if not (len(hdr_offs) == len(frag_offs) == len(pack_offs) == n):
        raise ValueError("slot fields differ in size")
    rec = np.zeros(n, dtype=np.dtype([("hdr_off", "<u8"), ("frag_off", "<u8"), ("pack_off", "<u8"),
                                      ("length", "<u4"), ("reserved", "<u4")]))
    assert rec.dtype.itemsize == ctypes.sizeof(HostTmapSlot)
    rec["hdr_off"], rec["frag_off"] = np.asarray(hdr_offs, np.uint64), np.asarray(frag_offs, np.uint64)
    rec["pack_off"], rec["length"] = np.asarray(pack_offs, np.uint64), np.asarray(lengths, np.uint32)
    return rec


def host_tmap_recv_unpack_batch(ring: np.ndarray, slots: np.ndarray, base: np.ndarray, origin: int,
                                tmap: HostTmapHandle, kind: int = HDR_GM, mode: int = CRC32):
    """The receive step over a host ring into the datatype at ``base[origin]``: returns (copied int64[n], csum
    uint32[n], hdr_mask uint32[ceil(n/32)], data_mask, nbad uint32[2]) as ``host_recv_unpack_batch`` does, the
    deliveries scattered through ``tmap`` (``slots`` from ``make_tmap_slots``)."""
    _bytes(ring, "ring")
    _bytes(base, "base")
    if not base.flags.writeable:
        raise ValueError("base must be writeable")
    n = len(slots)
    words = max(1, (n + 31) // 32)
    copied, csum = np.empty(max(n, 1), np.int64), np.empty(max(n, 1), np.uint32)
    hmask, dmask, nbad = np.zeros(words, np.uint32), np.zeros(words, np.uint32), np.empty(2, np.uint32)
    check(lib().lampi_host_tmap_recv_unpack_batch(ring.ctypes.data, ring.size, slots.ctypes.data if n else None, n,
                                                  kind, base.ctypes.data + origin, tmap.addr(), copied.ctypes.data,
                                                  csum.ctypes.data, hmask.ctypes.data, dmask.ctypes.data,
                                                  nbad.ctypes.data, mode), "lampi_host_tmap_recv_unpack_batch")
    return copied[:n], csum[:n], hmask, dmask, nbad


def host_register(a: np.ndarray) -> None:
    """Page-lock ``a`` for direct DMA (lampi_host_register); undo with ``host_unregister``."""
    check(lib().lampi_host_register(a.ctypes.data, a.nbytes), "lampi_host_register")


def host_unregister(a: np.ndarray) -> None:
    check(lib().lampi_host_unregister(a.ctypes.data), "lampi_host_unregister")
