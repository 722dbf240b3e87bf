"""Device-resident batched checksums over torch CUDA tensors (HIP on ROCm).

PyTorch is only plumbing here: it owns HBM buffers and streams.  Every checksum is
computed by the gfx950 kernels behind the C ABI (lampi_frag_csum_batch, lampi_frag_bcopy_batch,
lampi_msg_csum).
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import (BY_BYTES, CRC32, CRC_INITIAL_REGISTER, HDR_GM, HDR_IB, HDR_QUADRICS, NONE, RECV_DATA_BAD, RECV_HDR_BAD,
                   SUM32, SendHdrFill, Tmap, check, lib, rows_hint_bits)

__all__ = ["CRC32", "SUM32", "NONE", "HDR_GM", "HDR_IB", "HDR_QUADRICS", "RECV_DATA_BAD", "RECV_HDR_BAD", "recv_unpack_batch", "msg_recv_unpack",
           "make_tmap", "tmap_send_pack", "tmap_recv_unpack",
           "make_tmap_msgs", "make_tmap_frags", "tmap_send_pack_batch", "tmap_recv_unpack_batch",
           "send_pack_batch", "msg_send_pack","chain_copy_to_app_batch", "frag_bcopy_batch_strided", "msg_bcopy_strided",
           "chain_csum_batch_strided", "header_csum_batch_strided", "frag_csum_batch", "diag_frag_csum_batch_per_wave", "frag_csum64_batch", "frag_bcopy_batch", "msg_bcopy", "msg_csum", "fill_stream", "fill_stream_frags",
           "make_descs", "make_copy_descs", "as_u32", "chain_csum_batch", "header_csum_batch", "header_check_batch", "check_data_batch",
           "mask_bits", "make_recv_descs", "copy_to_app_batch"]


def _stream_handle(stream: torch.cuda.Stream | None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{what} must be a device (cuda) tensor")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def as_u32(t: torch.Tensor) -> np.ndarray:
    """Checksum tensor (int32 storage) -> numpy uint32 on the host."""
    return t.detach().cpu().numpy().view(np.uint32)


def make_descs(base: torch.Tensor, offsets, lengths, partials=None) -> torch.Tensor:
    """Build a device array of ``lampi_frag_desc`` (n x 16 bytes, int64 [n, 2] storage)."""
    _require_cuda(base, "base")
    off = np.asarray(offsets, dtype=np.uint64)
    ln = np.asarray(lengths, dtype=np.uint64)
    n = off.size
    if ln.size != n:
        raise ValueError("offsets and lengths differ in size")
    if n and int((off + ln).max()) > base.numel() * base.element_size():
        raise ValueError("a fragment extends past the end of the base tensor")
    if n and int(ln.max()) > 0xFFFFFFFF:
        raise ValueError("fragment length exceeds 32 bits")
    pt = (np.full(n, CRC_INITIAL_REGISTER, dtype=np.uint64) if partials is None
          else np.asarray(partials, dtype=np.uint64) & 0xFFFFFFFF)
    host = np.empty((n, 2), dtype=np.uint64)
    host[:, 0] = np.uint64(base.data_ptr()) + off
    host[:, 1] = ln | (pt << np.uint64(32))
    return torch.from_numpy(host.view(np.int64)).to(base.device)


def make_copy_descs(src: torch.Tensor, src_offsets, dst: torch.Tensor, dst_offsets, copylens, csumlens,
                    partials=None) -> torch.Tensor:
    """Build a device array of ``lampi_copy_desc`` (n x 32 bytes, int64 [n, 4] storage)."""
    _require_cuda(src, "src")
    _require_cuda(dst, "dst")
    so = np.asarray(src_offsets, dtype=np.uint64)
    do = np.asarray(dst_offsets, dtype=np.uint64)
    cl = np.asarray(copylens, dtype=np.uint64)
    sl = np.asarray(csumlens, dtype=np.uint64)
    n = so.size
    if not (do.size == cl.size == sl.size == n):
        raise ValueError("descriptor fields differ in size")
    if n:
        if int(np.maximum(cl, sl).max()) > 0xFFFFFFFF:
            raise ValueError("length exceeds 32 bits")
        if int((so + np.maximum(cl, sl)).max()) > src.numel() * src.element_size():
            raise ValueError("a source fragment extends past the end of src")
        if int((do + cl).max()) > dst.numel() * dst.element_size():
            raise ValueError("a copy extends past the end of dst")
    pt = (np.full(n, CRC_INITIAL_REGISTER, dtype=np.uint64) if partials is None
          else np.asarray(partials, dtype=np.uint64) & 0xFFFFFFFF)
    host = np.empty((n, 4), dtype=np.uint64)
    host[:, 0] = np.uint64(src.data_ptr()) + so
    host[:, 1] = np.uint64(dst.data_ptr()) + do
    host[:, 2] = cl | (sl << np.uint64(32))
    host[:, 3] = pt
    return torch.from_numpy(host.view(np.int64)).to(src.device)


def frag_bcopy_batch(descs: torch.Tensor, n: int | None = None, mode: int = CRC32, out: torch.Tensor | None = None,
                     stream: torch.cuda.Stream | None = None, rows_hint: int = 0) -> torch.Tensor:
    """Fused bcopy_uicrc / bcopy_uicsum per ``lampi_copy_desc``; returns the checksums.
    rows_hint: LAMPI_CSUM_ROWS_HINT -- fragments span about that many 4 KiB rows (row groups)."""
    _require_cuda(descs, "descs")
    count = descs.numel() * descs.element_size() // 32 if n is None else int(n)
    if mode == NONE:  # checksumming off: copies only, no output (returns None)
        check(lib().lampi_frag_bcopy_batch(descs.data_ptr(), count, None, mode | rows_hint_bits(rows_hint),
                                           _stream_handle(stream)), "lampi_frag_bcopy_batch")
        return None
    if out is None:
        out = torch.empty(count, dtype=torch.int32, device=descs.device)
    _require_cuda(out, "out")
    if out.numel() < count:
        raise ValueError("out is too small")
    check(lib().lampi_frag_bcopy_batch(descs.data_ptr(), count, out.data_ptr(), mode | rows_hint_bits(rows_hint),
                                       _stream_handle(stream)),
          "lampi_frag_bcopy_batch")
    return out


def _strided_dst(dst: torch.Tensor | None, count: int, stride: int, offset: int, mode: int) -> int | None:
    """Device address of record 0's output word (None with mode NONE: nothing is written)."""
    if mode == NONE:
        return None
    if dst is None:
        raise ValueError("dst is required unless mode is NONE")
    _records(dst.view(torch.uint8)[offset:], count, stride, "dst")
    return dst.data_ptr() + offset


def frag_bcopy_batch_strided(descs: torch.Tensor, dst: torch.Tensor | None, stride: int, offset: int = 0,
                             n: int | None = None, mode: int = CRC32, stream: torch.cuda.Stream | None = None,
                             rows_hint: int = 0) -> torch.Tensor | None:
    """frag_bcopy_batch with checksum i written at byte offset + i*stride of ``dst`` (e.g. dataChecksum @64
    of each buffer of a GM send ring, src/path/gm/sendFrag.cc:149-151); returns ``dst``."""
    _require_cuda(descs, "descs")
    count = descs.numel() * descs.element_size() // 32 if n is None else int(n)
    ptr = _strided_dst(dst, count, stride, offset, mode)
    check(lib().lampi_frag_bcopy_batch_strided(descs.data_ptr(), count, ptr, stride, mode | rows_hint_bits(rows_hint),
                                               _stream_handle(stream)), "lampi_frag_bcopy_batch_strided")
    return dst


def frag_csum_batch(descs: torch.Tensor, n: int | None = None, mode: int = CRC32, out: torch.Tensor | None = None,
                    stream: torch.cuda.Stream | None = None, by_bytes: bool = False, rows_hint: int = 0) -> torch.Tensor:
    """out[i] = checksum of fragment descs[i] (piece streams: fragments of any size share rows).
    by_bytes: LAMPI_CSUM_BY_BYTES -- plan the work by bytes (large fragments split across workgroups).
    rows_hint: LAMPI_CSUM_ROWS_HINT -- fragments span about that many 4 KiB rows: each runs as that many
    row segments computed on the device (no plan launch)."""
    _require_cuda(descs, "descs")
    count = descs.numel() * descs.element_size() // 16 if n is None else int(n)
    if out is None:
        out = torch.empty(count, dtype=torch.int32, device=descs.device)
    _require_cuda(out, "out")
    if out.numel() < count:
        raise ValueError("out is too small")
    check(lib().lampi_frag_csum_batch(descs.data_ptr(), count, out.data_ptr(),
                                      mode | (BY_BYTES if by_bytes else 0) | rows_hint_bits(rows_hint),
                                      _stream_handle(stream)), "lampi_frag_csum_batch")
    return out


def diag_frag_csum_batch_per_wave(descs: torch.Tensor, n: int | None = None, mode: int = CRC32,
                                  out: torch.Tensor | None = None,
                                  stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """lampi_frag_csum_batch's results on the one-wavefront-per-fragment schedule: the internal diagnostic
    lampi_diag_frag_csum_batch_per_wave (not part of include/lampi_csum.h since round 5; bench.py's config C
    comparison and the parity tests)."""
    import ctypes

    fn = lib().lampi_diag_frag_csum_batch_per_wave
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    _require_cuda(descs, "descs")
    count = descs.numel() * descs.element_size() // 16 if n is None else int(n)
    if out is None:
        out = torch.empty(count, dtype=torch.int32, device=descs.device)
    _require_cuda(out, "out")
    if out.numel() < count:
        raise ValueError("out is too small")
    check(fn(descs.data_ptr(), count, out.data_ptr(), mode, _stream_handle(stream)),
          "lampi_diag_frag_csum_batch_per_wave")
    return out


def frag_csum_batch_strided(descs: torch.Tensor, dst: torch.Tensor, stride: int, offset: int = 0,
                            n: int | None = None, mode: int = CRC32,
                            stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Checksum i of the batch written at byte offset + i*stride of ``dst`` (e.g. the
    dataChecksum field, offset 64, of 72-byte gmHeaderData records); returns ``dst``."""
    _require_cuda(descs, "descs")
    count = descs.numel() * descs.element_size() // 16 if n is None else int(n)
    _records(dst[offset:] if dst.element_size() == 1 else dst.view(torch.uint8)[offset:], count, stride, "dst")
    check(lib().lampi_frag_csum_batch_strided(descs.data_ptr(), count, dst.data_ptr() + offset, stride, mode,
                                              _stream_handle(stream)), "lampi_frag_csum_batch_strided")
    return dst


def frag_csum64_batch(descs: torch.Tensor, n: int | None = None, out: torch.Tensor | None = None,
                      stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """out[i] = 64-bit csum (fresh state) of fragment descs[i] (int64 storage, read as uint64)."""
    _require_cuda(descs, "descs")
    count = descs.numel() * descs.element_size() // 16 if n is None else int(n)
    if out is None:
        out = torch.empty(count, dtype=torch.int64, device=descs.device)
    _require_cuda(out, "out")
    if out.numel() * out.element_size() < 8 * count:
        raise ValueError("out is too small")
    check(lib().lampi_frag_csum64_batch(descs.data_ptr(), count, out.data_ptr(), _stream_handle(stream)),
          "lampi_frag_csum64_batch")
    return out


def msg_csum(msg: torch.Tensor, frag_len: int, partial: int = CRC_INITIAL_REGISTER, mode: int = CRC32,
             msg_len: int | None = None, out: torch.Tensor | None = None,
             stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Checksums of the fragments of a contiguous device message (src/path/gm/path.cc:98-121)."""
    _require_cuda(msg, "msg")
    nbytes = msg.numel() * msg.element_size() if msg_len is None else int(msg_len)
    if nbytes > msg.numel() * msg.element_size():
        raise ValueError("msg_len exceeds the tensor")
    n = (nbytes + frag_len - 1) // frag_len if nbytes else 1
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=msg.device)
    _require_cuda(out, "out")
    if out.numel() < n:
        raise ValueError("out is too small")
    check(lib().lampi_msg_csum(msg.data_ptr(), nbytes, frag_len, partial & 0xFFFFFFFF, out.data_ptr(), mode,
                               _stream_handle(stream)), "lampi_msg_csum")
    return out


def msg_bcopy(msg: torch.Tensor, frag_len: int, dst: torch.Tensor, dst_stride: int | None = None,
              partial: int = CRC_INITIAL_REGISTER, mode: int = CRC32, msg_len: int | None = None,
              out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Fragment ``msg`` and copy fragment k to ``dst`` + k*dst_stride with its checksum fused."""
    _require_cuda(msg, "msg")
    _require_cuda(dst, "dst")
    nbytes = msg.numel() * msg.element_size() if msg_len is None else int(msg_len)
    if nbytes > msg.numel() * msg.element_size():
        raise ValueError("msg_len exceeds the tensor")
    stride = frag_len if dst_stride is None else int(dst_stride)
    n = (nbytes + frag_len - 1) // frag_len if nbytes else 1
    if nbytes and (n - 1) * stride + (nbytes - (n - 1) * frag_len) > dst.numel() * dst.element_size():
        raise ValueError("dst is too small")
    if mode == NONE:  # checksumming off: copies only (returns None)
        check(lib().lampi_msg_bcopy(msg.data_ptr(), nbytes, frag_len, dst.data_ptr(), stride, partial & 0xFFFFFFFF,
                                    None, mode, _stream_handle(stream)), "lampi_msg_bcopy")
        return None
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=msg.device)
    _require_cuda(out, "out")
    if out.numel() < n:
        raise ValueError("out is too small")
    check(lib().lampi_msg_bcopy(msg.data_ptr(), nbytes, frag_len, dst.data_ptr(), stride, partial & 0xFFFFFFFF,
                                out.data_ptr(), mode, _stream_handle(stream)), "lampi_msg_bcopy")
    return out


def msg_bcopy_strided(msg: torch.Tensor, frag_len: int, dst: torch.Tensor, dst_stride: int, out: torch.Tensor | None,
                      out_stride: int, out_offset: int = 0, partial: int = CRC_INITIAL_REGISTER, mode: int = CRC32,
                      msg_len: int | None = None, stream: torch.cuda.Stream | None = None) -> None:
    """msg_bcopy with fragment k's checksum written at byte out_offset + k*out_stride of ``out``: a GM send into
    a ring of header + payload buffers (dst = ring[72:], out = ring, out_offset 64, both strides the buffer size)."""
    _require_cuda(msg, "msg")
    _require_cuda(dst, "dst")
    nbytes = msg.numel() * msg.element_size() if msg_len is None else int(msg_len)
    if nbytes > msg.numel() * msg.element_size():
        raise ValueError("msg_len exceeds the tensor")
    n = (nbytes + frag_len - 1) // frag_len if nbytes else 1
    if nbytes and (n - 1) * dst_stride + (nbytes - (n - 1) * frag_len) > dst.numel() * dst.element_size():
        raise ValueError("dst is too small")
    ptr = _strided_dst(out, n, out_stride, out_offset, mode)
    check(lib().lampi_msg_bcopy_strided(msg.data_ptr(), nbytes, frag_len, dst.data_ptr(), dst_stride,
                                        partial & 0xFFFFFFFF, ptr, out_stride, mode, _stream_handle(stream)),
          "lampi_msg_bcopy_strided")


SEND_HDR_BYTES = 72  # gmHeaderData / ibDataHdr_t (dataChecksum @64, checksum @68)
QUADRICS_HDR_BYTES = 128  # quadricsCtlHdr_t (dataChecksum @64, dataElanAddr @68, data[52] @72, checksum @124)
QUADRICS_INLINE_BYTES = 52  # CTLHDR_DATABYTES: a fragment of at most this many bytes travels inside the header


def hdr_bytes(kind: int) -> int:
    """The data header's length for ``kind``: 72 (HDR_GM, HDR_IB) or 128 (HDR_QUADRICS)."""
    return QUADRICS_HDR_BYTES if kind == HDR_QUADRICS else SEND_HDR_BYTES


def send_pack_batch(descs: torch.Tensor, hdrs: torch.Tensor | None, hdr_stride: int, offset: int = 0,
                    kind: int = HDR_GM, mode: int = CRC32, n: int | None = None,
                    stream: torch.cuda.Stream | None = None, rows_hint: int = 0) -> torch.Tensor | None:
    """The send step in one call (src/path/gm/sendFrag.cc:143-226, src/path/ib/sendFrag.cc:289-320): every
    ``lampi_copy_desc`` copied with its checksum fused, and header i -- 72 bytes at byte offset + i*hdr_stride of
    ``hdrs``, bytes [0, 64) already filled -- given dataChecksum @64 and the header checksum @68 of ``kind``
    (HDR_GM / HDR_IB).  ``hdrs`` may be None only for HDR_GM with mode NONE; returns ``hdrs``.

    HDR_QUADRICS (src/path/quadrics/sendFrag.h:766-880): 128-byte headers, bytes [0, 64) and [68, 124) already
    filled; a fragment of at most 52 bytes is copied into its header at +72 (its ``dst`` is ignored), a longer one
    to ``dst`` -- or, with copylen 0, only checksummed -- then dataChecksum @64 and the header checksum @124.
    ``hdrs`` is required in every mode."""
    _require_cuda(descs, "descs")
    count = descs.numel() * descs.element_size() // 32 if n is None else int(n)
    if count * 32 > descs.numel() * descs.element_size():
        raise ValueError("n exceeds the descriptor tensor")
    ptr = None
    if hdrs is None:
        if not (kind == HDR_GM and mode == NONE):
            raise ValueError("hdrs is required unless kind is HDR_GM and mode is NONE")
    else:
        _require_cuda(hdrs, "hdrs")
        if count and offset + (count - 1) * hdr_stride + hdr_bytes(kind) > hdrs.numel() * hdrs.element_size():
            raise ValueError(f"hdrs is too small for {count} headers of stride {hdr_stride}")
        ptr = hdrs.data_ptr() + offset
    check(lib().lampi_send_pack_batch(descs.data_ptr(), count, ptr, hdr_stride, kind, mode | rows_hint_bits(rows_hint),
                                      _stream_handle(stream)), "lampi_send_pack_batch")
    return hdrs


def msg_send_pack(msg: torch.Tensor, frag_len: int, ring: torch.Tensor, slot_stride: int, tmpl, frag_seq0: int = 0,
                  frag_seq_step: int = 0, desc_ptr0: int = 0, desc_ptr_stride: int = 0, seq_offset0: int = 0,
                  kind: int = HDR_GM, mode: int = CRC32, msg_len: int | None = None,
                  stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """A device message made a wire-ready ring: fragment k copied to ``ring`` + k*slot_stride + 72 with its checksum
    fused, and slot k's whole 72-byte header built on the device from ``tmpl`` (72 bytes; dataLength @20,
    frag_seq @32 = frag_seq0 + k*frag_seq_step, sendFragDescPtr @48 = desc_ptr0 + k*desc_ptr_stride,
    dataSeqOffset @56 = seq_offset0 + k*frag_len, then @64 / @68 of ``kind``).  Returns ``ring``.

    HDR_QUADRICS: slot k is a 128-byte envelope -- ``tmpl``'s 72 bytes with the fields above, dataElanAddr @68 =
    tmpl's + k*frag_len, data[] @72 zero, then @64 / @124 -- with a fragment of at most 52 bytes placed in data[] and
    a longer one copied to slot + 128 (slot_stride >= 128 + frag_len) or, with slot_stride == 128 (a bare envelope
    queue), checksummed only."""
    _require_cuda(msg, "msg")
    _require_cuda(ring, "ring")
    nbytes = msg.numel() * msg.element_size() if msg_len is None else int(msg_len)
    if nbytes > msg.numel() * msg.element_size():
        raise ValueError("msg_len exceeds the tensor")
    hb = hdr_bytes(kind)
    n = (nbytes + frag_len - 1) // frag_len if nbytes and frag_len >= 1 else 1
    last = nbytes - (n - 1) * frag_len
    if kind == HDR_QUADRICS:
        if frag_len < 1 or slot_stride < hb or (frag_len > QUADRICS_INLINE_BYTES and slot_stride != hb
                                                and slot_stride < hb + frag_len):
            raise ValueError("slot_stride must be 128 (envelopes only) or hold the envelope and a whole fragment")
        if slot_stride == hb or last <= QUADRICS_INLINE_BYTES:
            last = 0  # (nothing is written after the last envelope)
    elif frag_len < 1 or slot_stride < hb + frag_len:
        raise ValueError("slot_stride must hold the header and a whole fragment")
    if (n - 1) * slot_stride + hb + last > ring.numel() * ring.element_size():
        raise ValueError("ring is too small")
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
    import ctypes

    check(lib().lampi_msg_send_pack(msg.data_ptr() if nbytes else None, nbytes, frag_len, ring.data_ptr(), slot_stride,
                                    ctypes.addressof(fill), kind, mode, _stream_handle(stream)), "lampi_msg_send_pack")
    return ring


class DeviceTmap:
    """A committed datatype's typemap on the device (make_tmap): ``struct`` is the host ``lampi_tmap`` the C ABI
    reads during a call, ``pairs`` the device tensor its d_pairs points into -- kept alive here beside it."""

    def __init__(self, struct: Tmap, pairs: torch.Tensor, lo: int, hi: int):
        self.struct, self.pairs = struct, pairs
        self.lo, self.hi = lo, hi  # the lowest piece offset and the highest piece end within an element

    extent = property(lambda self: int(self.struct.extent))
    packed_size = property(lambda self: int(self.struct.packed_size))
    count = property(lambda self: int(self.struct.count))
    num_pairs = property(lambda self: int(self.struct.num_pairs))

    def span(self) -> tuple[int, int]:
        """[lo, hi) byte range, relative to the base address, that the message's pieces lie in."""
        if self.count == 0:
            return 0, 0
        steps = (0, (self.count - 1) * self.extent)
        return self.lo + min(steps), self.hi + max(steps)


def make_tmap(pairs, extent: int, count: int, device) -> DeviceTmap:
    """Upload a typemap: ``pairs`` is [num_pairs, 2] (size, offset) in packed order -- seq_offset is the running sum
    of the sizes -- or [num_pairs, 3] with seq_offset given (ULMTypeMapElt_t as it is); ``extent`` the datatype's
    extent, ``count`` the elements in the message."""
    a = np.asarray(pairs, dtype=np.int64)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] not in (2, 3):
        raise ValueError("pairs must be [num_pairs >= 1, 2 or 3]")
    if np.any(a[:, 0] < 1):
        raise ValueError("every pair's size must be at least 1")
    seq = np.concatenate(([0], np.cumsum(a[:-1, 0])))
    if a.shape[1] == 3 and not np.array_equal(a[:, 2], seq):
        raise ValueError("seq_offset must be the running sum of the sizes")
    host = np.empty((a.shape[0], 3), dtype=np.int64)
    host[:, 0], host[:, 1], host[:, 2] = a[:, 0], a[:, 1], seq
    t = torch.from_numpy(host).to(device)
    st = Tmap()
    st.d_pairs = t.data_ptr()
    st.extent, st.packed_size, st.count = int(extent), int(a[:, 0].sum()), int(count)
    st.num_pairs, st.reserved = a.shape[0], 0
    return DeviceTmap(st, t, int(a[:, 1].min()), int((a[:, 1] + a[:, 0]).max()))


def _tmap_base(base: torch.Tensor, base_offset: int, tmap: DeviceTmap) -> int:
    """The device address of the typemap's origin: byte ``base_offset`` of ``base``; every piece must lie inside."""
    _require_cuda(base, "base")
    lo, hi = tmap.span()
    if base_offset + lo < 0 or base_offset + hi > base.numel() * base.element_size():
        raise ValueError("the typemap's pieces reach outside the base tensor")
    return base.data_ptr() + base_offset


def tmap_send_pack(base: torch.Tensor, tmap: DeviceTmap, frag_len: int, ring: torch.Tensor, slot_stride: int, tmpl,
                   frag_seq0: int = 0, frag_seq_step: int = 0, desc_ptr0: int = 0, desc_ptr_stride: int = 0,
                   seq_offset0: int = 0, kind: int = HDR_GM, mode: int = CRC32, pack_off: int = 0,
                   pack_len: int | None = None, base_offset: int = 0,
                   stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """msg_send_pack through a datatype's typemap (src/path/gm/sendFrag.cc:157-217): fragment j = packed bytes
    [pack_off + j*frag_len, ...) of the ``tmap.count`` elements whose origin is byte ``base_offset`` of ``base``
    (default window: everything from pack_off on), gathered to ``ring`` + j*slot_stride + 72 with the checksum of
    the packed bytes, the 72-byte headers built as msg_send_pack builds them.  HDR_GM / HDR_IB.  Returns ``ring``."""
    _require_cuda(ring, "ring")
    total = tmap.count * tmap.packed_size
    plen = max(total - pack_off, 0) if pack_len is None else int(pack_len)
    if frag_len < 1 or slot_stride < SEND_HDR_BYTES + frag_len:
        raise ValueError("slot_stride must hold the header and a whole fragment")
    n = (plen + frag_len - 1) // frag_len if plen else 1
    last = plen - (n - 1) * frag_len
    if (n - 1) * slot_stride + SEND_HDR_BYTES + last > ring.numel() * ring.element_size():
        raise ValueError("ring is too small")
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
    import ctypes

    check(lib().lampi_tmap_send_pack(_tmap_base(base, base_offset, tmap), ctypes.addressof(tmap.struct), pack_off, plen,
                                     frag_len, ring.data_ptr(), slot_stride, ctypes.addressof(fill), kind, mode,
                                     _stream_handle(stream)), "lampi_tmap_send_pack")
    return ring


def chain_csum_batch(pieces: torch.Tensor, first, mode: int = CRC32, out: torch.Tensor | None = None,
                     stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Chained checksum per fragment over its typemap pieces (``lampi_copy_desc`` rows of
    ``pieces``; fragment f = pieces first[f] .. first[f+1]-1)."""
    _require_cuda(pieces, "pieces")
    npieces = pieces.numel() * pieces.element_size() // 32
    fa = np.asarray(first, dtype=np.uint32) if not isinstance(first, torch.Tensor) else None
    if fa is not None:
        if fa.size < 1 or (fa.size > 1 and (np.any(np.diff(fa.astype(np.int64)) < 0) or int(fa[-1]) > npieces)):
            raise ValueError("first must be nondecreasing and end at most at the piece count")
        first_t = torch.from_numpy(fa.view(np.int32)).to(pieces.device)
    else:
        _require_cuda(first, "first")
        first_t = first
    nfrags = first_t.numel() - 1
    if mode == NONE:  # checksumming off: the pieces are copied, no output (returns None)
        check(lib().lampi_chain_csum_batch(pieces.data_ptr(), npieces, first_t.data_ptr(), nfrags, None, mode,
                                           _stream_handle(stream)), "lampi_chain_csum_batch")
        return None
    if out is None:
        out = torch.empty(max(nfrags, 0), dtype=torch.int32, device=pieces.device)
    check(lib().lampi_chain_csum_batch(pieces.data_ptr(), npieces, first_t.data_ptr(), nfrags, out.data_ptr(), mode,
                                       _stream_handle(stream)), "lampi_chain_csum_batch")
    return out


def chain_csum_batch_strided(pieces: torch.Tensor, first: torch.Tensor, dst: torch.Tensor | None, stride: int,
                             offset: int = 0, mode: int = CRC32, stream: torch.cuda.Stream | None = None):
    """chain_csum_batch with fragment f's checksum written at byte offset + f*stride of ``dst`` (the typemap
    send's dataChecksum, src/path/gm/sendFrag.cc:216); ``first`` a device int32 tensor of nfrags + 1 offsets."""
    _require_cuda(pieces, "pieces")
    _require_cuda(first, "first")
    npieces = pieces.numel() * pieces.element_size() // 32
    nfrags = first.numel() - 1
    ptr = _strided_dst(dst, nfrags, stride, offset, mode)
    check(lib().lampi_chain_csum_batch_strided(pieces.data_ptr(), npieces, first.data_ptr(), nfrags, ptr, stride,
                                               mode, _stream_handle(stream)), "lampi_chain_csum_batch_strided")
    return dst


def chain_copy_to_app_batch(pieces: torch.Tensor, first, expected: torch.Tensor | None, expected_stride: int = 4,
                            mode: int = CRC32, stream: torch.cuda.Stream | None = None):
    """RecvDesc_t::CopyToApp's non-contiguous branch (src/path/common/BaseDesc.cc:326-340): the typemap
    pieces of each received fragment copied, the checksum from CRC_INITIAL_REGISTER compared with
    expected (None with mode NONE).  Returns (copied int64 -- len_copied or -1 --, csum int32, mask, nbad)."""
    _require_cuda(pieces, "pieces")
    npieces = pieces.numel() * pieces.element_size() // 32
    fa = np.asarray(first, dtype=np.uint32) if not isinstance(first, torch.Tensor) else None
    if fa is not None:
        if fa.size < 1 or (fa.size > 1 and (np.any(np.diff(fa.astype(np.int64)) < 0) or int(fa[-1]) > npieces)):
            raise ValueError("first must be nondecreasing and end at most at the piece count")
        first_t = torch.from_numpy(fa.view(np.int32)).to(pieces.device)
    else:
        _require_cuda(first, "first")
        first_t = first
    nfrags = first_t.numel() - 1
    if expected is not None:
        _records(expected, nfrags, expected_stride, "expected")
    copied = torch.empty(max(nfrags, 1), dtype=torch.int64, device=pieces.device)
    csum = torch.empty(max(nfrags, 1), dtype=torch.int32, device=pieces.device)
    mask = torch.empty(max((nfrags + 31) // 32, 1), dtype=torch.int32, device=pieces.device)
    nbad = torch.empty(1, dtype=torch.int32, device=pieces.device)
    check(lib().lampi_chain_copy_to_app_batch(pieces.data_ptr(), npieces, first_t.data_ptr(), nfrags,
                                              0 if expected is None else expected.data_ptr(), expected_stride,
                                              copied.data_ptr(), csum.data_ptr(), mask.data_ptr(), nbad.data_ptr(),
                                              mode, _stream_handle(stream)), "lampi_chain_copy_to_app_batch")
    return copied[:nfrags], csum[:nfrags], mask, nbad


def _records(t: torch.Tensor, n: int, stride: int, what: str) -> None:
    _require_cuda(t, what)
    if n and (n - 1) * stride + 4 > t.numel() * t.element_size():
        raise ValueError(f"{what} is too small for {n} records of stride {stride}")


def header_csum_batch(hdrs: torch.Tensor, n: int, stride: int, crclen: int, word_count: int, mode: int = CRC32,
                      out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """BasePath_t::headerChecksum of n headers ``stride`` bytes apart (src/path/common/path.h:280-314)."""
    _records(hdrs, n, stride, "hdrs")
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=hdrs.device)
    check(lib().lampi_header_csum_batch(hdrs.data_ptr(), n, stride, crclen, word_count, out.data_ptr(), mode,
                                        _stream_handle(stream)), "lampi_header_csum_batch")
    return out


def header_csum_batch_strided(hdrs: torch.Tensor, n: int, stride: int, crclen: int, word_count: int,
                              dst: torch.Tensor, out_stride: int, offset: int = 0, mode: int = CRC32,
                              stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """headerChecksum of n headers written at byte offset + i*out_stride of ``dst``: in place into the headers
    with dst = hdrs, offset 68, out_stride = stride (src/path/gm/sendFrag.cc:218-225); mode NONE writes nothing."""
    _records(hdrs, n, stride, "hdrs")
    ptr = _strided_dst(dst, n, out_stride, offset, mode)
    check(lib().lampi_header_csum_batch_strided(hdrs.data_ptr(), n, stride, crclen, word_count, ptr, out_stride, mode,
                                                _stream_handle(stream)), "lampi_header_csum_batch_strided")
    return dst


def _mask_out(n: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    return (torch.zeros(max(1, (n + 31) // 32), dtype=torch.int32, device=device),
            torch.zeros(1, dtype=torch.int32, device=device))


def header_check_batch(hdrs: torch.Tensor, n: int, stride: int, hdr_bytes: int, word_count: int, csum_offset: int,
                       mode: int = CRC32, stream: torch.cuda.Stream | None = None):
    """Receiver header check (src/path/gm/path.cc:364-393); returns (mask, nbad), mask bit set = bad."""
    _records(hdrs, n, stride, "hdrs")
    mask, nbad = _mask_out(n, hdrs.device)
    check(lib().lampi_header_check_batch(hdrs.data_ptr(), n, stride, hdr_bytes, word_count, csum_offset,
                                         mask.data_ptr(), nbad.data_ptr(), mode, _stream_handle(stream)),
          "lampi_header_check_batch")
    return mask, nbad


def header_compare_batch(hdrs: torch.Tensor, n: int, stride: int, crclen: int, csum_offset: int, mode: int = CRC32,
                         stream: torch.cuda.Stream | None = None):
    """The IB receiver's header check (src/path/ib/path.cc:652-680): uicrc / uicsum of crclen bytes vs the
    stored, unswapped word at csum_offset; returns (mask, nbad), mask bit set = bad."""
    _records(hdrs, n, stride, "hdrs")
    mask, nbad = _mask_out(n, hdrs.device)
    check(lib().lampi_header_compare_batch(hdrs.data_ptr(), n, stride, crclen, csum_offset, mask.data_ptr(),
                                           nbad.data_ptr(), mode, _stream_handle(stream)),
          "lampi_header_compare_batch")
    return mask, nbad


def check_data_batch(calc: torch.Tensor, expected: torch.Tensor, expected_stride: int = 4,
                     lengths: torch.Tensor | None = None, lengths_stride: int = 4, n: int | None = None,
                     expected_offset: int = 0, lengths_offset: int = 0, stream: torch.cuda.Stream | None = None):
    """CheckData over a batch (src/path/gm/recvFrag.h:213-257); returns (mask, nbad), bit set = corrupt."""
    _require_cuda(calc, "calc")
    count = calc.numel() if n is None else int(n)
    _records(expected, count, expected_stride, "expected")
    lp = 0
    if lengths is not None:
        _records(lengths, count, lengths_stride, "lengths")
        lp = lengths.data_ptr() + lengths_offset
    mask, nbad = _mask_out(count, calc.device)
    check(lib().lampi_check_data_batch(calc.data_ptr(), expected.data_ptr() + expected_offset, expected_stride,
                                       lp or None, lengths_stride, count, mask.data_ptr(), nbad.data_ptr(),
                                       _stream_handle(stream)), "lampi_check_data_batch")
    return mask, nbad


def make_recv_descs(frag: torch.Tensor, frag_offsets, app: torch.Tensor, app_offsets, lengths,
                    app_lens) -> torch.Tensor:
    """Build a device array of ``lampi_recv_desc`` (n x 32 bytes, int64 [n, 4] storage): fragment i
    = ``lengths[i]`` received bytes at frag + frag_offsets[i], delivered to app + app_offsets[i]
    with ``app_lens[i]`` bytes of room left in the posted buffer (posted length - offset, may be
    <= 0; ref src/path/common/BaseDesc.cc:300-307)."""
    _require_cuda(frag, "frag")
    _require_cuda(app, "app")
    fo = np.asarray(frag_offsets, dtype=np.uint64)
    ao = np.asarray(app_offsets, dtype=np.uint64)
    ln = np.asarray(lengths, dtype=np.uint64)
    al = np.asarray(app_lens, dtype=np.int64)
    n = fo.size
    if not (ao.size == ln.size == al.size == n):
        raise ValueError("descriptor fields differ in size")
    if n:
        if int(ln.max()) > 0xFFFFFFFF:
            raise ValueError("fragment length exceeds 32 bits")
        if int((fo + ln).max()) > frag.numel() * frag.element_size():
            raise ValueError("a fragment extends past the end of frag")
        copy = np.minimum(ln.astype(np.int64), np.maximum(al, 0))
        if int((ao.astype(np.int64) + copy).max()) > app.numel() * app.element_size():
            raise ValueError("a delivery extends past the end of app")
    host = np.empty((n, 4), dtype=np.uint64)
    host[:, 0] = np.uint64(frag.data_ptr()) + fo
    host[:, 1] = np.uint64(app.data_ptr()) + ao
    host[:, 2] = al.view(np.uint64)
    host[:, 3] = ln
    return torch.from_numpy(host.view(np.int64)).to(frag.device)


def copy_to_app_batch(descs: torch.Tensor, expected: torch.Tensor, expected_stride: int = 4, expected_offset: int = 0,
                      n: int | None = None, mode: int = CRC32, stream: torch.cuda.Stream | None = None,
                      rows_hint: int = 0):
    """RecvDesc_t::CopyToApp over a batch (src/path/common/BaseDesc.cc:288-342): returns
    (copied int64[n] -- bytes copied or -1 when corrupt --, csum int32[n], mask, nbad).
    rows_hint: as for frag_bcopy_batch (GM's 65,456-byte payloads: 16)."""
    _require_cuda(descs, "descs")
    count = descs.numel() * descs.element_size() // 32 if n is None else int(n)
    if expected is None:  # (mode NONE: nothing compared; the C call refuses a null pointer in the other modes)
        if (mode & 0xFF) != NONE:
            raise ValueError("expected is required unless mode is NONE (checksumming off)")
        exp_ptr, expected_stride = 0, 0
    else:
        _records(expected.view(torch.uint8)[expected_offset:] if count else expected, count, expected_stride,
                 "expected")
        exp_ptr = expected.data_ptr() + expected_offset
    copied = torch.empty(max(count, 1), dtype=torch.int64, device=descs.device)
    csum = torch.empty(max(count, 1), dtype=torch.int32, device=descs.device)
    # (the call zeroes the mask words and the count itself: no fill kernels here, except for an empty batch)
    mask, nbad = (_mask_out(count, descs.device) if count == 0 else
                  (torch.empty((count + 31) // 32, dtype=torch.int32, device=descs.device),
                   torch.empty(1, dtype=torch.int32, device=descs.device)))
    check(lib().lampi_copy_to_app_batch(descs.data_ptr(), count, exp_ptr or None, expected_stride,
                                        copied.data_ptr(), csum.data_ptr(), mask.data_ptr(), nbad.data_ptr(),
                                        mode | rows_hint_bits(rows_hint), _stream_handle(stream)),
          "lampi_copy_to_app_batch")
    return copied[:count], csum[:count], mask, nbad


def _unpack_out(count: int, device):
    """(copied, csum, hdr_mask, data_mask, nbad[2]) for ``count`` fragments; the call overwrites all of them."""
    words = max(1, (count + 31) // 32)
    make = torch.zeros if count == 0 else torch.empty  # (an empty batch zeroes the counts only)
    return (torch.empty(max(count, 1), dtype=torch.int64, device=device),
            torch.empty(max(count, 1), dtype=torch.int32, device=device),
            make(words, dtype=torch.int32, device=device), make(words, dtype=torch.int32, device=device),
            torch.empty(2, dtype=torch.int32, device=device))


def recv_unpack_batch(descs: torch.Tensor, hdrs: torch.Tensor | None, hdr_stride: int, offset: int = 0,
                      kind: int = HDR_GM, mode: int = CRC32, rows_hint: int = 0, stream: torch.cuda.Stream | None = None,
                      n: int | None = None):
    """The receive step in one call (src/path/gm/path.cc:364-393, src/path/ib/path.cc:652-680, then
    src/path/common/BaseDesc.cc:288-342): header i -- 72 bytes at byte offset + i*hdr_stride of ``hdrs`` -- is
    tested as ``kind`` (HDR_GM / HDR_IB) says; a fragment whose header fails is dropped (copied RECV_HDR_BAD, nothing
    read or delivered), the others go through CopyToApp against the header's dataChecksum @64 (copied = bytes
    delivered, or RECV_DATA_BAD).  Returns (copied int64[n], csum int32[n], hdr_mask, data_mask, nbad int32[2] --
    bad headers, corrupt payloads).  ``hdrs`` may be None with mode NONE (no header is read).

    HDR_QUADRICS (src/path/quadrics/path.cc:839-900): 128-byte headers; a fragment of 1..52 bytes is read from its
    header at +72 (the descriptor's ``frag`` is ignored), so ``hdrs`` is required in every mode."""
    _require_cuda(descs, "descs")
    count = descs.numel() * descs.element_size() // 32 if n is None else int(n)
    if count * 32 > descs.numel() * descs.element_size():
        raise ValueError("n exceeds the descriptor tensor")
    ptr = None
    if hdrs is None:
        if (mode & 0xFF) != NONE or kind == HDR_QUADRICS:
            raise ValueError("hdrs is required unless mode is NONE (checksumming off) and kind is not HDR_QUADRICS")
    else:
        _require_cuda(hdrs, "hdrs")
        if count and offset + (count - 1) * hdr_stride + hdr_bytes(kind) > hdrs.numel() * hdrs.element_size():
            raise ValueError(f"hdrs is too small for {count} headers of stride {hdr_stride}")
        ptr = hdrs.data_ptr() + offset
    copied, csum, hmask, dmask, nbad = _unpack_out(count, descs.device)
    check(lib().lampi_recv_unpack_batch(descs.data_ptr(), count, ptr, hdr_stride, kind, copied.data_ptr(),
                                        csum.data_ptr(), hmask.data_ptr(), dmask.data_ptr(), nbad.data_ptr(),
                                        mode | rows_hint_bits(rows_hint), _stream_handle(stream)),
          "lampi_recv_unpack_batch")
    return copied[:count], csum[:count], hmask, dmask, nbad


def msg_recv_unpack(ring: torch.Tensor, nslots: int, slot_stride: int, app: torch.Tensor, kind: int = HDR_GM,
                    mode: int = CRC32, seq_offset0: int = 0, app_len: int | None = None,
                    stream: torch.cuda.Stream | None = None):
    """The receive step over a ring of header + payload slots, no descriptors (the mirror of msg_send_pack): slot k
    = the 72-byte header at ``ring`` + k*slot_stride and its payload at +72, in any order; its length is the
    header's dataLength @20 (more than slot_stride - 72: malformed, dropped like a failed header), its destination
    ``app`` + (dataSeqOffset @56 - seq_offset0 mod 2^64), cut at ``app_len`` (default: the whole tensor).  Returns
    (copied, csum, hdr_mask, data_mask, nbad) as recv_unpack_batch, indexed by slot.

    HDR_QUADRICS: 128-byte envelopes, the payload at slot + 72 when dataLength <= 52, else at slot + 128 (more than
    slot_stride - 128: malformed)."""
    _require_cuda(ring, "ring")
    _require_cuda(app, "app")
    count = int(nslots)
    if count < 0 or slot_stride < hdr_bytes(kind):
        raise ValueError("slot_stride must hold the header")
    if count * slot_stride > ring.numel() * ring.element_size():
        raise ValueError("ring is too small (every slot may be read whole)")
    room = app.numel() * app.element_size()
    alen = room if app_len is None else int(app_len)
    if not 0 <= alen <= room:
        raise ValueError("app_len exceeds the tensor")
    copied, csum, hmask, dmask, nbad = _unpack_out(count, ring.device)
    check(lib().lampi_msg_recv_unpack(ring.data_ptr(), count, slot_stride, kind, app.data_ptr(), alen,
                                      seq_offset0 & (2**64 - 1), copied.data_ptr(), csum.data_ptr(), hmask.data_ptr(),
                                      dmask.data_ptr(), nbad.data_ptr(), mode, _stream_handle(stream)),
          "lampi_msg_recv_unpack")
    return copied[:count], csum[:count], hmask, dmask, nbad


def tmap_recv_unpack(ring: torch.Tensor, nslots: int, slot_stride: int, base: torch.Tensor, tmap: DeviceTmap,
                     kind: int = HDR_GM, mode: int = CRC32, seq_offset0: int = 0, base_offset: int = 0,
                     stream: torch.cuda.Stream | None = None):
    """msg_recv_unpack through a datatype's typemap (src/path/common/BaseDesc.cc:72-163, 326-340): the same rules
    with app_len = tmap.count * tmap.packed_size, the delivered packed bytes scattered to the typemap's pieces of
    the elements whose origin is byte ``base_offset`` of ``base``; nothing is written between the pieces or past
    ``tmap.count`` elements.  HDR_GM / HDR_IB.  Returns (copied, csum, hdr_mask, data_mask, nbad), indexed by slot."""
    import ctypes

    _require_cuda(ring, "ring")
    count = int(nslots)
    if count < 0 or slot_stride < SEND_HDR_BYTES:
        raise ValueError("slot_stride must hold the header")
    if count * slot_stride > ring.numel() * ring.element_size():
        raise ValueError("ring is too small (every slot may be read whole)")
    copied, csum, hmask, dmask, nbad = _unpack_out(count, ring.device)
    check(lib().lampi_tmap_recv_unpack(ring.data_ptr(), count, slot_stride, kind, _tmap_base(base, base_offset, tmap),
                                       ctypes.addressof(tmap.struct), seq_offset0 & (2**64 - 1), copied.data_ptr(),
                                       csum.data_ptr(), hmask.data_ptr(), dmask.data_ptr(), nbad.data_ptr(), mode,
                                       _stream_handle(stream)), "lampi_tmap_recv_unpack")
    return copied[:count], csum[:count], hmask, dmask, nbad


class TmapMsgs:
    """The descriptor forms' message table on the device (make_tmap_msgs): ``table`` is the array of
    ``lampi_tmap_msg`` (int64 [nmsgs, 8] storage); the pair tensors its d_pairs point into and the tensors its bases
    point into are kept alive here beside it."""

    def __init__(self, table: torch.Tensor, tmaps: list, bases: list):
        self.table, self.tmaps, self.bases = table, tmaps, bases
        self.pairs = [t.pairs for t in tmaps]

    def __len__(self) -> int:
        return self.table.shape[0]


def make_tmap_msgs(entries, device) -> TmapMsgs:
    """Build the message table of tmap_send_pack_batch / tmap_recv_unpack_batch: ``entries`` is a list of
    (DeviceTmap, base tensor, base_offset) -- message k's typemap and element count, and byte ``base_offset`` of
    ``base`` as the datatype's origin; every piece must lie inside its tensor."""
    host = np.zeros((len(entries), 8), dtype=np.uint64)
    tmaps, bases = [], []
    for k, (tmap, base, base_offset) in enumerate(entries):
        addr = _tmap_base(base, int(base_offset), tmap)
        host[k, 0] = tmap.pairs.data_ptr()
        host[k, 1], host[k, 2], host[k, 3] = tmap.extent, tmap.packed_size, tmap.count
        host[k, 4] = tmap.num_pairs  # (reserved @36 = 0)
        host[k, 5] = addr
        tmaps.append(tmap)
        bases.append(base)
    return TmapMsgs(torch.from_numpy(host.view(np.int64)).to(device), tmaps, bases)


def make_tmap_frags(payload_addr, pack_off, length, msg, device) -> torch.Tensor:
    """Build a device array of ``lampi_tmap_frag`` (n x 32 bytes, int64 [n, 4] storage): fragment i = ``length[i]``
    packed bytes from packed byte ``pack_off[i]`` of message ``msg[i]`` of the table, its payload at the device
    address ``payload_addr[i]``."""
    pa = np.asarray(payload_addr, dtype=np.uint64)
    po = np.asarray(pack_off, dtype=np.uint64)
    ln = np.asarray(length, dtype=np.uint64)
    mi = np.asarray(msg, dtype=np.uint64)
    n = pa.size
    if not (po.size == ln.size == mi.size == n):
        raise ValueError("record fields differ in size")
    if n and (int(ln.max()) > 0xFFFFFFFF or int(mi.max()) > 0xFFFFFFFF):
        raise ValueError("length and msg are 32-bit fields")
    host = np.zeros((n, 4), dtype=np.uint64)
    host[:, 0], host[:, 1] = pa, po
    host[:, 2] = ln | (mi << np.uint64(32))
    return torch.from_numpy(host.view(np.int64)).to(device)


def _tmap_batch_args(frags: torch.Tensor, msgs, n, hdrs, hdr_stride: int, offset: int):
    _require_cuda(frags, "frags")
    table = msgs.table if isinstance(msgs, TmapMsgs) else msgs
    _require_cuda(table, "msgs")
    count = frags.numel() * frags.element_size() // 32 if n is None else int(n)
    if count * 32 > frags.numel() * frags.element_size():
        raise ValueError("n exceeds the record tensor")
    ptr = None
    if hdrs is not None:
        _require_cuda(hdrs, "hdrs")
        if count and offset + (count - 1) * hdr_stride + SEND_HDR_BYTES > hdrs.numel() * hdrs.element_size():
            raise ValueError(f"hdrs is too small for {count} headers of stride {hdr_stride}")
        ptr = hdrs.data_ptr() + offset
    return table, table.numel() * table.element_size() // 64, count, ptr


def tmap_send_pack_batch(frags: torch.Tensor, msgs, max_len: int, hdrs: torch.Tensor | None, hdr_stride: int,
                         offset: int = 0, kind: int = HDR_GM, mode: int = CRC32, n: int | None = None,
                         stream: torch.cuda.Stream | None = None) -> torch.Tensor | None:
    """send_pack_batch through typemaps, for the fragments of several messages in one call: record i
    (make_tmap_frags) names its message in ``msgs`` (make_tmap_msgs), its window [pack_off, pack_off + length) of
    that message's packed bytes and the payload address they are gathered to; header i -- 72 bytes at byte offset +
    i*hdr_stride of ``hdrs``, bytes [0, 64) already filled -- gets dataChecksum @64 and the header checksum @68 of
    ``kind`` (HDR_GM / HDR_IB).  ``max_len``: an upper bound on every record's length (it fixes the rows per
    fragment; batch by size class).  A record that is invalid (msg outside the table, length > max_len, an entry
    without pairs, a window past the message) is skipped.  ``hdrs`` may be None only for HDR_GM with mode NONE;
    returns ``hdrs``."""
    if hdrs is None and not (kind == HDR_GM and mode == NONE):
        raise ValueError("hdrs is required unless kind is HDR_GM and mode is NONE")
    table, nmsgs, count, ptr = _tmap_batch_args(frags, msgs, n, hdrs, hdr_stride, offset)
    check(lib().lampi_tmap_send_pack_batch(frags.data_ptr(), count, table.data_ptr(), nmsgs, int(max_len), ptr,
                                           hdr_stride, kind, mode, _stream_handle(stream)),
          "lampi_tmap_send_pack_batch")
    return hdrs


def tmap_recv_unpack_batch(frags: torch.Tensor, msgs, max_len: int, hdrs: torch.Tensor | None, hdr_stride: int,
                           offset: int = 0, kind: int = HDR_GM, mode: int = CRC32,
                           stream: torch.cuda.Stream | None = None, n: int | None = None):
    """recv_unpack_batch through typemaps, for the drained fragments of several posted receives in one call: header
    i is tested as ``kind`` says; a fragment that passes is delivered through its own message's typemap -- the
    first min(length, count * packed_size - pack_off) packed bytes at its payload address scattered to their
    pieces, all ``length`` bytes checksummed against the word @64.  A failed header or an invalid record (as for
    tmap_send_pack_batch, without the window test) drops the fragment as RECV_HDR_BAD.  Returns (copied, csum,
    hdr_mask, data_mask, nbad) as recv_unpack_batch.  ``hdrs`` may be None with mode NONE (no header is read)."""
    if hdrs is None and mode != NONE:
        raise ValueError("hdrs is required unless mode is NONE (checksumming off)")
    table, nmsgs, count, ptr = _tmap_batch_args(frags, msgs, n, hdrs, hdr_stride, offset)
    copied, csum, hmask, dmask, nbad = _unpack_out(count, frags.device)
    check(lib().lampi_tmap_recv_unpack_batch(frags.data_ptr(), count, table.data_ptr(), nmsgs, int(max_len), ptr,
                                             hdr_stride, kind, copied.data_ptr(), csum.data_ptr(), hmask.data_ptr(),
                                             dmask.data_ptr(), nbad.data_ptr(), mode, _stream_handle(stream)),
          "lampi_tmap_recv_unpack_batch")
    return copied[:count], csum[:count], hmask, dmask, nbad


def mask_bits(mask: torch.Tensor, n: int) -> np.ndarray:
    """Device mask words -> bool array of length n (True = failed)."""
    w = mask.cpu().numpy().view(np.uint32)
    return ((w[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1).astype(bool)


def fill_stream(dst: torch.Tensor, seed: int, byte_off: int = 0, nbytes: int | None = None,
                stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Write the SURVEY.md 8(d) synthetic stream (splitmix64 words, LE) into ``dst`` on device."""
    _require_cuda(dst, "dst")
    n = dst.numel() * dst.element_size() if nbytes is None else int(nbytes)
    check(lib().lampi_fill_stream(dst.data_ptr(), n, seed & (2**64 - 1), byte_off, _stream_handle(stream)),
          "lampi_fill_stream")
    return dst


def fill_stream_frags(dst: torch.Tensor, n: int, frag_len: int, seed: int, k0: int = 0, kstep: int = 1,
                      stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Round-robin shard of a global batch: fragment i of ``dst`` = global fragment k0 + i*kstep."""
    _require_cuda(dst, "dst")
    if n * frag_len > dst.numel() * dst.element_size():
        raise ValueError("dst is too small")
    check(lib().lampi_fill_stream_frags(dst.data_ptr(), n, frag_len, seed & (2**64 - 1), k0, kstep,
                                        _stream_handle(stream)), "lampi_fill_stream_frags")
    return dst
