"""CPU: what every device entry point of the C ABI refuses, and what it answers before it asks for the device.

One table for all of lampi_amd._lib.PROTOTYPES that takes a stream.  A row is a well-formed call with one thing (or
two, where a refusal meets an empty call) changed, and the value it must return:

  1  hipErrorInvalidValue -- the argument is refused;
  0  an empty call, answered before the device is asked for.

The order "refuse -> an empty call returns 0 -> ask for the device" differs from entry point to entry point
(lampi_header_csum_batch refuses NONE where its strided form returns 0 for it; lampi_send_pack_batch refuses a bad
kind even when n == 0), so the rows where the two meet pin it.

The table runs in one child process with the devices hidden: the pointers are host addresses that stand in for
device memory, and a call that got past validation -- by a mistake in the table or by a regression -- returns
hipErrorNoDevice there instead of launching on them.  Every entry point's well-formed call is run too and must get
that far (neither 0 nor 1): a row is then refused for what it changes, not for something else in it.  This process
only compares the child's output.
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
OVER = 1 << 32  # one more than a count, a fragment length or a message table may be
STREAM = 0

# Host memory the rows point into (never read: every row ends before a launch); P is 4096-byte aligned.
_ARENA = ctypes.create_string_buffer(3 * 4096)
P = (ctypes.addressof(_ARENA) + 4095) & ~4095
_KEEP = []  # the host structs of the rows


class _Tmap(ctypes.Structure):
    _fields_ = [("d_pairs", ctypes.c_void_p), ("extent", ctypes.c_uint64), ("packed_size", ctypes.c_uint64),
                ("count", ctypes.c_uint64), ("num_pairs", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def tmap(d_pairs=P, extent=64, packed_size=48, count=1000, num_pairs=2, reserved=0):
    """The host address of a lampi_tmap (total = count * packed_size = 48,000 bytes unless changed)."""
    t = _Tmap(d_pairs, extent, packed_size, count, num_pairs, reserved)
    _KEEP.append(t)
    return ctypes.addressof(t)


FILL = ctypes.create_string_buffer(112)  # a lampi_send_hdr_fill, zeroed
H_FILL = ctypes.addressof(FILL)

# name -> the argument names in order and a well-formed call (which reaches the device)
BASE = {
    "lampi_frag_csum64_batch": dict(d_descs=P, n=8, d_out=P, stream=STREAM),
    "lampi_frag_csum_batch": dict(d_descs=P, n=8, d_out=P, mode=CRC, stream=STREAM),
    "lampi_frag_csum_batch_strided": dict(d_descs=P, n=8, d_out=P, out_stride=72, mode=CRC, stream=STREAM),
    "lampi_frag_bcopy_batch": dict(d_descs=P, n=8, d_out=P, mode=CRC, stream=STREAM),
    "lampi_frag_bcopy_batch_strided": dict(d_descs=P, n=8, d_out=P, out_stride=72, mode=CRC, stream=STREAM),
    "lampi_msg_bcopy": dict(d_msg=P, msg_len=4096, frag_len=512, d_dst=P, dst_stride=512, partial=0, d_out=P,
                            mode=CRC, stream=STREAM),
    "lampi_msg_bcopy_strided": dict(d_msg=P, msg_len=4096, frag_len=512, d_dst=P, dst_stride=512, partial=0, d_out=P,
                                    out_stride=72, mode=CRC, stream=STREAM),
    "lampi_chain_csum_batch": dict(d_pieces=P, npieces=8, d_first=P, nfrags=4, d_out=P, mode=CRC, stream=STREAM),
    "lampi_chain_csum_batch_strided": dict(d_pieces=P, npieces=8, d_first=P, nfrags=4, d_out=P, out_stride=72,
                                           mode=CRC, stream=STREAM),
    "lampi_header_csum_batch": dict(d_hdrs=P, n=8, stride=72, crclen=68, word_count=17, d_out=P, mode=CRC,
                                    stream=STREAM),
    "lampi_header_csum_batch_strided": dict(d_hdrs=P, n=8, stride=72, crclen=68, word_count=17, d_out=P,
                                            out_stride=72, mode=CRC, stream=STREAM),
    "lampi_header_check_batch": dict(d_hdrs=P, n=8, stride=72, hdr_bytes=72, word_count=18, csum_offset=68, d_mask=P,
                                     d_nbad=P, mode=CRC, stream=STREAM),
    "lampi_header_compare_batch": dict(d_hdrs=P, n=8, stride=72, crclen=68, csum_offset=68, d_mask=P, d_nbad=P,
                                       mode=CRC, stream=STREAM),
    "lampi_check_data_batch": dict(d_calc=P, d_expected=P, expected_stride=72, d_lengths=P, lengths_stride=72, n=8,
                                   d_mask=P, d_nbad=P, stream=STREAM),
    "lampi_copy_to_app_batch": dict(d_descs=P, n=8, d_expected=P, expected_stride=72, d_copied=P, d_csum=P, d_mask=P,
                                    d_nbad=P, mode=CRC, stream=STREAM),
    "lampi_chain_copy_to_app_batch": dict(d_pieces=P, npieces=8, d_first=P, nfrags=4, d_expected=P,
                                          expected_stride=72, d_copied=P, d_csum=P, d_mask=P, d_nbad=P, mode=CRC,
                                          stream=STREAM),
    "lampi_msg_csum": dict(d_msg=P, msg_len=4096, frag_len=512, partial=0, d_out=P, mode=CRC, stream=STREAM),
    "lampi_send_pack_batch": dict(d_descs=P, n=8, d_hdrs=P, hdr_stride=128, hdr_kind=GM, mode=CRC, stream=STREAM),
    "lampi_msg_send_pack": dict(d_msg=P, msg_len=4096, frag_len=512, d_ring=P, slot_stride=1024, h_fill=H_FILL,
                                hdr_kind=GM, mode=CRC, stream=STREAM),
    "lampi_recv_unpack_batch": dict(d_descs=P, n=8, d_hdrs=P, hdr_stride=128, hdr_kind=GM, d_copied=P, d_csum=P,
                                    d_hdr_mask=P, d_data_mask=P, d_nbad=P, mode=CRC, stream=STREAM),
    "lampi_msg_recv_unpack": dict(d_ring=P, nslots=8, slot_stride=1024, hdr_kind=GM, d_app=P, app_len=4096,
                                  seq_offset0=0, d_copied=P, d_csum=P, d_hdr_mask=P, d_data_mask=P, d_nbad=P,
                                  mode=CRC, stream=STREAM),
    "lampi_tmap_send_pack": dict(d_base=P, h_tmap=tmap(), pack_off=0, pack_len=4096, frag_len=512, d_ring=P,
                                 slot_stride=1024, h_fill=H_FILL, hdr_kind=GM, mode=CRC, stream=STREAM),
    "lampi_tmap_recv_unpack": dict(d_ring=P, nslots=8, slot_stride=1024, hdr_kind=GM, d_base=P, h_tmap=tmap(),
                                   seq_offset0=0, d_copied=P, d_csum=P, d_hdr_mask=P, d_data_mask=P, d_nbad=P,
                                   mode=CRC, stream=STREAM),
    "lampi_tmap_send_pack_batch": dict(d_frags=P, n=8, d_msgs=P, nmsgs=2, max_len=4096, d_hdrs=P, hdr_stride=128,
                                       hdr_kind=GM, mode=CRC, stream=STREAM),
    "lampi_tmap_recv_unpack_batch": dict(d_frags=P, n=8, d_msgs=P, nmsgs=2, max_len=4096, d_hdrs=P, hdr_stride=128,
                                         hdr_kind=GM, d_copied=P, d_csum=P, d_hdr_mask=P, d_data_mask=P, d_nbad=P,
                                         mode=CRC, stream=STREAM),
    "lampi_fill_stream": dict(d_dst=P, nbytes=4096, seed=1, byte_off=0, stream=STREAM),
    "lampi_fill_stream_frags": dict(d_dst=P, n=8, frag_len=512, seed=1, k0=0, kstep=1, stream=STREAM),
}


def _null(*names):
    return {k: 0 for k in names}


def _each_null(want, *names, **also):
    """One row per name: that pointer null."""
    return [(f"{k} null", dict(also, **{k: 0}), want) for k in names]


_TMAP_BAD = [  # what both typemap message forms refuse in the typemap itself
    ("typemap null", dict(h_tmap=0), 1),
    ("typemap pairs null", dict(h_tmap=tmap(d_pairs=0)), 1),
    ("typemap of zero pairs", dict(h_tmap=tmap(num_pairs=0)), 1),
    ("typemap packed_size 0", dict(h_tmap=tmap(packed_size=0)), 1),
    ("typemap reserved set", dict(h_tmap=tmap(reserved=1)), 1),
    ("typemap count * packed_size overflows", dict(h_tmap=tmap(count=1 << 62, packed_size=4)), 1),
    ("typemap form, Quadrics", dict(hdr_kind=QUADRICS), 1),
    ("kind 2", dict(hdr_kind=2), 1),
    ("mode 3", dict(mode=3), 1),
    ("hint bits", dict(mode=CRC | HINT), 1),
    ("BY_BYTES", dict(mode=CRC | BY_BYTES), 1),
]

_TMAP_BATCH_BAD = [  # what both typemap descriptor forms refuse
    ("mode 3", dict(mode=3), 1),
    ("hint bits", dict(mode=SUM | HINT), 1),
    ("typemap form, Quadrics", dict(hdr_kind=QUADRICS), 1),
    ("kind 2", dict(hdr_kind=2), 1),
    ("headers misaligned", dict(d_hdrs=P + 2), 1),
    ("header stride not a multiple of 4", dict(hdr_stride=74), 1),
    ("header stride shorter than the header", dict(hdr_stride=68), 1),
    ("no messages", dict(nmsgs=0), 1),
    ("no messages, n == 0", dict(nmsgs=0, n=0), 1),
    ("nmsgs over 2^32 - 1", dict(nmsgs=OVER), 1),
    ("n over 2^32 - 1", dict(n=OVER), 1),
    ("headers null, CRC", dict(d_hdrs=0), 1),
    ("headers null, CRC, n == 0", dict(d_hdrs=0, n=0), 1),
]

# name -> [(what the row changes, the changed arguments, the value the call must return)]
ROWS = {
    "lampi_frag_csum64_batch": [
        ("n == 0", dict(n=0), 0),
        ("n == 0, pointers null", dict(n=0, **_null("d_descs", "d_out")), 0),
    ] + _each_null(1, "d_descs", "d_out"),
    "lampi_frag_csum_batch": [
        ("NONE", dict(mode=NONE), 1),
        ("mode 3", dict(mode=3), 1),
        ("NONE with BY_BYTES", dict(mode=NONE | BY_BYTES), 1),
        ("mode 3, n == 0", dict(mode=3, n=0), 1),
        ("n == 0", dict(n=0, **_null("d_descs", "d_out")), 0),
        ("n == 0, BY_BYTES and hint bits", dict(n=0, mode=SUM | BY_BYTES | HINT), 0),
    ] + _each_null(1, "d_descs", "d_out"),
    "lampi_frag_csum_batch_strided": [
        ("NONE", dict(mode=NONE), 1),
        ("mode 3", dict(mode=3), 1),
        ("NONE, n == 0", dict(mode=NONE, n=0), 1),
        ("n == 0", dict(n=0, **_null("d_descs", "d_out")), 0),
        ("n == 0, BY_BYTES and hint bits", dict(n=0, mode=CRC | BY_BYTES | HINT), 0),
        ("n == 0, stride 0", dict(n=0, out_stride=0), 0),
        ("output misaligned", dict(d_out=P + 2), 1),
        ("output stride not a multiple of 4", dict(out_stride=70), 1),
        ("output stride 0", dict(out_stride=0), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
    ] + _each_null(1, "d_descs", "d_out"),
    "lampi_frag_bcopy_batch": [
        ("mode 3", dict(mode=3), 1),
        ("BY_BYTES", dict(mode=CRC | BY_BYTES), 1),
        ("mode 3, n == 0", dict(mode=3, n=0), 1),
        ("n == 0", dict(n=0, **_null("d_descs", "d_out")), 0),
        ("n == 0, NONE with hint bits", dict(n=0, mode=NONE | HINT), 0),
        ("output misaligned", dict(d_out=P + 2), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
        ("n over 2^32 - 1, NONE", dict(n=OVER, mode=NONE), 1),
        ("descriptors null, NONE", dict(d_descs=0, mode=NONE), 1),
    ] + _each_null(1, "d_descs", "d_out"),
    "lampi_frag_bcopy_batch_strided": [
        ("mode 3", dict(mode=3), 1),
        ("BY_BYTES", dict(mode=SUM | BY_BYTES), 1),
        ("BY_BYTES, n == 0", dict(mode=SUM | BY_BYTES, n=0), 1),
        ("n == 0", dict(n=0, **_null("d_descs", "d_out")), 0),
        ("n == 0, stride 0", dict(n=0, out_stride=0), 0),
        ("output misaligned", dict(d_out=P + 1), 1),
        ("output stride not a multiple of 4", dict(out_stride=70), 1),
        ("output stride 0", dict(out_stride=0), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
        ("n over 2^32 - 1, NONE", dict(n=OVER, mode=NONE, d_out=0), 1),
        ("descriptors null, NONE", dict(d_descs=0, mode=NONE), 1),
    ] + _each_null(1, "d_descs", "d_out"),
    "lampi_msg_bcopy": [
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("BY_BYTES", dict(mode=SUM | BY_BYTES), 1),
        ("frag_len 0", dict(frag_len=0), 1),
        ("frag_len over 2^32 - 1", dict(frag_len=OVER, dst_stride=OVER), 1),
        ("destination stride shorter than a fragment", dict(dst_stride=508), 1),
        ("output misaligned", dict(d_out=P + 2), 1),
        ("fragments over 2^32 - 1", dict(msg_len=OVER, frag_len=1), 1),
        ("NONE, empty message", dict(mode=NONE, msg_len=0, **_null("d_msg", "d_dst", "d_out")), 0),
        ("NONE, empty message, frag_len 0", dict(mode=NONE, msg_len=0, frag_len=0), 1),
        ("NONE, empty message, short destination stride", dict(mode=NONE, msg_len=0, dst_stride=8), 1),
        ("NONE, message null", dict(mode=NONE, d_msg=0), 1),
    ] + _each_null(1, "d_msg", "d_dst", "d_out"),
    "lampi_msg_bcopy_strided": [
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=NONE | HINT), 1),
        ("frag_len 0", dict(frag_len=0), 1),
        ("frag_len over 2^32 - 1", dict(frag_len=OVER, dst_stride=OVER), 1),
        ("destination stride shorter than a fragment", dict(dst_stride=508), 1),
        ("output misaligned", dict(d_out=P + 2), 1),
        ("output stride not a multiple of 4", dict(out_stride=70), 1),
        ("output stride 0", dict(out_stride=0), 1),
        ("fragments over 2^32 - 1", dict(msg_len=OVER, frag_len=1), 1),
        ("NONE, empty message", dict(mode=NONE, msg_len=0, out_stride=0, **_null("d_msg", "d_dst", "d_out")), 0),
        ("NONE, empty message, frag_len over 2^32 - 1", dict(mode=NONE, msg_len=0, frag_len=OVER, dst_stride=OVER), 1),
        ("empty message, output null", dict(msg_len=0, d_out=0), 1),
        ("NONE, destination null", dict(mode=NONE, d_dst=0), 1),
    ] + _each_null(1, "d_msg", "d_dst", "d_out"),
    "lampi_chain_csum_batch": [
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("mode 3, nfrags == 0", dict(mode=3, nfrags=0), 1),
        ("nfrags == 0", dict(nfrags=0, **_null("d_pieces", "d_first", "d_out")), 0),
        ("output misaligned", dict(d_out=P + 2), 1),
        ("npieces over 2^32 - 1", dict(npieces=OVER), 1),
        ("nfrags over 2^32 - 1", dict(nfrags=OVER), 1),
        ("nfrags over 2^32 - 1, NONE", dict(nfrags=OVER, mode=NONE), 1),
        ("first null, NONE", dict(d_first=0, mode=NONE, d_out=0), 1),
    ] + _each_null(1, "d_pieces", "d_first", "d_out"),
    "lampi_chain_csum_batch_strided": [
        ("mode 3", dict(mode=3), 1),
        ("BY_BYTES", dict(mode=SUM | BY_BYTES), 1),
        ("BY_BYTES, nfrags == 0", dict(mode=SUM | BY_BYTES, nfrags=0), 1),
        ("nfrags == 0", dict(nfrags=0, out_stride=0, **_null("d_pieces", "d_first", "d_out")), 0),
        ("nfrags == 0, NONE", dict(nfrags=0, mode=NONE), 0),
        ("output misaligned", dict(d_out=P + 2), 1),
        ("output stride not a multiple of 4", dict(out_stride=70), 1),
        ("output stride 0", dict(out_stride=0), 1),
        ("npieces over 2^32 - 1", dict(npieces=OVER), 1),
        ("nfrags over 2^32 - 1", dict(nfrags=OVER), 1),
        ("nfrags over 2^32 - 1, NONE", dict(nfrags=OVER, mode=NONE, d_out=0), 1),
        ("pieces null, NONE", dict(d_pieces=0, mode=NONE), 1),
    ] + _each_null(1, "d_pieces", "d_first", "d_out"),
    "lampi_header_csum_batch": [
        ("NONE", dict(mode=NONE), 1),
        ("NONE, n == 0", dict(mode=NONE, n=0), 1),
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("n == 0", dict(n=0, **_null("d_hdrs", "d_out")), 0),
        ("n == 0, headers misaligned", dict(n=0, d_hdrs=P + 2), 0),
        ("headers misaligned", dict(d_hdrs=P + 2), 1),
        ("header stride not a multiple of 4", dict(stride=74), 1),
        ("output misaligned", dict(d_out=P + 2), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
    ] + _each_null(1, "d_hdrs", "d_out"),
    "lampi_header_csum_batch_strided": [
        ("NONE", dict(mode=NONE), 0),
        ("NONE, everything else refusable", dict(mode=NONE, n=OVER, d_hdrs=0, d_out=P + 2, out_stride=0, stride=74), 0),
        ("mode 3", dict(mode=3), 1),
        ("mode 3, n == 0", dict(mode=3, n=0), 1),
        ("NONE with hint bits", dict(mode=NONE | HINT), 1),
        ("n == 0", dict(n=0, **_null("d_hdrs", "d_out")), 0),
        ("n == 0, strides refusable", dict(n=0, stride=74, out_stride=0), 0),
        ("headers misaligned", dict(d_hdrs=P + 2), 1),
        ("header stride not a multiple of 4", dict(stride=74), 1),
        ("output misaligned", dict(d_out=P + 2), 1),
        ("output stride not a multiple of 4", dict(out_stride=70), 1),
        ("output stride 0", dict(out_stride=0), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
    ] + _each_null(1, "d_hdrs", "d_out"),
    "lampi_header_check_batch": [
        ("NONE", dict(mode=NONE), 1),
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=SUM | HINT), 1),
        ("NONE, n == 0", dict(mode=NONE, n=0), 1),
        ("nbad null, n == 0", dict(d_nbad=0, n=0), 1),
        ("headers misaligned", dict(d_hdrs=P + 2), 1),
        ("headers misaligned, n == 0", dict(d_hdrs=P + 2, n=0), 1),
        ("header stride not a multiple of 4", dict(stride=74), 1),
        ("checksum offset not a multiple of 4", dict(csum_offset=66), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
    ] + _each_null(1, "d_hdrs", "d_mask", "d_nbad"),
    "lampi_header_compare_batch": [
        ("NONE", dict(mode=NONE), 1),
        ("mode 3", dict(mode=3), 1),
        ("BY_BYTES", dict(mode=CRC | BY_BYTES), 1),
        ("mode 3, n == 0", dict(mode=3, n=0), 1),
        ("nbad null, n == 0", dict(d_nbad=0, n=0), 1),
        ("headers misaligned", dict(d_hdrs=P + 1), 1),
        ("header stride not a multiple of 4", dict(stride=74), 1),
        ("header stride not a multiple of 4, n == 0", dict(stride=74, n=0), 1),
        ("checksum offset not a multiple of 4", dict(csum_offset=66), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
    ] + _each_null(1, "d_hdrs", "d_mask", "d_nbad"),
    "lampi_check_data_batch": [
        ("nbad null, n == 0", dict(d_nbad=0, n=0), 1),
        ("expected misaligned", dict(d_expected=P + 2), 1),
        ("expected misaligned, n == 0", dict(d_expected=P + 2, n=0), 1),
        ("expected stride not a multiple of 4", dict(expected_stride=74), 1),
        ("lengths misaligned", dict(d_lengths=P + 2), 1),
        ("lengths stride not a multiple of 4", dict(lengths_stride=74), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
    ] + _each_null(1, "d_calc", "d_expected", "d_mask", "d_nbad"),
    "lampi_copy_to_app_batch": [
        ("mode 3", dict(mode=3), 1),
        ("BY_BYTES", dict(mode=CRC | BY_BYTES), 1),
        ("mode 3, n == 0", dict(mode=3, n=0), 1),
        ("nbad null, n == 0", dict(d_nbad=0, n=0), 1),
        ("nbad null, NONE", dict(d_nbad=0, mode=NONE), 1),
        ("expected misaligned", dict(d_expected=P + 2), 1),
        ("expected misaligned, n == 0", dict(d_expected=P + 2, n=0), 1),
        ("expected stride not a multiple of 4", dict(expected_stride=74), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
        ("copied null, NONE", dict(d_copied=0, mode=NONE, d_expected=0), 1),
    ] + _each_null(1, "d_descs", "d_expected", "d_copied", "d_csum", "d_mask", "d_nbad"),
    "lampi_chain_copy_to_app_batch": [
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("mode 3, nfrags == 0", dict(mode=3, nfrags=0), 1),
        ("nbad null, nfrags == 0", dict(d_nbad=0, nfrags=0), 1),
        ("expected misaligned", dict(d_expected=P + 2), 1),
        ("expected stride not a multiple of 4", dict(expected_stride=74), 1),
        ("npieces over 2^32 - 1", dict(npieces=OVER), 1),
        ("nfrags over 2^32 - 1", dict(nfrags=OVER), 1),
        ("first null, NONE", dict(d_first=0, mode=NONE, d_expected=0), 1),
    ] + _each_null(1, "d_pieces", "d_first", "d_expected", "d_copied", "d_csum", "d_mask", "d_nbad"),
    "lampi_msg_csum": [
        ("NONE", dict(mode=NONE), 1),
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("BY_BYTES", dict(mode=SUM | BY_BYTES), 1),
        ("frag_len 0", dict(frag_len=0), 1),
        ("frag_len 0, empty message", dict(frag_len=0, msg_len=0), 1),
        ("frag_len over 2^32 - 1", dict(frag_len=OVER), 1),
        ("output null, empty message", dict(d_out=0, msg_len=0), 1),
    ] + _each_null(1, "d_msg", "d_out"),
    "lampi_send_pack_batch": [
        ("mode 3", dict(mode=3), 1),
        ("BY_BYTES", dict(mode=CRC | BY_BYTES), 1),
        ("kind 2", dict(hdr_kind=2), 1),
        ("kind 4", dict(hdr_kind=4), 1),
        ("kind 2, n == 0", dict(hdr_kind=2, n=0), 1),
        ("mode 3, n == 0", dict(mode=3, n=0), 1),
        ("headers misaligned", dict(d_hdrs=P + 2), 1),
        ("headers misaligned, n == 0", dict(d_hdrs=P + 2, n=0), 1),
        ("header stride not a multiple of 4", dict(hdr_stride=74), 1),
        ("header stride shorter than the header", dict(hdr_stride=68), 1),
        ("header stride shorter than the header, n == 0", dict(hdr_stride=68, n=0), 1),
        ("header stride shorter than the Quadrics header", dict(hdr_stride=72, hdr_kind=QUADRICS), 1),
        ("n == 0", dict(n=0, **_null("d_descs", "d_hdrs")), 0),
        ("n == 0, NONE with hint bits, Quadrics", dict(n=0, mode=NONE | HINT, hdr_kind=QUADRICS), 0),
        ("headers null, NONE, IB", dict(d_hdrs=0, mode=NONE, hdr_kind=IB), 1),
        ("headers null, NONE, Quadrics", dict(d_hdrs=0, mode=NONE, hdr_kind=QUADRICS), 1),
        ("descriptors null, NONE, GM", dict(d_descs=0, d_hdrs=0, mode=NONE), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
    ] + _each_null(1, "d_descs", "d_hdrs"),
    "lampi_msg_send_pack": [
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("kind 2", dict(hdr_kind=2), 1),
        ("frag_len 0", dict(frag_len=0), 1),
        ("frag_len over 2^32 - 1", dict(frag_len=OVER, slot_stride=2 * OVER), 1),
        ("ring misaligned", dict(d_ring=P + 4), 1),
        ("slot stride not a multiple of 8", dict(slot_stride=1028), 1),
        ("slot stride shorter than the header", dict(slot_stride=64, frag_len=8), 1),
        ("slot stride shorter than the Quadrics header", dict(slot_stride=120, frag_len=8, hdr_kind=QUADRICS), 1),
        ("no room for a fragment after the header", dict(slot_stride=576), 1),
        ("no room for a fragment after the header, IB, empty message", dict(slot_stride=576, hdr_kind=IB, msg_len=0), 1),
        ("Quadrics: no room for a fragment over 52 bytes", dict(hdr_kind=QUADRICS, frag_len=100, slot_stride=200), 1),
        ("Quadrics: no room for a fragment of 53 bytes", dict(hdr_kind=QUADRICS, frag_len=53, slot_stride=176), 1),
        ("fragments over 2^32 - 1", dict(msg_len=2 * OVER, frag_len=2), 1),
        ("message null, NONE", dict(d_msg=0, mode=NONE), 1),
    ] + _each_null(1, "d_msg", "d_ring", "h_fill"),
    "lampi_recv_unpack_batch": [
        ("mode 3", dict(mode=3), 1),
        ("BY_BYTES", dict(mode=CRC | BY_BYTES), 1),
        ("kind 2", dict(hdr_kind=2), 1),
        ("kind 2, n == 0", dict(hdr_kind=2, n=0), 1),
        ("headers misaligned", dict(d_hdrs=P + 2), 1),
        ("header stride not a multiple of 4", dict(hdr_stride=74), 1),
        ("header stride shorter than the header", dict(hdr_stride=68), 1),
        ("header stride shorter than the Quadrics header", dict(hdr_stride=72, hdr_kind=QUADRICS), 1),
        ("nbad null, n == 0", dict(d_nbad=0, n=0), 1),
        ("n over 2^32 - 1", dict(n=OVER), 1),
        ("headers null, NONE, Quadrics", dict(d_hdrs=0, mode=NONE, hdr_kind=QUADRICS), 1),
        ("copied null, NONE", dict(d_copied=0, d_hdrs=0, mode=NONE), 1),
    ] + _each_null(1, "d_descs", "d_hdrs", "d_copied", "d_csum", "d_hdr_mask", "d_data_mask", "d_nbad"),
    "lampi_msg_recv_unpack": [
        ("mode 3", dict(mode=3), 1),
        ("hint bits", dict(mode=CRC | HINT), 1),
        ("kind 2", dict(hdr_kind=2), 1),
        ("ring misaligned", dict(d_ring=P + 4), 1),
        ("ring misaligned, no slots", dict(d_ring=P + 4, nslots=0), 1),
        ("slot stride not a multiple of 8", dict(slot_stride=1028), 1),
        ("slot stride shorter than the header", dict(slot_stride=64), 1),
        ("slot stride shorter than the Quadrics header", dict(slot_stride=120, hdr_kind=QUADRICS), 1),
        ("nbad null, no slots", dict(d_nbad=0, nslots=0), 1),
        ("nslots over 2^32 - 1", dict(nslots=OVER), 1),
        ("application buffer null, no slots", dict(d_app=0, nslots=0), 1),
    ] + _each_null(1, "d_ring", "d_app", "d_copied", "d_csum", "d_hdr_mask", "d_data_mask", "d_nbad"),
    "lampi_tmap_send_pack": _TMAP_BAD + [
        ("window starts past the message", dict(pack_off=48001, pack_len=0), 1),
        ("window ends past the message", dict(pack_off=47000, pack_len=1001), 1),
        ("window longer than the message", dict(pack_len=48001), 1),
        ("frag_len 0", dict(frag_len=0), 1),
        ("frag_len 0, empty window", dict(frag_len=0, pack_len=0), 1),
        ("frag_len over 2^32 - 1", dict(frag_len=OVER, slot_stride=2 * OVER), 1),
        ("ring misaligned", dict(d_ring=P + 4), 1),
        ("slot stride not a multiple of 8", dict(slot_stride=1028), 1),
        ("slot stride shorter than the header", dict(slot_stride=64, frag_len=8), 1),
        ("no room for a fragment after the header", dict(slot_stride=576), 1),
        ("fragments over 2^32 - 1", dict(h_tmap=tmap(count=1 << 40), pack_len=2 * OVER, frag_len=2), 1),
        ("base null, NONE", dict(d_base=0, mode=NONE), 1),
    ] + _each_null(1, "d_base", "d_ring", "h_fill"),
    "lampi_tmap_recv_unpack": _TMAP_BAD + [
        ("ring misaligned", dict(d_ring=P + 4), 1),
        ("slot stride not a multiple of 8", dict(slot_stride=1028), 1),
        ("slot stride shorter than the header", dict(slot_stride=64), 1),
        ("nbad null, no slots", dict(d_nbad=0, nslots=0), 1),
        ("nslots over 2^32 - 1", dict(nslots=OVER), 1),
        ("base null, no slots", dict(d_base=0, nslots=0), 1),
    ] + _each_null(1, "d_ring", "d_base", "d_copied", "d_csum", "d_hdr_mask", "d_data_mask", "d_nbad"),
    "lampi_tmap_send_pack_batch": _TMAP_BATCH_BAD + [
        ("headers null, NONE, IB", dict(d_hdrs=0, mode=NONE, hdr_kind=IB), 1),
        ("n == 0", dict(n=0, **_null("d_frags", "d_msgs")), 0),
        ("n == 0, headers null, NONE, GM", dict(n=0, d_hdrs=0, mode=NONE, **_null("d_frags", "d_msgs")), 0),
        ("records null, headers null, NONE, GM", dict(d_frags=0, d_hdrs=0, mode=NONE), 1),
    ] + _each_null(1, "d_frags", "d_msgs"),
    "lampi_tmap_recv_unpack_batch": _TMAP_BATCH_BAD + [
        ("headers null, SUM", dict(d_hdrs=0, mode=SUM), 1),
        ("copied null, n == 0", dict(d_copied=0, n=0), 1),
        ("nbad null, n == 0, NONE", dict(d_nbad=0, n=0, mode=NONE, d_hdrs=0), 1),
        ("records null, headers null, NONE", dict(d_frags=0, d_hdrs=0, mode=NONE), 1),
    ] + _each_null(1, "d_frags", "d_msgs", "d_copied", "d_csum", "d_hdr_mask", "d_data_mask", "d_nbad"),
    "lampi_fill_stream": [
        ("nbytes == 0", dict(nbytes=0), 0),
        ("nbytes == 0, destination null", dict(nbytes=0, d_dst=0), 0),
        ("destination null", dict(d_dst=0), 1),
    ],
    "lampi_fill_stream_frags": [
        ("n == 0", dict(n=0), 0),
        ("n == 0, everything else refusable", dict(n=0, d_dst=0, frag_len=0), 0),
        ("destination null", dict(d_dst=0), 1),
        ("frag_len 0", dict(frag_len=0), 1),
        ("frag_len not a multiple of 8", dict(frag_len=508), 1),
        ("destination misaligned", dict(d_dst=P + 4), 1),
    ],
}


def table():
    """[(entry point, what the row changes, arguments, expected)]: every entry point's well-formed call (expected
    None: it must reach the device), then its rows."""
    out = []
    for name, base in BASE.items():
        out.append((name, "well-formed", tuple(base.values()), None))
        for what, change, want in ROWS[name]:
            assert set(change) <= set(base), (name, what)
            out.append((name, what, tuple(dict(base, **change).values()), want))
    return out


def _child():
    sys.path.insert(0, ROOT)
    from lampi_amd import _lib

    lib = _lib.lib()
    print(json.dumps([getattr(lib, name)(*args) for name, _, args, _ in table()]))


def test_table_covers_every_device_entry_point():
    from lampi_amd import _lib

    device = {name for name, (res, args) in _lib.PROTOTYPES.items()
              if res is ctypes.c_int and not name.startswith("lampi_host_")}
    assert device == set(BASE) == set(ROWS)
    for name, base in BASE.items():
        assert len(base) == len(_lib.PROTOTYPES[name][1]), name
        assert list(base)[-1] == "stream", name
        assert {want for _, _, want in ROWS[name]} <= {0, 1} and any(want == 1 for _, _, want in ROWS[name]), name


def test_refusals_and_early_successes_without_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    rows = table()
    assert len(got) == len(rows)
    wrong = []
    for (name, what, _, want), rc in zip(rows, got):
        if want is None:
            if rc in (0, 1):  # the well-formed call must get as far as the device (hipErrorNoDevice there)
                wrong.append(f"{name}: the well-formed call returned {rc}")
        elif rc != want:
            wrong.append(f"{name}: {what}: returned {rc}, expected {want}")
    assert not wrong, "\n".join(wrong)


if __name__ == "__main__":
    _child()
