"""lampi_amd -- MI355X-native engine for LA-MPI's per-fragment data-integrity checksums.

Hot path (BASELINE.json north_star): the 32-bit CRC (``uicrc``, CRC-32/MPEG-2) and additive
(``uicsum``) checksums that LA-MPI computes over every message fragment
(ref src/util/MemFunctions.cc, applied in src/path/{gm,ib,quadrics}), as hand-written HIP
kernels for gfx950 behind the C ABI in include/lampi_csum.h (liblampi_csum.so).

* :mod:`lampi_amd.memfunctions` -- the reference's host API (``uicrc``, ``bcopy_uicrc``,
  ``uicsum``, ``bcopy_uicsum``, ``header_checksum``), computed on the GPU.
* :mod:`lampi_amd.device` -- batched device-resident checksums over torch tensors
  (imported lazily: it needs torch).
* :mod:`lampi_amd.host` -- the one-call send and receive steps over numpy arrays in host memory.
"""
from ._lib import (CRC32, CRC_INITIAL_REGISTER, CRC_POLYNOMIAL, HDR_GM, HDR_IB, HDR_QUADRICS, NONE,  # noqa: F401
                   RECV_DATA_BAD, RECV_HDR_BAD, SUM32, FragDesc, lib)
from .memfunctions import (PartialState, PartialState64, bcopy_csum, bcopy_uicrc, bcopy_uicsum,  # noqa: F401
                           csum, header_checksum, uicrc, uicsum)

__version__ = "0.1.0"

# The receive step in one call lives in :mod:`lampi_amd.device`; the names resolve on first use, so importing the
# package still needs no torch.
_DEVICE_EXPORTS = ("recv_unpack_batch", "msg_recv_unpack", "tmap_send_pack", "tmap_recv_unpack", "make_tmap_msgs",
                   "make_tmap_frags", "tmap_send_pack_batch", "tmap_recv_unpack_batch")


def __getattr__(name):
    if name in _DEVICE_EXPORTS:
        from . import device

        return getattr(device, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
