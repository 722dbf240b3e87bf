"""CPU: the Quadrics header kind (LAMPI_SEND_HDR_QUADRICS = 3) is declared in include/lampi_csum.h with that value,
mirrored in lampi_amd._lib, lampi_amd.device and the package, and the Python wrappers size their bounds checks by
the kind (72 or 128 bytes) and require the headers in every mode.  The kernels are exercised by
tests/test_gpu_quadrics_*.py.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lampi_csum.h")


def test_enum_value_in_c(tmp_path):
    prog = tmp_path / "kinds.c"
    prog.write_text('#include "lampi_csum.h"\n#include <stdio.h>\n'
                    'int main(void) { enum lampi_send_hdr_kind k = LAMPI_SEND_HDR_QUADRICS;\n'
                    'printf("%d %d %d\\n", LAMPI_SEND_HDR_GM, LAMPI_SEND_HDR_IB, (int)k); return 0; }\n')
    exe = tmp_path / "kinds"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)],
                   check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals == [0, 1, 3]


def test_python_constants():
    import lampi_amd
    from lampi_amd import _lib
    from lampi_amd import device as dv

    assert _lib.HDR_QUADRICS == 3 and dv.HDR_QUADRICS == 3 and lampi_amd.HDR_QUADRICS == 3
    assert (_lib.HDR_GM, _lib.HDR_IB) == (0, 1)
    assert "HDR_QUADRICS" in dv.__all__
    assert (dv.hdr_bytes(dv.HDR_GM), dv.hdr_bytes(dv.HDR_IB), dv.hdr_bytes(dv.HDR_QUADRICS)) == (72, 72, 128)
    assert (dv.QUADRICS_HDR_BYTES, dv.QUADRICS_INLINE_BYTES) == (128, 52)


class _Dev:
    """A device tensor as far as the wrappers' argument checks look: they must raise before any call is made."""

    is_cuda = True

    def __init__(self, nbytes):
        self.nbytes = nbytes

    def is_contiguous(self):
        return True

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1

    def data_ptr(self):
        raise AssertionError("the wrapper went past its argument checks")

    device = "cuda:0"


def test_wrappers_reject_before_calling():
    from lampi_amd import device as dv

    Q = dv.HDR_QUADRICS
    descs = _Dev(4 * 32)
    for mode in (dv.CRC32, dv.SUM32, dv.NONE):  # the headers are required in every mode
        with pytest.raises(ValueError):
            dv.send_pack_batch(descs, None, 128, kind=Q, mode=mode)
        with pytest.raises(ValueError):
            dv.recv_unpack_batch(descs, None, 128, kind=Q, mode=mode)
    # four headers at stride 256: 3 * 256 + 128 bytes are needed -- 72 more than the last header's start is not enough
    short = _Dev(3 * 256 + 72)
    with pytest.raises(ValueError):
        dv.send_pack_batch(descs, short, 256, kind=Q, mode=dv.CRC32)
    with pytest.raises(ValueError):
        dv.recv_unpack_batch(descs, short, 256, kind=Q, mode=dv.CRC32)
    msg, ring = _Dev(8192), _Dev(1 << 20)
    tmpl = bytes(72)
    with pytest.raises(ValueError):  # neither a bare envelope queue nor room for a fragment
        dv.msg_send_pack(msg, 2048, ring, 136, tmpl, kind=Q)
    with pytest.raises(ValueError):
        dv.msg_send_pack(msg, 2048, ring, 120, tmpl, kind=Q)
    with pytest.raises(ValueError):  # four envelopes need 3 * 128 + 128 bytes
        dv.msg_send_pack(msg, 2048, _Dev(3 * 128 + 72), 128, tmpl, kind=Q)
    with pytest.raises(ValueError):  # the last fragment's payload too
        dv.msg_send_pack(msg, 2048, _Dev(3 * 2176 + 128 + 2047), 2176, tmpl, kind=Q)
    with pytest.raises(ValueError):
        dv.msg_recv_unpack(ring, 4, 120, _Dev(4096), kind=Q)
