"""CPU: the one-call receive step (lampi_recv_unpack_batch, lampi_msg_recv_unpack) is declared in
include/lampi_csum.h, exported by the library and bound in lampi_amd._lib.PROTOTYPES; its two return codes have the
documented values in C and in Python.  The kernels are exercised by tests/test_gpu_recv_unpack.py.
"""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lampi_csum.h")
NAMES = ("lampi_recv_unpack_batch", "lampi_msg_recv_unpack")


def test_entry_points_declared_exported_and_bound():
    import lampi_amd

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lampi_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", lampi_amd._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (lampi_[a-z0-9_]+)", out))
    lib = lampi_amd.lib()
    for name in NAMES:
        assert name in declared, name
        assert name in exported, name
        assert name in lampi_amd._lib.PROTOTYPES, name
        assert getattr(lib, name).restype is ctypes.c_int
    assert len(lampi_amd._lib.PROTOTYPES["lampi_recv_unpack_batch"][1]) == 12
    assert len(lampi_amd._lib.PROTOTYPES["lampi_msg_recv_unpack"][1]) == 14


def test_return_code_constants(tmp_path):
    import lampi_amd
    from lampi_amd import device as dv
    from lampi_amd._lib import RECV_DATA_BAD, RECV_HDR_BAD

    assert (RECV_DATA_BAD, RECV_HDR_BAD) == (-1, -2)
    assert (dv.RECV_DATA_BAD, dv.RECV_HDR_BAD) == (-1, -2)
    assert (lampi_amd.RECV_DATA_BAD, lampi_amd.RECV_HDR_BAD) == (-1, -2)
    prog = tmp_path / "codes.c"
    prog.write_text('#include "lampi_csum.h"\n#include <stdio.h>\n'
                    'int main(void) { printf("%d %d %d %d\\n", LAMPI_RECV_DATA_BAD, LAMPI_RECV_HDR_BAD, '
                    'LAMPI_SEND_HDR_GM, LAMPI_SEND_HDR_IB); return 0; }\n')
    exe = tmp_path / "codes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)],
                   check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals == [-1, -2, 0, 1]


def test_device_functions_exist():
    import lampi_amd
    from lampi_amd import device as dv

    for name in ("recv_unpack_batch", "msg_recv_unpack"):
        assert callable(getattr(dv, name)) and name in dv.__all__
        assert getattr(lampi_amd, name) is getattr(dv, name)
