"""CPU: the one-call send step (lampi_send_pack_batch, lampi_msg_send_pack) is declared in include/lampi_csum.h,
exported by the library and bound in lampi_amd._lib.PROTOTYPES; the header kinds and the host-side fill struct have
the documented values and layout.  The kernels are exercised by tests/test_gpu_send_pack.py.
"""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lampi_csum.h")
NAMES = ("lampi_send_pack_batch", "lampi_msg_send_pack")


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
    assert len(lampi_amd._lib.PROTOTYPES["lampi_send_pack_batch"][1]) == 7
    assert len(lampi_amd._lib.PROTOTYPES["lampi_msg_send_pack"][1]) == 9


def test_header_kind_constants(tmp_path):
    from lampi_amd import device as dv
    from lampi_amd._lib import HDR_GM, HDR_IB

    assert (HDR_GM, HDR_IB) == (0, 1) and (dv.HDR_GM, dv.HDR_IB) == (0, 1)
    prog = tmp_path / "kinds.c"
    prog.write_text('#include "lampi_csum.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                    'int main(void) { printf("%d %d %zu %zu %zu %zu\\n", LAMPI_SEND_HDR_GM, LAMPI_SEND_HDR_IB, '
                    'sizeof(lampi_send_hdr_fill), offsetof(lampi_send_hdr_fill, tmpl), '
                    'offsetof(lampi_send_hdr_fill, frag_seq0), offsetof(lampi_send_hdr_fill, seq_offset0)); '
                    'return 0; }\n')
    exe = tmp_path / "kinds"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)],
                   check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals == [0, 1, 112, 0, 72, 104]


def test_fill_struct_mirror_layout():
    from lampi_amd._lib import SendHdrFill

    assert ctypes.sizeof(SendHdrFill) == 112
    assert SendHdrFill.tmpl.offset == 0 and SendHdrFill.tmpl.size == 72
    assert [getattr(SendHdrFill, f).offset for f in ("frag_seq0", "frag_seq_step", "desc_ptr0", "desc_ptr_stride",
                                                      "seq_offset0")] == [72, 80, 88, 96, 104]


def test_device_functions_exist():
    from lampi_amd import device as dv

    assert callable(dv.send_pack_batch) and callable(dv.msg_send_pack)
    assert "send_pack_batch" in dv.__all__ and "msg_send_pack" in dv.__all__
