"""CPU: the descriptor forms of the typemap steps (lampi_tmap_send_pack_batch, lampi_tmap_recv_unpack_batch) are
declared in include/lampi_csum.h, exported by the library and bound in lampi_amd._lib.PROTOTYPES; lampi_tmap_msg and
lampi_tmap_frag have the documented layout in C and in ctypes.  The kernels are exercised by
tests/test_gpu_tmap_batch_*.py.
"""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lampi_csum.h")
NAMES = ("lampi_tmap_send_pack_batch", "lampi_tmap_recv_unpack_batch")
MSG_FIELDS = ("d_pairs", "extent", "packed_size", "count", "num_pairs", "reserved", "base", "reserved2")
FRAG_FIELDS = ("payload", "pack_off", "length", "msg", "reserved")


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
    assert len(lampi_amd._lib.PROTOTYPES["lampi_tmap_send_pack_batch"][1]) == 10
    assert len(lampi_amd._lib.PROTOTYPES["lampi_tmap_recv_unpack_batch"][1]) == 15


def test_struct_layout_in_c_and_ctypes(tmp_path):
    from lampi_amd._lib import TmapFrag, TmapMsg

    def line(struct, fields):
        args = ", ".join([f"sizeof({struct})"] + [f"offsetof({struct}, {f})" for f in fields])
        return f'    printf("{" ".join(["%zu"] * (len(fields) + 1))}\\n", {args});\n'

    prog = tmp_path / "layout.c"
    prog.write_text('#include "lampi_csum.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n'
                    + line("lampi_tmap_msg", MSG_FIELDS) + line("lampi_tmap_frag", FRAG_FIELDS) + '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)],
                   check=True)
    msg, frag = [[int(x) for x in ln.split()]
                 for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert msg == [64, 0, 8, 16, 24, 32, 36, 40, 48]
    assert frag == [32, 0, 8, 16, 20, 24]
    assert [ctypes.sizeof(TmapMsg)] + [getattr(TmapMsg, f).offset for f in MSG_FIELDS] == msg
    assert [ctypes.sizeof(TmapFrag)] + [getattr(TmapFrag, f).offset for f in FRAG_FIELDS] == frag


def test_device_functions_exist():
    import lampi_amd
    from lampi_amd import device as dv

    for name in ("make_tmap_msgs", "make_tmap_frags", "tmap_send_pack_batch", "tmap_recv_unpack_batch"):
        assert callable(getattr(dv, name)) and name in dv.__all__
        assert getattr(lampi_amd, name) is getattr(dv, name)
