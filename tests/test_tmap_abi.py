"""CPU: the typemap forms of the one-call steps (lampi_tmap_send_pack, lampi_tmap_recv_unpack) are declared in
include/lampi_csum.h, exported by the library and bound in lampi_amd._lib.PROTOTYPES; lampi_tmap_elt and lampi_tmap
have the documented layout in C and in ctypes.  The kernels are exercised by tests/test_gpu_tmap_*.py.
"""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lampi_csum.h")
NAMES = ("lampi_tmap_send_pack", "lampi_tmap_recv_unpack")


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
    assert len(lampi_amd._lib.PROTOTYPES["lampi_tmap_send_pack"][1]) == 11
    assert len(lampi_amd._lib.PROTOTYPES["lampi_tmap_recv_unpack"][1]) == 14


def test_struct_layout_in_c_and_ctypes(tmp_path):
    from lampi_amd._lib import Tmap, TmapElt

    prog = tmp_path / "layout.c"
    prog.write_text('#include "lampi_csum.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                    'int main(void) {\n'
                    '    printf("%zu %zu %zu %zu\\n", sizeof(lampi_tmap_elt), offsetof(lampi_tmap_elt, size),\n'
                    '           offsetof(lampi_tmap_elt, offset), offsetof(lampi_tmap_elt, seq_offset));\n'
                    '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(lampi_tmap), offsetof(lampi_tmap, d_pairs),\n'
                    '           offsetof(lampi_tmap, extent), offsetof(lampi_tmap, packed_size),\n'
                    '           offsetof(lampi_tmap, count), offsetof(lampi_tmap, num_pairs),\n'
                    '           offsetof(lampi_tmap, reserved));\n'
                    '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)],
                   check=True)
    elt, tm = [[int(x) for x in line.split()]
               for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert elt == [24, 0, 8, 16]
    assert tm == [40, 0, 8, 16, 24, 32, 36]
    assert [ctypes.sizeof(TmapElt)] + [getattr(TmapElt, f).offset for f in ("size", "offset", "seq_offset")] == elt
    assert [ctypes.sizeof(Tmap)] + [getattr(Tmap, f).offset for f in
                                    ("d_pairs", "extent", "packed_size", "count", "num_pairs", "reserved")] == tm


def test_device_functions_exist():
    import lampi_amd
    from lampi_amd import device as dv

    for name in ("tmap_send_pack", "tmap_recv_unpack"):
        assert callable(getattr(dv, name)) and name in dv.__all__
        assert getattr(lampi_amd, name) is getattr(dv, name)
    assert callable(dv.make_tmap) and "make_tmap" in dv.__all__
