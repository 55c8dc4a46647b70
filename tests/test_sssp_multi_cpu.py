"""CPU tests of the many-source calls' boundary (include/mpfmt.h "many-source fields and cost matrices"): the C caller with the documented
ccall widths compiles and links against libmpfmt.so under -Wcast-function-type -Werror, the ctypes struct of the matrix info has the size
and field offsets gcc gives the C struct, and the two calls are documented with the ccall a Julia user would write (the glue itself gets
no new ccall: tests/test_abi.py ties every ccall of the glue to two C callers that stay as they are)."""
import ctypes
import os
import re
import subprocess

import motionplanning_jl_amd as mp

L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include")]


def test_the_c_caller_compiles_and_links(tmp_path):
    exe = str(tmp_path / "abi_caller8")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc"] + FLAGS + [os.path.join(ROOT, "tests", "abi_c", "abi_caller8.c"), "-o", exe, "-L", pkg, "-lmpfmt",
                                             "-Wl,-rpath," + pkg])
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "tests", "abi_c", "abi_caller8.c")).read()
    assert "mpfmt_graph_sssp_multi" in src and "mpfmt_roadmap_matrix" in src


def test_matrix_info_struct_matches_the_c_layout(tmp_path):
    names = [n for n, _ in L.RoadmapMatrixInfo._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpfmt.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(mpfmt_roadmap_matrix_info));\n' +
                    "".join('  printf(" %%zu", offsetof(mpfmt_roadmap_matrix_info, %s));\n' % n for n in names) +
                    '  printf(" %zu\\n", sizeof(mpfmt_sssp_info));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc"] + FLAGS + [str(prog), "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).split()]
    assert out[0] == ctypes.sizeof(L.RoadmapMatrixInfo)
    assert out[1:-1] == [getattr(L.RoadmapMatrixInfo, n).offset for n in names]
    assert out[-1] == ctypes.sizeof(L.SsspInfo)


def test_the_two_calls_are_bound_exported_and_documented():
    table = {n: (res, args) for n, res, args in L.SYMBOLS}
    assert table["mpfmt_graph_sssp_multi"] == table["mpfmt_graph_sssp"]      # the same contract, argument for argument
    assert len(table["mpfmt_roadmap_matrix"][1]) == 9
    lib = ctypes.CDLL(L.so_path())
    assert hasattr(lib, "mpfmt_graph_sssp_multi") and hasattr(lib, "mpfmt_roadmap_matrix")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in ("mpfmt_graph_sssp_multi", "mpfmt_roadmap_matrix"):
        assert re.search(r"ccall\(\(:%s, libmpfmt\)" % sym, doc), sym
    jl = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    assert "mpfmt_graph_sssp_multi" not in jl and "mpfmt_roadmap_matrix" not in jl
    assert hasattr(mp.Context, "graph_sssp_multi") and hasattr(mp.Context, "roadmap_matrix") and hasattr(mp, "roadmap_matrix_")
