"""CPU tests of what carrying a tracked field across a growth of the sample set rests on (include/mpfmt.h, "growing the sample set",
TRACKED FIELDS; option "samples_add_keeps_fields").  No GPU is needed.

The host statement of the contract: mpfmt_host_graph_grow followed by mpfmt_host_field_repair on the extended arrays -- C padded with
+Inf, A padded with 0, dirty = the new columns and the old columns that gained or lost an entry -- returns exactly
mpfmt_host_graph_sssp of the grown graph.  Every comparison is on bytes.

Status of these tests: the composition tests call host code that exists without the feature, so they pass before it as well; they pin
the contract the device side is held to (tests/test_gpu_growfield.py), they do not demonstrate the feature.  The tests at the end of
the file (the export, the option, the stats, the Python surface) are the ones that fail without it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grow_cases as gc  # noqa: E402
import growfield_cases as gf  # noqa: E402

L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = gc.WORLDS[:4]
_old, _grown = {}, {}


def old_graph(world):
    """(w, colptr0, rowval0 int32, nzval, efree) of the world's own samples at w.r, from the oracle; computed once."""
    if world not in _old:
        w = gc.box_world(*world)
        cp, rv, nz = orc.rdisc_graph(w.X, w.r)
        ef = orc.graph_edges_free(w.X, cp, rv, w.lohi, w.ss_lo, w.ss_hi)
        _old[world] = (w, cp, rv.astype(np.int32), nz, ef)
    return _old[world]


def grown_graph(world, tag, shrink):
    """(X_all, r_new, the grown graph of mpfmt_host_graph_grow, its info); computed once and left unchanged."""
    key = (world, tag, shrink)
    if key not in _grown:
        w, cp, rv, nz, ef = old_graph(world)
        n_add = gc.n_add_of(tag, w.N)
        X_all = np.concatenate([w.X, gc.batch(w, n_add, world[3])])
        r_new = gc.shrunk_radius(w, len(X_all)) if shrink else w.r
        g = L.host_graph_grow(X_all, w.N, cp, rv, nz, ef, w.lohi, w.ss_lo, w.ss_hi, r_new)
        _grown[key] = (X_all, r_new, g[:4], g[4])
    return _grown[key]


def compose(world, tag, shrink, checkpts, source):
    """The old field, carried on the host and repaired; returns (got C, A, invalidated), (want C, A), old C, the dirty bits, info."""
    w, cp, rv, nz, ef = old_graph(world)
    X_all, r_new, g, info = grown_graph(world, tag, shrink)
    F_old = orc.points_free(w.X, w.lohi, w.ss_lo, w.ss_hi) if checkpts else None
    F_new = orc.points_free(X_all, w.lohi, w.ss_lo, w.ss_hi) if checkpts else None
    C0, A0 = L.host_graph_sssp(cp, rv, nz, ef, F=F_old, source=source)
    dirty = gf.changed_columns(cp, rv, g[0], g[1])
    Cp, Ap = gf.padded_field(C0, A0, len(X_all))
    got = L.host_field_repair(g[0], g[1], g[2], g[3], F_new, L.pack_bits(dirty), Cp, Ap, source=source)
    want = L.host_graph_sssp(g[0], g[1], g[2], g[3], F=F_new, source=source)
    return got, want, C0, dirty, info


@pytest.mark.parametrize("checkpts", [False, True], ids=["nocheck", "checkpts"])
@pytest.mark.parametrize("shrink", [False, True], ids=["same_r", "smaller_r"])
@pytest.mark.parametrize("tag", ("1", "65", "N"))
@pytest.mark.parametrize("world", WORLDS, ids=lambda t: "N%d_d%d" % (t[0], t[1]))
def test_grow_then_repair_equals_a_fresh_field(world, tag, shrink, checkpts):
    for source in (1, 8):
        got, want, C0, dirty, info = compose(world, tag, shrink, checkpts, source)
        assert gc.same(got[0], want[0]) and gc.same(got[1], want[1]), source
        assert shrink or got[2] == 0                                              # (no entry lost, no bit cleared: nothing to invalidate)


@pytest.mark.parametrize("world", WORLDS, ids=lambda t: "N%d_d%d" % (t[0], t[1]))
def test_the_scenes_exercise_the_branches_of_the_repair(world):
    """Source 1, a batch of 65: at the kept radius nothing is invalidated, old labels fall and new samples are reached; at the shrunk
    radius samples lose their labels.  A repair whose branches no scene takes would be tested by nothing."""
    n_old = world[0]
    got, want, C0, dirty, info = compose(world, "65", False, False, 1)
    assert got[2] == 0 and info["dropped"] == 0
    assert int((want[0][:n_old] != C0).sum()) > 0, "no old label changed"
    assert int(np.isfinite(want[0][n_old:]).sum()) > 0, "no new sample reached"
    assert dirty[n_old:].all() and 0 < int(dirty[:n_old].sum()) < n_old
    got, want, C0, dirty, info = compose(world, "65", True, False, 1)
    assert got[2] > 0 and info["dropped"] > 0
    print("N %d: kept radius: dirty %d; shrunk radius: invalidated %d, dropped %d, dirty %d" % (n_old, 0, got[2], info["dropped"], int(dirty.sum())))


def test_the_empty_field_stays_empty():
    """Source 8 of the world (5003, 3, 40, 13) reaches no other sample, before and after the growth (the batch's bit-copy of sample 8, a
    new sample at distance 0, is all it can get)."""
    world = (5003, 3, 40, 13)
    for shrink in (False, True):
        got, want, C0, dirty, info = compose(world, "65", shrink, False, 8)
        assert int(np.isfinite(C0).sum()) == 1 and int(np.isfinite(want[0][:world[0]]).sum()) == 1 and got[2] == 0
        assert int(np.isfinite(want[0][world[0] + 1:]).sum()) == 0
        assert gc.same(got[0], want[0]) and gc.same(got[1], want[1])


@pytest.mark.parametrize("world, invalidated, dropped", [(gc.WORLDS[0], 16, 12), (gc.WORLDS[1], 10, 10)], ids=["N130", "N2000"])
def test_a_dropped_parent_edge_counts_as_lost(world, invalidated, dropped):
    """One new sample at the shrunk radius, source 8: the smallest scenes in which entries that the radius rule drops are parent edges.
    The dropped entries clear no mask bit -- they are gone -- and the repair still has to invalidate their children."""
    got, want, C0, dirty, info = compose(world, "1", True, False, 8)
    assert info["dropped"] == dropped and got[2] == invalidated
    assert gc.same(got[0], want[0]) and gc.same(got[1], want[1])


def test_the_changed_columns_are_what_the_merge_flags():
    """The dirty set in closed form on a scene small enough to check by hand: every new column, and exactly the old columns whose list of
    rows below n_old shrank (lost) or that hold a row >= n_old (gained)."""
    world = gc.WORLDS[0]
    w, cp, rv, nz, ef = old_graph(world)
    X_all, r_new, g, info = grown_graph(world, "65", True)
    dirty = gf.changed_columns(cp, rv, g[0], g[1])
    for x in range(w.N):
        old = set(rv[cp[x]:cp[x + 1]].tolist()); new = set(g[1][g[0][x]:g[0][x + 1]].tolist())
        assert dirty[x] == (old != new), x
    assert dirty[w.N:].all() and len(dirty) == len(X_all)


# ---- the feature's surface: these fail without it ------------------------------------------------------------------------------------

def test_the_header_declares_the_export_the_option_and_the_stats():
    hdr = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    assert re.search(r"MPFMT_API int32_t mpfmt_togo_targets_add\(mpfmt_ctx\* ctx, const int64_t\* targets, int64_t ntgt\);", hdr)
    assert re.search(r'"samples_add_keeps_fields"\s*\(default 0\)', hdr)
    for stat in ("samples_add_flagged_columns", "samples_add_fields_carried"):
        assert '"%s"' % stat in hdr, stat
    src = open(os.path.join(ROOT, "motionplanning.jl_amd", "csrc", "mpfmt_capi.hip")).read()
    for name in ("samples_add_keeps_fields", "samples_add_flagged_columns", "samples_add_fields_carried"):
        assert '"%s"' % name in src, name


def test_the_python_surface_carries_the_export():
    names = [s[0] for s in L.SYMBOLS]
    assert "mpfmt_togo_targets_add" in names
    assert hasattr(L.lib(), "mpfmt_togo_targets_add") and callable(getattr(mp.Context, "togo_targets_add", None))
    assert L.OPT_SAMPLES_ADD_KEEPS_FIELDS == "samples_add_keeps_fields"
    for fn in (mp.replan_, mp.repolicy_, mp.prmstar_, mp.cost_to_go_):
        assert "grow_" in fn.__doc__, fn.__name__
    assert "samples_add_keeps_fields" in mp.grow_.__doc__ and "samples_add_keeps_fields" in mp.Context.samples_add.__doc__


def test_the_documents_name_the_feature():
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md", "LABNOTES.md"):
        assert "samples_add_keeps_fields" in open(os.path.join(ROOT, doc)).read(), doc
    assert "mpfmt_togo_targets_add" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    jl = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    assert not re.search(r"ccall\(\s*\(?\s*:mpfmt_togo_targets_add", jl)           # (documented in INTEGRATION.md, executed by tests/abi_c)


def test_c_caller_builds_against_the_header_with_the_documented_widths(tmp_path):
    """tests/abi_c/abi_caller15.c calls the option, mpfmt_samples_add and mpfmt_togo_targets_add with the widths INTEGRATION.md gives (a
    differing width fails the build); tests/test_gpu_growfield.py runs it."""
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    src = os.path.join(ROOT, "tests", "abi_c", "abi_caller15.c")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           src, "-o", str(tmp_path / "abi_caller15"), "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    called = set(re.findall(r"\b(mpfmt_[A-Za-z0-9_]+)\b", open(src).read()))
    assert {"mpfmt_togo_targets_add", "mpfmt_samples_add", "mpfmt_set_option", "mpfmt_togo_update"} <= called
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`mpfmt_togo_targets_add` `(Ptr{Void}, Ptr{Int64}, Int64)`" in doc and "abi_caller15.c" in doc
