"""CPU tests of what the in-place shape edits (mpfmt_shapes2d_add / mpfmt_shapes2d_remove, csrc/kernels_shapedelta.hip) rest on.
The free bit of the 2-D shape world is  in_ss(v) && (gate(e, B(L)) || no shape of L hits)  and the gate is not inert in floating point,
so the box rule "old AND free against the added alone" does not carry over: the two rules of DESIGN.md 7o, restated in numpy
(tests/shapedelta_cases.py), are held to the oracle's whole-graph mask for every prefix and deletion of ISRR_POLY and in the tie world,
where the naive rule is shown to fail.  Also: the flagged-column rule covers every changed entry and point bit, the C caller builds
against the header, and binding, header and library agree on the two calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp
from oracle import oracle as orc

import shapedelta_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def graph(X, r=sc.R):
    colptr, rowval, _ = orc.rdisc_graph(X, r)
    col = np.repeat(np.arange(len(X)), np.diff(colptr))
    return colptr, rowval, col, X[rowval], X[col]                           # segment (row state, column state), k2d_graph


def oracle_bits(X, colptr, rowval, shapes):
    m = orc.graph_edges_free_2d(X, colptr, rowval, orc.Shapes2D(shapes), sc.LO, sc.HI)
    return orc.unpack(m, len(rowval)).astype(bool)


def covered(X, col, changed, flags, old_pts, new_pts):
    """Every column with a changed entry, and every sample whose point bit changed, is flagged."""
    cols = np.zeros(len(X), dtype=bool)
    cols[col[changed]] = True
    return not (cols & ~flags).any() and not ((old_pts != new_pts) & ~flags).any()


def test_the_restated_predicate_is_the_oracles():
    X = sc.samples(1)
    colptr, rowval, col, V, W = graph(X)
    assert len(rowval) > 20000
    for shapes in (sc.isrr_poly(), [], sc.TIE_WORLD, sc.isrr_poly() + sc.small_shapes(np.random.default_rng(2), 6)):
        L = [sc.build(s) for s in shapes]
        assert np.array_equal(sc.bit(V, W, L), oracle_bits(X, colptr, rowval, shapes))
        assert np.array_equal(sc.point_bit(X, L), orc.unpack(orc.points_free_2d(X, orc.Shapes2D(shapes), sc.LO, sc.HI), len(X)).astype(bool))
    outside = ~sc.in_ss(V)
    assert outside.any() and not oracle_bits(X, colptr, rowval, [])[outside].any()


def test_both_rules_reproduce_every_prefix_and_deletion_of_isrr_poly():
    X = sc.samples(3)
    colptr, rowval, col, V, W = graph(X)
    shapes = sc.isrr_poly()
    L = [sc.build(s) for s in shapes]
    full = oracle_bits(X, colptr, rowval, shapes)
    assert full.any() and not full.all()
    changed_any = False
    for k in range(len(L) + 1):                                             # add the tail to every prefix, the empty one included
        old = oracle_bits(X, colptr, rowval, shapes[:k])
        new = sc.rule_add(old, V, W, L[:k], L[k:])
        assert np.array_equal(new, full)
        if k < len(L):
            flags = sc.flagged(X, L[k:], L[:k], L, sc.R)
            assert covered(X, col, old != full, flags, sc.point_bit(X, L[:k]), sc.point_bit(X, L))
            one = sc.rule_add(old, V, W, L[:k], L[k:k + 1])                  # and one shape at a time
            assert np.array_equal(one, oracle_bits(X, colptr, rowval, shapes[:k + 1]))
    for ids in ([0], [1], [2], [3], [0, 3], [1, 2], [2, 0, 1], [0, 1, 2, 3]):
        rest = [s for i, s in enumerate(shapes) if i not in ids]
        want = oracle_bits(X, colptr, rowval, rest)
        assert np.array_equal(sc.rule_remove(full, V, W, L, ids), want)
        assert not (full & ~want).any()                                     # bits are only set
        changed_any |= bool((want & ~full).any())
        Lr = [S for i, S in enumerate(L) if i not in ids]
        flags = sc.flagged(X, [L[i] for i in ids], Lr, L, sc.R)
        assert covered(X, col, want != full, flags, sc.point_bit(X, L), sc.point_bit(X, Lr))
        assert flags.sum() < len(X) or sc.compound_box(Lr) != sc.compound_box(L)
    assert changed_any


def test_the_tie_world_flips_the_bit_the_naive_rule_keeps():
    cx, r, px = sc.TIE_C[0], sc.TIE_R, sc.TIE_P[0]
    assert px < cx - r and px - cx == -r                                    # outside the circle's own box, and still "inside" the circle
    X = sc.samples(4, first=(sc.TIE_P, sc.TIE_Q))
    colptr, rowval, col, V, W = graph(X)
    e = np.flatnonzero((col == 0) & (rowval == 1))                           # row q in column p
    assert len(e) == 1
    e = int(e[0])
    L, thin = [sc.build(s) for s in sc.TIE_WORLD], [sc.build(sc.THIN)]
    assert sc.line_hits(V[e:e + 1], W[e:e + 1], L[0])[0]                     # the circle "hits" the segment (q, p) ...
    assert sc.gate(V[e:e + 1], W[e:e + 1], L)[0]                             # ... which the gate calls free
    before = oracle_bits(X, colptr, rowval, sc.TIE_WORLD)
    after = oracle_bits(X, colptr, rowval, sc.TIE_WORLD + [sc.THIN])
    assert before[e] and not after[e]
    assert np.linalg.norm(X[:2] - np.array([-0.1, 0.05]), axis=1).min() > 10 * sc.R      # the thin polygon is nowhere near
    assert np.array_equal(sc.rule_add(before, V, W, L, thin), after)
    naive = sc.naive_add(before, V, W, thin)
    assert naive[e] and not np.array_equal(naive, after)                    # the box rule gets it wrong
    again = sc.rule_remove(after, V, W, L + thin, [2])
    assert again[e] and np.array_equal(again, before)
    # rule (a) alone misses column p; rule (b) visits it
    rpad = sc.R * (1.0 + 1e-9) + 1e-300
    assert X[0, 0] > thin[0]["xr"][1] + rpad
    for small, big, delta in ((L, L + thin, thin),):
        flags = sc.flagged(X, delta, small, big, sc.R)
        assert flags[0] and flags[1]
        assert covered(X, col, before != after, flags, sc.point_bit(X, small), sc.point_bit(X, big))


def test_random_edit_sequences_follow_the_oracle():
    rng = np.random.default_rng(5)
    X = sc.samples(6, n=800)
    colptr, rowval, col, V, W = graph(X, 0.1)
    shapes = sc.isrr_poly()
    cur = oracle_bits(X, colptr, rowval, shapes)
    far = [("circle", (1.6, 1.7), 0.05), sc.THIN]                            # shapes that move the compound box
    for step in range(8):
        L = [sc.build(s) for s in shapes]
        if step % 2 == 0:
            add = sc.small_shapes(rng, 1 + step, 0.1, 0.9) + ([far[(step // 2) % 2]] if step % 4 == 0 else [])
            new = sc.rule_add(cur, V, W, L, [sc.build(s) for s in add])
            flags = sc.flagged(X, [sc.build(s) for s in add], L, L + [sc.build(s) for s in add], 0.1)
            shapes = shapes + add
        else:
            ids = sorted(rng.choice(len(shapes), size=min(3, len(shapes)), replace=False).tolist())
            new = sc.rule_remove(cur, V, W, L, ids)
            Lr = [S for i, S in enumerate(L) if i not in ids]
            flags = sc.flagged(X, [L[i] for i in ids], Lr, L, 0.1)
            shapes = [s for i, s in enumerate(shapes) if i not in ids]
        want = oracle_bits(X, colptr, rowval, shapes)
        assert np.array_equal(new, want), step
        cols = np.zeros(len(X), dtype=bool)
        cols[col[cur != want]] = True
        assert not (cols & ~flags).any(), step
        cur = want


def test_c_caller_builds_against_the_header(tmp_path):
    """tests/abi_c/abi_caller13.c carries the widths of the two ccall signatures of julia/MPFmtHIP.jl and INTEGRATION.md; under
    -Wcast-function-type -Werror it builds only while include/mpfmt.h agrees with them."""
    src = os.path.join(ROOT, "tests", "abi_c", "abi_caller13.c")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", str(tmp_path / "abi_caller13.o")])
    text = open(src).read()
    assert "mpfmt_shapes2d_add" in text and "mpfmt_shapes2d_remove" in text
    add = "Int32, (Ptr{Void}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64})"
    rem = "Int32, (Ptr{Void}, Ptr{Int64}, Int32)"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "(:mpfmt_shapes2d_add, libmpfmt), " + add in doc and "(:mpfmt_shapes2d_remove, libmpfmt), " + rem in doc
    jl = re.sub(r"\s+", " ", open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read())
    assert "const sym_shapes2d_add = :mpfmt_shapes2d_add" in jl and "const sym_shapes2d_remove = :mpfmt_shapes2d_remove" in jl
    assert "ccall((sym_shapes2d_add, libmpfmt), " + add in jl and "ccall((sym_shapes2d_remove, libmpfmt), " + rem in jl


def test_binding_header_and_library_declare_the_two_calls():
    hdr = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    assert re.search(r"int32_t\s+mpfmt_shapes2d_add\(mpfmt_ctx\*\s*\w*,\s*int32_t\s+\w+,\s*const int32_t\*\s*\w+,\s*const int32_t\*\s*\w+,"
                     r"\s*const double\*\s*\w+\);", hdr)
    assert re.search(r"int32_t\s+mpfmt_shapes2d_remove\(mpfmt_ctx\*\s*\w*,\s*const int64_t\*\s*\w+,\s*int32_t\s+\w+\);", hdr)
    C = ctypes
    i32p, f64p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    table = {n: (res, args) for n, res, args in mp._lib.SYMBOLS}
    assert table["mpfmt_shapes2d_add"] == (C.c_int32, [C.c_void_p, C.c_int32, i32p, i32p, f64p])
    assert table["mpfmt_shapes2d_remove"] == (C.c_int32, [C.c_void_p, i64p, C.c_int32])
    lib = ctypes.CDLL(mp._lib.so_path())
    assert hasattr(lib, "mpfmt_shapes2d_add") and hasattr(lib, "mpfmt_shapes2d_remove")
    assert hasattr(mp.Context, "shapes_add") and hasattr(mp.Context, "shapes_remove")


class _Ctx:
    """Stands in for a device context: counts uploads and delta calls (the mirror's bookkeeping needs no GPU)."""

    def __init__(self):
        self._cc_epoch = 0
        self.uploads, self.adds, self.removes = 0, [], []

    def upload_shapes2d(self, shapes, lo=None, hi=None):
        self._cc_epoch += 1
        self.uploads += 1

    def shapes_add(self, shapes):
        self._cc_epoch += 1
        self.adds.append(list(shapes))

    def shapes_remove(self, ids):
        self._cc_epoch += 1
        self.removes.append(list(ids))


def test_bind_skips_a_list_the_context_holds_and_the_in_place_forms_keep_it_bound():
    SS = mp.UnitHypercube(2)
    CC = mp.PointRobot2D(mp.Compound2D(mp.Circle((0.5, 0.5), 0.1), mp.Compound2D(mp.Box2D((0.1, 0.2), (0.1, 0.2)), mp.Circle((0.8, 0.2), 0.05))))
    ctx = _Ctx()

    class P:
        pass
    P.CC, P.SS, P.ctx = CC, SS, ctx
    CC._bind(ctx, SS)
    CC._bind(ctx, SS)
    assert ctx.uploads == 1                                                 # unchanged list: not uploaded again
    mp.addblocker_(P, [0.8, 0.8], 0.05)
    assert ctx.adds == [[("circle", (0.8, 0.8), 0.05)]] and len(CC.obstacles.parts()) == 4
    mp.addobstacle_(P, mp.Compound2D(mp.Circle((0.3, 0.3), 0.02), mp.Polygon([(0.6, 0.6), (0.7, 0.6), (0.65, 0.7)])))
    assert len(ctx.adds[1]) == 2 and ctx.adds[1][1][0] == "polygon" and len(CC.obstacles.parts()) == 6
    CC._bind(ctx, SS)
    assert ctx.uploads == 1                                                 # the context holds the edited list
    mp.removeobstacle_(P, 2)                                                # the flattened list: the box inside the nested compound
    assert ctx.removes == [[2]] and [q[0] for q in CC.obstacles.parts()] == ["circle", "circle", "circle", "circle", "polygon"]
    assert CC.obstacles.parts()[1] == ("circle", (0.8, 0.2), 0.05)
    CC._bind(ctx, SS)
    assert ctx.uploads == 1
    CC.obstacles = mp.Compound2D(CC.obstacles, mp.Circle((0.4, 0.4), 0.01))   # edited behind the mirror's back: uploaded
    CC._bind(ctx, SS)
    assert ctx.uploads == 2
    ctx.upload_shapes2d([])                                                 # somebody else changed the context's checker: uploaded again
    CC._bind(ctx, SS)
    assert ctx.uploads == 4
    with pytest.raises(IndexError):
        mp.removeobstacle_(P, 9)
    with pytest.raises(TypeError):
        mp.addobstacle_(P, mp.BoxBounds([0.0, 0.0], [0.1, 0.1]))
    # an unbound checker is edited on the host only
    P.CC = mp.PointRobot2D(mp.Compound2D())
    mp.addblocker_(P, (0.5, 0.5), 0.1)
    assert len(P.CC.obstacles.parts()) == 1 and len(ctx.adds) == 2
    # the functional forms are the reference's: a new checker, the old one untouched
    CC3 = P.CC.addblocker((0.2, 0.2), 0.1)
    assert len(CC3.obstacles.parts()) == 2 and len(P.CC.obstacles.parts()) == 1
