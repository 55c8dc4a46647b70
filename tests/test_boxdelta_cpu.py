"""CPU tests of what the in-place box edits (mpfmt_boxes_add / mpfmt_boxes_remove, csrc/kernels_boxdelta.hip) rest on, checked on the
oracle and the golden box worlds: the free bit of an edge is a conjunction over the boxes, so the mask for a longer list is the AND of
the masks of its parts, and taking a box out can change only blocked edges whose bounding box meets it.  Also builds the C caller of
the two entry points against the header (tests/test_gpu_boxdelta.py runs it) and ties the Python binding to the header."""
import os
import re
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def world(name, N, seed):
    z = np.load(os.path.join(GOLD, "segments_%s.npz" % name))
    d = z["lohi"].shape[2]
    X = np.random.default_rng(seed).random((N, d)) * 1.1 - 0.05           # a few samples outside the state-space bounds
    colptr, rowval, _ = orc.rdisc_graph(X, 0.25 if d == 2 else 0.4)
    return X, colptr, rowval, z["lohi"], z["ss_lo"], z["ss_hi"]


def bits(mask, n):
    return orc.unpack(mask, n).astype(bool)


@pytest.mark.parametrize("name,N,seed", [("BOXES2D", 300, 1), ("BOXES3D", 300, 2)])
def test_the_mask_of_a_longer_list_is_the_and_of_its_parts(name, N, seed):
    X, colptr, rowval, lohi, lo, hi = world(name, N, seed)
    nnz = len(rowval)
    assert nnz > 1000
    full = bits(orc.graph_edges_free(X, colptr, rowval, lohi, lo, hi), nnz)
    assert full.any() and not full.all()
    for k in range(len(lohi) + 1):
        old = bits(orc.graph_edges_free(X, colptr, rowval, lohi[:k], lo, hi), nnz)
        delta = bits(orc.graph_edges_free(X, colptr, rowval, lohi[k:], None, None), nnz)      # the added boxes ALONE, no bounds
        assert np.array_equal(full, old & delta)
    # any order: the list reversed gives the same bits
    assert np.array_equal(full, bits(orc.graph_edges_free(X, colptr, rowval, lohi[::-1].copy(), lo, hi), nnz))


@pytest.mark.parametrize("name,N,seed", [("BOXES2D", 300, 3), ("BOXES3D", 300, 4)])
def test_removing_a_box_touches_only_blocked_edges_whose_box_meets_it(name, N, seed):
    X, colptr, rowval, lohi, lo, hi = world(name, N, seed)
    nnz = len(rowval)
    col = np.repeat(np.arange(N), np.diff(colptr))
    V, W = X[rowval], X[col]                                                # segment (row state, column state), kernels_sweep.hip
    l, h = np.minimum(V, W), np.maximum(V, W)
    full = bits(orc.graph_edges_free(X, colptr, rowval, lohi, lo, hi), nnz)
    changed_any = False
    for b in range(len(lohi)):
        rest = np.delete(lohi, b, axis=0)
        after = bits(orc.graph_edges_free(X, colptr, rowval, rest, lo, hi), nnz)
        misses = np.any((lohi[b, 1] < l) | (lohi[b, 0] > h), axis=1)        # is_free_motion_broadphase, boxesND.jl:44-45
        assert np.array_equal(after[misses], full[misses])
        assert not (full & ~after).any()                                    # bits are only set
        changed_any |= bool((after & ~full).any())
        # the rule of k_bd_remove, restated: blocked and meeting -> the whole test against the rest; everything else keeps its bit
        again = full.copy()
        sel = ~full & ~misses
        again[sel] = after[sel]
        assert np.array_equal(again, after)
    assert changed_any
    # the rows outside the bounds stay blocked whatever is removed
    outside = ~np.all((lo <= V) & (V <= hi), axis=1)
    assert outside.any()
    assert not bits(orc.graph_edges_free(X, colptr, rowval, lohi[:0], lo, hi), nnz)[outside].any()


def test_c_caller_builds_against_the_header(tmp_path):
    """tests/abi_c/abi_caller5.c carries the widths of the two ccall signatures of INTEGRATION.md; under -Wcast-function-type -Werror
    it builds only while include/mpfmt.h agrees with them."""
    src = os.path.join(ROOT, "tests", "abi_c", "abi_caller5.c")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", str(tmp_path / "abi_caller5.o")])
    text = open(src).read()
    assert "mpfmt_boxes_add" in text and "mpfmt_boxes_remove" in text
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "(:mpfmt_boxes_add, libmpfmt), Int32, (Ptr{Void}, Ptr{Float64}, Int32)" in doc
    assert "(:mpfmt_boxes_remove, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Int32)" in doc


def test_binding_and_header_declare_the_two_calls():
    hdr = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    assert re.search(r"int32_t\s+mpfmt_boxes_add\(mpfmt_ctx\*\s*\w*,\s*const double\*\s*\w+,\s*int32_t\s+\w+\);", hdr)
    assert re.search(r"int32_t\s+mpfmt_boxes_remove\(mpfmt_ctx\*\s*\w*,\s*const int64_t\*\s*\w+,\s*int32_t\s+\w+\);", hdr)
    names = [n for n, _, _ in mp._lib.SYMBOLS]
    assert "mpfmt_boxes_add" in names and "mpfmt_boxes_remove" in names
    assert hasattr(mp.Context, "boxes_add") and hasattr(mp.Context, "boxes_remove")
    for f in ("addobstacle_", "addblocker_", "removeobstacle_"):
        assert callable(getattr(mp, f))


class _Ctx:
    """Stands in for a device context: counts uploads and delta calls (the mirror's bookkeeping needs no GPU)."""

    def __init__(self):
        self._cc_epoch = 0
        self.uploads, self.adds, self.removes = 0, [], []

    def upload_boxes(self, lohi, lo=None, hi=None, dw=None):
        self._cc_epoch += 1
        self.uploads += 1

    def boxes_add(self, lohi):
        self._cc_epoch += 1
        self.adds.append(np.array(lohi))

    def boxes_remove(self, ids):
        self._cc_epoch += 1
        self.removes.append(list(ids))


def test_bind_skips_a_list_the_context_holds_and_the_in_place_forms_keep_it_bound():
    SS = mp.UnitHypercube(2)
    CC = mp.PointRobotNDBoxes([mp.BoxBounds([0.1, 0.1], [0.2, 0.2]), mp.BoxBounds([0.5, 0.5], [0.6, 0.7])])
    ctx = _Ctx()

    class P:
        pass
    P.CC, P.SS, P.ctx = CC, SS, ctx
    CC._bind(ctx, SS)
    CC._bind(ctx, SS)
    assert ctx.uploads == 1                                                 # unchanged list: not uploaded again
    mp.addblocker_(P, [0.8, 0.8], 0.05)
    assert len(CC.boxes) == 3 and len(ctx.adds) == 1 and ctx.adds[0].shape == (1, 2, 2)
    assert np.array_equal(ctx.adds[0][0], [[0.8 - 0.05] * 2, [0.8 + 0.05] * 2])
    CC._bind(ctx, SS)
    assert ctx.uploads == 1                                                 # the context holds the edited list
    mp.removeobstacle_(P, 1)
    assert len(CC.boxes) == 2 and ctx.removes == [[1]] and CC.boxes[0].lo[0] == 0.5
    CC._bind(ctx, SS)
    assert ctx.uploads == 1
    CC.boxes.append(mp.BoxBounds([0.3, 0.3], [0.4, 0.4]))                   # edited behind the mirror's back: uploaded
    CC._bind(ctx, SS)
    assert ctx.uploads == 2
    ctx.upload_boxes(None)                                                  # somebody else changed the context's checker: uploaded again
    CC._bind(ctx, SS)
    assert ctx.uploads == 4
    with pytest.raises(IndexError):
        mp.removeobstacle_(P, 9)
    # an unbound checker is edited on the host only
    CC2 = mp.PointRobotNDBoxes([])
    P.CC = CC2
    mp.addobstacle_(P, mp.BoxBounds([0.0, 0.0], [0.1, 0.1]))
    assert len(CC2.boxes) == 1 and len(ctx.adds) == 1
    # the functional forms are the reference's: a new checker, the old one untouched
    CC3 = CC2.addblocker([0.5, 0.5], 0.1)
    assert len(CC3.boxes) == 2 and len(CC2.boxes) == 1
