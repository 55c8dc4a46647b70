"""CPU tests of k-nearest connections: the default k of fmtstar! (fmt.jl:6) and the forward mask of the directed host recursion
(csrc/mpfmt_host.cpp), driven through a small host-only caller (tests/knn_host/directed_toy.cpp; no device, no library)."""
import os
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_k_table_and_clamp():
    # cfg1, cfg2, north star, cfg3
    assert mp.default_k(1, 2, 1000) == 38
    assert mp.default_k(1, 6, 100_000) == 334
    assert mp.default_k(1, 6, 1_000_000) == 401
    assert mp.default_k(1, 12, 1_000_000) == 12819
    assert mp.default_k(1, 12, 5000) == 4999 and mp.default_k(1, 6, 50) == 49          # clamps to N - 1
    assert mp.default_k(1.5, 2, 1000) == int(np.ceil(9 * (np.e / 2) * np.log(1000)))


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knn_host") / "directed_toy")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "knn_host", "directed_toy.cpp"),
                           os.path.join(ROOT, "motionplanning.jl_amd", "csrc", "mpfmt_host.cpp"), "-o", exe])

    def run(tmp, N, init, goal, colptr, rowval, nzval, efree=None, mask=None):
        nnz = len(rowval)
        efree = np.ones(nnz, int) if efree is None else efree
        p = os.path.join(str(tmp), "g.txt")
        with open(p, "w") as f:
            f.write("%d %d %d %d %d\n" % (N, init, goal, nnz, mask is not None))
            for arr in (colptr, rowval):
                f.write(" ".join(str(int(v)) for v in arr) + "\n")
            f.write(" ".join(repr(float(v)) for v in nzval) + "\n")
            f.write(" ".join(str(int(v)) for v in efree) + "\n")
            if mask is not None:
                f.write(" ".join(str(int(v)) for v in mask) + "\n")
        out = subprocess.run([exe, p], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
        st, checks, plen, cost = out[0].split()
        return dict(status=int(st), checks=int(checks), cost=float(cost), A=[int(v) for v in out[1].split()],
                    C=[float(v) for v in out[2].split()], path=[int(v) for v in out[3].split()])
    return run


def test_null_mask_equals_all_ones_mask(toy, tmp_path):
    rng = np.random.default_rng(3)
    N, deg = 300, 12
    rows = np.stack([np.sort(rng.choice(np.delete(np.arange(N), v), deg, replace=False)) for v in range(N)])
    colptr = np.arange(N + 1) * deg
    nz = rng.random(N * deg) + 0.05
    efree = (rng.random(N * deg) < 0.8).astype(int)
    a = toy(tmp_path, N, 1, N, colptr, rows.reshape(-1), nz, efree)
    b = toy(tmp_path, N, 1, N, colptr, rows.reshape(-1), nz, efree, mask=np.ones(N * deg, int))
    assert a == b and a["status"] == 1 and a["checks"] > N // 2


# Six nodes, init 1, goal 6; column x = the candidate parents of x.  Entries: e0 (1 in col 2), e1 (1 in col 3), e2 (2 in col 4),
# e3 (3 in col 5), e4 (4 in col 5), e5 (5 in col 6).
COLPTR = [0, 0, 1, 2, 3, 5, 6]
ROWVAL = [0, 0, 1, 2, 3, 4]


def test_mask_drops_a_forward_entry_but_not_a_parent(toy, tmp_path):
    """Node 4 (cost 1.5) is popped while node 3 (cost 2) is still open; 3 -> 5 costs 0.1, 4 -> 5 costs 1.  By hand: 1 opens 2 (1.0)
    and 3 (2.0); 2 opens 4 (1.5); 4 examines 5, whose open parents are 3 (2.1) and 4 (2.5): parent 3; then 3, 5 are popped, 5 opens 6
    (3.1).  Dropping the forward entry (3 in column 5) -- 5 is no forward neighbour of 3 -- must not change that: 5 is still examined from
    4, and the open 3 is still its best parent (a mask applied to the parent relaxation would give parent 4, cost 2.5)."""
    nz = [1.0, 2.0, 0.5, 0.1, 1.0, 1.0]
    want = dict(status=1, checks=5, cost=3.1, A=[0, 1, 1, 2, 3, 5], C=[0.0, 1.0, 2.0, 1.5, 2.1, 3.1], path=[1, 3, 5, 6])
    want["cost"] = want["C"][5] = 2.1 + 1.0
    assert toy(tmp_path, 6, 1, 6, COLPTR, ROWVAL, nz) == want
    assert toy(tmp_path, 6, 1, 6, COLPTR, ROWVAL, nz, mask=[1, 1, 1, 0, 1, 1]) == want


def test_mask_changes_who_examines_a_sample(toy, tmp_path):
    """3 -> 5 costs 1, 4 -> 5 costs 0.2.  Unmasked: 4 (1.5) examines 5 with open parents 3 (3.0) and 4 (1.7): parent 4, cost 1.7; 6 costs
    2.7 over the path 1 2 4 5 6.  With the forward entry (4 in column 5) dropped, 4 does not examine 5; 3 (popped at 2.0, 4 closed by
    then) does: parent 3, cost 3.0; 6 costs 4.0 over 1 3 5 6.  Five checks either way."""
    nz = [1.0, 2.0, 0.5, 1.0, 0.2, 1.0]
    free = toy(tmp_path, 6, 1, 6, COLPTR, ROWVAL, nz)
    assert free == dict(status=1, checks=5, cost=1.7 + 1.0, A=[0, 1, 1, 2, 4, 5], C=[0.0, 1.0, 2.0, 1.5, 1.7, 1.7 + 1.0], path=[1, 2, 4, 5, 6])
    masked = toy(tmp_path, 6, 1, 6, COLPTR, ROWVAL, nz, mask=[1, 1, 1, 1, 0, 1])
    assert masked == dict(status=1, checks=5, cost=4.0, A=[0, 1, 1, 2, 3, 5], C=[0.0, 1.0, 2.0, 1.5, 3.0, 4.0], path=[1, 3, 5, 6])


def test_host_recursion_with_mutual_mask_equals_the_restatement(orc, toy, tmp_path):
    """cfg1's k-nearest graph from the numpy brute force, edge bits from the oracle: the C++ recursion with the mutual bits as its
    forward mask builds the tree of the Python restatement of fmt.jl:43-101 (tests/test_gpu_knn.py), checkpts off."""
    import test_gpu_knn as T
    w = mp.workloads.cfg1()
    for k in (38, 8):
        colptr, rowval, nzval, mutual, ties = T.knn_ref(w.X, k)
        assert ties == 0 and 0.5 < mutual.mean() < 0.95
        efree = orc.unpack(orc.graph_edges_free(w.X, colptr, rowval, w.lohi, w.ss_lo, w.ss_hi), len(rowval))
        want = T.fmt_knn_ref(orc, w.X, colptr, rowval, nzval, mutual, efree, None, orc.GOAL_BALL, w.goal_params())
        assert want["status"] == 1
        got = toy(tmp_path, w.N, 1, int(want["path"][-1]), colptr, rowval, nzval, efree, mask=mutual)
        assert got["status"] == 1 and got["checks"] == want["collision_checks"] and got["cost"] == want["cost"]
        assert got["A"] == list(want["A"]) and got["C"] == list(want["C"]) and got["path"] == list(want["path"])
        # ... and the mask matters: without it the tree is another one
        other = toy(tmp_path, w.N, 1, int(want["path"][-1]), colptr, rowval, nzval, efree)
        assert other["A"] != got["A"]
