"""CPU tests of the roadmap queries for states that are not samples (include/mpfmt.h, "roadmap queries for external states"):
mpfmt_host_roadmap_query -- through the library's export and through a host-only caller built with the sanitizers
(tests/roadmap_host/roadmap_toy.cpp; no device) -- against the pure-Python reference of tests/roadmap_cases.py.  Cost and path are
compared bit for bit: no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roadmap_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_KEYS = ("status", "near_s", "usable_s", "near_g", "usable_g", "path_len")


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("roadmap_host")
    exe = str(d / "roadmap_toy")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "roadmap_host", "roadmap_toy.cpp"),
                           os.path.join(ROOT, "motionplanning.jl_amd", "csrc", "mpfmt_host.cpp"), "-o", exe])

    def run(X, colptr, rowval, nzval, efree, F, lohi, lo, hi, r, S, G):
        N, dd = X.shape
        nnz, nq = len(rowval), len(S)
        pin, pout = str(d / "in.bin"), str(d / "out.bin")
        with open(pin, "wb") as f:
            f.write(np.array([N, dd, nnz, len(lohi), F is not None, 1, nq], dtype=np.int64).tobytes())
            f.write(np.array([r], np.float64).tobytes()); f.write(X.tobytes())
            f.write(np.asarray(colptr, np.int64).tobytes()); f.write(np.asarray(rowval, np.int32).tobytes())
            f.write(np.asarray(nzval, np.float64).tobytes()); f.write(np.asarray(efree, np.uint64)[:mp._lib.nwords(nnz)].tobytes())
            if F is not None:
                f.write(np.asarray(F, np.uint64)[:mp._lib.nwords(N)].tobytes())
            f.write(np.ascontiguousarray(lohi).tobytes()); f.write(lo.tobytes()); f.write(hi.tobytes())
            f.write(np.ascontiguousarray(S).tobytes()); f.write(np.ascontiguousarray(G).tobytes())
        p = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "ERROR" not in p.stderr, p.stdout + p.stderr
        buf = open(pout, "rb").read()
        isz = mp._lib.C.sizeof(mp._lib.RoadmapInfo)
        out, off = [], 0
        for _ in range(nq):
            assert np.frombuffer(buf, np.int32, 1, off)[0] == 0
            cost = float(np.frombuffer(buf, np.float64, 1, off + 4)[0])
            info = mp._lib.RoadmapInfo.from_buffer_copy(buf[off + 12:off + 12 + isz])
            off += 12 + isz
            path = np.frombuffer(buf, np.int64, info.path_len, off).copy()
            off += 8 * info.path_len
            out.append((cost, path, mp._lib._roadmap_info(info)))
        assert off == len(buf)
        return out
    return run


def bits(x):
    return np.float64(x).tobytes()


@pytest.mark.parametrize("d,N,r,nboxes", [(2, 300, 0.12, 6), (3, 500, 0.2, 8), (6, 500, 0.62, 8)])
def test_host_query_equals_the_python_reference(orc, toy, d, N, r, nboxes):
    sc = rc.Scene(d, N, r, nboxes, seed=11 + d)
    X, lohi, lo, hi = sc.X, sc.lohi, sc.lo, sc.hi
    colptr, rowval, nzval = orc.rdisc_graph(X, r)
    efree = orc.graph_edges_free(X, colptr, rowval, lohi, lo, hi)
    F = orc.points_free(X, lohi, lo, hi)
    eb, Fb = mp._lib.unpack_bits(efree, len(rowval)), mp._lib.unpack_bits(F, N)
    assert not Fb[N - 1] and not eb.all()
    qs = sc.queries(orc)
    S = np.array([q[1] for q in qs]); G = np.array([q[2] for q in qs])
    seen = set()
    for Fm, Fbits in ((F, Fb), (None, None)):
        toyres = toy(X, colptr, rowval.astype(np.int32), nzval, efree, Fm, lohi, lo, hi, r, S, G)
        for i, (name, s, g) in enumerate(qs):
            ref = rc.query_ref(orc, X, colptr, rowval, nzval, eb, Fbits, lohi, lo, hi, r, s, g)
            want_cost, want_path, want_info = ref[0], ref[1], ref[2]
            cost, path, info = mp._lib.host_roadmap_query(X, colptr, rowval, nzval, efree, Fm, lohi, lo, hi, r, s, g)
            assert bits(cost) == bits(want_cost), (name, cost, want_cost)
            assert list(path) == want_path, name
            assert {k: info[k] for k in INFO_KEYS} == want_info, (name, info, want_info)
            tc, tp, ti = toyres[i]
            assert bits(tc) == bits(cost) and list(tp) == list(path) and ti == info, name
            seen.add((name, info["status"], info["path_len"] == 0))
            if name == "start on a sample":
                assert info["status"] == 0 and info["near_s"] >= 1
                k = list(rc.near_ref(X, s, r)[0])
                v = next(y for y in k if np.array_equal(X[y], s))
                assert sorted(set(k) - {v}) == list(rowval[colptr[v]:colptr[v + 1]])        # column v plus v itself
            if name == "direct edge free":
                assert info["status"] == 0 and info["path_len"] == 0 and bits(cost) == bits(np.sqrt(rc.fold_d2(s, g)))
            if name == "direct edge blocked by the wall":
                assert rc.fold_d2(s, g) <= r * r and (info["status"] == 1 or info["path_len"] >= 1)
            if name == "goal far from every sample":
                assert info["status"] == 1 and info["near_g"] == 0 and cost == rc.INF
            if name == "start inside a box":
                assert info["status"] == 2 and cost == rc.INF and len(path) == 0
            if name == "goal outside the bounds":
                assert info["status"] == 3 and cost == rc.INF and len(path) == 0
            if name == "the only seed has F = 0":
                assert info["near_s"] == 1 and info["usable_s"] == (0 if Fm is not None else 1) and info["status"] == 1
    assert sum(1 for n, st, _ in seen if st == 0) >= 6


def test_host_roadmap_query_rejects_bad_arguments():
    X = np.array([[0.0, 0.0], [1.0, 0.0]]); cp = np.array([0, 1, 2], np.int64); rv = np.array([1, 0], np.int32); nz = np.array([1.0, 1.0])
    m = np.array([3], np.uint64); lohi = np.zeros((0, 2, 2))
    cost, path, info = mp._lib.host_roadmap_query(X, cp, rv, nz, m, None, lohi, None, None, 1.0, [0.0, 0.5], [1.0, 0.5])
    assert info["status"] == 0 and cost == 1.0 and len(path) == 0                           # the direct edge wins the tie of three routes
    cost, path, info = mp._lib.host_roadmap_query(X, cp, rv, nz, m, None, lohi, None, None, 0.6, [0.0, 0.5], [1.0, 0.5])
    assert info["status"] == 0 and list(path) == [1, 2] and cost == 0.5 + 1.0 + 0.5
    with pytest.raises(mp.MPFMTError):
        mp._lib.host_roadmap_query(X, cp, rv, nz, m, None, lohi, None, None, 1.0, [np.nan, 0.5], [1.0, 0.5])
    with pytest.raises(mp.MPFMTError):
        mp._lib.host_roadmap_query(X, np.array([1, 2, 3], np.int64), rv, nz, m, None, lohi, None, None, 1.0, [0.0, 0.5], [1.0, 0.5])
    with pytest.raises(mp.MPFMTError):
        mp._lib.host_roadmap_query(X, cp, rv, nz, m, None, lohi, None, None, -1.0, [0.0, 0.5], [1.0, 0.5])


def test_host_roadmap_query_rejects_null_arrays():
    Lb = mp._lib
    X = np.array([[0.0, 0.0], [1.0, 0.0]]); cp = np.array([0, 1, 2], np.int64); rv = np.array([1, 0], np.int32); nz = np.array([1.0, 1.0])
    m = np.array([3], np.uint64); s = np.array([0.0, 0.5]); g = np.array([1.0, 0.5]); path = np.zeros(4, np.int64)
    cost = Lb.C.c_double(0.0); info = Lb.RoadmapInfo()
    i32 = Lb.C.POINTER(Lb.C.c_int32)
    good = [2, 2, Lb._dp(X), Lb._ip(cp), rv.ctypes.data_as(i32), Lb._dp(nz), Lb._up(m), None, None, 0, None, None, 1.0, Lb._dp(s), Lb._dp(g),
            Lb.C.byref(cost), Lb._ip(path), 4, Lb.C.byref(info)]
    assert Lb.lib().mpfmt_host_roadmap_query(*good) == 0 and info.status == 0
    for k in (2, 3, 4, 5, 6, 13, 14, 15, 16, 18):                             # X, colptr, rowval, nzval, efree, s, g, cost, path, info
        bad = list(good)
        bad[k] = None
        assert Lb.lib().mpfmt_host_roadmap_query(*bad) == Lb.ERR_ARG, k
    bad = list(good); bad[9] = 1                                              # M > 0 without lohi
    assert Lb.lib().mpfmt_host_roadmap_query(*bad) == Lb.ERR_ARG
    bad = list(good); bad[10] = Lb._dp(s)                                     # one state bound without the other
    assert Lb.lib().mpfmt_host_roadmap_query(*bad) == Lb.ERR_ARG


def test_python_surface_exists():
    for name in ("roadmap_near", "roadmap_attach", "roadmap_query"):
        assert callable(getattr(mp.Context, name))
    assert callable(mp.roadmap_query_) and callable(mp._lib.host_roadmap_query)
