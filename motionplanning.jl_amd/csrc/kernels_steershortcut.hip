// Shortcutting of a batch of solution paths in the steering spaces on gfx950 (include/mpfmt.h, "steering shortcut"): the double
// integrator, the Dubins and the Reeds-Shepp car.  Two entry points share one pair function per space:
//   pair(v, w) = (cost, dur, bit, nseg): the space's exact steer (di_steer_core.h, car_motion.h) and the waypoint motion test of the
//                space's graph sweep (di_motion_free, car_motion_free), unchanged.
//   k_ssc_pairs      : lane = pair of the caller's list (mpfmt_steer_motions_free).
//   k_steer_shortcut : one wavefront per path, 4 paths per workgroup, no host round trip between passes, shaped like k_shortcut
//                      (kernels_shortcut.hip).  The procedure is a pure function of the pair results, so what the wavefront evaluates
//                      speculatively never shows in a result:
//     shortcut : the split tree of a path of n states depends on n alone; ALL inner nodes are steered and tested, one per lane in strips
//                of 64, against the cum fold of the pass (one lane: the fold is sequential by definition, n additions beside n steers).  A
//                node was ASKED iff every ancestor is blocked; the kept states are the two ends and the split states of the asked, blocked
//                nodes; the leg that leaves a kept state is the old leg when the next state is kept too, else the asked, accepted node
//                that starts there (legnode).  States, leg costs, leg durations and origins are compacted in place.
//     refine   : one lane per leg: the state at fl(T / 2) through the control steps of discretize_core.h, the two re-steered halves, the
//                acceptance; the expanded path goes to the second buffer through a ballot prefix, so the first buffer still holds the
//                path the iteration began with (the TRUNCATED result, and what early termination compares against).
// Layout: the obstacle boxes are staged in LDS once per workgroup when they fit (else read from HBM through the same generic pointer);
// the two working paths, the tree and the flags live in a per-path slab of HBM that only one wavefront touches, whose vector memory
// operations execute in program order (SSC_FENCE keeps the compiler from reordering them).
// Loops: every loop is bounded by a path length (<= max_states), by the node count (<= max_states), by `iterations`, or is the Newton
// search of di_steer, unchanged; a fixed point of shortcut strictly shortens the path until it stops.
#include "mpfmt_internal.h"
#include <algorithm>
#include <cmath>
#include <vector>
#include "discretize_core.h"
#include "di_motion.h"
#include "car_motion.h"

#define SSC_WAVES 4
#define SSC_THREADS (SSC_WAVES * 64)
#define SSC_LDS_BYTES (60 * 1024)
#define SSC_INTS 9                       // int32 arrays of max_states entries per path (see ssc_slab)
#define SSC_SLACK (1.0 + 0x1p-30)        // exact in binary64

#define SSC_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// the checker as the sweeps bind it, and the steer's parameters
struct ssc_env {
    const double* bx; int nbox;          // double integrator: the box list (LDS or HBM), 0 boxes under the shape world
    mpfmt_ws2d cc;
    mpfmt_ss ss;
    double prm[2];                       // {rho, tmax} or {turn_radius, speed}
};
static_assert(sizeof(ssc_env) % 16 == 0, "the workgroup's copy precedes the dynamic LDS region: it must not shift that region's 16-byte base");

// ---- one policy per space ---------------------------------------------------------------------------------------------------------------
template <int M>
struct ssc_di {
    static constexpr int d = 2 * M, wdim = M;
    using disc = disc_di<M>;
    static __device__ __forceinline__ bool pair(const ssc_env& E, const mpfmt_ws2d& cc, const double (&v)[2 * M], const double (&w)[2 * M],
                                                double& cost, double& dur, int& nseg)
    {
        di_steer<M>(v, w, E.prm[0], E.prm[1], cost, dur);
        return di_motion_free<M>(v, w, dur, E.bx, cc.kind == 0 ? E.nbox : 0, E.ss, cc, nseg);
    }
};
template <int KIND>
struct ssc_car {
    static constexpr int d = 3, wdim = 2;
    using disc = disc_car<KIND>;
    static __device__ __forceinline__ bool pair(const ssc_env& E, const mpfmt_ws2d& cc, const double (&v)[3], const double (&w)[3], double& cost,
                                                double& dur, int& nseg)
    {
        car_step path[5];
        int L;
        cost = car_steer<KIND>(v, w, E.prm[0], E.prm[1], path, L);
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 5; ++q) if (q < L) t = t + path[q].t;
        dur = t;
        return car_motion_free<KIND>(v, w, E.prm[0], E.prm[1], cc, E.ss, &nseg);
    }
};

// the state at fl(tf / 2) of the pair's control steps, as mpfmt_discretize samples it (k_disc_chain / k_disc_sample with 3 samples):
// tf the left-to-right fold of the durations, the step the first one with t < T0_j+1 (else the last), then S_j, the full or the partial
// propagate
template <class SP>
__device__ __forceinline__ void ssc_mid(const double* v, const double* w, const double* prm, double* out)
{
    constexpr int d = SP::d, nc = SP::nc, maxs = SP::maxs;
    double t[maxs], c[maxs * nc];
    const int L = SP::steer(v, w, prm, t, c);
    double tf = 0.0;
#pragma unroll
    for (int s = 0; s < maxs; ++s) if (s < L) tf = tf + t[s];
    const double tm = 0.5 * tf;
    double S[d], nv[d];
#pragma unroll
    for (int i = 0; i < d; ++i) { S[i] = v[i]; out[i] = v[i]; }
    double t0 = 0.0;
    bool found = false;
#pragma unroll
    for (int s = 0; s < maxs; ++s) {
        if (s < L && !found) {
            const double t1 = t0 + t[s];
            SP::full(S, v, w, t[s], &c[s * nc], nv);
            if (tm < t1 || s == L - 1) {
                const double sl = tm - t0;
                if (sl <= 0) {
#pragma unroll
                    for (int i = 0; i < d; ++i) out[i] = S[i];
                } else if (sl >= t[s]) {
#pragma unroll
                    for (int i = 0; i < d; ++i) out[i] = nv[i];
                } else {
                    SP::part(S, v, w, t[s], &c[s * nc], sl, out);
                }
                found = true;
            } else {
#pragma unroll
                for (int i = 0; i < d; ++i) S[i] = nv[i];
                t0 = t1;
            }
        }
    }
}

template <int D>
__device__ __forceinline__ void ssc_load(const double* p, int64_t i, double (&v)[D])
{
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = p[i * D + c];
}
template <int D>
__device__ __forceinline__ void ssc_store(double* p, int64_t i, const double (&v)[D])
{
#pragma unroll
    for (int c = 0; c < D; ++c) p[i * D + c] = v[c];
}
__device__ __forceinline__ int ssc_popc(unsigned long long m) { return __popcll(m); }
__device__ __forceinline__ long long ssc_wave_sum(long long v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }

// the boxes of a workgroup: LDS when staged
template <class SP, int CK>
__device__ __forceinline__ void ssc_bind(ssc_env& E, const double* boxes, int32_t M, const mpfmt_shape2d* shapes, const mpfmt_aabb2d& aabb,
                                         const mpfmt_ss& ss, const double* prm)
{
    E.bx = boxes; E.nbox = CK == 0 ? M : 0;
    E.cc.kind = CK; E.cc.boxes = boxes; E.cc.M = CK == 0 ? M : 0;
    E.cc.shapes = shapes; E.cc.ns = CK == 1 ? M : 0; E.cc.aabb = aabb;
    E.ss = ss; E.prm[0] = prm[0]; E.prm[1] = prm[1];
}

// The pair function is the heavy part of every lane (the Reeds-Shepp steer runs 46 word evaluations, and the motion test steers again):
// it is ONE outlined function per instantiation, called from the input legs, the node strips and both halves of refine, so the
// kernel holds one copy of it and its registers are not live across the bookkeeping around the calls.  The environment is the
// workgroup's copy in LDS; the states travel by value.
template <int D> struct ssc_vec { double x[D]; };
struct ssc_res { double cost, dur; int32_t nseg, fr; };
template <class SP, int CK>
__device__ __attribute__((noinline)) ssc_res ssc_pair(const ssc_env* Ep, const ssc_vec<SP::d> v, const ssc_vec<SP::d> w)
{
    mpfmt_ws2d cc = Ep->cc;
    cc.kind = CK;                                                        // a constant again on this side of the call
    ssc_res r;
    int ns = 0;
    r.fr = SP::pair(*Ep, cc, v.x, w.x, r.cost, r.dur, ns) ? 1 : 0;
    r.nseg = ns;
    return r;
}
// refine's mid state, outlined like the pair function.  This noinline carries CORRECTNESS, not only registers: with ssc_mid inlined in
// k_steer_shortcut the Dubins instantiation decided refine wrongly and not repeatably on the device (cause unknown, the
// scratch accounting is ruled out).  Do not inline it without running tests/test_gpu_steershortcut.py on the device.
template <class SP>
__device__ __attribute__((noinline)) ssc_vec<SP::d> ssc_mid_call(const ssc_vec<SP::d> v, const ssc_vec<SP::d> w, const double p0, const double p1)
{
    const double prm[2] = {p0, p1};
    ssc_vec<SP::d> m;
    ssc_mid<typename SP::disc>(v.x, w.x, prm, m.x);
    return m;
}
template <int D>
__device__ __forceinline__ ssc_vec<D> ssc_loadv(const double* p, int64_t i)
{
    ssc_vec<D> v;
#pragma unroll
    for (int c = 0; c < D; ++c) v.x[c] = p[i * D + c];
    return v;
}

// ---- the pair primitive -------------------------------------------------------------------------------------------------------------------
struct ssp_args {
    const double *P, *Q;                 // [n][d]
    int64_t n;
    double* cost; double* dur; int32_t* nseg; unsigned long long* mask;      // cost / dur / nseg may be null
    const double* boxes; int32_t M; int32_t boxes_in_lds;
    const mpfmt_shape2d* shapes; mpfmt_aabb2d aabb;
    mpfmt_ss ss;
    double prm[2];
};

template <class SP, int CK>
__global__ __launch_bounds__(SSC_THREADS) void k_ssc_pairs(ssp_args a)
{
    constexpr int D = SP::d;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ ssc_env sE;
    double* sbox = (double*)smem;
    if (CK == 0 && a.boxes_in_lds) {
        const int nd = a.M * 2 * SP::wdim;
        for (int t = threadIdx.x; t < nd; t += SSC_THREADS) sbox[t] = a.boxes[t];
    }
    if (threadIdx.x == 0) ssc_bind<SP, CK>(sE, (CK == 0 && a.boxes_in_lds) ? (const double*)sbox : a.boxes, a.M, a.shapes, a.aabb, a.ss, a.prm);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool fr = false;
    if (e < a.n) {
        const ssc_res r = ssc_pair<SP, CK>(&sE, ssc_loadv<D>(a.P, e), ssc_loadv<D>(a.Q, e));
        fr = r.fr != 0;
        if (a.cost) a.cost[e] = r.cost;
        if (a.dur) a.dur[e] = r.dur;
        if (a.nseg) a.nseg[e] = r.nseg;
    }
    const unsigned long long bits = __ballot(fr);
    if (lane == 0 && (e - lane) < a.n) a.mask[(e - lane) >> 6] = bits;
}

// ---- the procedure ------------------------------------------------------------------------------------------------------------------------
struct ssc_args {
    const double* P;                     // [sum n][d] the batch
    const int64_t* off;                  // [B + 1]
    int64_t b0, nb;                      // paths [b0, b0 + nb) run in this launch
    int32_t iterations, ms;
    double* dbl;                         // [nb][(2 d + 7) ms]
    int32_t* ints;                       // [nb][SSC_INTS][ms]
    const double* boxes; int32_t M; int32_t boxes_in_lds;
    const mpfmt_shape2d* shapes; mpfmt_aabb2d aabb;
    mpfmt_ss ss;
    double prm[2];
    mpfmt_steer_shortcut_info* info;     // [B]
};

// one working path: states [ms][d], the cost and the duration of the leg that leaves each state, the 1-based input index (0: inserted)
struct ssc_buf { double* p; double* c; double* t; int32_t* org; };

struct ssc_slab {
    double *cum, *ncost, *ndur;          // the fold of the pass; per node: the steer's cost and duration
    int32_t *nlo, *nhi, *npar, *nflag, *nnseg;      // split tree: inner node i tests (nlo, nhi); parent; 1 = accepted; segment tests counted
    int32_t *keep, *legnode;             // per state of the working path: kept; the asked, accepted node that starts here (-1: none)
};

__host__ __device__ __forceinline__ size_t ssc_dbl_per_path(int d, int64_t ms) { return (size_t)(2 * d + 7) * (size_t)ms; }

// the split tree of a path of n >= 3 states (n - 2 inner nodes), breadth first: the tree of sc_build_tree (kernels_shortcut.hip)
__device__ __forceinline__ int ssc_build_tree(const ssc_slab& S, int n, int ms, int lane)
{
    const unsigned long long ltm = (1ull << lane) - 1ull;
    if (lane == 0) { S.nlo[0] = 0; S.nhi[0] = n - 1; S.npar[0] = -1; }
    SSC_FENCE();
    int ls = 0, le = 1;
    while (ls < le) {
        int tail = le;
        for (int base = ls; base < le; base += 64) {
            const int i = base + lane;
            const bool act = i < le;
            const int lo = act ? S.nlo[i] : 0, hi = act ? S.nhi[i] : 0;
            const int split = lo + (hi - lo + 2) / 2 - 1;               // ceil(len / 2), len = hi - lo + 1
            const bool L = act && (split - lo >= 2), R = act && (hi - split >= 2);
            const unsigned long long mL = __ballot(L), mR = __ballot(R);
            const int pos = tail + ssc_popc(mL & ltm) + ssc_popc(mR & ltm);
            if (L && pos < ms) { S.nlo[pos] = lo; S.nhi[pos] = split; S.npar[pos] = i; }
            const int p2 = pos + (L ? 1 : 0);
            if (R && p2 < ms) { S.nlo[p2] = split; S.nhi[p2] = hi; S.npar[p2] = i; }
            tail += ssc_popc(mL) + ssc_popc(mR);
        }
        SSC_FENCE();
        ls = le; le = min(tail, ms);
    }
    return le;
}

// cum_1 = 0, cum_i+1 = fl(cum_i + c_i) on one lane; returns cum_n to every lane
__device__ __forceinline__ double ssc_fold(const ssc_slab& S, const double* c, int n, int lane)
{
    double a = 0.0;
    if (lane == 0) {
        S.cum[0] = 0.0;
        for (int i = 0; i + 1 < n; ++i) { a = a + c[i]; S.cum[i + 1] = a; }
    }
    SSC_FENCE();
    return __shfl(a, 0);
}

// one shortcut(path) in place; returns the new length
template <class SP, int CK>
__device__ __forceinline__ int ssc_shortcut_pass(const ssc_env* E, const ssc_slab& S, const ssc_buf& W, int n, int nn, int lane, long long& checks,
                                                 long long& tests)
{
    constexpr int D = SP::d;
    const unsigned long long ltm = (1ull << lane) - 1ull;
    ssc_fold(S, W.c, n, lane);
    for (int base = 0; base < nn; base += 64) {                          // every inner node, speculatively
        const int i = base + lane;
        const bool act = i < nn;
        if (act) {
            const int lo = S.nlo[i], hi = S.nhi[i];
            const ssc_res r = ssc_pair<SP, CK>(E, ssc_loadv<D>(W.p, lo), ssc_loadv<D>(W.p, hi));
            const double span = S.cum[hi] - S.cum[lo];
            const double thr = SSC_SLACK * span;
            S.nflag[i] = (r.fr && r.cost <= thr) ? 1 : 0;
            S.nnseg[i] = r.nseg; S.ncost[i] = r.cost; S.ndur[i] = r.dur;
        }
        tests += ssc_popc(__ballot(act));
    }
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        if (j < n) { S.keep[j] = (j == 0 || j == n - 1) ? 1 : 0; S.legnode[j] = -1; }
    }
    SSC_FENCE();
    long long cs = 0;
    for (int base = 0; base < nn; base += 64) {                          // asked = every ancestor blocked
        const int i = base + lane;
        if (i < nn) {
            bool asked = true;
            int p = S.npar[i];
            for (int hop = 0; hop < nn && p >= 0 && asked; ++hop) { asked = !(S.nflag[p] & 1); p = S.npar[p]; }
            if (asked) {
                const int lo = S.nlo[i], hi = S.nhi[i];
                cs += S.nnseg[i];
                if (S.nflag[i] & 1) S.legnode[lo] = i;
                else S.keep[lo + (hi - lo + 2) / 2 - 1] = 1;
            }
        }
    }
    checks += ssc_wave_sum(cs);
    SSC_FENCE();
    int nnew = 0;
    for (int base = 0; base < n; base += 64) {                           // compaction in place: a state moves to a position <= its own
        const int j = base + lane;
        const bool k = j < n && S.keep[j] != 0;
        double v[D], cj = 0.0, tj = 0.0;
        int og = 0;
        ssc_load<D>(W.p, k ? j : 0, v);
        if (k) {
            og = W.org[j];
            const int ln = S.legnode[j];
            if (j < n - 1) { cj = ln >= 0 ? S.ncost[ln] : W.c[j]; tj = ln >= 0 ? S.ndur[ln] : W.t[j]; }
        }
        const unsigned long long m = __ballot(k);
        const int pos = nnew + ssc_popc(m & ltm);
        SSC_FENCE();
        if (k) { ssc_store<D>(W.p, pos, v); W.c[pos] = cj; W.t[pos] = tj; W.org[pos] = og; }
        nnew += ssc_popc(m);
        SSC_FENCE();
    }
    return nnew;
}

template <class SP, int CK>
__global__ __launch_bounds__(SSC_THREADS) void k_steer_shortcut(ssc_args a)
{
    constexpr int D = SP::d;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ ssc_env sE;
    double* sbox = (double*)smem;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (CK == 0 && a.boxes_in_lds) {
        const int nd = a.M * 2 * SP::wdim;
        for (int t = threadIdx.x; t < nd; t += SSC_THREADS) sbox[t] = a.boxes[t];
    }
    if (threadIdx.x == 0) ssc_bind<SP, CK>(sE, (CK == 0 && a.boxes_in_lds) ? (const double*)sbox : a.boxes, a.M, a.shapes, a.aabb, a.ss, a.prm);
    __syncthreads();                                                     // the only workgroup barrier: wavefronts are on their own from here
    const int64_t pl = (int64_t)blockIdx.x * SSC_WAVES + wave;
    if (pl >= a.nb) return;
    const int64_t b = a.b0 + pl;
    const int ms = a.ms;
    const unsigned long long ltm = (1ull << lane) - 1ull;
    const int n0 = (int)(a.off[b + 1] - a.off[b]);
    const double* src = a.P + a.off[b] * D;

    double* dp = a.dbl + pl * (int64_t)ssc_dbl_per_path(D, ms);
    int32_t* ip = a.ints + pl * (int64_t)SSC_INTS * ms;
    ssc_buf W0, W1;
    W0.p = dp; W0.c = dp + (int64_t)ms * D; W0.t = W0.c + ms;
    W1.p = W0.t + ms; W1.c = W1.p + (int64_t)ms * D; W1.t = W1.c + ms;
    ssc_slab S;
    S.cum = W1.t + ms; S.ncost = S.cum + ms; S.ndur = S.ncost + ms;
    S.nlo = ip; S.nhi = ip + ms; S.npar = ip + 2 * (int64_t)ms; S.nflag = ip + 3 * (int64_t)ms; S.nnseg = ip + 4 * (int64_t)ms;
    S.keep = ip + 5 * (int64_t)ms; S.legnode = ip + 6 * (int64_t)ms;
    W0.org = ip + 7 * (int64_t)ms; W1.org = ip + 8 * (int64_t)ms;

    const ssc_env* E = &sE;
    const double prm[2] = {a.prm[0], a.prm[1]};

    ssc_buf cur = W0, nxt = W1;
    long long checks = 0, tests = 0, inserted = 0;
    int blocked = 0;

    // the input into the first buffer; its legs, steered and tested once
    for (int base = 0; base < n0; base += 64) {
        const int j = base + lane;
        if (j < n0) { double v[D]; ssc_load<D>(src, j, v); ssc_store<D>(cur.p, j, v); cur.org[j] = j + 1; }
    }
    {
        long long cs = 0;
        for (int base = 0; base < n0; base += 64) {
            const int j = base + lane;
            const bool act = j < n0 - 1;
            bool bad = false;
            if (act) {
                const ssc_res r = ssc_pair<SP, CK>(E, ssc_loadv<D>(src, j), ssc_loadv<D>(src, j + 1));
                bad = !r.fr;
                cur.c[j] = r.cost; cur.t[j] = r.dur;
                cs += r.nseg;
            } else if (j == n0 - 1) { cur.c[j] = 0.0; cur.t[j] = 0.0; }
            tests += ssc_popc(__ballot(act));
            blocked += ssc_popc(__ballot(bad));
        }
        checks += ssc_wave_sum(cs);
    }
    SSC_FENCE();
    const double cost_in = ssc_fold(S, cur.c, n0, lane);

    int n = n0, tree_n = -1, nn = 0;
    int maxlen = n0, status = MPFMT_SHORTCUT_DONE, iters = 0;

    auto fixed_point = [&]() {                                            // `while (short_path = shortcut(path)) != path`
        for (;;) {
            if (n <= 2) return;
            if (n != tree_n) { nn = ssc_build_tree(S, n, ms, lane); tree_n = n; }
            const int nnew = ssc_shortcut_pass<SP, CK>(E, S, cur, n, nn, lane, checks, tests);
            if (nnew == n) return;
            n = nnew;
        }
    };
    fixed_point();

    for (int it = 0; it < a.iterations; ++it) {
        // refine: one lane per leg, the expanded path into nxt
        int k = 0;
        long long cs = 0;
        for (int base = 0; base < n - 1; base += 64) {
            const int i = base + lane;
            const bool act = i < n - 1;
            double ci = 0.0, Ti = 0.0, c1 = 0.0, t1 = 0.0, c2 = 0.0, t2 = 0.0;
            const ssc_vec<D> v = ssc_loadv<D>(cur.p, act ? i : 0), w = ssc_loadv<D>(cur.p, act ? i + 1 : 0);
            ssc_vec<D> m = v;
            if (act) { ci = cur.c[i]; Ti = cur.t[i]; }
            const bool prop = act && (Ti > 0.0);
            bool ins = false;
            if (prop) {
                m = ssc_mid_call<SP>(v, w, prm[0], prm[1]);
                const ssc_res r1 = ssc_pair<SP, CK>(E, v, m);
                const ssc_res r2 = ssc_pair<SP, CK>(E, m, w);
                c1 = r1.cost; t1 = r1.dur; c2 = r2.cost; t2 = r2.dur;
                cs += r1.nseg + r2.nseg;
                const double sum = c1 + c2;
                const double thr = SSC_SLACK * ci;
                ins = r1.fr && r2.fr && (sum <= thr);
            }
            tests += 2 * ssc_popc(__ballot(prop));
            const unsigned long long mi = __ballot(ins);
            const int pos = i + k + ssc_popc(mi & ltm);
            if (act) {
                if (pos < ms) { ssc_store<D>(nxt.p, pos, v.x); nxt.c[pos] = ins ? c1 : ci; nxt.t[pos] = ins ? t1 : Ti; nxt.org[pos] = cur.org[i]; }
                if (ins && pos + 1 < ms) { ssc_store<D>(nxt.p, pos + 1, m.x); nxt.c[pos + 1] = c2; nxt.t[pos + 1] = t2; nxt.org[pos + 1] = 0; }
            }
            k += ssc_popc(mi);
        }
        checks += ssc_wave_sum(cs);
        if (n + k > ms) { status = MPFMT_SHORTCUT_TRUNCATED; break; }     // cur still holds the path of the last completed iteration
        if (lane == 0) {
            double v[D];
            ssc_load<D>(cur.p, n - 1, v); ssc_store<D>(nxt.p, n - 1 + k, v);
            nxt.c[n - 1 + k] = 0.0; nxt.t[n - 1 + k] = 0.0; nxt.org[n - 1 + k] = cur.org[n - 1];
        }
        SSC_FENCE();
        const int nbeg = n;
        { const ssc_buf tb = cur; cur = nxt; nxt = tb; }
        n += k; inserted += k;
        maxlen = max(maxlen, n);
        fixed_point();
        ++iters;
        if (n == nbeg) {                                                  // the bit-identical path: later iterations would repeat this one
            int diff = 0;
            for (int base = 0; base < n; base += 64) {
                const int j = base + lane;
                if (j < n) {
#pragma unroll
                    for (int c = 0; c < D; ++c) diff |= (int)(__double_as_longlong(cur.p[(int64_t)j * D + c]) != __double_as_longlong(nxt.p[(int64_t)j * D + c]));
                }
            }
            if (!__ballot(diff != 0)) break;
        }
    }

    if (cur.p != W0.p) {                                                  // the result leaves in the first buffer
        for (int base = 0; base < n; base += 64) {
            const int j = base + lane;
            if (j < n) { double v[D]; ssc_load<D>(cur.p, j, v); ssc_store<D>(W0.p, j, v); W0.c[j] = cur.c[j]; W0.org[j] = cur.org[j]; }
        }
        SSC_FENCE();
    }
    const double cost_out = ssc_fold(S, W0.c, n, lane);                   // S.cum: the cumcost of the result
    if (lane == 0) {
        mpfmt_steer_shortcut_info r;
        r.status = status; r.iterations_done = iters; r.n_out = n; r.max_working_len = maxlen; r.inserted = inserted; r.legs_blocked = blocked;
        r.collision_checks = checks; r.tests_evaluated = tests; r.cost_in = cost_in; r.cost_out = cost_out;
        a.info[b] = r;
    }
}

// the results out of the slabs into the caller's dense layout: one lane per path
template <int D>
__global__ __launch_bounds__(256) void k_ssc_gather(const double* __restrict__ dbl, const int32_t* __restrict__ ints, int64_t b0, int64_t nb,
                                                    int32_t ms, const int64_t* __restrict__ out_off, double* __restrict__ out_P,
                                                    double* __restrict__ cumcost, int32_t* __restrict__ origin)
{
    const int64_t pl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pl >= nb) return;
    const int64_t b = b0 + pl, o = out_off[b], n = out_off[b + 1] - o;
    const double* p = dbl + pl * (int64_t)ssc_dbl_per_path(D, ms);
    const double* cum = p + 2 * ((int64_t)ms * D + 2 * (int64_t)ms);
    const int32_t* org = ints + pl * (int64_t)SSC_INTS * ms + 7 * (int64_t)ms;
    for (int64_t i = 0; i < n && i < ms; ++i) {
        double v[D];
        ssc_load<D>(p, i, v);
        ssc_store<D>(out_P, o + i, v);
        cumcost[o + i] = cum[i];
        origin[o + i] = org[i];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// SP / CK from (space, d, ctx->cc_kind); EXPR sees `SP` and `CK`
#define SSC_DISPATCH(EXPR)                                                                                              \
    do {                                                                                                                \
        if (space == MPFMT_SPACE_DUBINS) { using SP = ssc_car<1>; if (ck) { constexpr int CK = 1; EXPR; } else { constexpr int CK = 0; EXPR; } } \
        else if (space == MPFMT_SPACE_REEDSSHEPP) { using SP = ssc_car<2>; if (ck) { constexpr int CK = 1; EXPR; } else { constexpr int CK = 0; EXPR; } } \
        else if (ck) { using SP = ssc_di<2>; constexpr int CK = 1; EXPR; }                                              \
        else switch (d / 2) {                                                                                           \
            case 1: { using SP = ssc_di<1>; constexpr int CK = 0; EXPR; } break;                                        \
            case 2: { using SP = ssc_di<2>; constexpr int CK = 0; EXPR; } break;                                        \
            case 3: { using SP = ssc_di<3>; constexpr int CK = 0; EXPR; } break;                                        \
            case 4: { using SP = ssc_di<4>; constexpr int CK = 0; EXPR; } break;                                        \
            case 5: { using SP = ssc_di<5>; constexpr int CK = 0; EXPR; } break;                                        \
            default: { using SP = ssc_di<6>; constexpr int CK = 0; EXPR; } break;                                       \
        }                                                                                                               \
    } while (0)

// the workspace dimension of the space's checker
static int ssc_wdim(int32_t space, int32_t d) { return space == MPFMT_SPACE_DI ? d / 2 : 2; }

int32_t mpfmt_steer_pairs_device(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const double* Q, int64_t n,
                                 uint64_t* mask, double* cost, double* dur, int32_t* nseg)
{
    const int ck = ctx->cc_kind;
    const int32_t M = ctx->M;
    const int64_t words = (n + 63) / 64;
    mpfmt_tmp tmp;
    double *dP = nullptr, *dQ = nullptr, *dcost = nullptr, *ddur = nullptr;
    int32_t* dnseg = nullptr;
    unsigned long long* dmask = nullptr;
    HIPCHK(ctx, tmp.get(&dP, sizeof(double) * (size_t)n * d));
    HIPCHK(ctx, tmp.get(&dQ, sizeof(double) * (size_t)n * d));
    HIPCHK(ctx, tmp.get(&dmask, sizeof(unsigned long long) * (size_t)words));
    if (cost) HIPCHK(ctx, tmp.get(&dcost, sizeof(double) * (size_t)n));
    if (dur) HIPCHK(ctx, tmp.get(&ddur, sizeof(double) * (size_t)n));
    if (nseg) HIPCHK(ctx, tmp.get(&dnseg, sizeof(int32_t) * (size_t)n));
    HIPCHK(ctx, hipMemcpyAsync(dP, P, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dQ, Q, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, ctx->stream));
    ssp_args a;
    a.P = dP; a.Q = dQ; a.n = n; a.cost = dcost; a.dur = ddur; a.nseg = dnseg; a.mask = dmask;
    a.boxes = ctx->boxes; a.M = M; a.shapes = ctx->shapes2d; a.aabb = ctx->aabb2d; a.ss = ctx->ss;
    a.prm[0] = params[0]; a.prm[1] = params[1];
    const size_t box_bytes = ck == 0 ? sizeof(double) * 2 * (size_t)ssc_wdim(space, d) * (size_t)M : 0;
    a.boxes_in_lds = (ck == 0 && M > 0 && box_bytes <= SSC_LDS_BYTES) ? 1 : 0;
    const size_t lds = a.boxes_in_lds ? box_bytes : 0;
    const unsigned nblk = (unsigned)((n + SSC_THREADS - 1) / SSC_THREADS);
    {
        mpfmt_timed tm(ctx);
        SSC_DISPATCH(hipLaunchKernelGGL((k_ssc_pairs<SP, CK>), dim3(nblk), dim3(SSC_THREADS), lds, ctx->stream, a));
        HIPCHK(ctx, hipGetLastError());
        tm.end("steer_motions_free");
    }
    HIPCHK(ctx, hipMemcpyAsync(mask, dmask, sizeof(uint64_t) * (size_t)words, hipMemcpyDeviceToHost, ctx->stream));
    if (cost) HIPCHK(ctx, hipMemcpyAsync(cost, dcost, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (dur) HIPCHK(ctx, hipMemcpyAsync(dur, ddur, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (nseg) HIPCHK(ctx, hipMemcpyAsync(nseg, dnseg, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

int32_t mpfmt_steer_shortcut_batch_device(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const int64_t* offsets,
                                          int64_t B, int32_t iterations, int64_t max_states, double* out_P, int64_t* out_offsets, int64_t out_cap,
                                          double* cumcost, int32_t* out_origin, mpfmt_steer_shortcut_info* info)
{
    const int ck = ctx->cc_kind;
    const int64_t total = offsets[B];
    const int32_t ms = (int32_t)max_states;
    const int32_t M = ctx->M;
    // paths per launch: the slabs of one launch stay below 1 GiB
    const size_t per_path = sizeof(double) * ssc_dbl_per_path(d, ms) + sizeof(int32_t) * (size_t)SSC_INTS * ms;
    const int64_t chunk = std::max<int64_t>(SSC_WAVES, std::min<int64_t>(B, (int64_t)(((size_t)1 << 30) / per_path) / SSC_WAVES * SSC_WAVES));
    mpfmt_tmp tmp;
    double *dP = nullptr, *ddbl = nullptr, *dout = nullptr, *dcc = nullptr;
    int64_t *doff = nullptr, *dooff = nullptr;
    int32_t *dints = nullptr, *dorg = nullptr;
    mpfmt_steer_shortcut_info* dinfo = nullptr;
    HIPCHK(ctx, tmp.get(&dP, sizeof(double) * (size_t)total * d));
    HIPCHK(ctx, tmp.get(&doff, sizeof(int64_t) * (size_t)(B + 1)));
    HIPCHK(ctx, tmp.get(&dooff, sizeof(int64_t) * (size_t)(B + 1)));
    HIPCHK(ctx, tmp.get(&dinfo, sizeof(mpfmt_steer_shortcut_info) * (size_t)B));
    HIPCHK(ctx, tmp.get(&ddbl, sizeof(double) * ssc_dbl_per_path(d, ms) * (size_t)chunk));
    HIPCHK(ctx, tmp.get(&dints, sizeof(int32_t) * (size_t)SSC_INTS * ms * (size_t)chunk));
    HIPCHK(ctx, hipMemcpyAsync(dP, P, sizeof(double) * (size_t)total * d, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(doff, offsets, sizeof(int64_t) * (size_t)(B + 1), hipMemcpyHostToDevice, ctx->stream));

    ssc_args a;
    a.P = dP; a.off = doff; a.iterations = iterations; a.ms = ms; a.dbl = ddbl; a.ints = dints;
    a.boxes = ctx->boxes; a.M = M; a.shapes = ctx->shapes2d; a.aabb = ctx->aabb2d; a.ss = ctx->ss; a.info = dinfo;
    a.prm[0] = params[0]; a.prm[1] = params[1];
    const size_t box_bytes = ck == 0 ? sizeof(double) * 2 * (size_t)ssc_wdim(space, d) * (size_t)M : 0;
    a.boxes_in_lds = (ck == 0 && M > 0 && box_bytes <= SSC_LDS_BYTES) ? 1 : 0;
    const size_t lds = a.boxes_in_lds ? box_bytes : 0;

    std::vector<mpfmt_steer_shortcut_info> hinfo((size_t)B);
    int64_t done_off = 0;
    out_offsets[0] = 0;
    bool over = false;
    // a launch runs a chunk of the batch start to end; the gather of a chunk needs its output offsets, which the host sums from the
    // chunk's lengths (one small copy per launch)
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        a.b0 = b0; a.nb = std::min(chunk, B - b0);
        const unsigned nblk = (unsigned)((a.nb + SSC_WAVES - 1) / SSC_WAVES);
        {
            mpfmt_timed tm(ctx);
            SSC_DISPATCH(hipLaunchKernelGGL((k_steer_shortcut<SP, CK>), dim3(nblk), dim3(SSC_THREADS), lds, ctx->stream, a));
            HIPCHK(ctx, hipGetLastError());
            tm.end("steer_shortcut_batch");
        }
        HIPCHK(ctx, hipMemcpyAsync(hinfo.data() + b0, dinfo + b0, sizeof(mpfmt_steer_shortcut_info) * (size_t)a.nb, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t q = 0; q < a.nb; ++q) { done_off += hinfo[(size_t)(b0 + q)].n_out; out_offsets[b0 + q + 1] = done_off; }
        if (done_off > out_cap) { over = true; continue; }               // keep running: info and out_offsets are part of the answer
        if (over) continue;
        if (!dout) {
            HIPCHK(ctx, tmp.get(&dout, sizeof(double) * (size_t)std::max<int64_t>(out_cap, 1) * d));
            HIPCHK(ctx, tmp.get(&dcc, sizeof(double) * (size_t)std::max<int64_t>(out_cap, 1)));
            HIPCHK(ctx, tmp.get(&dorg, sizeof(int32_t) * (size_t)std::max<int64_t>(out_cap, 1)));
        }
        HIPCHK(ctx, hipMemcpyAsync(dooff + b0, out_offsets + b0, sizeof(int64_t) * (size_t)(a.nb + 1), hipMemcpyHostToDevice, ctx->stream));
        const unsigned gb = (unsigned)((a.nb + 255) / 256);
        SSC_DISPATCH(hipLaunchKernelGGL((k_ssc_gather<SP::d>), dim3(gb), dim3(256), 0, ctx->stream, ddbl, dints, b0, a.nb, ms, dooff, dout, dcc, dorg));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                  // (out_offsets is pageable host memory: the copy above must have left it)
    }
    int64_t ev = 0, ch = 0;
    for (int64_t q = 0; q < B; ++q) { info[q] = hinfo[(size_t)q]; ev += hinfo[(size_t)q].tests_evaluated; ch += hinfo[(size_t)q].collision_checks; }
    ctx->ssc_tests = ev; ctx->ssc_checks = ch;
    if (over) return mpfmt_fail(ctx, MPFMT_ERR_CAPACITY, "steer_shortcut: the shortcut paths hold %lld states, out_cap is %lld", (long long)done_off,
                                (long long)out_cap);
    if (done_off > 0) {
        HIPCHK(ctx, hipMemcpyAsync(out_P, dout, sizeof(double) * (size_t)done_off * d, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(cumcost, dcc, sizeof(double) * (size_t)done_off, hipMemcpyDeviceToHost, ctx->stream));
        if (out_origin) HIPCHK(ctx, hipMemcpyAsync(out_origin, dorg, sizeof(int32_t) * (size_t)done_off, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MPFMT_OK;
}
