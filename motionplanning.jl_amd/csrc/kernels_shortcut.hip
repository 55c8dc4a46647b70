// Adaptive shortcutting of a batch of paths on gfx950 (include/mpfmt.h, "adaptive shortcutting"): shortcut / cut_corner /
// adaptive_shortcut of src/postprocessors.jl:6-39 for B paths in ONE launch, one wavefront per path, no host round trip between passes.
//
// Every test bit is the one mpfmt_motions_free returns: in_state_space of the first point (statespaces.jl:153-158), then the predicates of
// sweep_predicates.h (AABBs) or sat2d_predicates.h (2-D shapes), unchanged.  The procedure is a pure function of those bits, so what the
// wavefront evaluates speculatively never shows in a result:
//   shortcut   : the split tree of a path of n states depends on n alone (n - 2 inner nodes: a node of more than two states is tested and,
//                when blocked, split at ceil(len / 2)).  ALL inner nodes are tested, one per lane in strips of 64; a node was ASKED by the
//                sequential recursion iff every ancestor is blocked, and the kept states are the two ends and the split states of the
//                asked, blocked nodes (a node's result always holds both its ends).  The kept states are compacted in place.
//   cut_corner : corner c holds its pair (m1, m2) after `lev` halvings in the two slots it will occupy in the expanded path.  A round
//                hands every unresolved corner K consecutive levels (K = the power of two that fills 64 lanes); lane o applies o + 1
//                halvings and tests.  The first lane of a corner that is free -- or whose halving changed nothing (stuck) -- decides it,
//                found with one ballot; otherwise the last lane's pair becomes the corner's new base.
//   counts     : collision_checks adds the in-bounds bits of the asked tests only (levels up to the deciding one; corners up to the first
//                stuck one); tests_evaluated adds every lane that ran a test.
// Layout: 4 paths per workgroup; the obstacle set is staged in LDS once per workgroup when it fits (else read from HBM through the
// same generic pointer), culled once per path against the path's bounding box (shortcut and cut points stay inside the convex hull of the
// input, so a box whose broad phase separates it from that bounding box separates it from every segment the path will ever test); the
// working path (two buffers of max_states states), the tree and the per-corner state live in a per-path slab of HBM that stays in cache.
// All cross-lane traffic through that slab is between lanes of ONE wavefront, whose vector memory operations execute in program order.
#include "mpfmt_internal.h"
#include <algorithm>
#include <cmath>
#include <vector>
#include "sweep_predicates.h"
#include "sat2d_predicates.h"

#define SC_WAVES 4
#define SC_THREADS (SC_WAVES * 64)
#define SC_LDS_BYTES (60 * 1024)
#define SC_MAX_LEVELS 8192               // cut_corner levels after which a corner is given up as stuck (never reached: see k_shortcut)
#define SC_INTS 10                       // int32 arrays of max_states entries per path (see sc_slab)

// orders the slab traffic of one wavefront: a compiler barrier for memory operations (the hardware keeps a wavefront's vector memory
// operations in program order)
#define SC_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

struct sc_args {
    const double* P;                     // [sum n][D] the batch
    const int64_t* off;                  // [B + 1]
    int64_t b0, nb;                      // paths [b0, b0 + nb) run in this launch
    int32_t iterations, ms;
    double* wp;                          // [nb][2][ms][D] working paths
    int32_t* ints;                       // [nb][SC_INTS][ms]
    int32_t* surv;                       // [nb][max(M, 1)] boxes that survive the path's cull
    const double* boxes; int32_t M; int32_t boxes_in_lds;
    const mpfmt_shape2d* shapes; mpfmt_aabb2d aabb;
    mpfmt_ss ss;
    mpfmt_shortcut_info* info;           // [B]
};

template <int D>
struct sc_env {
    const double* bx; const int32_t* surv; int ns;
    const mpfmt_shape2d* shapes; int nshapes; mpfmt_aabb2d aabb;
    mpfmt_ss ss;
};

template <int D>
__device__ __forceinline__ void sc_load(const double* p, int64_t i, double (&v)[D])
{
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = p[i * D + c];
}
template <int D>
__device__ __forceinline__ void sc_store(double* p, int64_t i, const double (&v)[D])
{
#pragma unroll
    for (int c = 0; c < D; ++c) p[i * D + c] = v[c];
}

// the bit of mpfmt_motions_free for the lane's segment (k_edges_free / k2d_edges); inb = the first point lies inside the state bounds.
// Wave-uniform control flow around the ballots; inactive lanes ride along with fr = false.
template <int D, int CC>
__device__ __forceinline__ bool sc_test(const sc_env<D>& E, const double (&v)[D], const double (&w)[D], bool active, bool& inb)
{
    if constexpr (CC == 1) {
        bool fr = false;
        inb = false;
        if (active) {
            inb = in_ss_2d(v[0], v[1], E.ss);
            fr = inb && motion_free_2d(v[0], v[1], w[0], w[1], E.shapes, E.nshapes, E.aabb);
        }
        return fr;
    } else {
        inb = active && in_state_space_sl<D>(v, E.ss);
        bool fr = inb;
        double l[D], h[D];
        seg_bbox<D>(v, w, l, h);
        for (int s = 0; s < E.ns; ++s) {
            if (!__ballot(fr)) break;
            const int k = __builtin_amdgcn_readfirstlane(E.surv[s]);
            const box_regs<D> b = load_box<D>(E.bx, k);                 // wave-uniform k: broadcast reads
            const bool pend = fr & !broadphase_free_sl<D>(l, h, b);
            if (__ballot(pend)) {
                if (pend) fr = narrow_free_sl<D>(v, w, b);
            }
        }
        return fr;
    }
}

__device__ __forceinline__ int sc_popc(unsigned long long m) { return __popcll(m); }
__device__ __forceinline__ int sc_wave_sum(int v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ int sc_wave_max(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }

// per-path slab of int32 arrays
struct sc_slab {
    int32_t *nlo, *nhi, *npar, *nflag;   // split tree: inner node i tests (nlo, nhi); parent; flags: 1 free, 2 first point in bounds
    int32_t *keep;                       // per state of the working path
    int32_t *clev, *ccnt, *cstat, *chalv;// per corner: halvings applied to its stored pair, counted tests, 0 open / 1 cut / 2 stuck, halvings
    int32_t *alist;                      // unresolved corners
};

// the split tree of a path of n >= 3 states (n - 2 inner nodes), breadth first
__device__ __forceinline__ int sc_build_tree(const sc_slab& S, int n, int ms, int lane)
{
    const unsigned long long ltm = (1ull << lane) - 1ull;
    if (lane == 0) { S.nlo[0] = 0; S.nhi[0] = n - 1; S.npar[0] = -1; }
    SC_FENCE();
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
            const int pos = tail + sc_popc(mL & ltm) + sc_popc(mR & ltm);
            if (L && pos < ms) { S.nlo[pos] = lo; S.nhi[pos] = split; S.npar[pos] = i; }
            const int p2 = pos + (L ? 1 : 0);
            if (R && p2 < ms) { S.nlo[p2] = split; S.nhi[p2] = hi; S.npar[p2] = i; }
            tail += sc_popc(mL) + sc_popc(mR);
        }
        SC_FENCE();
        ls = le; le = min(tail, ms);
    }
    return le;
}

// one shortcut(path) in place; returns the new length
template <int D, int CC>
__device__ __forceinline__ int sc_shortcut_pass(const sc_env<D>& E, const sc_slab& S, double* cur, int n, int nn, int lane, long long& checks,
                                                long long& tests)
{
    const unsigned long long ltm = (1ull << lane) - 1ull;
    for (int base = 0; base < nn; base += 64) {                          // every inner node, speculatively
        const int i = base + lane;
        const bool act = i < nn;
        const int lo = act ? S.nlo[i] : 0, hi = act ? S.nhi[i] : 0;
        double v[D], w[D];
        sc_load<D>(cur, lo, v); sc_load<D>(cur, hi, w);
        bool inb;
        const bool fr = sc_test<D, CC>(E, v, w, act, inb);
        if (act) S.nflag[i] = (fr ? 1 : 0) | (inb ? 2 : 0);
        tests += sc_popc(__ballot(act));
    }
    for (int base = 0; base < n; base += 64) { const int j = base + lane; if (j < n) S.keep[j] = (j == 0 || j == n - 1) ? 1 : 0; }
    SC_FENCE();
    for (int base = 0; base < nn; base += 64) {                          // asked = every ancestor blocked
        const int i = base + lane;
        const bool act = i < nn;
        bool asked = act;
        int f = 0;
        if (act) {
            f = S.nflag[i];
            int p = S.npar[i];
            while (p >= 0 && asked) { asked = !(S.nflag[p] & 1); p = S.npar[p]; }
            if (asked && !(f & 1)) { const int lo = S.nlo[i], hi = S.nhi[i]; S.keep[lo + (hi - lo + 2) / 2 - 1] = 1; }
        }
        checks += sc_popc(__ballot(asked && (f & 2)));
    }
    SC_FENCE();
    int nnew = 0;
    for (int base = 0; base < n; base += 64) {                           // compaction in place: a state moves to a position <= its own
        const int j = base + lane;
        const bool k = j < n && S.keep[j] != 0;
        double v[D];
        sc_load<D>(cur, k ? j : 0, v);
        const unsigned long long m = __ballot(k);
        const int pos = nnew + sc_popc(m & ltm);
        SC_FENCE();
        if (k) sc_store<D>(cur, pos, v);
        nnew += sc_popc(m);
        SC_FENCE();
    }
    return nnew;
}

template <int D, int CC>
__global__ __launch_bounds__(SC_THREADS) void k_shortcut(sc_args a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* sbox = (double*)smem;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (CC == 0 && a.boxes_in_lds) {
        const int nd = a.M * 2 * D;
        for (int t = threadIdx.x; t < nd; t += SC_THREADS) sbox[t] = a.boxes[t];
    }
    __syncthreads();                                                     // the only workgroup barrier: wavefronts are on their own from here
    const int64_t pl = (int64_t)blockIdx.x * SC_WAVES + wave;
    if (pl >= a.nb) return;
    const int64_t b = a.b0 + pl;
    const int ms = a.ms;
    const unsigned long long ltm = (1ull << lane) - 1ull;
    const int n0 = (int)(a.off[b + 1] - a.off[b]);
    const double* src = a.P + a.off[b] * D;
    double* cur = a.wp + pl * 2 * (int64_t)ms * D;
    double* nxt = cur + (int64_t)ms * D;
    double* const buf0 = cur;
    int32_t* ip = a.ints + pl * (int64_t)SC_INTS * ms;
    sc_slab S;
    S.nlo = ip; S.nhi = ip + ms; S.npar = ip + 2 * (int64_t)ms; S.nflag = ip + 3 * (int64_t)ms; S.keep = ip + 4 * (int64_t)ms;
    S.clev = ip + 5 * (int64_t)ms; S.ccnt = ip + 6 * (int64_t)ms; S.cstat = ip + 7 * (int64_t)ms; S.chalv = ip + 8 * (int64_t)ms;
    S.alist = ip + 9 * (int64_t)ms;
    int32_t* surv = a.surv + pl * (int64_t)max(a.M, 1);

    sc_env<D> E;
    E.bx = (CC == 0 && a.boxes_in_lds) ? (const double*)sbox : a.boxes;
    E.surv = surv; E.ns = 0;
    E.shapes = a.shapes; E.nshapes = a.M; E.aabb = a.aabb; E.ss = a.ss;

    // the input into the working buffer; its bounding box; the boxes that survive it
    double ulo[D], uhi[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { ulo[c] = __builtin_inf(); uhi[c] = -__builtin_inf(); }
    for (int base = 0; base < n0; base += 64) {
        const int j = base + lane;
        if (j < n0) {
            double v[D];
            sc_load<D>(src, j, v);
            sc_store<D>(cur, j, v);
#pragma unroll
            for (int c = 0; c < D; ++c) { ulo[c] = (v[c] < ulo[c]) ? v[c] : ulo[c]; uhi[c] = (v[c] > uhi[c]) ? v[c] : uhi[c]; }
        }
    }
#pragma unroll
    for (int c = 0; c < D; ++c)
        for (int o = 32; o > 0; o >>= 1) {
            const double x = __shfl_xor(ulo[c], o), y = __shfl_xor(uhi[c], o);
            ulo[c] = (x < ulo[c]) ? x : ulo[c];
            uhi[c] = (y > uhi[c]) ? y : uhi[c];
        }
    if constexpr (CC == 0) {
        int ns = 0;
        for (int base = 0; base < a.M; base += 64) {
            const int k = base + lane;
            const box_regs<D> bb = load_box<D>(E.bx, min(k, a.M - 1));
            int out = 0;
#pragma unroll
            for (int c = 0; c < D; ++c) out |= (int)(bb.hi[c] < ulo[c]) | (int)(bb.lo[c] > uhi[c]);
            const bool kp = k < a.M && !out;
            const unsigned long long m = __ballot(kp);
            if (kp) surv[ns + sc_popc(m & ltm)] = k;
            ns += sc_popc(m);
        }
        E.ns = ns;
    }
    SC_FENCE();

    int n = n0, tree_n = -1, nn = 0;
    long long checks = 0, tests = 0;
    int maxlen = n0, maxhalv = 0, status = MPFMT_SHORTCUT_DONE, iters = 0;

    auto fixed_point = [&]() {                                            // `while (short_path = shortcut(path, CC)) != path`
        for (;;) {
            if (n <= 2) return;
            if (n != tree_n) { nn = sc_build_tree(S, n, ms, lane); tree_n = n; }
            const int nnew = sc_shortcut_pass<D, CC>(E, S, cur, n, nn, lane, checks, tests);
            if (nnew == n) return;
            n = nnew;
        }
    };
    fixed_point();

    for (int it = 0; it < a.iterations; ++it) {
        if (n <= 2) { iters = a.iterations; break; }                     // nothing left to cut: the remaining iterations ask for no test
        if (2 * n - 2 > ms) { status = MPFMT_SHORTCUT_TRUNCATED; break; }
        const int nc = n - 2;
        for (int base = 0; base < nc; base += 64) {                      // corner c = states (c, c + 1, c + 2); its pair starts as (v1, v3)
            const int c = base + lane;
            if (c < nc) {
                double v[D];
                sc_load<D>(cur, c, v); sc_store<D>(nxt, 1 + 2 * c, v);
                sc_load<D>(cur, c + 2, v); sc_store<D>(nxt, 2 + 2 * c, v);
                S.clev[c] = 0; S.ccnt[c] = 0; S.cstat[c] = 0; S.chalv[c] = 0; S.alist[c] = c;
            }
        }
        if (lane == 0) { double v[D]; sc_load<D>(cur, 0, v); sc_store<D>(nxt, 0, v); sc_load<D>(cur, n - 1, v); sc_store<D>(nxt, 2 * n - 3, v); }
        SC_FENCE();
        int na = nc;
        while (na > 0) {
            int K = 1;
            while (K < 64 && 2 * K * na <= 64) K *= 2;
            const int per = 64 / K;                                      // corners per strip
            const int o = lane & (K - 1), g = lane / K;
            int newna = 0;
            for (int base = 0; base < na; base += per) {
                const int ci = base + g;
                const bool act = ci < na;
                const int c = act ? S.alist[ci] : 0;
                double v2[D], pa[D], pb[D], qa[D], qb[D];
                sc_load<D>(cur, c + 1, v2); sc_load<D>(nxt, 1 + 2 * c, pa); sc_load<D>(nxt, 2 + 2 * c, pb);
                const int lev0 = S.clev[c];
                bool same = false;
                const int steps = act ? o + 1 : 0;
                for (int s = 0; s < steps; ++s) {                        // (m + v2) / 2: one add, one halving
                    same = true;
#pragma unroll
                    for (int q = 0; q < D; ++q) {
                        const double sa = pa[q] + v2[q]; qa[q] = sa / 2;
                        const double sb = pb[q] + v2[q]; qb[q] = sb / 2;
                        same = same & (qa[q] == pa[q]) & (qb[q] == pb[q]);
                    }
#pragma unroll
                    for (int q = 0; q < D; ++q) { pa[q] = qa[q]; pb[q] = qb[q]; }
                }
                const int level = lev0 + o;                              // halvings of the cut_corner loop that lead to this pair
                bool inb;
                const bool fr = sc_test<D, CC>(E, pa, pb, act, inb);
                const int ev = !act ? 0 : (level >= 1 && same) ? 2 : fr ? 1 : 0;
                const unsigned long long mev = __ballot(ev != 0);
                const unsigned long long fmask = (K == 64) ? ~0ull : ((1ull << K) - 1ull);
                const unsigned long long field = (mev >> (lane - o)) & fmask;
                const int first = field ? (__ffsll((long long)field) - 1) : K;
                const int evf = __shfl(ev, (lane - o) + min(first, K - 1));
                const bool counted = act && (o < first || (o == first && evf == 1));
                const unsigned long long mc = __ballot(counted && inb);
                const int cinc = sc_popc((mc >> (lane - o)) & fmask);
                tests += sc_popc(__ballot(act));
                SC_FENCE();
                if (act && o == 0) S.ccnt[c] += cinc;
                if (act && first < K && o == first) {
                    if (ev == 1) { sc_store<D>(nxt, 1 + 2 * c, pa); sc_store<D>(nxt, 2 + 2 * c, pb); }
                    S.cstat[c] = ev; S.chalv[c] = level;
                }
                // (the halvings reach their fixed point within ~1100 levels in binary64; the cap only bounds the loop should they ever not)
                const bool giveup = lev0 + K > SC_MAX_LEVELS;
                if (act && first == K && o == K - 1) {
                    sc_store<D>(nxt, 1 + 2 * c, pa); sc_store<D>(nxt, 2 + 2 * c, pb); S.clev[c] = lev0 + K;
                    if (giveup) { S.cstat[c] = 2; S.chalv[c] = level; }
                }
                const bool open = act && o == 0 && first == K && !giveup;
                const unsigned long long mo = __ballot(open);
                if (open) S.alist[newna + sc_popc(mo & ltm)] = c;        // in place: written at an index <= the one it was read from
                newna += sc_popc(mo);
                SC_FENCE();
            }
            na = newna;
        }
        // corners are cut in order: the first stuck one ends the path; the counts stop there
        int jst = nc;
        for (int base = 0; base < nc && jst == nc; base += 64) {
            const int c = base + lane;
            const unsigned long long m = __ballot(c < nc && S.cstat[c] == 2);
            if (m) jst = base + __ffsll((long long)m) - 1;
        }
        int cs = 0, hm = 0;
        for (int base = 0; base < nc; base += 64) {
            const int c = base + lane;
            if (c < nc && c <= jst) { cs += S.ccnt[c]; hm = max(hm, S.chalv[c]); }
        }
        checks += sc_wave_sum(cs);
        maxhalv = max(maxhalv, sc_wave_max(hm));
        if (jst < nc) { status = MPFMT_SHORTCUT_STUCK; break; }
        { double* t = cur; cur = nxt; nxt = t; }
        n = 2 * n - 2;
        maxlen = max(maxlen, n);
        fixed_point();
        ++iters;
    }

    if (cur != buf0) {                                                   // the result leaves in the first buffer
        for (int base = 0; base < n; base += 64) {
            const int j = base + lane;
            if (j < n) { double v[D]; sc_load<D>(cur, j, v); sc_store<D>(buf0, j, v); }
        }
    }
    if (lane == 0) {
        mpfmt_shortcut_info r;
        r.status = status; r.iterations_done = iters; r.n_out = n; r.max_working_len = maxlen; r.max_halvings = maxhalv;
        r.collision_checks = checks; r.tests_evaluated = tests;
        a.info[b] = r;
    }
}

// the results out of the slabs into the caller's dense layout, and cumcost = cumsum([0; norm.(diff(path))]): one lane per path
template <int D>
__global__ __launch_bounds__(256) void k_shortcut_gather(const double* __restrict__ wp, int64_t b0, int64_t nb, int32_t ms,
                                                         const int64_t* __restrict__ out_off, double* __restrict__ out_P,
                                                         double* __restrict__ cumcost)
{
    const int64_t pl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pl >= nb) return;
    const int64_t b = b0 + pl, o = out_off[b], n = out_off[b + 1] - o;
    const double* p = wp + pl * 2 * (int64_t)ms * D;
    double prev[D], acc = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double v[D];
        sc_load<D>(p, i, v);
        sc_store<D>(out_P, o + i, v);
        if (i > 0) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) { const double t = v[c] - prev[c]; const double tt = t * t; s = (c == 0) ? tt : s + tt; }
            acc = acc + sqrt(s);
        }
        cumcost[o + i] = acc;
#pragma unroll
        for (int c = 0; c < D; ++c) prev[c] = v[c];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
namespace {
}  // namespace

template <int D>
static void sc_launch(mpfmt_ctx* ctx, const sc_args& a, size_t lds)
{
    const unsigned nblk = (unsigned)((a.nb + SC_WAVES - 1) / SC_WAVES);
    if (ctx->cc_kind == 1) {
        if constexpr (D == 2) hipLaunchKernelGGL((k_shortcut<2, 1>), dim3(nblk), dim3(SC_THREADS), 0, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((k_shortcut<D, 0>), dim3(nblk), dim3(SC_THREADS), lds, ctx->stream, a);
    }
}

int32_t mpfmt_shortcut_batch_device(mpfmt_ctx* ctx, const double* P, const int64_t* offsets, int64_t B, int32_t iterations, int64_t max_states,
                                    double* out_P, int64_t* out_offsets, int64_t out_cap, double* cumcost, mpfmt_shortcut_info* info)
{
    const int d = ctx->dw;
    const int64_t total = offsets[B];
    const int32_t ms = (int32_t)max_states;
    const int32_t M = ctx->M;
    // paths per launch: the slabs of one launch stay below 1 GiB
    const size_t per_path = sizeof(double) * 2 * (size_t)ms * d + sizeof(int32_t) * (size_t)SC_INTS * ms + sizeof(int32_t) * (size_t)std::max(M, 1);
    const int64_t chunk = std::max<int64_t>(SC_WAVES, std::min<int64_t>(B, (int64_t)(((size_t)1 << 30) / per_path) / SC_WAVES * SC_WAVES));
    mpfmt_tmp tmp;
    double *dP = nullptr, *dwp = nullptr, *dout = nullptr, *dcc = nullptr;
    int64_t *doff = nullptr, *dooff = nullptr;
    int32_t *dints = nullptr, *dsurv = nullptr;
    mpfmt_shortcut_info* dinfo = nullptr;
    HIPCHK(ctx, tmp.get(&dP, sizeof(double) * (size_t)total * d));
    HIPCHK(ctx, tmp.get(&doff, sizeof(int64_t) * (size_t)(B + 1)));
    HIPCHK(ctx, tmp.get(&dooff, sizeof(int64_t) * (size_t)(B + 1)));
    HIPCHK(ctx, tmp.get(&dinfo, sizeof(mpfmt_shortcut_info) * (size_t)B));
    HIPCHK(ctx, tmp.get(&dwp, sizeof(double) * 2 * (size_t)ms * d * (size_t)chunk));
    HIPCHK(ctx, tmp.get(&dints, sizeof(int32_t) * (size_t)SC_INTS * ms * (size_t)chunk));
    HIPCHK(ctx, tmp.get(&dsurv, sizeof(int32_t) * (size_t)std::max(M, 1) * (size_t)chunk));
    HIPCHK(ctx, hipMemcpyAsync(dP, P, sizeof(double) * (size_t)total * d, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(doff, offsets, sizeof(int64_t) * (size_t)(B + 1), hipMemcpyHostToDevice, ctx->stream));

    sc_args a;
    a.P = dP; a.off = doff; a.iterations = iterations; a.ms = ms; a.wp = dwp; a.ints = dints; a.surv = dsurv;
    a.boxes = ctx->boxes; a.M = M; a.shapes = ctx->shapes2d; a.aabb = ctx->aabb2d; a.ss = ctx->ss; a.info = dinfo;
    const size_t box_bytes = ctx->cc_kind == 0 ? sizeof(double) * 2 * (size_t)d * (size_t)M : 0;
    a.boxes_in_lds = (ctx->cc_kind == 0 && M > 0 && box_bytes <= SC_LDS_BYTES) ? 1 : 0;
    const size_t lds = a.boxes_in_lds ? box_bytes : 0;

    std::vector<mpfmt_shortcut_info> hinfo((size_t)B);
    int64_t done_off = 0;
    out_offsets[0] = 0;
    bool over = false;
    // a launch runs a chunk of the batch start to end; the gather of a chunk needs its output offsets, which the host sums from the
    // chunk's lengths (one small copy per launch)
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        a.b0 = b0; a.nb = std::min(chunk, B - b0);
        {
            mpfmt_timed tm(ctx);
            DISPATCH_D(d, sc_launch<DD>(ctx, a, lds));
            HIPCHK(ctx, hipGetLastError());
            tm.end("shortcut_batch");
        }
        HIPCHK(ctx, hipMemcpyAsync(hinfo.data() + b0, dinfo + b0, sizeof(mpfmt_shortcut_info) * (size_t)a.nb, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t q = 0; q < a.nb; ++q) { done_off += hinfo[(size_t)(b0 + q)].n_out; out_offsets[b0 + q + 1] = done_off; }
        if (done_off > out_cap) { over = true; continue; }               // keep running: info and out_offsets are part of the answer
        if (over) continue;
        if (!dout) {
            HIPCHK(ctx, tmp.get(&dout, sizeof(double) * (size_t)std::max<int64_t>(out_cap, 1) * d));
            HIPCHK(ctx, tmp.get(&dcc, sizeof(double) * (size_t)std::max<int64_t>(out_cap, 1)));
        }
        HIPCHK(ctx, hipMemcpyAsync(dooff + b0, out_offsets + b0, sizeof(int64_t) * (size_t)(a.nb + 1), hipMemcpyHostToDevice, ctx->stream));
        const unsigned gb = (unsigned)((a.nb + 255) / 256);
        DISPATCH_D(d, hipLaunchKernelGGL((k_shortcut_gather<DD>), dim3(gb), dim3(256), 0, ctx->stream, dwp, b0, a.nb, ms, dooff, dout, dcc));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                  // (out_offsets is pageable host memory: the copy above must have left it)
    }
    int64_t ev = 0, ch = 0;
    for (int64_t q = 0; q < B; ++q) { info[q] = hinfo[(size_t)q]; ev += hinfo[(size_t)q].tests_evaluated; ch += hinfo[(size_t)q].collision_checks; }
    ctx->shortcut_tests = ev; ctx->shortcut_checks = ch;
    if (over) return mpfmt_fail(ctx, MPFMT_ERR_CAPACITY, "adaptive_shortcut: the smoothed paths hold %lld states, out_cap is %lld", (long long)done_off,
                                (long long)out_cap);
    if (done_off > 0) {
        HIPCHK(ctx, hipMemcpyAsync(out_P, dout, sizeof(double) * (size_t)done_off * d, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(cumcost, dcc, sizeof(double) * (size_t)done_off, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MPFMT_OK;
}
