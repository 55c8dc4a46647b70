// Dubins car: DubinsQuasiMetricSpace of src/statespaces/simplecars.jl -- SE2 states (x, y, theta),
// workspace (x, y), exact Dubins length as a quasi-metric "chopped" by the Euclidean lower bound on positions:
//   backward set of j = { i : |xy_i - xy_j| <= r  and  dubins(i -> j) <= r }      (nearneighbors.jl:185-198)
// Built here as: (1) the Euclidean r-disc graph of the positions with the library's own MFMA pair path (a helper ctx holding
// the N x 2 positions), (2) one lane per candidate edge: the six Dubins words (simplecars.jl:106-194), keep cost <= r,
// (3) ordered compaction into the CSC the planner consumes.  The collision sweep regenerates the steering controls per edge,
// walks the reference's collision waypoints (arcs sampled every pi/12, :68-83; target appended, statespaces.jl:135) and tests
// consecutive pairs on (x, y) against the AABB set with the SE2 bounds on the first point (statespaces.jl:153-158).
// Arithmetic: the reference's expressions in the written order, unfused; sin / cos / atan2 / acos come from mp_math.h (fixed
// reductions and polynomials from + - * / sqrt, the SAME header the CPU oracle compiles: results are bit-identical); fmod / sqrt are the device
// libm's, so costs agree with a CPU libm to a few ulp rather than bit for bit (the tests bound it).
#include <cstring>
#include "mpfmt_internal.h"
#include "mp_math.h"
#include "car_steer.h"
#include "sat2d_predicates.h"
#include "steer_delta.h"
#include "steer_roadmap.h"
#include "car_motion.h"

// ---- kernels -----------------------------------------------------------------------------------------------------------
// lane = candidate entry e of the positions graph (row i, column j): Dubins: cost(i -> j) (backward set of j); Reeds-Shepp:
// cost(j -> i) (inball(j), ds = colwise(dist, V[j], V[inds])); keep bit = cost <= r
template <int KIND>
__global__ __launch_bounds__(256) void k_car_cost(const double* __restrict__ X, int64_t N, const int64_t* __restrict__ ccolptr,
                                                  const int32_t* __restrict__ crowval, int64_t cnnz, double rt, double sp, double r,
                                                  double* __restrict__ cost, uint64_t* __restrict__ keep)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool k = false;
    if (e < cnnz) {
        int64_t lo = 0, hi = N;
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (ccolptr[mid] <= e) lo = mid; else hi = mid; }
        const int64_t j = lo, i = crowval[e];
        double c;
        if constexpr (KIND == 2) c = rs_cost(X + 3 * j, X + 3 * i, rt);
        else {
            car_step path[5];
            int L;
            c = car_steer<KIND>(X + 3 * i, X + 3 * j, rt, sp, path, L);
        }
        cost[e] = c;
        k = c <= r;
    }
    const unsigned long long bits = __ballot(k);
    if (lane == 0 && (e - lane) < cnnz) keep[(e - lane) >> 6] = bits;
}

__device__ __forceinline__ int popc_range(const uint64_t* __restrict__ keep, int64_t b, int64_t e)      // set bits in [b, e)
{
    int n = 0;
    for (int64_t w = b >> 6; w <= (e - 1) >> 6 && e > b; ++w) {
        uint64_t m = keep[w];
        if (w == (b >> 6)) m &= ~0ull << (b & 63);
        if (w == ((e - 1) >> 6) && ((e & 63) != 0)) m &= (1ull << (e & 63)) - 1ull;
        n += __popcll(m);
    }
    return n;
}

__global__ __launch_bounds__(256) void k_car_degree(const int64_t* __restrict__ ccolptr, const uint64_t* __restrict__ keep, int64_t N,
                                                    int64_t* __restrict__ deg)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < N) deg[j] = popc_range(keep, ccolptr[j], ccolptr[j + 1]);
}

// one wavefront per column: kept entries keep their (ascending) order
__global__ __launch_bounds__(64) void k_car_compact(const int64_t* __restrict__ ccolptr, const int32_t* __restrict__ crowval,
                                                    const double* __restrict__ cost, const uint64_t* __restrict__ keep, int64_t N,
                                                    const int64_t* __restrict__ colptr, int32_t* __restrict__ rowval, double* __restrict__ nzval)
{
    const int lane = threadIdx.x;
    for (int64_t j = blockIdx.x; j < N; j += gridDim.x) {
        const int64_t b = ccolptr[j], en = ccolptr[j + 1];
        int64_t out = colptr[j];
        for (int64_t e0 = b; e0 < en; e0 += 64) {
            const int64_t e = e0 + lane;
            const bool k = e < en && ((keep[e >> 6] >> (e & 63)) & 1ull);
            const unsigned long long m = __ballot(k);
            if (k) {
                const int64_t p = out + __popcll(m & ((1ull << lane) - 1ull));
                rowval[p] = crowval[e];
                nzval[p] = cost[e];
            }
            out += __popcll(m);
        }
    }
}

// lane = CSC entry (row y -> column x): bit = is_free_motion(V[y], V[x]), nseg = segment tests the reference would count
template <int KIND>
__global__ __launch_bounds__(256) void k_car_sweep(const double* __restrict__ X, int64_t N, const int64_t* __restrict__ colptr,
                                                   const int32_t* __restrict__ rowval, int64_t nnz, double rt, double sp,
                                                   mpfmt_ws2d cc, mpfmt_ss ss, uint64_t* __restrict__ mask,
                                                   uint8_t* __restrict__ nseg)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool fr = false;
    if (e < nnz) {
        int64_t lo = 0, hi = N;
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (colptr[mid] <= e) lo = mid; else hi = mid; }
        const int64_t x = lo, y = rowval[e];
        int ns = 0;
        fr = car_motion_free<KIND>(X + 3 * y, X + 3 * x, rt, sp, cc, ss, &ns);
        nseg[e] = (uint8_t)min(ns, 255);
    }
    const unsigned long long bits = __ballot(fr);
    if (lane == 0 && (e - lane) < nnz) mask[(e - lane) >> 6] = bits;
}

// ---- in-place box edits (steer_delta.h): add / remove on the flagged columns ---------------------------------------------------
// F(list) of an entry is car_motion_free with cc.boxes / cc.M pointed at that list: the delta boxes (from LDS when lds_delta, else
// from memory as the whole sweep reads its list) or the remaining list.  ctr[1] += entries whose F(delta) was evaluated.
#define CAR_DELTA_LDS_BOXES 512
template <int KIND, bool REMOVE>
__global__ __launch_bounds__(SD_THREADS) void k_car_delta(const double* __restrict__ X, const int64_t* __restrict__ colptr,
                                                         const int32_t* __restrict__ rowval, const int32_t* __restrict__ cols,
                                                         unsigned long long* __restrict__ ctr, const double* __restrict__ delta, int nd,
                                                         int lds_delta, const double* __restrict__ rem, int nrem, double rt, double sp,
                                                         mpfmt_ss ss, unsigned long long* __restrict__ mask, uint8_t* __restrict__ nseg)
{
    __shared__ __attribute__((aligned(16))) double sdel[CAR_DELTA_LDS_BOXES * 4];
    if (lds_delta) for (int t = threadIdx.x; t < nd * 4; t += blockDim.x) sdel[t] = delta[t];
    __syncthreads();
    mpfmt_ws2d cd, cr;
    cd.kind = 0; cd.boxes = lds_delta ? (const double*)sdel : delta; cd.M = nd; cd.shapes = nullptr; cd.ns = 0; cd.aabb = mpfmt_aabb2d();
    cr = cd; cr.boxes = rem; cr.M = nrem;
    const int lane = threadIdx.x & 63;
    const int64_t gwave = ((int64_t)blockIdx.x * SD_THREADS + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t)gridDim.x * (SD_THREADS / 64);
    const int64_t ncols = (int64_t)ctr[0];
    unsigned long long tested_n = 0;
    for (int64_t ci = gwave; ci < ncols; ci += nwaves) {
        const int64_t x = (int64_t)__builtin_amdgcn_readfirstlane(cols[ci]);
        const int64_t beg = colptr[x], end = colptr[x + 1];
        for (int64_t wd = beg >> 6; wd * 64 < end; ++wd) {
            const int64_t e = wd * 64 + lane;
            const unsigned long long cur = sd_word(mask, wd);
            const bool mine = e >= beg && e < end;
            const bool isfree = (cur >> lane) & 1ull;
            // add: every entry (a blocked one keeps its bit, but its count can drop); remove: free entries stay as they are
            const bool cand = REMOVE ? (mine && !isfree) : mine;
            if (__ballot(cand) == 0) continue;
            bool change = false;
            if (cand) {
                const int64_t y = rowval[e];
                int sd = 0;
                const bool fd = car_motion_free<KIND>(X + 3 * y, X + 3 * x, rt, sp, cd, ss, &sd);
                if (REMOVE) {
                    if (!fd) {                                 // from nothing against what is left
                        int sr = 0;
                        change = car_motion_free<KIND>(X + 3 * y, X + 3 * x, rt, sp, cr, ss, &sr);
                        nseg[e] = (uint8_t)min(sr, 255);
                    }
                } else {
                    const int old = (int)nseg[e];
                    sd = min(sd, 255);
                    if (sd < old) nseg[e] = (uint8_t)sd;
                    change = isfree && !fd;
                }
            }
            const unsigned long long ch = __ballot(change);
            if (lane == 0 && ch) {
                if (REMOVE) atomicOr(&mask[wd], ch); else atomicAnd(&mask[wd], ~ch);
            }
            tested_n += (unsigned long long)__popcll(__ballot(cand));
        }
    }
    if (lane == 0 && tested_n) atomicAdd(ctr + 1, tested_n);
}

// ---- in-place shape edits under the 2-D SAT world (steer_delta.h) ------------------------------------------------------
// The structure of k_car_delta; F(delta) is car_motion_free under the edit's delta predicate in the place of the segment test, and a
// remove's candidates are evaluated again by the whole sweep's own call against what remains.  Shapes are read at wave-uniform
// addresses as kernels_sat2d.hip reads them.  ctr[1] += entries whose walk under the delta predicate was evaluated.
template <int KIND, bool REMOVE>
__global__ __launch_bounds__(SD_THREADS) void k_car_sdelta(const double* __restrict__ X, const int64_t* __restrict__ colptr,
                                                          const int32_t* __restrict__ rowval, const int32_t* __restrict__ cols,
                                                          unsigned long long* __restrict__ ctr, sd_shapes_edit E, double rt, double sp,
                                                          mpfmt_ss ss, unsigned long long* __restrict__ mask, uint8_t* __restrict__ nseg)
{
    mpfmt_ws2d cc;                                           // what remains (remove) -- kind 1 also routes the walk to the predicate
    cc.kind = 1; cc.boxes = nullptr; cc.M = 0; cc.shapes = E.list; cc.ns = E.nl; cc.aabb = E.Bnew;
    const int lane = threadIdx.x & 63;
    const int64_t gwave = ((int64_t)blockIdx.x * SD_THREADS + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t)gridDim.x * (SD_THREADS / 64);
    const int64_t ncols = (int64_t)ctr[0];
    unsigned long long tested_n = 0;
    for (int64_t ci = gwave; ci < ncols; ci += nwaves) {
        const int64_t x = (int64_t)__builtin_amdgcn_readfirstlane(cols[ci]);
        const int64_t beg = colptr[x], end = colptr[x + 1];
        for (int64_t wd = beg >> 6; wd * 64 < end; ++wd) {
            const int64_t e = wd * 64 + lane;
            const unsigned long long cur = sd_word(mask, wd);
            const bool mine = e >= beg && e < end;
            const bool isfree = (cur >> lane) & 1ull;
            const bool cand = REMOVE ? (mine && !isfree) : mine;
            if (__ballot(cand) == 0) continue;
            bool change = false;
            if (cand) {
                const int64_t y = rowval[e];
                int sd = 0;
                if (REMOVE) {
                    const bool fd = car_motion_free<KIND>(X + 3 * y, X + 3 * x, rt, sp, cc, ss, &sd, seg_shapes_remove{E});
                    if (!fd) {                                 // from nothing against what is left
                        int sr = 0;
                        change = car_motion_free<KIND>(X + 3 * y, X + 3 * x, rt, sp, cc, ss, &sr);
                        nseg[e] = (uint8_t)min(sr, 255);
                    }
                } else {
                    const bool fd = car_motion_free<KIND>(X + 3 * y, X + 3 * x, rt, sp, cc, ss, &sd, seg_shapes_add{E});
                    const int old = (int)nseg[e];
                    sd = min(sd, 255);
                    if (sd < old) nseg[e] = (uint8_t)sd;
                    change = isfree && !fd;
                }
            }
            const unsigned long long ch = __ballot(change);
            if (lane == 0 && ch) {
                if (REMOVE) atomicOr(&mask[wd], ch); else atomicAnd(&mask[wd], ~ch);
            }
            tested_n += (unsigned long long)__popcll(__ballot(cand));
        }
    }
    if (lane == 0 && tested_n) atomicAdd(ctr + 1, tested_n);
}

// ---- external states on the resident graph (steer_roadmap.h) ---------------------------------------------------------
// One wavefront per query state q: the entries q would have had as a sample.  Dense loop: the positions fold of the candidate graph
// (d2 <= r * r, the canonical 2-D fold -- exact, so it is also the first membership test).  Survivors, 64 at a time: the cost of
// k_car_cost in the build's direction -- head (dir 1): Dubins steer(V[y] -> q), Reeds-Shepp rs_cost(q, V[y]); tail: Dubins
// steer(q -> V[y]), Reeds-Shepp rs_cost(V[y], q) --, cost <= r, and in modes 1 and 2 the whole sweep's car_motion_free from the row
// to the column (head: V[y] -> q, tail: q -> V[y]).  Boxes are read through mpfmt_ws2d as k_car_sweep reads them.
template <int KIND>
__global__ __launch_bounds__(SRM_WAVES * 64) void k_car_roadmap(srm_args a, mpfmt_ws2d cc, mpfmt_ss ss)
{
    __shared__ int32_t s_q[SRM_WAVES][SRM_QCAP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t qi = (int64_t)blockIdx.x * SRM_WAVES + wv;
    if (qi >= a.nq) return;
    const double q[3] = {a.Q[3 * qi], a.Q[3 * qi + 1], a.Q[3 * qi + 2]};
    const double r2 = a.r * a.r;
    auto pre = [&](int64_t y) -> bool {
        const double t0 = q[0] - a.X[3 * y], t1 = q[1] - a.X[3 * y + 1];
        const double tt0 = t0 * t0, tt1 = t1 * t1;
        return tt0 + tt1 <= r2;
    };
    auto exact = [&](int64_t y, bool motion, double& w, bool& fr, int& st) -> bool {
        const double v[3] = {a.X[3 * y], a.X[3 * y + 1], a.X[3 * y + 2]};
        const double* from = a.dir ? v : q;
        const double* to = a.dir ? q : v;
        double c;
        if constexpr (KIND == 2) c = a.dir ? rs_cost(q, v, a.rt) : rs_cost(v, q, a.rt);
        else {
            car_step path[5];
            int L;
            c = car_steer<KIND>(from, to, a.rt, a.sp, path, L);
        }
        st = 1;
        if (!(c <= a.r)) return false;
        w = c;
        if (motion) {
            int ns = 0;
            fr = car_motion_free<KIND>(from, to, a.rt, a.sp, cc, ss, &ns);
        }
        return true;
    };
    srm_wave(a, qi, lane, s_q[wv], pre, exact);
}

// controls: [n][5][3] = (duration, speed, signed curvature), unused segments zero; nseg[i] = segments used
template <int KIND>
__global__ __launch_bounds__(256) void k_car_steer(const double* __restrict__ X0, const double* __restrict__ X1, int64_t n, double rt,
                                                   double sp, double* __restrict__ cost, double* __restrict__ ctrl, int32_t* __restrict__ nseg)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    car_step path[5];
    int L;
    cost[i] = car_steer<KIND>(X0 + 3 * i, X1 + 3 * i, rt, sp, path, L);
    for (int q = 0; q < 5; ++q) { ctrl[15 * i + 3 * q] = path[q].t; ctrl[15 * i + 3 * q + 1] = path[q].s; ctrl[15 * i + 3 * q + 2] = path[q].k; }
    if (nseg) nseg[i] = L;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static int32_t car_check(mpfmt_ctx* ctx, double rt, double sp, double r)
{
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (ctx->d != 3) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "Dubins states are SE2 (x, y, theta): state dimension must be 3 (got %d)", ctx->d);
    if (!(rt > 0.0) || !std::isfinite(rt) || !(sp > 0.0) || !std::isfinite(sp)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "turning radius and speed must be finite and > 0");
    if (!(r > 0.0) || !std::isfinite(r)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "cost radius must be finite and > 0");
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the Dubins build needs an unsharded ctx");
    return MPFMT_OK;
}

static int32_t car_scan(mpfmt_ctx* ctx, const int64_t* in, int64_t* out, size_t n) { return mpfmt_scan_i64(ctx, in, out, n); }

int32_t mpfmt_car_build(mpfmt_ctx* ctx, mpfmt_steer kind, double rt, double sp, double r)
{
    int32_t rc;
    if ((rc = car_check(ctx, rt, sp, r))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t N = ctx->N;
    // (1) Euclidean r-disc graph of the positions in a helper ctx (same device)
    if (!ctx->aux && (rc = mpfmt_ctx_create(ctx->device, &ctx->aux))) return mpfmt_fail(ctx, rc, "helper ctx: %s", mpfmt_last_error(nullptr));
    mpfmt_ctx* ax = ctx->aux;
    {
        std::vector<double> Xh, xy;
        if ((rc = mpfmt_states_host(ctx, 2, Xh, xy))) return rc;
        if ((rc = mpfmt_upload_samples(ax, xy.data(), N, 2))) return mpfmt_fail(ctx, rc, "helper ctx: %s", mpfmt_last_error(ax));
    }
    int64_t cnnz = 0;
    if ((rc = mpfmt_graph_build_device(ax, r, &cnnz))) return mpfmt_fail(ctx, rc, "helper ctx: %s", mpfmt_last_error(ax));
    HIPCHK(ctx, hipStreamSynchronize(ax->stream));
    // (2) exact Dubins cost per candidate edge
    mpfmt_timed tm1(ctx);
    const int64_t cw = (cnnz + 63) / 64;
    if ((rc = ctx->valtmp.ensure(ctx, sizeof(double) * (size_t)std::max<int64_t>(cnnz, 1)))) return rc;
    if ((rc = ctx->car_keep.ensure(ctx, sizeof(uint64_t) * (size_t)std::max<int64_t>(cw, 1)))) return rc;
    if ((rc = ctx->deg.ensure(ctx, sizeof(int64_t) * (size_t)(N + 1)))) return rc;
    if ((rc = ctx->colptr.ensure(ctx, sizeof(int64_t) * (size_t)(N + 1)))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->deg, 0, sizeof(int64_t) * (size_t)(N + 1), ctx->stream));
    ctx->deg_zero_valid = false;
    if (cnnz > 0) {
        if (kind == MPFMT_STEER_REEDSSHEPP)
            hipLaunchKernelGGL(k_car_cost<2>, dim3((unsigned)((cnnz + 255) / 256)), dim3(256), 0, ctx->stream, ctx->Xo, N, ax->colptr, ax->rowval,
                               cnnz, rt, sp, r, ctx->valtmp, ctx->car_keep);
        else
            hipLaunchKernelGGL(k_car_cost<1>, dim3((unsigned)((cnnz + 255) / 256)), dim3(256), 0, ctx->stream, ctx->Xo, N, ax->colptr, ax->rowval,
                               cnnz, rt, sp, r, ctx->valtmp, ctx->car_keep);
        hipLaunchKernelGGL(k_car_degree, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, ax->colptr, ctx->car_keep, N, ctx->deg);
        HIPCHK(ctx, hipGetLastError());
    }
    if ((rc = car_scan(ctx, ctx->deg, ctx->colptr, (size_t)(N + 1)))) return rc;
    int64_t nnz = 0;
    HIPCHK(ctx, hipMemcpyAsync(&nnz, ctx->colptr + N, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // (3) ordered compaction
    if ((rc = ctx->rowval.ensure(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(nnz, 1)))) return rc;
    if ((rc = ctx->nzval.ensure(ctx, sizeof(double) * (size_t)std::max<int64_t>(nnz, 1)))) return rc;
    if (cnnz > 0) {
        hipLaunchKernelGGL(k_car_compact, dim3((unsigned)std::min<int64_t>(N, 1 << 20)), dim3(64), 0, ctx->stream, ax->colptr, ax->rowval,
                           ctx->valtmp, ctx->car_keep, N, ctx->colptr, ctx->rowval, ctx->nzval);
        HIPCHK(ctx, hipGetLastError());
    }
    tm1.end("car_graph");
    ctx->nnz = nnz;
    ctx->pairs_tested = cnnz;
    ctx->car_rt = rt; ctx->car_sp = sp; ctx->steer_r = r;
    ctx->steer_kind = kind;
    ctx->steer_counted = ctx->steer_filled = true; ctx->steer_swept = false; ctx->steer_epoch += 1;
    ctx->graph_r = -1.0; ctx->graph_counted = ctx->graph_filled = ctx->graph_swept = false; ctx->knn_k = 0;
    return MPFMT_OK;
}

int32_t mpfmt_car_sweep(mpfmt_ctx* ctx)
{
    if (!(ctx->steer_filled && ctx->steer_kind != MPFMT_STEER_DI)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "car sweep before the car graph is built");
    if (!ctx->have_boxes || ctx->dw != 2)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the car sweep needs a 2-D workspace checker (mpfmt_upload_boxes with dw = 2, or mpfmt_upload_shapes2d) and the 3 SE2 bounds");
    mpfmt_ws2d cc;
    cc.kind = ctx->cc_kind; cc.boxes = ctx->boxes; cc.M = ctx->cc_kind == 0 ? ctx->M : 0;
    cc.shapes = ctx->shapes2d; cc.ns = ctx->cc_kind == 1 ? ctx->M : 0; cc.aabb = ctx->aabb2d;
    if (ctx->ss.has && ctx->ss.d != 3) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "state-space bounds must have 3 dims for SE2 states");
    int32_t rc;
    const int64_t nnz = ctx->nnz, words = (nnz + 63) / 64;
    if ((rc = ctx->graph_free.ensure(ctx, sizeof(uint64_t) * (size_t)std::max<int64_t>(words, 1)))) return rc;
    if ((rc = ctx->steer_nseg.ensure(ctx, (size_t)std::max<int64_t>(nnz, 1)))) return rc;
    mpfmt_timed tm2(ctx);
    HIPCHK(ctx, hipMemsetAsync(ctx->graph_free, 0, sizeof(uint64_t) * (size_t)std::max<int64_t>(words, 1), ctx->stream));
    if (nnz > 0) {
        if (ctx->steer_kind == MPFMT_STEER_REEDSSHEPP)
            hipLaunchKernelGGL(k_car_sweep<2>, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, ctx->stream, ctx->Xo, ctx->N, ctx->colptr,
                               ctx->rowval, nnz, ctx->car_rt, ctx->car_sp, cc, ctx->ss, ctx->graph_free, ctx->steer_nseg);
        else
            hipLaunchKernelGGL(k_car_sweep<1>, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, ctx->stream, ctx->Xo, ctx->N, ctx->colptr,
                               ctx->rowval, nnz, ctx->car_rt, ctx->car_sp, cc, ctx->ss, ctx->graph_free, ctx->steer_nseg);
        HIPCHK(ctx, hipGetLastError());
    }
    tm2.end("car_sweep");
    ctx->steer_swept = true; ctx->steer_sweep_epoch += 1;
    return MPFMT_OK;
}

// flag + update on ctx->stream for a resident, swept car graph: d_delta = the nd boxes added (already at the end of ctx->boxes) or a
// copy of the nd boxes removed (ctx->boxes / ctx->M: the remaining list).  The caller owns bd_cols / bd_ctr.
// Column cull: every waypoint lies on the steered path, no farther along it from the column's position than the
// path is long, and the graph keeps length = cost <= steer_r.
int32_t mpfmt_car_delta_launch(mpfmt_ctx* ctx, const double* d_delta, int32_t nd, bool remove)
{
    const int64_t N = ctx->N;
    const unsigned nbf = (unsigned)((N + SD_THREADS - 1) / SD_THREADS), nbu = sd_update_blocks(ctx);
    const double rpad = ctx->steer_r * (1.0 + 1e-6) + 1e-300;
    const int lds_delta = nd <= CAR_DELTA_LDS_BOXES ? 1 : 0;
    const int nrem = remove ? ctx->M : 0;
    const double* rem = remove ? (const double*)ctx->boxes.get() : nullptr;
    unsigned long long* mask = (unsigned long long*)ctx->graph_free.get();
    hipLaunchKernelGGL((k_sd_flag<3, 2, false>), dim3(nbf), dim3(SD_THREADS), 0, ctx->stream, ctx->Xo, N, d_delta, (int)nd, rpad, 0.0,
                       ctx->bd_cols, ctx->bd_ctr);
#define CAR_DELTA_GO(KIND, REM)                                                                                                       \
    hipLaunchKernelGGL((k_car_delta<KIND, REM>), dim3(nbu), dim3(SD_THREADS), 0, ctx->stream, ctx->Xo, ctx->colptr, ctx->rowval, ctx->bd_cols, \
                       ctx->bd_ctr, d_delta, (int)nd, lds_delta, rem, nrem, ctx->car_rt, ctx->car_sp, ctx->ss, mask, ctx->steer_nseg)
    if (ctx->steer_kind == MPFMT_STEER_REEDSSHEPP) { if (remove) CAR_DELTA_GO(2, true); else CAR_DELTA_GO(2, false); }
    else { if (remove) CAR_DELTA_GO(1, true); else CAR_DELTA_GO(1, false); }
#undef CAR_DELTA_GO
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

// the same for an edit of the shape list of the 2-D SAT world: d_delta = the nd shapes added (the tail of ctx->shapes2d) or a copy of
// the nd shapes removed; Bold / M_before: the compound box and the list length before the edit
int32_t mpfmt_car_sdelta_launch(mpfmt_ctx* ctx, const mpfmt_shape2d* d_delta, int32_t nd, bool remove, const mpfmt_aabb2d& Bold, int32_t M_before)
{
    const int64_t N = ctx->N;
    sd_shapes_edit E;
    int rule_b;
    mpfmt_aabb2d small;
    sd_shapes_edit_of(ctx, d_delta, nd, remove, Bold, M_before, E, rule_b, small);
    const unsigned nbf = (unsigned)((N + SD_THREADS - 1) / SD_THREADS), nbu = sd_update_blocks(ctx);
    const double rpad = ctx->steer_r * (1.0 + 1e-6) + 1e-300;
    unsigned long long* mask = (unsigned long long*)ctx->graph_free.get();
    hipLaunchKernelGGL((k_sd_flag_shapes<3, false>), dim3(nbf), dim3(SD_THREADS), 0, ctx->stream, ctx->Xo, N, d_delta, (int)nd, rpad, 0.0, rule_b,
                       small, ctx->bd_cols, ctx->bd_ctr);
#define CAR_SDELTA_GO(KIND, REM)                                                                                                      \
    hipLaunchKernelGGL((k_car_sdelta<KIND, REM>), dim3(nbu), dim3(SD_THREADS), 0, ctx->stream, ctx->Xo, ctx->colptr, ctx->rowval, ctx->bd_cols, \
                       ctx->bd_ctr, E, ctx->car_rt, ctx->car_sp, ctx->ss, mask, ctx->steer_nseg)
    if (ctx->steer_kind == MPFMT_STEER_REEDSSHEPP) { if (remove) CAR_SDELTA_GO(2, true); else CAR_SDELTA_GO(2, false); }
    else { if (remove) CAR_SDELTA_GO(1, true); else CAR_SDELTA_GO(1, false); }
#undef CAR_SDELTA_GO
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

// external states on the resident car graph: a.Q / nq / dir / mode / X / N / pair and the outputs are the caller's
int32_t mpfmt_car_roadmap_launch(mpfmt_ctx* ctx, srm_args& a)
{
    a.r = ctx->steer_r; a.rt = ctx->car_rt; a.sp = ctx->car_sp;
    a.rho = a.i2 = a.i3 = a.i4 = a.r2 = 0.0;
    a.boxes = ctx->boxes; a.M = ctx->M; a.stage = 0;
    mpfmt_ws2d cc;
    cc.kind = 0; cc.boxes = ctx->boxes; cc.M = ctx->M; cc.shapes = nullptr; cc.ns = 0; cc.aabb = ctx->aabb2d;
    const unsigned nb = (unsigned)((a.nq + SRM_WAVES - 1) / SRM_WAVES);
    if (ctx->steer_kind == MPFMT_STEER_REEDSSHEPP) hipLaunchKernelGGL(k_car_roadmap<2>, dim3(nb), dim3(SRM_WAVES * 64), 0, ctx->stream, a, cc, ctx->ss);
    else hipLaunchKernelGGL(k_car_roadmap<1>, dim3(nb), dim3(SRM_WAVES * 64), 0, ctx->stream, a, cc, ctx->ss);
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

int32_t mpfmt_car_steer_batch(mpfmt_ctx* ctx, mpfmt_steer kind, const double* d_X0, const double* d_X1, int64_t n, double rt, double sp, double* d_cost,
                              double* d_ctrl, int32_t* d_nseg)
{
    if (kind == MPFMT_STEER_REEDSSHEPP) hipLaunchKernelGGL(k_car_steer<2>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_X0, d_X1, n, rt, sp, d_cost, d_ctrl, d_nseg);
    else hipLaunchKernelGGL(k_car_steer<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_X0, d_X1, n, rt, sp, d_cost, d_ctrl, d_nseg);
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}
