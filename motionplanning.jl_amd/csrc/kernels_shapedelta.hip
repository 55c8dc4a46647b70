// In-place update of the resident free-edge mask when shapes are added to or removed from the 2-D SAT world (PointRobot2D over
// Circle / convex Polygon parts, kernels_sat2d.hip) (gfx950): mpfmt_shapes2d_add / mpfmt_shapes2d_remove.
//
// The bit k2d_graph writes for entry e (row y in column x, segment (v, w) = (V[y], V[x])) under the list L with compound box B(L) is
//   bit(e, L)  = in_ss_2d(v) && ( gate(e, B(L)) || !exists S in L: line_hits(v, w, S) )
//   gate(e, B) = the segment's bounding box does not overlap B                                  (motion_free_2d)
// The gate is NOT inert in floating point: point_hits of a circle has no box test, and an endpoint one ulp outside the circle's own box
// can still round to fl(px - cx) == -r, so a shape can "hit" a segment that the gate calls free.  "old AND free against the added
// shapes" is therefore wrong, and an edit that moves the compound box changes bits far from the edited shape.  The rules that give
// bit(e, L') exactly (DESIGN.md 7o has the case analysis); an EMPTY list counts as "gate always true, nothing hits":
//   add    (L' = L ++ added, B <= B'):  a blocked entry stays blocked.  A free entry: gate(e, B') -> keep; else an added shape hits
//          -> clear; else, when the compound box changed and L is not empty, gate(e, B) held (the old bit was the gate's, not the
//          shapes') -> clear if a shape of L hits; else keep.
//   remove (L' <= L, B' <= B):  a free entry stays free.  A blocked entry with in_ss_2d(v): gate(e, B') -> set; else a removed shape
//          hits (the exact line_hits) -> evaluated again against all of L'; else keep.
// The predicates are those of sat2d_predicates.h, unchanged (same operations, same order, unfused): the result is the mask a whole
// sweep of the resulting list writes, bit for bit.
//
// Column cull (k_sd_flag, lane = column, one ballot and one atomic per wavefront): column x is visited when
//   (a) V[x] lies within rpad = graph_r (1 + 1e-9) + 1e-300 of a delta shape's box on both axes (every entry of an r-disc column is
//       no longer than graph_r; the circle tie lies less than an ulp outside the box, which the 1e-9 r margin covers), or
//   (b) the edit changes the compound box bitwise and the list on the SMALLER side of the edit (L for add, L' for remove) is not
//       empty, and V[x] is not inside that smaller box: an entry whose bit follows the gate alone has its whole segment box clear of
//       the smaller compound box on one axis, so both its ends lie outside it.
// Both tests are written "not (...)" so that a NaN coordinate is visited.  A k-nearest graph has no length bound: all columns.
//
// Update kernels: the structure of kernels_boxdelta.hip -- a wavefront takes a flagged column and walks the mask WORDS its run touches,
// lane = bit; the first and last word of a run are shared with the neighbouring columns, so a word is never stored: the change of
// its 64 entries is one ballot applied with one 64-bit atomicAnd (add) / atomicOr (remove) from lane 0.
// Shapes (800 B each) are read at wave-uniform addresses, i.e. through the scalar cache, exactly as kernels_sat2d.hip reads them:
// line_hits / point_hits take a shape pointer and are used as they stand, and a polygon's loops run over S->n, which a staged LDS copy
// would have to carry through generic pointers (flat loads) for no traffic saved -- the delta lists are a few shapes.
#include <algorithm>
#include <cstring>
#include "mpfmt_internal.h"
#include "sat2d_predicates.h"

#define SD_THREADS 256

__device__ __forceinline__ int sd_lane_rank(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the word of the mask as it is NOW (device scope: not a line an earlier stage left in this CU's vector cache)
__device__ __forceinline__ unsigned long long sd_word(const unsigned long long* mask, int64_t wd)
{
    return __hip_atomic_load(mask + wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// gate(e, B) of motion_free_2d, on the segment box it computes
__device__ __forceinline__ bool sd_gate(double vx, double vy, double wx, double wy, const mpfmt_aabb2d& B)
{
    const double lx0 = (vx < wx) ? vx : wx, lx1 = (vx < wx) ? wx : vx;
    const double ly0 = (vy < wy) ? vy : wy, ly1 = (vy < wy) ? wy : vy;
    return !(overlapping(B.xr[0], B.xr[1], lx0, lx1) && overlapping(B.yr[0], B.yr[1], ly0, ly1));
}

// does a shape of S[0 .. ns) hit the segment, for the lanes in `on` (wave-uniform k: scalar loads of the shape)
__device__ __forceinline__ bool sd_any_hits(bool on, double vx, double vy, double wx, double wy, const mpfmt_shape2d* __restrict__ S, int ns)
{
    bool hit = false;
    for (int k = 0; k < ns; ++k) {
        const bool pend = on & !hit;
        if (__ballot(pend) == 0) break;
        if (pend) hit = line_hits(vx, vy, wx, wy, S + k);
    }
    return hit;
}

// ---- column cull -----------------------------------------------------------------------------------------------------------
// cols[0 .. ctr[0]) = the flagged columns (any order); cull == 0: all columns.  delta: the nd shapes added or removed; rule_b != 0:
// columns outside `small` (the compound box of the smaller side of the edit) are flagged too
__global__ __launch_bounds__(SD_THREADS) void k_sd_flag(const double* __restrict__ X, int64_t N, const mpfmt_shape2d* __restrict__ delta, int nd,
                                                       double rpad, int cull, int rule_b, mpfmt_aabb2d small, int32_t* __restrict__ cols,
                                                       unsigned long long* __restrict__ ctr)
{
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * SD_THREADS + threadIdx.x;
    const bool in = x < N;
    const double px = in ? X[2 * x] : 0.0, py = in ? X[2 * x + 1] : 0.0;
    int flag = cull ? 0 : 1;
    if (cull) {
        for (int k = 0; k < nd; ++k) {
            const mpfmt_shape2d* S = delta + k;                // wave-uniform
            // NaN: neither comparison holds -> not outside -> visited
            const int out = (int)(px < S->xr[0] - rpad) | (int)(px > S->xr[1] + rpad) | (int)(py < S->yr[0] - rpad) | (int)(py > S->yr[1] + rpad);
            flag |= !out;
        }
        if (rule_b) flag |= !(ininterval(px, small.xr[0], small.xr[1]) && ininterval(py, small.yr[0], small.yr[1]));
    }
    const unsigned long long m = __ballot(in && flag);
    if (m == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    if (in && flag) cols[base + sd_lane_rank(m)] = (int32_t)x;
}

// ---- add -------------------------------------------------------------------------------------------------------------------
// shapes: the NEW list, M_old shapes of the old one followed by the nd added; Bold / Bnew: the compound boxes; walk_old != 0: the
// compound box changed and the old list is not empty (the third clause of the add rule exists)
__global__ __launch_bounds__(SD_THREADS) void k_sd_add(const double* __restrict__ X, const int64_t* __restrict__ colptr,
                                                      const int32_t* __restrict__ rowval, const int32_t* __restrict__ cols,
                                                      unsigned long long* __restrict__ ctr, const mpfmt_shape2d* __restrict__ shapes, int M_old,
                                                      int nd, mpfmt_aabb2d Bold, mpfmt_aabb2d Bnew, int walk_old,
                                                      unsigned long long* __restrict__ mask)
{
    const int lane = threadIdx.x & 63;
    const int64_t gwave = ((int64_t)blockIdx.x * SD_THREADS + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t)gridDim.x * (SD_THREADS / 64);
    const int64_t ncols = (int64_t)ctr[0];
    unsigned long long reached_n = 0;
    for (int64_t ci = gwave; ci < ncols; ci += nwaves) {
        const int64_t x = (int64_t)__builtin_amdgcn_readfirstlane(cols[ci]);
        const int64_t beg = colptr[x], end = colptr[x + 1];
        const double wx = X[2 * x], wy = X[2 * x + 1];
        for (int64_t wd = beg >> 6; wd * 64 < end; ++wd) {
            const int64_t e = wd * 64 + lane;
            const unsigned long long cur = sd_word(mask, wd);
            const bool cand = e >= beg && e < end && ((cur >> lane) & 1ull);          // blocked entries stay blocked
            if (__ballot(cand) == 0) continue;
            const int64_t y = cand ? (int64_t)rowval[e] : x;
            const double vx = X[2 * y], vy = X[2 * y + 1];
            const bool reach = cand && !sd_gate(vx, vy, wx, wy, Bnew);                // gate(e, B') holds: the bit stays
            if (__ballot(reach) == 0) continue;
            bool hit = sd_any_hits(reach, vx, vy, wx, wy, shapes + M_old, nd);
            if (walk_old) {                                                          // the old bit was the gate's, not the shapes'
                const bool again = reach && !hit && sd_gate(vx, vy, wx, wy, Bold);
                if (__ballot(again)) hit |= sd_any_hits(again, vx, vy, wx, wy, shapes, M_old);
            }
            const unsigned long long clr = __ballot(reach && hit);
            if (lane == 0 && clr) atomicAnd(&mask[wd], ~clr);
            reached_n += (unsigned long long)__popcll(__ballot(reach));
        }
    }
    if (lane == 0 && reached_n) atomicAdd(ctr + 1, reached_n);
}

// ---- remove ----------------------------------------------------------------------------------------------------------------
// removed: a copy of the nr shapes taken out; shapes / M: the remaining list with its compound box Bnew (M == 0: the gate always holds)
__global__ __launch_bounds__(SD_THREADS) void k_sd_remove(const double* __restrict__ X, const int64_t* __restrict__ colptr,
                                                         const int32_t* __restrict__ rowval, const int32_t* __restrict__ cols,
                                                         unsigned long long* __restrict__ ctr, const mpfmt_shape2d* __restrict__ removed, int nr,
                                                         const mpfmt_shape2d* __restrict__ shapes, int M, mpfmt_aabb2d Bnew, mpfmt_ss ss,
                                                         unsigned long long* __restrict__ mask)
{
    const int lane = threadIdx.x & 63;
    const int64_t gwave = ((int64_t)blockIdx.x * SD_THREADS + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t)gridDim.x * (SD_THREADS / 64);
    const int64_t ncols = (int64_t)ctr[0];
    unsigned long long reached_n = 0;
    for (int64_t ci = gwave; ci < ncols; ci += nwaves) {
        const int64_t x = (int64_t)__builtin_amdgcn_readfirstlane(cols[ci]);
        const int64_t beg = colptr[x], end = colptr[x + 1];
        const double wx = X[2 * x], wy = X[2 * x + 1];
        for (int64_t wd = beg >> 6; wd * 64 < end; ++wd) {
            const int64_t e = wd * 64 + lane;
            const unsigned long long cur = sd_word(mask, wd);
            bool cand = e >= beg && e < end && !((cur >> lane) & 1ull);               // free entries stay free
            if (__ballot(cand) == 0) continue;
            const int64_t y = cand ? (int64_t)rowval[e] : x;
            const double vx = X[2 * y], vy = X[2 * y + 1];
            cand = cand && in_ss_2d(vx, vy, ss);                                      // a row outside the bounds stays blocked
            const bool gate = cand && (M == 0 || sd_gate(vx, vy, wx, wy, Bnew));      // gate(e, B') holds: free
            const bool reach = cand && !gate;
            bool fr = gate;
            if (__ballot(reach)) {
                const bool again = sd_any_hits(reach, vx, vy, wx, wy, removed, nr);   // a candidate: evaluated again from nothing
                if (__ballot(again)) fr |= again && !sd_any_hits(again, vx, vy, wx, wy, shapes, M);
            }
            const unsigned long long set = __ballot(fr);
            if (lane == 0 && set) atomicOr(&mask[wd], set);
            reached_n += (unsigned long long)__popcll(__ballot(reach));
        }
    }
    if (lane == 0 && reached_n) atomicAdd(ctr + 1, reached_n);
}

// the resident mask of a swept, unsharded Euclidean graph brought up to date on ctx->stream.  ctx->shapes2d / M / aabb2d: the
// resulting list; d_delta: the nd shapes added (the tail of ctx->shapes2d) or a copy of the nd shapes removed; Bold: the compound box
// before the edit, M_before the list length before it
static int32_t shapedelta_apply(mpfmt_ctx* ctx, const mpfmt_shape2d* d_delta, int32_t nd, bool remove, const mpfmt_aabb2d& Bold, int32_t M_before)
{
    int32_t rc;
    if ((rc = mpfmt_side_join(ctx))) return rc;
    if ((rc = ctx->bd_cols.ensure(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(ctx->N, 1)))) return rc;
    if ((rc = ctx->bd_ctr.ensure(ctx, sizeof(unsigned long long) * 2))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->bd_ctr, 0, sizeof(unsigned long long) * 2, ctx->stream));
    // "no entry longer than graph_r" holds for the r-disc graphs (built here or imported with their radius); the columns of a k-nearest
    // graph are all visited
    const int cull = (ctx->knn_k == 0 && ctx->graph_r >= 0.0) ? 1 : 0;
    const double rpad = ctx->graph_r * (1.0 + 1e-9) + 1e-300;
    const mpfmt_aabb2d Bnew = ctx->aabb2d;
    const bool moved = memcmp(&Bold, &Bnew, sizeof(mpfmt_aabb2d)) != 0;              // bitwise: -0.0 and 0.0 differ, which only visits more
    const int32_t M_small = remove ? ctx->M : M_before;
    const int rule_b = (moved && M_small > 0) ? 1 : 0;
    const mpfmt_aabb2d small = remove ? Bnew : Bold;
    const int64_t N = ctx->N;
    mpfmt_timed tm(ctx);
    hipLaunchKernelGGL(k_sd_flag, dim3((unsigned)((N + SD_THREADS - 1) / SD_THREADS)), dim3(SD_THREADS), 0, ctx->stream, ctx->Xo, N, d_delta,
                       nd, rpad, cull, rule_b, small, ctx->bd_cols.get(), ctx->bd_ctr.get());
    HIPCHK(ctx, hipGetLastError());
    // one wavefront per flagged column, at most a resident set (the count lives on the device: wavefronts beyond it leave at once)
    const int64_t waves = SD_THREADS / 64;
    const unsigned nbu = (unsigned)std::max<int64_t>(1, std::min<int64_t>((N + waves - 1) / waves, (int64_t)ctx->num_cus * 8));
    unsigned long long* mask = (unsigned long long*)ctx->graph_free.get();
    if (remove)
        hipLaunchKernelGGL(k_sd_remove, dim3(nbu), dim3(SD_THREADS), 0, ctx->stream, ctx->Xo, ctx->colptr, ctx->rowval, ctx->bd_cols.get(),
                           ctx->bd_ctr.get(), d_delta, nd, ctx->shapes2d.get(), ctx->M, Bnew, ctx->ss, mask);
    else
        hipLaunchKernelGGL(k_sd_add, dim3(nbu), dim3(SD_THREADS), 0, ctx->stream, ctx->Xo, ctx->colptr, ctx->rowval, ctx->bd_cols.get(),
                           ctx->bd_ctr.get(), ctx->shapes2d.get(), M_before, nd, Bold, Bnew, rule_b, mask);
    HIPCHK(ctx, hipGetLastError());
    tm.end("shapes_delta");
    unsigned long long h[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h, ctx->bd_ctr, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->bd_columns = (int64_t)h[0]; ctx->bd_entries = (int64_t)h[1];
    return MPFMT_OK;
}

// the mask can be brought up to date instead of being thrown away: an unsharded ctx, a filled and swept Euclidean graph (r-disc,
// imported, k-nearest; a steering build clears graph_filled), no speculative step in flight
static bool shapes_delta_in_place(const mpfmt_ctx* ctx)
{
    return ctx->world == 1 && ctx->cc_kind == 1 && ctx->d == 2 && !ctx->steer_filled && ctx->graph_filled && ctx->graph_swept && ctx->nnz > 0 &&
           ctx->graph_free && ctx->step_state != 1;
}

// the same for a resident, swept steering graph (double integrator in R^4, cars) when the ctx opted in (option "steer_shapes_delta"):
// mask and segment counts follow (steer_delta.h).  The conditions are those under which the space's whole sweep would
// accept the resulting list.
static bool steer_shapes_delta_in_place(const mpfmt_ctx* ctx)
{
    if (!(ctx->steer_shapes_delta && ctx->world == 1 && ctx->cc_kind == 1 && ctx->dw == 2 && ctx->steer_filled && ctx->steer_swept && ctx->nnz > 0 &&
          ctx->graph_free && ctx->steer_nseg))
        return false;
    if (ctx->steer_kind == MPFMT_STEER_DI) return ctx->d == 4 && (!ctx->ss.has || ctx->ss.d == 4);
    return ctx->d == 3 && (!ctx->ss.has || ctx->ss.d == 3);
}

static int32_t steer_shapedelta_apply(mpfmt_ctx* ctx, const mpfmt_shape2d* d_delta, int32_t nd, bool remove, const mpfmt_aabb2d& Bold, int32_t M_before)
{
    return mpfmt_steer_delta_run(ctx, [&]() {
        return ctx->steer_kind == MPFMT_STEER_DI ? mpfmt_di_sdelta_launch(ctx, d_delta, nd, remove, Bold, M_before)
                                                 : mpfmt_car_sdelta_launch(ctx, d_delta, nd, remove, Bold, M_before);
    });
}

// the list has been edited: the mask follows in place or goes stale, as after an upload
static int32_t shapes_delta_finish(mpfmt_ctx* ctx, const mpfmt_shape2d* d_delta, int32_t nd, bool remove, const mpfmt_aabb2d& Bold, int32_t M_before)
{
    ctx->bd_columns = ctx->bd_entries = 0;
    ctx->pend_valid = false;
    if (steer_shapes_delta_in_place(ctx)) {                  // (a steering graph is resident: the Euclidean graph state is not)
        ctx->bd_path = 1;
        ctx->graph_swept = false;
        const int32_t rc = steer_shapedelta_apply(ctx, d_delta, nd, remove, Bold, M_before);
        if (rc) { ctx->steer_swept = false; ctx->bd_path = 0; return rc; }   // (the list stands, the mask is swept again)
        return mpfmt_togo_mark_dirty(ctx);                   // (a tracked cost-to-go field learns which columns the edit read)
    }
    ctx->bd_path = shapes_delta_in_place(ctx) ? 1 : 0;
    ctx->steer_swept = false;
    if (!ctx->bd_path) { ctx->graph_swept = false; return MPFMT_OK; }
    const int32_t rc = shapedelta_apply(ctx, d_delta, nd, remove, Bold, M_before);
    if (rc) { ctx->graph_swept = false; ctx->bd_path = 0; return rc; }               // (the list stands, the mask is swept again)
    const int32_t rf = mpfmt_field_mark_dirty(ctx);          // (the tracked fields learn which columns the edit read: each has a dirty
    if (rf) return rf;                                       //  bitmap of its own)
    return mpfmt_togo_mark_dirty(ctx);
}

// the compound box of a list (Compound2D ctor, SAT2D.jl:90-97), as mpfmt_upload_shapes2d computes it
static mpfmt_aabb2d compound_box(const std::vector<mpfmt_shape2d>& S)
{
    mpfmt_aabb2d box;
    box.xr[0] = box.yr[0] = INFINITY; box.xr[1] = box.yr[1] = -INFINITY;
    for (const mpfmt_shape2d& s : S) {
        box.xr[0] = std::min(box.xr[0], s.xr[0]); box.xr[1] = std::max(box.xr[1], s.xr[1]);
        box.yr[0] = std::min(box.yr[0], s.yr[0]); box.yr[1] = std::max(box.yr[1], s.yr[1]);
    }
    if (S.empty()) box.xr[0] = box.xr[1] = box.yr[0] = box.yr[1] = 0.0;
    return box;
}

// the new list beside the old one on the device, then swapped in: a failure before the swap leaves the ctx as it was
static int32_t install_shapes(mpfmt_ctx* ctx, std::vector<mpfmt_shape2d>& L)
{
    int32_t rc;
    mpfmt_dbuf<mpfmt_shape2d> nb;
    if ((rc = nb.ensure(ctx, sizeof(mpfmt_shape2d) * std::max<size_t>(L.size(), 1)))) return rc;
    if (!L.empty()) HIPCHK(ctx, hipMemcpyAsync(nb, L.data(), sizeof(mpfmt_shape2d) * L.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->aabb2d = compound_box(L);
    ctx->M = (int32_t)L.size();
    ctx->shapes_host.swap(L);
    ctx->shapes2d.swap(nb);
    return MPFMT_OK;
}

int32_t mpfmt_shapes2d_add(mpfmt_ctx* ctx, int32_t n_add, const int32_t* kinds, const int32_t* nverts, const double* data)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n_add < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "n_add = %d < 0", n_add);
    if (n_add > 0 && (!kinds || !nverts || !data)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "kinds / nverts / data is NULL");
    if (!ctx->have_boxes || ctx->cc_kind != 1)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "shapes are added to a 2-D SAT world (mpfmt_upload_shapes2d), not to a PointRobotNDBoxes set");
    if (n_add == 0) return MPFMT_OK;
    const int32_t M = ctx->M;
    if ((int64_t)M + n_add > INT32_MAX) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "more than 2^31 - 1 shapes");
    if ((int64_t)ctx->shapes_host.size() != (int64_t)M) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the host copy of the shape list is not whole");
    std::vector<mpfmt_shape2d> L(ctx->shapes_host);
    L.resize((size_t)M + (size_t)n_add);
    const double* p = data;
    int32_t rc;
    for (int32_t i = 0; i < n_add; ++i) {
        if ((rc = mpfmt_build_shape2d(ctx, i, kinds[i], nverts[i], p, &L[(size_t)M + i]))) return rc;
        p += (kinds[i] == MPFMT_SHAPE_CIRCLE) ? 3 : 2 * nverts[i];
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const mpfmt_aabb2d Bold = ctx->aabb2d;
    if ((rc = install_shapes(ctx, L))) return rc;
    return shapes_delta_finish(ctx, ctx->shapes2d.get() + M, n_add, false, Bold, M);
}

int32_t mpfmt_shapes2d_remove(mpfmt_ctx* ctx, const int64_t* ids, int32_t n_ids)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n_ids < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "n_ids = %d < 0", n_ids);
    if (n_ids > 0 && !ids) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "ids is NULL");
    if (!ctx->have_boxes || ctx->cc_kind != 1)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "shapes are removed from a 2-D SAT world (mpfmt_upload_shapes2d), not from a PointRobotNDBoxes set");
    const int32_t M = ctx->M;
    std::vector<char> out((size_t)std::max(M, 1), 0);
    for (int32_t j = 0; j < n_ids; ++j) {
        if (ids[j] < 1 || ids[j] > M) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "shape id %lld out of range 1..%d", (long long)ids[j], M);
        if (out[(size_t)(ids[j] - 1)]) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "shape id %lld given twice", (long long)ids[j]);
        out[(size_t)(ids[j] - 1)] = 1;
    }
    if (n_ids == 0) return MPFMT_OK;
    if ((int64_t)ctx->shapes_host.size() != (int64_t)M) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the host copy of the shape list is not whole");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<mpfmt_shape2d> keep, gone;
    keep.reserve((size_t)(M - n_ids)); gone.reserve((size_t)n_ids);
    for (int32_t k = 0; k < M; ++k) (out[(size_t)k] ? gone : keep).push_back(ctx->shapes_host[(size_t)k]);
    int32_t rc;
    mpfmt_dbuf<mpfmt_shape2d> removed;                       // a copy of what leaves, for the kernel
    if ((rc = removed.ensure(ctx, sizeof(mpfmt_shape2d) * gone.size()))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(removed, gone.data(), sizeof(mpfmt_shape2d) * gone.size(), hipMemcpyHostToDevice, ctx->stream));
    const mpfmt_aabb2d Bold = ctx->aabb2d;
    if ((rc = install_shapes(ctx, keep))) return rc;         // (synchronises: `gone` is on the device)
    return shapes_delta_finish(ctx, removed, n_ids, true, Bold, M);      // (synchronises before `removed` goes)
}
