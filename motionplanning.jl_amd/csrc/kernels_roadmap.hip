// Roadmap queries for external states (include/mpfmt.h, "roadmap queries for external states"; DESIGN.md has the section of the same
// name): states that are not samples are attached to the resident cell grid, graph and box set.
//
//   k_roadmap : one wavefront per query state q.  It walks the cells of the resident grid that meet q's r-box (cell coordinates clamped
//               per axis: a query may lie outside the samples' bounding box; farther than r outside on any axis it has no neighbours),
//               lanes over the candidates of a cell run read from the tiled cell-sorted copy (Xt), exact fp64 distances in the canonical
//               fold.  Members (d2 <= r * r) are queued in LDS and tested 64 at a time -- in R^6 one candidate in twenty is a member, a
//               test in the round that found it would idle the wavefront -- against the boxes that meet q's r-box (culled once per
//               query, the box set staged in LDS when it fits) with the predicates of sweep_predicates.h, in the order of k_edges_free:
//               the bit is the one mpfmt_motions_free returns.
//               mode 0 counts the near set, mode 1 fills idx / dist / bits at the scanned offsets (cell order; k_roadmap_sort puts the
//               segment into ascending index order), mode 2 reduces (fl(C[y] + d), C[y], y) over the usable members by wave shuffle and
//               stores no list.
//   k_roadmap_goal : the last hop and the path of ONE pair query from its goal's list, the finished field and its parents.
#include "mpfmt_internal.h"
#include "sweep_predicates.h"
#include "steer_roadmap.h"
#include <cmath>
#include <algorithm>

#define RM_WAVES 4               // queries per workgroup
#define RM_QCAP 128              // members queued per wavefront (a round adds at most 64 to fewer than 64)
#define RM_CULL 512              // boxes a wavefront lists after the cull (a larger set is walked whole)
#define RM_LDS_BOXES (40 * 1024) // the box set is staged when it fits
#define RM_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

struct rm_args {
    const double* Q; int64_t nq; int dir, mode;
    const double* Xt; const int32_t* perm; const int32_t* cellstart;
    double r2, rpad;
    double bb_hi[MPFMT_MAX_DIM];
    const double* boxes; int M, stage;
    const uint64_t* F;                                     // tail direction of a pair query: usable = free and F[y]
    int64_t* near_cnt; int64_t* usable_cnt;
    const int64_t* ptr; int32_t* idx; double* dist; uint8_t* bits;      // mode 1 (bits: 1 free, 2 usable)
    const double* C; double* best_cost; int64_t* best_parent;           // mode 2
    unsigned long long* ncand;
};

template <int D>
__global__ __launch_bounds__(RM_WAVES * 64) void k_roadmap(rm_args a, mpfmt_grid G, mpfmt_ss ss)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int32_t s_qp[RM_WAVES][RM_QCAP];
    __shared__ double s_qd[RM_WAVES][RM_QCAP];
    __shared__ int32_t s_cull[RM_WAVES][RM_CULL];
    double* sbox = (double*)smem;
    if (a.stage && a.mode != 0) stage_boxes<D>(sbox, a.boxes, 0, a.M);
    __syncthreads();                                         // (the only workgroup barrier: the wavefronts are on their own from here)
    const double* bx = (a.stage && a.mode != 0) ? (const double*)sbox : a.boxes;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t qi = (int64_t)blockIdx.x * RM_WAVES + wv;
    if (qi >= a.nq) return;
    const unsigned long long lt = (1ull << lane) - 1ull;
    double q[D];
    int clo[D], chi[D];
    bool far = false;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        q[i] = a.Q[qi * D + i];
        far = far || (G.lo[i] - q[i] > a.rpad) || (q[i] - a.bb_hi[i] > a.rpad);
        clo[i] = mpfmt_cell_of(q[i] - a.rpad, G.lo[i], G.inv_w[i], G.g[i]);
        chi[i] = mpfmt_cell_of(q[i] + a.rpad, G.lo[i], G.inv_w[i], G.g[i]);
    }
    // the boxes that meet q's r-box: every segment between q and a member lies inside it
    int nsurv = a.M;
    bool listed = false;
    if (a.mode != 0 && a.M <= RM_CULL) {
        listed = true; nsurv = 0;
        for (int k0 = 0; k0 < a.M; k0 += 64) {
            const int k = k0 + lane;
            const box_regs<D> b = load_box<D>(bx, min(k, a.M - 1));
            int out = 0;
#pragma unroll
            for (int i = 0; i < D; ++i) out |= (int)(b.hi[i] < q[i] - a.rpad) | (int)(b.lo[i] > q[i] + a.rpad);
            const bool keep = k < a.M && !out;
            const unsigned long long m = __ballot(keep);
            if (keep) s_cull[wv][nsurv + __popcll(m & lt)] = k;
            nsurv += __popcll(m);
        }
        RM_FENCE();
    }
    int64_t nnear = 0, nus = 0, nwritten = 0;
    unsigned long long ncand = 0;
    double bc = INFINITY, bcy = INFINITY;
    int32_t by = 0x7fffffff;
    int qn = 0;
    const int64_t base = a.mode == 1 ? a.ptr[qi] : 0, lim = a.mode == 1 ? a.ptr[qi + 1] : 0;

    // the first n queued members, lane = member: segment test, then the list entry or the reduction
    auto process = [&](int n) {
        const bool on = lane < n;
        const int32_t p = s_qp[wv][on ? lane : 0];
        const double d2 = s_qd[wv][on ? lane : 0];
        const int32_t y = a.perm[p];
        double v[D], w[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double c = a.Xt[(((int64_t)p >> 6) * D + i) * 64 + (p & 63)];
            v[i] = a.dir == 0 ? q[i] : c;
            w[i] = a.dir == 0 ? c : q[i];
        }
        bool fr = on && in_state_space_sl<D>(v, ss);
        double l[D], h[D];
        seg_bbox<D>(v, w, l, h);
        for (int j = 0; j < nsurv; ++j) {
            const int k = listed ? s_cull[wv][j] : j;
            const box_regs<D> b = load_box<D>(bx, k);        // wave-uniform k: broadcast reads
            const bool pend = fr & !broadphase_free_sl<D>(l, h, b);
            if (__ballot(pend)) {
                if (pend) fr = narrow_free_sl<D>(v, w, b);
            }
        }
        const bool us = fr && (!a.F || ((a.F[y >> 6] >> (y & 63)) & 1ull));
        nus += __popcll(__ballot(us));
        if (a.mode == 1) {
            const int64_t slot = base + nwritten + lane;
            if (on && slot < lim) { a.idx[slot] = y; a.dist[slot] = sqrt(d2); a.bits[slot] = (uint8_t)((fr ? 1 : 0) | (us ? 2 : 0)); }
            nwritten += n;
        } else if (us) {
            const double cy = a.C[y];
            if (cy < INFINITY) {
                const double c = cy + sqrt(d2);
                if (c < bc || (c == bc && (cy < bcy || (cy == bcy && y < by)))) { bc = c; bcy = cy; by = y; }
            }
        }
    };

    if (!far) {
        constexpr int L = D - 1;
        int64_t rows = 1;
#pragma unroll
        for (int i = 0; i < L; ++i) rows *= (chi[i] - clo[i] + 1);
        for (int64_t row = 0; row < rows; ++row) {
            int64_t rem = row, cbase = 0;
#pragma unroll
            for (int i = L - 1; i >= 0; --i) {
                const int span = chi[i] - clo[i] + 1;
                cbase += mpfmt_cell_term(G, i, clo[i] + (int)(rem % span));
                rem /= span;
            }
            const int64_t ra = a.cellstart[cbase + clo[L]], rb = a.cellstart[cbase + chi[L] + 1];
            for (int64_t p0 = ra; p0 < rb; p0 += 64) {
                const bool valid = p0 + lane < rb;
                const int64_t p = valid ? p0 + lane : ra;
                double d2 = 0.0;
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const double t = q[i] - a.Xt[((p >> 6) * D + i) * 64 + (p & 63)];
                    const double tt = t * t;
                    d2 = (i == 0) ? tt : d2 + tt;
                }
                ncand += (unsigned long long)min((int64_t)64, rb - p0);
                const bool member = valid && d2 <= a.r2;
                const unsigned long long m = __ballot(member);
                if (!m) continue;
                nnear += __popcll(m);
                if (a.mode == 0) continue;
                if (member) { const int slot = qn + __popcll(m & lt); s_qp[wv][slot] = (int32_t)p; s_qd[wv][slot] = d2; }
                qn += __popcll(m);
                RM_FENCE();
                if (qn >= 64) {
                    process(64);
                    const int rest = qn - 64;
                    int32_t tp = 0; double td = 0.0;
                    if (lane < rest) { tp = s_qp[wv][64 + lane]; td = s_qd[wv][64 + lane]; }
                    RM_FENCE();
                    if (lane < rest) { s_qp[wv][lane] = tp; s_qd[wv][lane] = td; }
                    RM_FENCE();
                    qn = rest;
                }
            }
        }
        if (a.mode != 0 && qn > 0) process(qn);
    }
    if (a.mode == 2) {
        for (int off = 32; off > 0; off >>= 1) {
            const double oc = __shfl_xor(bc, off), ocy = __shfl_xor(bcy, off);
            const int32_t oy = __shfl_xor(by, off);
            if (oc < bc || (oc == bc && (ocy < bcy || (ocy == bcy && oy < by)))) { bc = oc; bcy = ocy; by = oy; }
        }
        if (lane == 0) { a.best_cost[qi] = bc; a.best_parent[qi] = by == 0x7fffffff ? 0 : (int64_t)by + 1; }
    }
    if (lane == 0) {
        a.near_cnt[qi] = nnear;
        if (a.mode != 0 && a.usable_cnt) a.usable_cnt[qi] = nus;
        if (ncand) atomicAdd(a.ncand, ncand);
    }
}

// a query's segment from cell order into ascending sample order (rank by counting: the indices of a near set are distinct); one wavefront per
// query.  Quadratic in the list: k * k / 64 loads per wavefront -- nothing at roadmap radii (lists of tens to a thousand entries), a cost to
// know of when r is a sizeable fraction of the cloud (include/mpfmt.h says so)
__global__ __launch_bounds__(256) void k_roadmap_sort(int64_t nq, const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx_in,
                                                      const double* __restrict__ dist_in, const uint8_t* __restrict__ bits_in,
                                                      int64_t* __restrict__ idx1_out, double* __restrict__ dist_out, uint8_t* __restrict__ bits_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const int64_t b0 = ptr[qi], b1 = ptr[qi + 1];
    for (int64_t e = b0 + lane; e < b1; e += 64) {
        const int32_t mine = idx_in[e];
        int64_t rank = 0;
        for (int64_t j = b0; j < b1; ++j) rank += (idx_in[j] < mine) ? 1 : 0;
        idx1_out[b0 + rank] = (int64_t)mine + 1; dist_out[b0 + rank] = dist_in[e]; bits_out[b0 + rank] = bits_in[e];
    }
}

// One pair query's goal side, one wavefront: the last hop = the free entry y of the goal's list with lowest (fl(C[y] + d), C[y], y), then
// lane 0 follows the parents (A[x] = -1: the start) and writes the samples goal-first.  res: [0] cost, [1] last-hop sample (1-based, 0 none),
// [2] hops written, [3 ...] the samples (at most N + 1: a walk that long has met a group of equal labels and is cut like the host's).
__global__ __launch_bounds__(64) void k_roadmap_goal(int64_t b0, int64_t b1, const int64_t* __restrict__ idx1, const double* __restrict__ dist,
                                                     const uint8_t* __restrict__ bits, const double* __restrict__ C, const int64_t* __restrict__ A,
                                                     int64_t N, int64_t* __restrict__ res)
{
    const int lane = threadIdx.x;
    double bc = INFINITY, bcy = INFINITY;
    int64_t by = INT64_MAX;
    for (int64_t e = b0 + lane; e < b1; e += 64) {
        if (!(bits[e] & 1)) continue;
        const int64_t y = idx1[e] - 1;
        const double cy = C[y];
        if (!(cy < INFINITY)) continue;
        const double c = cy + dist[e];
        if (c < bc || (c == bc && (cy < bcy || (cy == bcy && y < by)))) { bc = c; bcy = cy; by = y; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double oc = __shfl_xor(bc, off), ocy = __shfl_xor(bcy, off);
        const int64_t oy = __shfl_xor(by, off);
        if (oc < bc || (oc == bc && (ocy < bcy || (ocy == bcy && oy < by)))) { bc = oc; bcy = ocy; by = oy; }
    }
    if (lane != 0) return;
    res[0] = __double_as_longlong(bc);
    res[1] = by == INT64_MAX ? 0 : by + 1;
    int64_t n = 0;
    if (by != INT64_MAX) {
        int64_t x = by;
        for (;;) {
            res[3 + n] = x + 1; ++n;
            if (n > N) break;
            const int64_t p = A[x];
            if (p <= 0) break;                               // -1: the start; 0: no parent (a group of equal labels)
            x = p - 1;
        }
    }
    res[2] = n;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------

// The resident grid for the graph's radius.  After a step the grid IS that grid and nothing happens (mpfmt_build_grid returns at once: the
// graph, rowpos, the mask and the pending list stay as they are).  An imported graph has no grid of its radius (a mpfmt_rdisc_query
// at another radius in between is no second case: mpfmt_build_grid then drops the graph, and the calls on external states refuse before
// they come here): it is built, which rewrites the cell order (perm, Xt, Xs) and nothing of the graph; the
// graph's own state is kept and what was expressed in the old cell order (row positions, pending list, hit logs) is marked stale.
int32_t mpfmt_roadmap_grid(mpfmt_ctx* ctx)
{
    const double r = ctx->graph_r;
    if (ctx->grid_r == r && ctx->Xt && ctx->index_rank == ctx->rank && ctx->index_world == ctx->world && !ctx->tileneed) return MPFMT_OK;
    const bool counted = ctx->graph_counted, filled = ctx->graph_filled, swept = ctx->graph_swept;
    const int64_t knn_k = ctx->knn_k;
    const int32_t rc = mpfmt_build_grid(ctx, r, true);
    ctx->graph_r = r; ctx->graph_counted = counted; ctx->graph_filled = filled; ctx->graph_swept = swept; ctx->knn_k = knn_k;
    ctx->rowpos_valid = false; ctx->pend_valid = false; ctx->pool_valid = false; ctx->spec_ready = false; ctx->tptr_valid = false;
    ctx->wf_seen_epoch = -1;
    return rc;
}

static int32_t rm_launch(mpfmt_ctx* ctx, rm_args& a)
{
    a.Xt = ctx->Xt; a.perm = ctx->perm; a.cellstart = ctx->cellstart;
    const double r = ctx->graph_r;
    a.r2 = r * r; a.rpad = r * (1.0 + 1e-9) + 1e-300;
    for (int i = 0; i < MPFMT_MAX_DIM; ++i) a.bb_hi[i] = i < ctx->d ? ctx->bb_hi[i] : 0.0;
    a.boxes = ctx->boxes; a.M = ctx->M;
    const size_t box_bytes = (size_t)ctx->M * 2 * ctx->d * sizeof(double);
    a.stage = (ctx->M > 0 && box_bytes <= RM_LDS_BOXES) ? 1 : 0;
    const size_t lds = (a.stage && a.mode != 0) ? box_bytes : 0;
    const unsigned nb = (unsigned)((a.nq + RM_WAVES - 1) / RM_WAVES);
    DISPATCH_D(ctx->d, hipLaunchKernelGGL((k_roadmap<DD>), dim3(nb), dim3(RM_WAVES * 64), lds, ctx->stream, a, ctx->grid, ctx->ss));
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

// ---- the host driver of both spaces ---------------------------------------------------------------------------------------------------------
// DESIGN.md 7f, "The host driver".  A space supplies its timer name, the number of counters its kernel keeps ([0] pairs (pre-)tested,
// [1] exact steers run), whether its fill needs the ordering pass, and a callable that copies the driver's slots into its own argument
// struct -- rm_args, srm_args -- next to the query's own fields, and launches its kernel.  A list or reduce call is ONE timed interval.

struct rm_slots {                        // what the driver owns of a launch
    int mode;
    int64_t* near_cnt; int64_t* usable_cnt; unsigned long long* ctr;
    const int64_t* ptr; double* dist; uint8_t* bits;      // mode 1: the offsets and where the fill writes ...
    int32_t* idx; int64_t* idx1;                           // ... 0-based in cell order ahead of the ordering pass, else 1-based and final
};
typedef std::function<int32_t(const rm_slots&)> rm_launcher;

// the stats of one list or reduce call, left in the ctx (a public call of several sums them: mpfmt_capi.hip)
static int32_t rm_stats(mpfmt_ctx* ctx, const unsigned long long* d_ctr, int nctr, int64_t near_total)
{
    unsigned long long c[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(c, d_ctr, sizeof(unsigned long long) * (size_t)nctr, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->roadmap_candidates = (int64_t)c[0]; ctx->roadmap_near_total = near_total;
    if (nctr > 1) ctx->steer_roadmap_steered = (int64_t)c[1];
    return MPFMT_OK;
}

// the list form.  Arrays live in tmp.  count_only: ptr_host / total alone (no list is filled)
static int32_t rm_drive_lists(mpfmt_ctx* ctx, mpfmt_tmp& tmp, int64_t nq, mpfmt_rm_list* out, bool count_only, const char* timer, int nctr, bool sort,
                              const rm_launcher& launch)
{
    int32_t rc;
    rm_slots s{};
    int64_t* d_ptr = nullptr;
    HIPCHK(ctx, tmp.get(&s.near_cnt, sizeof(int64_t) * (size_t)nq));
    HIPCHK(ctx, tmp.get(&s.usable_cnt, sizeof(int64_t) * (size_t)nq));
    HIPCHK(ctx, tmp.get(&d_ptr, sizeof(int64_t) * (size_t)(nq + 1)));
    HIPCHK(ctx, tmp.get(&s.ctr, sizeof(unsigned long long) * (size_t)nctr));
    HIPCHK(ctx, hipMemsetAsync(s.ctr, 0, sizeof(unsigned long long) * (size_t)nctr, ctx->stream));
    mpfmt_timed tm(ctx);
    s.mode = 0;
    if ((rc = launch(s))) return rc;
    out->ptr_host.assign((size_t)nq + 1, 0);
    HIPCHK(ctx, hipMemcpyAsync(out->ptr_host.data() + 1, s.near_cnt, sizeof(int64_t) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < nq; ++i) out->ptr_host[(size_t)i + 1] += out->ptr_host[(size_t)i];
    const int64_t total = out->ptr_host[(size_t)nq];
    out->total = total;
    if (count_only) {
        tm.end(timer);
        return rm_stats(ctx, s.ctr, nctr, total);
    }
    HIPCHK(ctx, hipMemcpyAsync(d_ptr, out->ptr_host.data(), sizeof(int64_t) * (size_t)(nq + 1), hipMemcpyHostToDevice, ctx->stream));
    double* d_dist2 = nullptr; uint8_t* d_bits2 = nullptr;
    if (sort) HIPCHK(ctx, tmp.get(&s.idx, sizeof(int32_t) * (size_t)total));
    HIPCHK(ctx, tmp.get(&s.dist, sizeof(double) * (size_t)total));
    HIPCHK(ctx, tmp.get(&s.bits, (size_t)total));
    HIPCHK(ctx, tmp.get(&s.idx1, sizeof(int64_t) * (size_t)total));
    if (sort) {
        HIPCHK(ctx, tmp.get(&d_dist2, sizeof(double) * (size_t)total));
        HIPCHK(ctx, tmp.get(&d_bits2, (size_t)total));
    }
    HIPCHK(ctx, hipMemsetAsync(s.ctr, 0, sizeof(unsigned long long) * (size_t)nctr, ctx->stream));
    s.mode = 1; s.ptr = d_ptr;
    if ((rc = launch(s))) return rc;
    if (sort) {
        hipLaunchKernelGGL(k_roadmap_sort, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, ctx->stream, nq, (const int64_t*)d_ptr, (const int32_t*)s.idx,
                           (const double*)s.dist, (const uint8_t*)s.bits, s.idx1, d_dist2, d_bits2);
        HIPCHK(ctx, hipGetLastError());
    }
    tm.end(timer);
    out->usable_host.assign((size_t)nq, 0);
    HIPCHK(ctx, hipMemcpyAsync(out->usable_host.data(), s.usable_cnt, sizeof(int64_t) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = rm_stats(ctx, s.ctr, nctr, total))) return rc;
    out->ptr = d_ptr; out->idx1 = s.idx1; out->dist = sort ? d_dist2 : s.dist; out->bits = sort ? d_bits2 : s.bits;
    return MPFMT_OK;
}

// the reduce form: one launch, no list
static int32_t rm_drive_reduce(mpfmt_ctx* ctx, mpfmt_tmp& tmp, int64_t nq, const char* timer, int nctr, const rm_launcher& launch)
{
    int32_t rc;
    rm_slots s{};
    HIPCHK(ctx, tmp.get(&s.near_cnt, sizeof(int64_t) * (size_t)nq));
    HIPCHK(ctx, tmp.get(&s.ctr, sizeof(unsigned long long) * (size_t)nctr));
    HIPCHK(ctx, hipMemsetAsync(s.ctr, 0, sizeof(unsigned long long) * (size_t)nctr, ctx->stream));
    mpfmt_timed tm(ctx);
    s.mode = 2;
    if ((rc = launch(s))) return rc;
    tm.end(timer);
    std::vector<int64_t> cnt((size_t)nq);
    HIPCHK(ctx, hipMemcpyAsync(cnt.data(), s.near_cnt, sizeof(int64_t) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    int64_t total = 0;
    for (int64_t c : cnt) total += c;
    return rm_stats(ctx, s.ctr, nctr, total);
}

// ---- the Euclidean space: k_roadmap (one counter; the fill is in cell order) ----------------------------------------------------------------

int32_t mpfmt_roadmap_lists(mpfmt_ctx* ctx, mpfmt_tmp& tmp, const double* d_Q, int64_t nq, int dir, const uint64_t* d_F, mpfmt_rm_list* out, bool count_only)
{
    int32_t rc;
    if ((rc = mpfmt_roadmap_grid(ctx))) return rc;
    return rm_drive_lists(ctx, tmp, nq, out, count_only, "roadmap_near", 1, true, [&](const rm_slots& s) {
        rm_args a{};
        a.Q = d_Q; a.nq = nq; a.dir = dir; a.mode = s.mode; a.F = d_F; a.near_cnt = s.near_cnt; a.usable_cnt = s.usable_cnt; a.ncand = s.ctr;
        a.ptr = s.ptr; a.idx = s.idx; a.dist = s.dist; a.bits = s.bits;
        return rm_launch(ctx, a);
    });
}

// the reduce form over a device field d_C [N]: head direction
int32_t mpfmt_roadmap_reduce(mpfmt_ctx* ctx, mpfmt_tmp& tmp, const double* d_Q, int64_t nq, const double* d_C, double* d_cost, int64_t* d_parent)
{
    int32_t rc;
    if ((rc = mpfmt_roadmap_grid(ctx))) return rc;
    return rm_drive_reduce(ctx, tmp, nq, "roadmap_attach", 1, [&](const rm_slots& s) {
        rm_args a{};
        a.Q = d_Q; a.nq = nq; a.dir = 1; a.mode = s.mode; a.near_cnt = s.near_cnt; a.C = d_C; a.best_cost = d_cost; a.best_parent = d_parent; a.ncand = s.ctr;
        return rm_launch(ctx, a);
    });
}

int32_t mpfmt_roadmap_goal(mpfmt_ctx* ctx, const mpfmt_rm_list& L, int64_t q, const double* d_C, const int64_t* d_A, int64_t* d_res)
{
    hipLaunchKernelGGL(k_roadmap_goal, dim3(1), dim3(64), 0, ctx->stream, L.ptr_host[(size_t)q], L.ptr_host[(size_t)q + 1], (const int64_t*)L.idx1,
                       (const double*)L.dist, (const uint8_t*)L.bits, d_C, d_A, ctx->N, d_res);
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

// ---- the steering spaces (steer_roadmap.h; k_di_roadmap in kernels_di.hip, k_car_roadmap in kernels_car.hip): two counters ------------------
// d_X / nx: the samples the queries meet -- ctx->Xo / N, or with pair the goals of a pair query (query i meets d_X[i] alone: the direct
// edge).  Lists come out of the fill in ascending order: no ordering pass.

static int32_t srm_launch(mpfmt_ctx* ctx, srm_args& a)
{
    return ctx->steer_kind == MPFMT_STEER_DI ? mpfmt_di_roadmap_launch(ctx, a) : mpfmt_car_roadmap_launch(ctx, a);
}

int32_t mpfmt_steer_roadmap_lists(mpfmt_ctx* ctx, mpfmt_tmp& tmp, const double* d_Q, int64_t nq, int dir, const uint64_t* d_F, mpfmt_rm_list* out,
                                  bool count_only, const double* d_X, int64_t nx, bool pair)
{
    return rm_drive_lists(ctx, tmp, nq, out, count_only, "steer_roadmap_near", 2, false, [&](const rm_slots& s) {
        srm_args a{};
        a.Q = d_Q; a.nq = nq; a.dir = dir; a.mode = s.mode; a.X = d_X; a.N = nx; a.pair = pair ? 1 : 0; a.F = d_F;
        a.near_cnt = s.near_cnt; a.usable_cnt = s.usable_cnt; a.ctr = s.ctr;
        a.ptr = s.ptr; a.idx1 = s.idx1; a.dist = s.dist; a.bits = s.bits;
        return srm_launch(ctx, a);
    });
}

// the reduce form over a device field d_C [N]: head direction
int32_t mpfmt_steer_roadmap_reduce(mpfmt_ctx* ctx, mpfmt_tmp& tmp, const double* d_Q, int64_t nq, const double* d_C, double* d_cost, int64_t* d_parent)
{
    return rm_drive_reduce(ctx, tmp, nq, "steer_roadmap_attach", 2, [&](const rm_slots& s) {
        srm_args a{};
        a.Q = d_Q; a.nq = nq; a.dir = 1; a.mode = s.mode; a.X = ctx->Xo; a.N = ctx->N; a.near_cnt = s.near_cnt; a.C = d_C; a.best_cost = d_cost;
        a.best_parent = d_parent; a.ctr = s.ctr;
        return srm_launch(ctx, a);
    });
}
