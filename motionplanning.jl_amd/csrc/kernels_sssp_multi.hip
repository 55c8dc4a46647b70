// Many-source roadmap fields: up to 64 cost-to-come fields per pass over the resident free-edge graph (include/mpfmt.h, "many-source
// fields and cost matrices"; DESIGN.md "Many sources per pass").  The relaxation of kernels_sssp.hip with the wavefront turned the other
// way: a lane carries one SOURCE, labels are stored L[sample][source] (64 doubles = one 512-byte row per sample), and one visit of an
// entry y -> x serves all fields of the group with one coalesced row read.
//
//   round t:  for every column x in which some lane may still improve:  L[x][s] = min(L[x][s], min over usable entries whose row y changed
//             in round t-1 -- for ANY source -- of fl(L[y][s] + w)); a column in which any lane improved marks itself for round t+1.
//
// * one wavefront per column, grid-stride; the column's entries are read 64 at a time (rowval, nzval, mask bit, the row's bit in the
//   changed-sample bitmap), a ballot picks the entries to visit, row index and weight are made wave-uniform by readlane and every lane
//   evaluates fl(L[y][lane] + w) -- unfused fp64, one add, what k_sssp_relax evaluates -- with four row loads in flight;
// * the changed-sample bitmaps are per SAMPLE (any source changed it), three in rotation, the ring of relax_core.h: a superset of every
//   source's own frontier, so each lane sees at least what its single-source round would, plus candidates that are labels of real paths
//   too: every value stays an upper bound of the source's least fixed point, and the fixed point is reached when nothing changes;
// * the cost band is per LANE: mlow[s](t) = the lowest label written for source s in round t-1.  A label written for s in round t is
//   fl(L[y][s] + w) for a row y of the bitmap.  If y changed for s in round t-1 or t, L[y][s] >= mlow[s](t) by induction over the writes.
//   If it changed for other sources only, x looked at L[y][s] in the round after its last change (or was skipped then because
//   L[x][s] <= mlow[s] <= L[y][s]) and cannot improve on it now.  So L[x][s] <= mlow[s](t) cannot improve, and a column is skipped before
//   any entry is read when that holds for every lane.  Lanes beyond a ragged group hold +Inf and mlow = +Inf from the start: they never
//   enter a column, never improve and are not counted;
// * checkpts: a column with F[x] clear is skipped for every lane.  A source with F clear keeps its label 0 (its exemption): 0 is never
//   above mlow, and no lane may enter an F-clear column;
// * round state: the ring of relax_core.h with a slot of its own (changed count, 64 band minima);
// * parents: a separate pass over the finished labels, lanes over sources (k_ms_parents), which also counts `reached` per lane;
// * copy-out: a tiled transpose [N][64] -> [64][chunk] through LDS (k_ms_transpose), then strided copies into the caller's arrays.
// The cost matrix between external starts and goals (mpfmt_roadmap_matrix) seeds a group's labels from the starts' near lists
// (k_ms_seed) and reduces every goal's head list over the 64 fields at once (k_ms_goal).
#include "relax_core.h"

#define MS_W 64                              // sources per group = lanes of a wavefront
#define MS_CHUNK 65536                       // samples per transposed chunk of the copy-out (32 MiB of staging)

struct ms_slot {                             // a band minimum per source; the first MS_W threads of the grid reset them
    unsigned long long changed, pad; unsigned long long minbits[MS_W];
    __device__ __forceinline__ void clear(int64_t gtid)
    {
        if (gtid < MS_W) minbits[gtid] = LABEL_INF_BITS;
        if (gtid == 0) changed = 0;
    }
};
struct ms_state {
    ms_slot slot[3];
    unsigned long long rows, rounds, pad[2];
    unsigned long long reached[MS_W];
};

__device__ __forceinline__ double ms_readlane(double v, int j)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

// fmin of fl(L[y][lane] + w) over the entries of mask m (bit j: the entry lane j holds in y / w), four rows in flight.  A short tail
// visits its last entry again: fmin does not mind.
__device__ __forceinline__ double ms_visit(unsigned long long m, int32_t y, double w, const double* L, int lane, double best)
{
    while (m) {
        const int j0 = __builtin_ctzll(m); m &= m - 1;
        const int j1 = m ? __builtin_ctzll(m) : j0; m &= m - 1 + (m == 0);
        const int j2 = m ? __builtin_ctzll(m) : j1; m &= m - 1 + (m == 0);
        const int j3 = m ? __builtin_ctzll(m) : j2; m &= m - 1 + (m == 0);
        const int64_t y0 = __builtin_amdgcn_readlane(y, j0), y1 = __builtin_amdgcn_readlane(y, j1);
        const int64_t y2 = __builtin_amdgcn_readlane(y, j2), y3 = __builtin_amdgcn_readlane(y, j3);
        const double c0 = L[y0 * MS_W + lane], c1 = L[y1 * MS_W + lane], c2 = L[y2 * MS_W + lane], c3 = L[y3 * MS_W + lane];
        const double w0 = ms_readlane(w, j0), w1 = ms_readlane(w, j1), w2 = ms_readlane(w, j2), w3 = ms_readlane(w, j3);
        best = fmin(fmin(best, c0 + w0), fmin(c1 + w1, fmin(c2 + w2, c3 + w3)));
    }
    return best;
}

__device__ __forceinline__ void ms_state_reset(ms_state* st, int64_t i, int n, unsigned long long changed0)
{
    if (i < MS_W) {
        st->slot[0].minbits[i] = i < n ? 0ull : LABEL_INF_BITS;
        st->slot[1].minbits[i] = LABEL_INF_BITS; st->slot[2].minbits[i] = LABEL_INF_BITS;
        st->reached[i] = 0;
    }
    if (i == 0) {
        st->slot[0].changed = changed0; st->slot[1].changed = 0; st->slot[2].changed = 0;
        st->slot[0].pad = st->slot[1].pad = st->slot[2].pad = 0;
        st->rows = 0; st->rounds = 0; st->pad[0] = st->pad[1] = 0;
    }
}

// labels, bitmaps and round state of a group of n sample sources src[0 .. n) (0-based; duplicates allowed)
__global__ __launch_bounds__(256) void k_ms_init(int64_t N, int64_t words, int n, const int64_t* __restrict__ src, double* __restrict__ L,
                                                 uint64_t* __restrict__ bm, ms_state* __restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (i < N * MS_W) L[i] = (lane < n && src[lane] == (i >> 6)) ? 0.0 : INFINITY;
    if (i < 3 * words) {
        uint64_t v = 0ull;
        if (i < words)
            for (int s = 0; s < n; ++s) if ((src[s] >> 6) == i) v |= 1ull << (src[s] & 63);
        bm[i] = v;
    }
    ms_state_reset(st, i, n, 1ull);
}

// the seeded form: labels +Inf, no bit set; k_ms_seed adds the starts' usable near entries
__global__ __launch_bounds__(256) void k_ms_clear(int64_t N, int64_t words, int n, double* __restrict__ L, uint64_t* __restrict__ bm,
                                                  ms_state* __restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N * MS_W) L[i] = INFINITY;
    if (i < 3 * words) bm[i] = 0ull;
    ms_state_reset(st, i, n, 0ull);
}

// block s = the start i0 + s of the group: L[y][s] = fl(0 + d(s, y)) over the usable entries of its near list (bits & 2), bit y set.  A start
// that is not a free state seeds nothing: its fields stay +Inf.  (The entries of one start are distinct samples: no two threads write
// one label.)
__global__ __launch_bounds__(256) void k_ms_seed(int64_t i0, const int64_t* __restrict__ ptr, const int64_t* __restrict__ idx1,
                                                 const double* __restrict__ dist, const uint8_t* __restrict__ bits,
                                                 const uint64_t* __restrict__ sfree, double* __restrict__ L, uint64_t* bm, ms_state* st)
{
    const int s = blockIdx.x;
    const int64_t i = i0 + s;
    if (!((sfree[i >> 6] >> (i & 63)) & 1ull)) return;
    unsigned long long cnt = 0;
    for (int64_t e = ptr[i] + threadIdx.x; e < ptr[i + 1]; e += blockDim.x) {
        if (!(bits[e] & 2)) continue;
        const int64_t y = idx1[e] - 1;
        L[y * MS_W + s] = 0.0 + dist[e];
        atomicOr((unsigned long long*)&bm[y >> 6], 1ull << (y & 63));
        ++cnt;
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&st->slot[0].changed, cnt);
}

__global__ __launch_bounds__(256) void k_ms_relax(int64_t N, int64_t words, int round, const int64_t* __restrict__ colptr,
                                                  const int32_t* __restrict__ rowval, const double* __restrict__ nzval,
                                                  const uint64_t* __restrict__ efree, const uint64_t* __restrict__ F, double* L, uint64_t* bm,
                                                  ms_state* st)
{
    __shared__ double s_min[4][MS_W];
    const ring_idx r = ring_at(round);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double mlow = label_of_bits(st->slot[r.in].minbits[lane]);
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const uint64_t* bin;
    unsigned long long* bout;
    if (!ring_round(st->slot, &st->rounds, bm, words, r, gtid, nthreads, bin, bout)) return;
    const int64_t nwaves = nthreads >> 6;
    unsigned long long nrows = 0, nchg = 0;
    double lmin = INFINITY;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        const double cx = L[x * MS_W + lane];
        if (!__ballot(cx > mlow)) continue;
        if (F && !bit_of(F, x)) continue;
        const int64_t b0 = colptr[x], b1 = colptr[x + 1];
        double best = INFINITY;
        for (int64_t c0 = b0; c0 < b1; c0 += 64) {
            const int64_t b = c0 + lane;
            const bool valid = b < b1;
            const int32_t y = valid ? rowval[b] : 0;
            const double w = valid ? nzval[b] : 0.0;
            const bool ok = valid && bit_of(bin, y) && bit_of(efree, b);
            const unsigned long long m = __ballot(ok);
            nrows += (unsigned long long)__popcll(m);
            best = ms_visit(m, y, w, L, lane, best);
        }
        const bool better = best < cx;
        if (better) { L[x * MS_W + lane] = best; lmin = fmin(lmin, best); }
        if (__ballot(better)) {
            if (lane == 0) atomicOr(&bout[x >> 6], 1ull << (x & 63));
            ++nchg;
        }
    }
    // the band minima of the block's four wavefronts, one atomicMin per lane and block -- and none where the slot already holds a lower
    // value (it only decreases during the round: a stale read asks for an atomic too many, never one too few)
    s_min[wv][lane] = lmin;
    __syncthreads();
    if (wv == 0) {
        lmin = fmin(fmin(s_min[0][lane], s_min[1][lane]), fmin(s_min[2][lane], s_min[3][lane]));
        const unsigned long long mb = label_bits(lmin);
        if (lmin < INFINITY && mb < st->slot[r.out].minbits[lane]) atomicMin(&st->slot[r.out].minbits[lane], mb);
    }
    if (lane == 0) {
        if (nrows) atomicAdd(&st->rows, nrows);
        if (nchg) atomicAdd(&st->slot[r.out].changed, nchg);
    }
}

// reached[lane] += the counts of the block's four wavefronts: one atomicAdd per lane and block
__device__ __forceinline__ void ms_count_reached(unsigned long long nreach, int lane, int wv, ms_state* st)
{
    __shared__ unsigned long long s_cnt[4][MS_W];
    s_cnt[wv][lane] = nreach;
    __syncthreads();
    if (wv == 0) {
        nreach = s_cnt[0][lane] + s_cnt[1][lane] + s_cnt[2][lane] + s_cnt[3][lane];
        if (nreach) atomicAdd(&st->reached[lane], nreach);
    }
}

// At[x][s] = the usable y of lowest (L[y][s], y) with fl(L[y][s] + w) == L[x][s], 1-based; 0 for the source itself and for unreached samples.
// Counts reached per lane.
__global__ __launch_bounds__(256) void k_ms_parents(int64_t N, int n, const int64_t* __restrict__ src, const int64_t* __restrict__ colptr,
                                                    const int32_t* __restrict__ rowval, const double* __restrict__ nzval,
                                                    const uint64_t* __restrict__ efree, const double* __restrict__ L, int64_t* __restrict__ At,
                                                    ms_state* st)
{
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t mine = lane < n ? src[lane] : -1;
    unsigned long long nreach = 0;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        const double cx = L[x * MS_W + lane];
        const bool reached = cx < INFINITY;
        nreach += reached ? 1 : 0;
        const bool want = reached && x != mine;
        double cb = INFINITY; int32_t yb = PARENT_NONE;
        if (__ballot(want)) {
            const int64_t b0 = colptr[x], b1 = colptr[x + 1];
            for (int64_t c0 = b0; c0 < b1; c0 += 64) {
                const int64_t b = c0 + lane;
                const bool valid = b < b1;
                const int32_t y = valid ? rowval[b] : 0;
                const double w = valid ? nzval[b] : 0.0;
                unsigned long long m = __ballot(valid && bit_of(efree, b));
                while (m) {
                    const int j0 = __builtin_ctzll(m); m &= m - 1;
                    const int j1 = m ? __builtin_ctzll(m) : j0; m &= m - 1 + (m == 0);
                    const int32_t y0 = __builtin_amdgcn_readlane(y, j0), y1 = __builtin_amdgcn_readlane(y, j1);
                    const double c0v = L[(int64_t)y0 * MS_W + lane], c1v = L[(int64_t)y1 * MS_W + lane];
                    const double w0 = ms_readlane(w, j0), w1 = ms_readlane(w, j1);
                    if (c0v + w0 == cx && parent_before(c0v, y0, cb, yb)) { cb = c0v; yb = y0; }
                    if (c1v + w1 == cx && parent_before(c1v, y1, cb, yb)) { cb = c1v; yb = y1; }
                }
            }
        }
        At[x * MS_W + lane] = (want && yb != PARENT_NONE) ? (int64_t)yb + 1 : 0;
    }
    ms_count_reached(nreach, lane, wv, st);
}

// reached per lane without a parent pass
__global__ __launch_bounds__(256) void k_ms_reached(int64_t N, const double* __restrict__ L, ms_state* st)
{
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long nreach = 0;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) nreach += L[x * MS_W + lane] < INFINITY ? 1 : 0;
    ms_count_reached(nreach, lane, wv, st);
}

// in [N][64] -> out [n][cnt] for the samples x0 .. x0 + cnt (8-byte items: labels, or parents); one 64 x 64 tile per workgroup through LDS
__global__ __launch_bounds__(256) void k_ms_transpose(int64_t x0, int64_t cnt, int n, const unsigned long long* __restrict__ in,
                                                      unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long tile[64][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * 64;
    for (int r = wv; r < 64; r += 4)
        if (t0 + r < cnt) tile[r][lane] = in[(x0 + t0 + r) * MS_W + lane];
    __syncthreads();
    for (int s = wv; s < n; s += 4)
        if (t0 + lane < cnt) out[(int64_t)s * cnt + t0 + lane] = tile[lane][s];
}

// One wavefront per goal j, lanes over the starts i0 .. i0 + n of the group: the least fl(L[y][lane] + d(y, g)) over the free entries of
// the goal's head list with finite labels, then the direct edge (d2(s, g) <= r * r in the canonical fold, and its motion bit), then the status.
struct ms_goal_args {
    int64_t i0, ns, ng; int n, d;
    const double* S; const double* G; double r2;
    const uint64_t* sfree; const uint64_t* gfree; const uint64_t* direct;      // bit i / bit j / bit i * ng + j
    const int64_t* ptr; const int64_t* idx1; const double* dist; const uint8_t* bits;
    const double* L; double* cost; int32_t* status;
};
__global__ __launch_bounds__(256) void k_ms_goal(ms_goal_args a)
{
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.ng) return;
    double best = INFINITY;
    const int64_t b0 = a.ptr[j], b1 = a.ptr[j + 1];
    for (int64_t c0 = b0; c0 < b1; c0 += 64) {
        const int64_t e = c0 + lane;
        const bool valid = e < b1;
        const int32_t y = valid ? (int32_t)(a.idx1[e] - 1) : 0;
        const double w = valid ? a.dist[e] : 0.0;
        best = ms_visit(__ballot(valid && (a.bits[e] & 1)), y, w, a.L, lane, best);      // (+Inf labels give +Inf candidates: fmin drops them)
    }
    if (lane >= a.n) return;
    const int64_t i = a.i0 + lane;
    double d2 = 0.0;
    for (int k = 0; k < a.d; ++k) { const double t = a.S[i * a.d + k] - a.G[j * a.d + k]; const double tt = t * t; d2 = (k == 0) ? tt : d2 + tt; }
    const int64_t p = i * a.ng + j;
    if (d2 <= a.r2 && ((a.direct[p >> 6] >> (p & 63)) & 1ull)) best = fmin(best, sqrt(d2));
    int32_t status;
    if (!((a.sfree[i >> 6] >> (i & 63)) & 1ull)) status = 2;
    else if (!((a.gfree[j >> 6] >> (j & 63)) & 1ull)) status = 3;
    else status = best < INFINITY ? 0 : 1;
    a.cost[p] = status == 0 ? best : INFINITY;
    a.status[p] = status;
}

// the ns * ng (start, goal) pairs as two state arrays for the motion-test kernel
__global__ __launch_bounds__(256) void k_ms_pairs(int64_t ns, int64_t ng, int d, const double* __restrict__ S, const double* __restrict__ G,
                                                  double* __restrict__ P, double* __restrict__ Q)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ns * ng * d) return;
    const int64_t p = t / d; const int k = (int)(t % d);
    P[t] = S[(p / ng) * d + k]; Q[t] = G[(p % ng) * d + k];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------

void mpfmt_sssp_multi_free(mpfmt_ctx* ctx)
{
    for (int k = 0; k < 2; ++k) if (ctx->ms_ev[k]) hipEventDestroy(ctx->ms_ev[k]);
    ctx->ms_ev[0] = ctx->ms_ev[1] = nullptr;
}

static void ms_bytes(mpfmt_ctx* ctx)
{
    ctx->ms_bytes = (int64_t)(ctx->ms_L.bytes() + ctx->ms_A.bytes() + ctx->ms_bm.bytes() + ctx->ms_state.bytes() + ctx->ms_stage.bytes() +
                              ctx->ms_src.bytes());
}

// the buffers of one group; parents and the copy-out's staging only when asked for
static int32_t ms_ensure(mpfmt_ctx* ctx, bool parents, bool stage)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = ctx->ms_L.ensure(ctx, sizeof(double) * MS_W * (size_t)N))) return rc;
    if (parents && (rc = ctx->ms_A.ensure(ctx, sizeof(int64_t) * MS_W * (size_t)N))) return rc;
    if (stage && (rc = ctx->ms_stage.ensure(ctx, sizeof(double) * MS_W * (size_t)std::min<int64_t>(N, MS_CHUNK)))) return rc;
    if ((rc = ctx->ms_bm.ensure(ctx, sizeof(uint64_t) * 3 * (size_t)words))) return rc;
    if ((rc = ctx->ms_state.ensure(ctx, sizeof(ms_state)))) return rc;
    if ((rc = ctx->ms_state_host.ensure(ctx, sizeof(ms_state)))) return rc;
    if ((rc = ctx->ms_src.ensure(ctx, sizeof(int64_t) * MS_W))) return rc;
    for (int k = 0; k < 2; ++k) if (!ctx->ms_ev[k]) HIPCHK(ctx, hipEventCreate(&ctx->ms_ev[k]));
    ms_bytes(ctx);
    return MPFMT_OK;
}

// the rounds of one group (relax_rounds of relax_core.h)
static int32_t ms_rounds(mpfmt_ctx* ctx, const uint64_t* d_F)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    ms_state* st = (ms_state*)ctx->ms_state.get();
    ms_state* sh = (ms_state*)ctx->ms_state_host.get();
    const unsigned nb = relax_wave_blocks(ctx, N);
    int32_t rc;
    mpfmt_timed tm(ctx);
    auto round = [&](int64_t t) {
        hipLaunchKernelGGL(k_ms_relax, dim3(nb), dim3(256), 0, ctx->stream, N, words, ring_slot(t), ctx->colptr, ctx->rowval, ctx->nzval,
                           ctx->graph_free, d_F, ctx->ms_L.get(), ctx->ms_bm.get(), st);
    };
    if ((rc = relax_rounds(ctx, N, st, sh, sh->slot, round, "shortest-path relaxation did not settle within N rounds"))) return rc;
    tm.end("sssp_multi_relax");
    return MPFMT_OK;
}

// [N][64] on the device -> rows [n][N] of a host array, MS_CHUNK samples at a time
static int32_t ms_copy_out(mpfmt_ctx* ctx, const void* d_in, int n, void* host)
{
    const int64_t N = ctx->N;
    for (int64_t x0 = 0; x0 < N; x0 += MS_CHUNK) {
        const int64_t cnt = std::min<int64_t>(MS_CHUNK, N - x0);
        hipLaunchKernelGGL(k_ms_transpose, dim3((unsigned)((cnt + 63) / 64)), dim3(256), 0, ctx->stream, x0, cnt, n, (const unsigned long long*)d_in,
                           (unsigned long long*)ctx->ms_stage.get());
        HIPCHK(ctx, hipMemcpy2DAsync((char*)host + 8 * (size_t)x0, 8 * (size_t)N, ctx->ms_stage.get(), 8 * (size_t)cnt, 8 * (size_t)cnt, (size_t)n,
                                     hipMemcpyDeviceToHost, ctx->stream));
    }
    return MPFMT_OK;
}

int32_t mpfmt_sssp_multi_device(mpfmt_ctx* ctx, const int64_t* sources1, int64_t nsrc, const uint64_t* d_F, double* C_host, int64_t* A_host,
                                mpfmt_sssp_info* info)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = ms_ensure(ctx, A_host != nullptr, true))) return rc;
    ms_state* st = (ms_state*)ctx->ms_state.get();
    ms_state* sh = (ms_state*)ctx->ms_state_host.get();
    const unsigned nb = relax_wave_blocks(ctx, ctx->N);
    const unsigned nb_init = (unsigned)((std::max<int64_t>(N * MS_W, 3 * words) + 255) / 256);
    ctx->ms_groups = ctx->ms_rounds = ctx->ms_rows = 0;
    for (int64_t q0 = 0; q0 < nsrc; q0 += MS_W) {
        const int n = (int)std::min<int64_t>(MS_W, nsrc - q0);
        int64_t src0[MS_W];
        for (int s = 0; s < n; ++s) src0[s] = sources1[q0 + s] - 1;
        HIPCHK(ctx, hipMemcpyAsync(ctx->ms_src.get(), src0, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // (src0 is a stack array)
        HIPCHK(ctx, hipEventRecord(ctx->ms_ev[0], ctx->stream));
        hipLaunchKernelGGL(k_ms_init, dim3(nb_init), dim3(256), 0, ctx->stream, N, words, n, (const int64_t*)ctx->ms_src.get(), ctx->ms_L.get(),
                           ctx->ms_bm.get(), st);
        if ((rc = ms_rounds(ctx, d_F))) return rc;
        {
            mpfmt_timed tm(ctx);
            if (A_host)
                hipLaunchKernelGGL(k_ms_parents, dim3(nb), dim3(256), 0, ctx->stream, N, n, (const int64_t*)ctx->ms_src.get(), ctx->colptr, ctx->rowval,
                                   ctx->nzval, ctx->graph_free, (const double*)ctx->ms_L.get(), ctx->ms_A.get(), st);
            else
                hipLaunchKernelGGL(k_ms_reached, dim3(nb), dim3(256), 0, ctx->stream, N, (const double*)ctx->ms_L.get(), st);
            tm.end("sssp_multi_parents");
        }
        HIPCHK(ctx, hipEventRecord(ctx->ms_ev[1], ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(sh, st, sizeof(ms_state), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = ms_copy_out(ctx, ctx->ms_L.get(), n, C_host + q0 * N))) return rc;
        if (A_host && (rc = ms_copy_out(ctx, ctx->ms_A.get(), n, A_host + q0 * N))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ms_ev[0], ctx->ms_ev[1]));
        ctx->ms_groups += 1; ctx->ms_rounds += (int64_t)sh->rounds; ctx->ms_rows += (int64_t)sh->rows;
        if (info)
            for (int s = 0; s < n; ++s) {
                info[q0 + s].reached = (int64_t)sh->reached[s]; info[q0 + s].rounds = (int64_t)sh->rounds;
                info[q0 + s].relaxations = (int64_t)sh->rows; info[q0 + s].ms_device = ms;
            }
    }
    return MPFMT_OK;
}

// the cost matrix: d_S [ns][d], d_G [ng][d], the three bit arrays (start free, goal free, direct motion of pair i * ng + j), the tail lists
// of the starts and the head lists of the goals; d_cost / d_status [ns][ng] on the device
int32_t mpfmt_roadmap_matrix_device(mpfmt_ctx* ctx, const double* d_S, int64_t ns, const double* d_G, int64_t ng, const uint64_t* d_F,
                                    const uint64_t* d_sfree, const uint64_t* d_gfree, const uint64_t* d_direct, const mpfmt_rm_list& Ls,
                                    const mpfmt_rm_list& Lg, double* d_cost, int32_t* d_status, mpfmt_roadmap_matrix_info* info)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = ms_ensure(ctx, false, false))) return rc;
    ms_state* st = (ms_state*)ctx->ms_state.get();
    ms_state* sh = (ms_state*)ctx->ms_state_host.get();
    const unsigned nb_init = (unsigned)((std::max<int64_t>(N * MS_W, 3 * words) + 255) / 256);
    ctx->ms_groups = ctx->ms_rounds = ctx->ms_rows = 0;
    HIPCHK(ctx, hipEventRecord(ctx->ms_ev[0], ctx->stream));
    mpfmt_timed tm(ctx);
    for (int64_t i0 = 0; i0 < ns; i0 += MS_W) {
        const int n = (int)std::min<int64_t>(MS_W, ns - i0);
        hipLaunchKernelGGL(k_ms_clear, dim3(nb_init), dim3(256), 0, ctx->stream, N, words, n, ctx->ms_L.get(), ctx->ms_bm.get(), st);
        hipLaunchKernelGGL(k_ms_seed, dim3((unsigned)n), dim3(256), 0, ctx->stream, i0, (const int64_t*)Ls.ptr, (const int64_t*)Ls.idx1,
                           (const double*)Ls.dist, (const uint8_t*)Ls.bits, d_sfree, ctx->ms_L.get(), ctx->ms_bm.get(), st);
        if ((rc = ms_rounds(ctx, d_F))) return rc;
        ms_goal_args a{};
        a.i0 = i0; a.ns = ns; a.ng = ng; a.n = n; a.d = ctx->d; a.S = d_S; a.G = d_G; a.r2 = ctx->graph_r * ctx->graph_r;
        a.sfree = d_sfree; a.gfree = d_gfree; a.direct = d_direct;
        a.ptr = Lg.ptr; a.idx1 = Lg.idx1; a.dist = Lg.dist; a.bits = Lg.bits;
        a.L = ctx->ms_L.get(); a.cost = d_cost; a.status = d_status;
        hipLaunchKernelGGL(k_ms_goal, dim3((unsigned)((ng + 3) / 4)), dim3(256), 0, ctx->stream, a);
        HIPCHK(ctx, hipGetLastError());
        ctx->ms_groups += 1; ctx->ms_rounds += (int64_t)sh->rounds; ctx->ms_rows += (int64_t)sh->rows;
    }
    tm.end("roadmap_matrix");
    HIPCHK(ctx, hipEventRecord(ctx->ms_ev[1], ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ms_ev[0], ctx->ms_ev[1]));
    if (info) { info->groups = ctx->ms_groups; info->rounds = ctx->ms_rounds; info->ms_device = ms; }
    return MPFMT_OK;
}

int32_t mpfmt_roadmap_pairs(mpfmt_ctx* ctx, const double* d_S, int64_t ns, const double* d_G, int64_t ng, double* d_P, double* d_Q)
{
    const int64_t t = ns * ng * ctx->d;
    hipLaunchKernelGGL(k_ms_pairs, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, ctx->stream, ns, ng, (int)ctx->d, d_S, d_G, d_P, d_Q);
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}
