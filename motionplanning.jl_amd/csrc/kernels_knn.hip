// Exact k-nearest graph (connections = :K of fmtstar!, fmt.jl:6,17-19; mutualknnF! / knnB!, nearneighbors.jl:9-11).
//
// knn(v) = the k_eff = min(k, N - 1) samples i != v smallest under the total order (d2(v, i), i), d2 in the canonical arithmetic of
// kernels_rdisc.hip (fp64, index order, unfused).  Column v of the CSC = knn(v), rows ascending by index, nzval = sqrt(d2).
//
// One workgroup answers one column.  Its candidates are the samples with d2 <= rho^2, found through the cell-sorted index of
// mpfmt_build_grid: the tiles (64 consecutive samples of the sorted order, with their tight boxes) are pruned box against ball in two
// levels -- a supertile is 64 consecutive tiles -- so the distance tests of a column go with the ball's content, not with N.  The
// k_eff smallest keys are found by a radix select over the 96-bit key (bit pattern of the non-negative d2, then the index), eight
// bits a pass with a 256-bin LDS histogram; every pass enumerates the candidates again (recomputing d2 is cheaper than keeping it),
// and the select stops at the first pass whose bucket is taken whole -- for samples in general position after four or five passes.
// The selected samples of a column of at most KNN_LDS_K entries are collected in LDS and put in index order by a bitonic network;
// a longer column marks them in a bitmap over the sample indices (one per resident workgroup, in HBM) and reads it back in index
// order -- N/64 words per column, next to an output of more than KNN_LDS_K entries.  Either way: the ascending-rows contract.  A column with fewer than k_eff candidates is appended to a list and
// answered by a later round at a larger radius; the last round has no radius (every tile survives: the exact scan of all N).
#include "mpfmt_internal.h"
#include <algorithm>
#include <cmath>
#include <string.h>

#define KNN_T 256                 // threads of a column's workgroup
#define KNN_ST 64                 // tiles per supertile
#define KNN_LDS_K 2048            // longest column that is put in index order in LDS (longer ones: the bitmap)

struct knn_args {
    const double* Xt;             // [ntiles][d][64]
    const double* Xo;             // [N][d]
    const int32_t* perm;          // [ntiles * 64] sorted position -> sample (-1: pad)
    const double* tile_lo; const double* tile_hi;      // [ntiles][d]
    const double* st_lo; const double* st_hi;          // [nst][d]
    int64_t N, ntiles, nst;
    int32_t d;
    int64_t keff;
    double rho2;                  // candidates: d2 <= rho2 (+inf: all)
    double rho2_pad;              // pruning threshold (rho2 with a margin for the rounding of the box distance)
    const int32_t* cols;          // the round's columns (nullptr: all of them)
    int64_t ncols;
    unsigned long long* bitmap;   // [workgroups][nwords], all zero between columns
    int64_t nwords;
    int32_t* rowval; double* nzval;
    int32_t* short_list; int32_t* short_cnt;
    unsigned long long* stats;    // [0] pairs tested (first pass of each column), [1] bit pattern of the longest selected d2
};

__global__ __launch_bounds__(64) void k_knn_supertiles(const double* __restrict__ tile_lo, const double* __restrict__ tile_hi, int64_t ntiles, int d,
                                                       double* __restrict__ st_lo, double* __restrict__ st_hi)
{
    const int lane = threadIdx.x;
    const int64_t st = blockIdx.x, t = st * KNN_ST + lane;
    for (int i = 0; i < d; ++i) {
        double lo = t < ntiles ? tile_lo[t * d + i] : INFINITY, hi = t < ntiles ? tile_hi[t * d + i] : -INFINITY;
        for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off)); hi = fmax(hi, __shfl_xor(hi, off)); }
        if (lane == 0) { st_lo[st * d + i] = lo; st_hi[st * d + i] = hi; }
    }
}

__global__ void k_knn_colptr(int64_t* __restrict__ colptr, int64_t N, int64_t keff)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v <= N) colptr[v] = v * keff;
}

// squared distance of v to a box (0 inside)
__device__ __forceinline__ double knn_box_d2(const double* __restrict__ lo, const double* __restrict__ hi, const double* s_v, int d)
{
    double s = 0.0;
    for (int i = 0; i < d; ++i) {
        const double x = s_v[i];
        const double t = fmax(fmax(lo[i] - x, x - hi[i]), 0.0);
        s += t * t;
    }
    return s;
}

// f(is_candidate, key, idx) for every sample of every tile that survives the pruning; whole wavefronts call it together.
template <class F>
__device__ __forceinline__ void knn_enumerate(const knn_args& a, const double* s_v, int32_t v, F&& f)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d = a.d;
    for (int64_t st = wave; st < a.nst; st += KNN_T / 64) {
        if (knn_box_d2(a.st_lo + st * d, a.st_hi + st * d, s_v, d) > a.rho2_pad) continue;
        const int64_t tl = st * KNN_ST + lane;
        bool ok = false;
        if (tl < a.ntiles) ok = !(knn_box_d2(a.tile_lo + tl * d, a.tile_hi + tl * d, s_v, d) > a.rho2_pad);
        unsigned long long m = __ballot(ok);
        while (m) {
            const int b = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int64_t t = st * KNN_ST + b;
            const int32_t idx = a.perm[t * 64 + lane];
            double d2 = 0.0;
            for (int i = 0; i < d; ++i) {
                double tt = s_v[i] - a.Xt[(t * d + i) * 64 + lane];
                tt = tt * tt;
                d2 = (i == 0) ? tt : d2 + tt;
            }
            const bool real = idx >= 0 && idx != v;
            f(real, real && d2 <= a.rho2, (unsigned long long)__double_as_longlong(d2), (uint32_t)idx);
        }
    }
}

// pass p of the select looks at digit p of the key (d2 bits: digits 0..7, index: digits 8..11) among the candidates whose first p
// digits equal the prefix
__device__ __forceinline__ bool knn_match(int p, unsigned long long key, uint32_t idx, unsigned long long pk, uint32_t pi)
{
    if (p == 0) return true;
    if (p <= 8) return (key >> (64 - 8 * p)) == (pk >> (64 - 8 * p));
    const int s = 32 - 8 * (p - 8);
    return key == pk && (idx >> s) == (pi >> s);
}
__device__ __forceinline__ uint32_t knn_digit(int p, unsigned long long key, uint32_t idx)
{
    return p < 8 ? (uint32_t)(key >> (56 - 8 * p)) & 255u : (idx >> (24 - 8 * (p - 8))) & 255u;
}
// the first p + 1 digits are not above the prefix's
__device__ __forceinline__ bool knn_selected(int p, unsigned long long key, uint32_t idx, unsigned long long pk, uint32_t pi)
{
    if (p < 8) return (key >> (56 - 8 * p)) <= (pk >> (56 - 8 * p));
    const int s = 24 - 8 * (p - 8);
    return key < pk || (key == pk && (idx >> s) <= (pi >> s));
}

__global__ __launch_bounds__(KNN_T) void k_knn_select(knn_args a)
{
    __shared__ uint32_t s_hist[256];
    __shared__ double s_v[MPFMT_MAX_DIM];
    __shared__ unsigned long long s_pk;
    __shared__ uint32_t s_pi;
    __shared__ long long s_krem;
    __shared__ int s_flag;                                    // 0: next pass, 1: selection known, 2: too few candidates
    __shared__ long long s_wsum[KNN_T / 64];
    __shared__ uint32_t s_sel[KNN_LDS_K];
    __shared__ int s_nsel;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long* bm = a.bitmap ? a.bitmap + (size_t)blockIdx.x * (size_t)a.nwords : nullptr;
    unsigned long long tested = 0, maxkey = 0;
    const int64_t W = (a.nwords + KNN_T - 1) / KNN_T;
    const bool in_lds = a.keff <= KNN_LDS_K;
    int n2 = 1;
    while (in_lds && n2 < a.keff) n2 <<= 1;
    for (int64_t c = blockIdx.x; c < a.ncols; c += gridDim.x) {
        const int32_t v = a.cols ? a.cols[c] : (int32_t)c;
        __syncthreads();
        if (tid < a.d) s_v[tid] = a.Xo[(int64_t)v * a.d + tid];
        s_hist[tid] = 0;
        if (tid == 0) { s_pk = 0; s_pi = 0; s_krem = a.keff; s_flag = 0; }
        __syncthreads();
        unsigned long long pk = 0;
        uint32_t pi = 0;
        int flag = 0, p = 0;
        for (; p < 12; ++p) {
            knn_enumerate(a, s_v, v, [&](bool real, bool cand, unsigned long long key, uint32_t idx) {
                if (p == 0 && real) ++tested;
                if (cand && knn_match(p, key, idx, pk, pi)) atomicAdd(&s_hist[knn_digit(p, key, idx)], 1u);
            });
            __syncthreads();
            if (wave == 0) {
                long long h[4], sum = 0;
                for (int j = 0; j < 4; ++j) { h[j] = s_hist[4 * lane + j]; sum += h[j]; s_hist[4 * lane + j] = 0; }
                long long inc = sum;
                for (int off = 1; off < 64; off <<= 1) { const long long u = __shfl_up(inc, off); if (lane >= off) inc += u; }
                const long long total = __shfl(inc, 63), krem = s_krem, exc = inc - sum;
                if (p == 0 && total < a.keff) {
                    if (lane == 0) s_flag = 2;
                } else if (exc < krem && krem <= inc) {           // the lane whose four bins hold the krem-th candidate
                    long long acc = exc;
                    for (int j = 0; j < 4; ++j) {
                        if (acc + h[j] >= krem) {
                            const unsigned long long bin = (unsigned long long)(4 * lane + j);
                            if (p < 8) s_pk = pk | (bin << (56 - 8 * p)); else s_pi = pi | ((uint32_t)bin << (24 - 8 * (p - 8)));
                            s_krem = krem - acc;
                            s_flag = (h[j] == krem - acc) ? 1 : 0;
                            break;
                        }
                        acc += h[j];
                    }
                }
            }
            __syncthreads();
            flag = s_flag; pk = s_pk; pi = s_pi;
            if (flag) break;
        }
        if (flag == 2) {
            if (tid == 0) a.short_list[atomicAdd(a.short_cnt, 1)] = v;
            continue;
        }
        if (p > 11) p = 11;
        int32_t* rv = a.rowval + (int64_t)v * a.keff;
        double* nz = a.nzval + (int64_t)v * a.keff;
        if (in_lds) {
            // a column of at most KNN_LDS_K entries: the selected indices are collected in LDS, put in ascending order by a bitonic
            // network (pads = 0xffffffff) and written out with their distances
            for (int i = tid; i < n2; i += KNN_T) s_sel[i] = 0xffffffffu;
            if (tid == 0) s_nsel = 0;
            __syncthreads();
            knn_enumerate(a, s_v, v, [&](bool real, bool cand, unsigned long long key, uint32_t idx) {
                if (cand && knn_selected(p, key, idx, pk, pi)) {
                    const int pos = atomicAdd(&s_nsel, 1);
                    if (pos < n2) s_sel[pos] = idx;
                    if (key > maxkey) maxkey = key;
                }
            });
            __syncthreads();
            for (int ks = 2; ks <= n2; ks <<= 1)
                for (int j = ks >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < n2; i += KNN_T) {
                        const int q = i ^ j;
                        if (q > i) {
                            const uint32_t x = s_sel[i], y = s_sel[q];
                            if ((x > y) == ((i & ks) == 0)) { s_sel[i] = y; s_sel[q] = x; }
                        }
                    }
                    __syncthreads();
                }
            for (int64_t o = tid; o < a.keff; o += KNN_T) {
                const int64_t i = s_sel[o];
                if (i >= a.N) continue;
                double d2 = 0.0;
                for (int q = 0; q < a.d; ++q) {
                    double tt = s_v[q] - a.Xo[i * a.d + q];
                    tt = tt * tt;
                    d2 = (q == 0) ? tt : d2 + tt;
                }
                rv[o] = (int32_t)i; nz[o] = sqrt(d2);
            }
            continue;
        }
        // a longer column: mark the selection in the bitmap ...
        knn_enumerate(a, s_v, v, [&](bool real, bool cand, unsigned long long key, uint32_t idx) {
            if (cand && knn_selected(p, key, idx, pk, pi)) {
                atomicOr(&bm[idx >> 6], 1ull << (idx & 63));
                if (key > maxkey) maxkey = key;
            }
        });
        __threadfence();
        __syncthreads();
        // ... and read it back in index order: thread = W consecutive words
        const int64_t w0 = std::min<int64_t>(a.nwords, (int64_t)tid * W), w1 = std::min<int64_t>(a.nwords, w0 + W);
        long long cnt = 0;
        for (int64_t w = w0; w < w1; ++w) cnt += __popcll(__hip_atomic_load(&bm[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        long long inc = cnt;
        for (int off = 1; off < 64; off <<= 1) { const long long u = __shfl_up(inc, off); if (lane >= off) inc += u; }
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        long long off = inc - cnt;
        for (int q = 0; q < wave; ++q) off += s_wsum[q];
        for (int64_t w = w0; w < w1; ++w) {
            unsigned long long word = __hip_atomic_load(&bm[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!word) continue;
            __hip_atomic_store(&bm[w], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (word) {
                const int b = __ffsll((long long)word) - 1;
                word &= word - 1;
                const int64_t i = w * 64 + b;
                double d2 = 0.0;
                for (int q = 0; q < a.d; ++q) {
                    double tt = s_v[q] - a.Xo[i * a.d + q];
                    tt = tt * tt;
                    d2 = (q == 0) ? tt : d2 + tt;
                }
                if (off < a.keff) { rv[off] = (int32_t)i; nz[off] = sqrt(d2); }
                ++off;
            }
        }
    }
    if (tested) atomicAdd(&a.stats[0], tested);
    if (maxkey) atomicMax(&a.stats[1], maxkey);
}

// mutual bit of entry e (row y in column x): x in knn(y) -- a binary search of x in the ascending column y
__global__ __launch_bounds__(256) void k_knn_mutual(const int32_t* __restrict__ rowval, int64_t keff, int64_t N, int64_t nnz, unsigned long long* __restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool m = false;
    if (e < nnz && (uint32_t)rowval[e] < (uint64_t)N) {
        const int32_t x = (int32_t)(e / keff);
        const int32_t* col = rowval + (int64_t)rowval[e] * keff;
        int64_t lo = 0, hi = keff;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (col[mid] < x) lo = mid + 1; else hi = mid; }
        m = lo < keff && col[lo] == x;
    }
    const unsigned long long bits = __ballot(m);
    if ((threadIdx.x & 63) == 0 && e < nnz) out[e >> 6] = bits;
}

// volume of the unit ball of R^n
static double unit_ball(int n) { return std::pow(M_PI, 0.5 * n) / std::tgamma(0.5 * n + 1.0); }

int32_t mpfmt_knn_build(mpfmt_ctx* ctx, int64_t k)
{
    const int64_t N = ctx->N;
    const int d = ctx->d;
    const int64_t keff = std::min<int64_t>(k, N - 1), nnz = N * std::max<int64_t>(keff, 0);
    int32_t rc;
    if ((rc = mpfmt_side_join(ctx))) return rc;
    // whatever graph the ctx held is gone (the arrays are shared); a failed build leaves none
    ctx->knn_k = 0;
    ctx->graph_r = -1.0; ctx->graph_counted = ctx->graph_filled = ctx->graph_swept = false;
    ctx->steer_counted = ctx->steer_filled = ctx->steer_swept = false;
    ctx->pool_valid = false; ctx->rowpos_valid = false; ctx->pend_valid = false; ctx->spec_ready = false; ctx->tptr_valid = false;
    ctx->knn_pairs = 0; ctx->knn_rounds = 0; ctx->knn_short = 0; ctx->knn_scan = 0;
    if ((rc = ctx->colptr.ensure(ctx, sizeof(int64_t) * (size_t)(N + 1)))) return rc;
    if ((rc = ctx->rowval.ensure(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(nnz, 1)))) return rc;
    if ((rc = ctx->nzval.ensure(ctx, sizeof(double) * (size_t)std::max<int64_t>(nnz, 1)))) return rc;
    const int64_t mwords = (nnz + 63) / 64;
    if ((rc = ctx->knn_mutual.ensure(ctx, sizeof(uint64_t) * (size_t)std::max<int64_t>(mwords, 1)))) return rc;
    hipLaunchKernelGGL(k_knn_colptr, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, ctx->stream, ctx->colptr, N, std::max<int64_t>(keff, 0));
    double longest = 0.0;
    if (nnz > 0) {
        // The first radius: the ball that holds KNN_C * k_eff samples of a uniform density over the bounding box (its axes of no
        // extent left out), so that an interior column finds its neighbours at once.  A column near m faces of the box sees 1 / 2^m of
        // that ball; the second round doubles the radius (2^d times the volume: a corner column is back at KNN_C * k_eff), the third
        // has none.  A k_eff of a quarter of the samples or more goes to the scan directly.
        const double KNN_C = 2.0;
        int de = 0;
        double vol = 1.0;
        for (int i = 0; i < d; ++i) { const double e = ctx->bb_hi[i] - ctx->bb_lo[i]; if (e > 0.0 && std::isfinite(e)) { vol *= e; ++de; } }
        double rho0 = INFINITY;
        if (de > 0 && keff * 4 < N) rho0 = std::pow(KNN_C * (double)keff * vol / ((double)N * unit_ball(de)), 1.0 / de);
        if (!(rho0 > 0.0)) rho0 = INFINITY;
        {
            mpfmt_timed tc(ctx);
            if ((rc = mpfmt_build_grid(ctx, std::isfinite(rho0) ? rho0 : 0.0, true))) return rc;
            const int64_t nst = (ctx->ntiles + KNN_ST - 1) / KNN_ST;
            if ((rc = ctx->knn_st.ensure(ctx, sizeof(double) * 2 * (size_t)nst * d))) return rc;
            hipLaunchKernelGGL(k_knn_supertiles, dim3((unsigned)nst), dim3(64), 0, ctx->stream, (const double*)ctx->tile_lo, (const double*)ctx->tile_hi,
                               ctx->ntiles, d, ctx->knn_st, ctx->knn_st + nst * d);
            tc.end("knn_candidates");
        }
        const int64_t nst = (ctx->ntiles + KNN_ST - 1) / KNN_ST;
        const int64_t nwords = (N + 63) / 64;
        const int64_t maxwg = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)8 * ctx->num_cus));
        const bool use_bitmap = keff > KNN_LDS_K;               // (columns of at most KNN_LDS_K entries are ordered in LDS)
        if (use_bitmap && (rc = ctx->knn_bitmap.ensure(ctx, sizeof(uint64_t) * (size_t)maxwg * (size_t)nwords))) return rc;
        // short lists A | B, then their counters and the two statistics words
        if ((rc = ctx->knn_lists.ensure(ctx, sizeof(int32_t) * 2 * (size_t)N + 64))) return rc;
        int32_t* listA = (int32_t*)ctx->knn_lists.get();
        int32_t* listB = listA + N;
        char* tail = (char*)(listB + N);
        tail += (8 - ((uintptr_t)tail & 7)) & 7;
        unsigned long long* stats = (unsigned long long*)tail;
        int32_t* cnts = (int32_t*)(stats + 2);
        if (use_bitmap) HIPCHK(ctx, hipMemsetAsync(ctx->knn_bitmap, 0, sizeof(uint64_t) * (size_t)maxwg * (size_t)nwords, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long) + 2 * sizeof(int32_t), ctx->stream));
        knn_args a;
        a.Xt = ctx->Xt; a.Xo = ctx->Xo; a.perm = ctx->perm; a.tile_lo = ctx->tile_lo; a.tile_hi = ctx->tile_hi;
        a.st_lo = ctx->knn_st; a.st_hi = ctx->knn_st + nst * d;
        a.N = N; a.ntiles = ctx->ntiles; a.nst = nst; a.d = d; a.keff = keff;
        a.bitmap = use_bitmap ? (unsigned long long*)ctx->knn_bitmap.get() : nullptr; a.nwords = nwords;
        a.rowval = ctx->rowval; a.nzval = ctx->nzval; a.stats = stats;
        mpfmt_timed ts(ctx);
        const double radius[3] = {rho0, 2.0 * rho0, INFINITY};
        const int32_t* cols = nullptr;
        int64_t ncols = N;
        for (int round = 0; round < 3 && ncols > 0; ++round) {
            const double rho = radius[round];
            if (round > 0 && !std::isfinite(radius[round - 1])) break;
            a.rho2 = std::isfinite(rho) ? rho * rho : INFINITY;
            a.rho2_pad = std::isfinite(rho) ? rho * rho * (1.0 + 1e-6) : INFINITY;
            a.cols = cols; a.ncols = ncols;
            a.short_list = (round & 1) ? listB : listA; a.short_cnt = cnts + (round & 1);
            if (round == 2) HIPCHK(ctx, hipMemsetAsync(cnts, 0, sizeof(int32_t), ctx->stream));
            hipLaunchKernelGGL(k_knn_select, dim3((unsigned)std::min<int64_t>(ncols, maxwg)), dim3(KNN_T), 0, ctx->stream, a);
            HIPCHK(ctx, hipGetLastError());
            int32_t nshort = 0;
            HIPCHK(ctx, hipMemcpyAsync(&nshort, a.short_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            ctx->knn_rounds += 1;
            if (!std::isfinite(rho)) ctx->knn_scan = ncols;
            if (round == 0) ctx->knn_short = nshort;
            if (!std::isfinite(rho) && nshort != 0) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "k-nearest scan left %d columns short", (int)nshort);
            cols = a.short_list; ncols = nshort;
        }
        unsigned long long st[2];
        HIPCHK(ctx, hipMemcpyAsync(st, stats, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ts.end("knn_select");
        ctx->knn_pairs = (int64_t)st[0];
        double maxd2;
        memcpy(&maxd2, &st[1], sizeof maxd2);
        longest = std::sqrt(maxd2);
        mpfmt_timed tmu(ctx);
        hipLaunchKernelGGL(k_knn_mutual, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, ctx->stream, (const int32_t*)ctx->rowval, keff, N, nnz,
                           (unsigned long long*)ctx->knn_mutual.get());
        HIPCHK(ctx, hipGetLastError());
        tmu.end("knn_mutual");
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->nnz = nnz;
    // the sweep culls the obstacles of a column with the graph's radius: every entry of this graph is at most `longest` long
    ctx->graph_r = longest * (1.0 + 1e-9);
    ctx->graph_counted = ctx->graph_filled = true; ctx->graph_epoch += 1; ctx->graph_imported = false;
    ctx->knn_k = k;
    return MPFMT_OK;
}
