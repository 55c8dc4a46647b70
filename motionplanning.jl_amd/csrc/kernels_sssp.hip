// PRM* roadmap queries: the cost-to-come field of one source over the resident free-edge graph (include/mpfmt.h, "roadmap queries";
// DESIGN.md "PRM* roadmap queries").  Label-correcting PULL relaxation over the device-native CSC -- entry b of column x with row y is
// the directed edge y -> x, so a column holds exactly the candidates of its own label and the directed k-nearest graph needs no
// transpose -- with the graph, the mask and the point bitmap read in place.
//
//   round t:  for every column x that may still improve:  C[x] = min(C[x], min over usable entries whose row y changed in round t-1
//             of fl(C[y] + w)); a column that improved marks itself in the next round's bitmap.
//
// * one wavefront per column, lanes over its entries, xor-shuffle minimum;
// * three sample bitmaps in rotation: round t reads B[t % 3], marks B[(t+1) % 3] and clears B[(t+2) % 3] (last read by round t-1),
//   so no round needs a memset of its own;
// * the cost band: mlow(t) = the lowest label written in round t-1.  Every label written in round t is fl(C[y] + w) >= C[y] >= mlow(t)
//   for a y of the bitmap (by induction over the writes of the round), so a column with C[x] <= mlow(t) cannot improve and is skipped
//   before any of its entries is read: the settled interior stops costing bandwidth.  (The source, C = 0, is always skipped: that is
//   its exemption from F.)
// * labels are read and written in place while the round runs (plain aligned 8-byte loads and stores, never torn).  A reader may see
//   the label of this round or the one before -- the L2 of another XCD may hold the older one -- both are upper bounds of the fixed
//   point that only ever decrease, and the writer's bit in B[(t+1) % 3] makes the reader look again next round: values are
//   independent of the schedule, `rounds` and `relaxations` are not;
// * the per-round counters live in a ring of three slots like the bitmaps; the host reads them once per SSSP_BATCH rounds, and a round
//   whose predecessor changed nothing returns at once, so the tail of a batch costs empty launches only;
// * parents come from a separate pass over the finished labels (k_sssp_parents), a function of C alone.
#include "mpfmt_internal.h"
#include <cmath>
#include <algorithm>

#define SSSP_BATCH 8                         // rounds issued between two reads of the round state
#define SSSP_INF_BITS 0x7FF0000000000000ull

struct sssp_slot { unsigned long long changed, minbits; };
struct sssp_state {
    sssp_slot slot[3];
    unsigned long long relax, rounds, reached, pad;
};

__device__ __forceinline__ double wave_min(double v)
{
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(256) void k_sssp_init(int64_t N, int64_t words, int64_t src, double* __restrict__ C, uint64_t* __restrict__ bm,
                                                   sssp_state* __restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) C[i] = i == src ? 0.0 : INFINITY;
    if (i < 3 * words) bm[i] = (i == (src >> 6)) ? 1ull << (src & 63) : 0ull;
    if (i == 0) {
        st->slot[0].changed = 1; st->slot[0].minbits = 0ull;
        st->slot[1].changed = 0; st->slot[1].minbits = SSSP_INF_BITS;
        st->slot[2].changed = 0; st->slot[2].minbits = SSSP_INF_BITS;
        st->relax = 0; st->rounds = 0; st->reached = 0; st->pad = 0;
    }
}

__global__ __launch_bounds__(256) void k_sssp_relax(int64_t N, int64_t words, int round, const int64_t* __restrict__ colptr,
                                                    const int32_t* __restrict__ rowval, const double* __restrict__ nzval,
                                                    const uint64_t* __restrict__ efree, const uint64_t* __restrict__ F, double* C,
                                                    uint64_t* bm, sssp_state* st)
{
    const int s_in = round % 3, s_out = (round + 1) % 3, s_clr = (round + 2) % 3;
    const unsigned long long cin = st->slot[s_in].changed;
    const double mlow = __longlong_as_double((long long)st->slot[s_in].minbits);
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gtid == 0) {                                        // (the slot round + 2 will mark: nobody reads or writes it during this round)
        st->slot[s_clr].changed = 0; st->slot[s_clr].minbits = SSSP_INF_BITS;
        if (cin) st->rounds += 1;
    }
    if (cin == 0) return;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    uint64_t* bclr = bm + (int64_t)s_clr * words;
    for (int64_t w = gtid; w < words; w += nthreads) bclr[w] = 0ull;
    const uint64_t* bin = bm + (int64_t)s_in * words;
    unsigned long long* bout = (unsigned long long*)(bm + (int64_t)s_out * words);
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = nthreads >> 6;
    unsigned long long nrel = 0, nchg = 0;
    double lmin = INFINITY;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        const double cx = C[x];
        if (cx <= mlow) continue;
        if (F && !((F[x >> 6] >> (x & 63)) & 1ull)) continue;
        const int64_t b0 = colptr[x], b1 = colptr[x + 1];
        double best = INFINITY;
        for (int64_t b = b0 + lane; b < b1; b += 64) {
            const int32_t y = rowval[b];
            if (!((bin[y >> 6] >> (y & 63)) & 1ull)) continue;
            if (!((efree[b >> 6] >> (b & 63)) & 1ull)) continue;
            const double c = C[y] + nzval[b];
            ++nrel;
            best = fmin(best, c);
        }
        best = wave_min(best);
        if (best < cx) {
            if (lane == 0) {
                C[x] = best;
                atomicOr(&bout[x >> 6], 1ull << (x & 63));
                ++nchg;
                lmin = fmin(lmin, best);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) nrel += __shfl_xor(nrel, off);
    if (lane == 0) {
        if (nrel) atomicAdd(&st->relax, nrel);
        if (nchg) {
            atomicAdd(&st->slot[s_out].changed, nchg);
            atomicMin(&st->slot[s_out].minbits, (unsigned long long)__double_as_longlong(lmin));      // (labels are >= 0: their bit patterns order like the values)
        }
    }
}

// A[x] = the usable y of lowest (C[y], y) with fl(C[y] + w) == C[x], 1-based; 0 for the source and for unreached samples
__global__ __launch_bounds__(256) void k_sssp_parents(int64_t N, int64_t src, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                      const double* __restrict__ nzval, const uint64_t* __restrict__ efree,
                                                      const double* __restrict__ C, int64_t* __restrict__ A, sssp_state* st)
{
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    unsigned long long nreach = 0;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        const double cx = C[x];
        if (!(cx < INFINITY)) { if (lane == 0) A[x] = 0; continue; }
        ++nreach;
        if (x == src) { if (lane == 0) A[x] = 0; continue; }
        double cb = INFINITY; int32_t yb = 0x7fffffff;
        for (int64_t b = colptr[x] + lane; b < colptr[x + 1]; b += 64) {
            if (!((efree[b >> 6] >> (b & 63)) & 1ull)) continue;
            const int32_t y = rowval[b];
            const double cy = C[y];
            if (!(cy + nzval[b] == cx)) continue;
            if (cy < cb || (cy == cb && y < yb)) { cb = cy; yb = y; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double oc = __shfl_xor(cb, off);
            const int32_t oy = __shfl_xor(yb, off);
            if (oc < cb || (oc == cb && oy < yb)) { cb = oc; yb = oy; }
        }
        if (lane == 0) A[x] = yb == 0x7fffffff ? 0 : (int64_t)yb + 1;
    }
    if (lane == 0 && nreach) atomicAdd(&st->reached, nreach);
}

void mpfmt_sssp_free(mpfmt_ctx* ctx)
{
    for (int k = 0; k < 2; ++k) if (ctx->sssp_ev[k]) hipEventDestroy(ctx->sssp_ev[k]);
    ctx->sssp_ev[0] = ctx->sssp_ev[1] = nullptr;
}

// ---- the seeded field: an external start (include/mpfmt.h, "roadmap queries for external states") ----------------------------------------
// The start s is not a sample: it enters the relaxation as upper bounds on the labels of its usable neighbours, seed[y] = fl(0 + d(s, y)).
// C starts from min(+Inf, seed) instead of (+Inf, C[src] = 0), the round-0 bitmap holds the seeds, slot[0].changed their number and
// slot[0].minbits = 0 -- every label written later is fl(C[y] + w) >= 0 = mlow(0), so the band skip of k_sssp_relax is valid from round 0 and
// k_sssp_relax runs unchanged.  An empty seed set leaves slot[0].changed = 0: every round returns at once.
__global__ __launch_bounds__(256) void k_sssp_seed_clear(int64_t N, int64_t words, double* __restrict__ C, double* __restrict__ seed,
                                                         uint64_t* __restrict__ bm, sssp_state* __restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) { C[i] = INFINITY; seed[i] = INFINITY; }
    if (i < 3 * words) bm[i] = 0ull;
    if (i == 0) {
        st->slot[0].changed = 0; st->slot[0].minbits = 0ull;
        st->slot[1].changed = 0; st->slot[1].minbits = SSSP_INF_BITS;
        st->slot[2].changed = 0; st->slot[2].minbits = SSSP_INF_BITS;
        st->relax = 0; st->rounds = 0; st->reached = 0; st->pad = 0;
    }
}

// scatter of the usable entries of the start's near list (distinct samples: no two threads write one label)
__global__ __launch_bounds__(256) void k_sssp_seed(int64_t n, const int64_t* __restrict__ idx1, const double* __restrict__ dist,
                                                   const uint8_t* __restrict__ bits, double* __restrict__ C, double* __restrict__ seed,
                                                   uint64_t* bm, sssp_state* st)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool us = e < n && (bits[e] & 2);
    if (us) {
        const int64_t y = idx1[e] - 1;
        const double sd = 0.0 + dist[e];
        C[y] = sd; seed[y] = sd;
        atomicOr((unsigned long long*)&bm[y >> 6], 1ull << (y & 63));
    }
    const unsigned long long m = __ballot(us);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st->slot[0].changed, (unsigned long long)__popcll(m));
}

// k_sssp_parents with the start as index 0 of label 0: seed[x] == C[x] makes s the parent of lowest (C, index), A[x] = -1
__global__ __launch_bounds__(256) void k_sssp_parents_seeded(int64_t N, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                             const double* __restrict__ nzval, const uint64_t* __restrict__ efree,
                                                             const double* __restrict__ C, const double* __restrict__ seed,
                                                             int64_t* __restrict__ A, sssp_state* st)
{
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    unsigned long long nreach = 0;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        const double cx = C[x];
        if (!(cx < INFINITY)) { if (lane == 0) A[x] = 0; continue; }
        ++nreach;
        if (seed[x] == cx) { if (lane == 0) A[x] = -1; continue; }
        double cb = INFINITY; int32_t yb = 0x7fffffff;
        for (int64_t b = colptr[x] + lane; b < colptr[x + 1]; b += 64) {
            if (!((efree[b >> 6] >> (b & 63)) & 1ull)) continue;
            const int32_t y = rowval[b];
            const double cy = C[y];
            if (!(cy + nzval[b] == cx)) continue;
            if (cy < cb || (cy == cb && y < yb)) { cb = cy; yb = y; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double oc = __shfl_xor(cb, off);
            const int32_t oy = __shfl_xor(yb, off);
            if (oc < cb || (oc == cb && oy < yb)) { cb = oc; yb = oy; }
        }
        if (lane == 0) A[x] = yb == 0x7fffffff ? 0 : (int64_t)yb + 1;
    }
    if (lane == 0 && nreach) atomicAdd(&st->reached, nreach);
}

// One field over the resident graph and mask: from a sample (source0 >= 0: k_sssp_init, k_sssp_parents) or from the usable entries of an
// external start's near list (source0 < 0: k_sssp_seed_clear + k_sssp_seed, k_sssp_parents_seeded); the rounds are the same.
struct sssp_seeds { const int64_t* idx1; const double* dist; const uint8_t* bits; int64_t n; };

static int32_t sssp_run(mpfmt_ctx* ctx, int64_t source0, const sssp_seeds* sd, const uint64_t* d_F, double* C_host, int64_t* A_host, mpfmt_sssp_info* info)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = ctx->sssp_C.ensure(ctx, sizeof(double) * (size_t)N))) return rc;
    if (sd && (rc = ctx->sssp_seed.ensure(ctx, sizeof(double) * (size_t)N))) return rc;
    if ((rc = ctx->sssp_A.ensure(ctx, sizeof(int64_t) * (size_t)N))) return rc;
    if ((rc = ctx->sssp_bm.ensure(ctx, sizeof(uint64_t) * 3 * (size_t)words))) return rc;
    if ((rc = ctx->sssp_state.ensure(ctx, sizeof(sssp_state)))) return rc;
    if ((rc = ctx->sssp_state_host.ensure(ctx, sizeof(sssp_state)))) return rc;
    for (int k = 0; k < 2; ++k) if (!ctx->sssp_ev[k]) HIPCHK(ctx, hipEventCreate(&ctx->sssp_ev[k]));
    sssp_state* st = (sssp_state*)ctx->sssp_state.get();
    sssp_state* sh = (sssp_state*)ctx->sssp_state_host.get();
    // one wavefront per column, grid-stride: enough waves to fill the chip several times over (a skipped column costs one load)
    const int64_t blocks_all = (N + 3) / 4;
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks_all, (int64_t)ctx->num_cus * 16));
    const unsigned nb_init = (unsigned)((std::max<int64_t>(N, 3 * words) + 255) / 256);
    HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[0], ctx->stream));
    {
        mpfmt_timed tm(ctx);
        if (!sd) {
            hipLaunchKernelGGL(k_sssp_init, dim3(nb_init), dim3(256), 0, ctx->stream, N, words, source0, ctx->sssp_C, ctx->sssp_bm, st);
        } else {
            hipLaunchKernelGGL(k_sssp_seed_clear, dim3(nb_init), dim3(256), 0, ctx->stream, N, words, ctx->sssp_C, ctx->sssp_seed, ctx->sssp_bm, st);
            if (sd->n > 0)
                hipLaunchKernelGGL(k_sssp_seed, dim3((unsigned)((sd->n + 255) / 256)), dim3(256), 0, ctx->stream, sd->n, sd->idx1, sd->dist, sd->bits,
                                   ctx->sssp_C, ctx->sssp_seed, ctx->sssp_bm, st);
        }
        // every non-final round lowers at least one label for good, and a label is the fold of a simple path: N rounds bound the loop
        int64_t round = 0;
        bool done = false;
        while (!done) {
            if (round > N + SSSP_BATCH) return mpfmt_fail(ctx, MPFMT_ERR_HIP, "shortest-path relaxation did not settle within N rounds");
            for (int q = 0; q < SSSP_BATCH; ++q, ++round)
                hipLaunchKernelGGL(k_sssp_relax, dim3(nb), dim3(256), 0, ctx->stream, N, words, (int)(round % 3), ctx->colptr, ctx->rowval, ctx->nzval,
                                   ctx->graph_free, d_F, ctx->sssp_C, ctx->sssp_bm, st);
            HIPCHK(ctx, hipMemcpyAsync(sh, st, sizeof(sssp_state), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            done = sh->slot[round % 3].changed == 0;        // what the batch's last round marked for the next one
        }
        tm.end("sssp_relax");
    }
    {
        mpfmt_timed tm(ctx);
        if (!sd)
            hipLaunchKernelGGL(k_sssp_parents, dim3(nb), dim3(256), 0, ctx->stream, N, source0, ctx->colptr, ctx->rowval, ctx->nzval, ctx->graph_free,
                               ctx->sssp_C, ctx->sssp_A, st);
        else
            hipLaunchKernelGGL(k_sssp_parents_seeded, dim3(nb), dim3(256), 0, ctx->stream, N, ctx->colptr, ctx->rowval, ctx->nzval, ctx->graph_free,
                               ctx->sssp_C, ctx->sssp_seed, ctx->sssp_A, st);
        tm.end("sssp_parents");
    }
    HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[1], ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sh, st, sizeof(sssp_state), hipMemcpyDeviceToHost, ctx->stream));
    if (C_host) HIPCHK(ctx, hipMemcpyAsync(C_host, ctx->sssp_C, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
    if (A_host) HIPCHK(ctx, hipMemcpyAsync(A_host, ctx->sssp_A, sizeof(int64_t) * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->sssp_ev[0], ctx->sssp_ev[1]));
    ctx->sssp_rounds = (int64_t)sh->rounds; ctx->sssp_relax = (int64_t)sh->relax; ctx->sssp_reached = (int64_t)sh->reached;
    if (info) { info->reached = ctx->sssp_reached; info->rounds = ctx->sssp_rounds; info->relaxations = ctx->sssp_relax; info->ms_device = ms; }
    return MPFMT_OK;
}

int32_t mpfmt_sssp_device(mpfmt_ctx* ctx, int64_t source0, const uint64_t* d_F, double* C_host, int64_t* A_host, mpfmt_sssp_info* info)
{
    return sssp_run(ctx, source0, nullptr, d_F, C_host, A_host, info);
}

int32_t mpfmt_sssp_seeded_device(mpfmt_ctx* ctx, const int64_t* d_idx1, const double* d_dist, const uint8_t* d_bits, int64_t n, const uint64_t* d_F,
                                 mpfmt_sssp_info* info)
{
    const sssp_seeds sd{d_idx1, d_dist, d_bits, n};
    return sssp_run(ctx, -1, &sd, d_F, nullptr, nullptr, info);
}
