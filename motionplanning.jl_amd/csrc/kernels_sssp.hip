// PRM* roadmap queries: the cost-to-come field of one source over the resident free-edge graph (include/mpfmt.h, "roadmap queries";
// DESIGN.md "PRM* roadmap queries").  Label-correcting PULL relaxation over the device-native CSC -- entry b of column x with row y is
// the directed edge y -> x, so a column holds exactly the candidates of its own label and the directed k-nearest graph needs no
// transpose -- with the graph, the mask and the point bitmap read in place.
//
//   round t:  for every column x that may still improve:  C[x] = min(C[x], min over usable entries whose row y changed in round t-1
//             of fl(C[y] + w)); a column that improved marks itself in the next round's bitmap.
//
// * one wavefront per column, lanes over its entries, xor-shuffle minimum (column_fold of relax_core.h);
// * the ring of three sample bitmaps and round slots, the cost band, the in-place label reads and the host loop are those of
//   relax_core.h, where their arguments are written down;
// * parents come from a separate pass over the finished labels (k_sssp_parents), a function of C alone.
#include "relax_core.h"

struct sssp_state {
    band_slot slot[3];
    unsigned long long relax, rounds, reached, pad;
};

__global__ __launch_bounds__(256) void k_sssp_init(int64_t N, int64_t words, int64_t src, double* __restrict__ C, uint64_t* __restrict__ bm,
                                                   sssp_state* __restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) C[i] = i == src ? 0.0 : INFINITY;
    if (i < 3 * words) bm[i] = (i == (src >> 6)) ? 1ull << (src & 63) : 0ull;
    if (i == 0) {
        band_ring_init(st->slot, 1);
        st->relax = 0; st->rounds = 0; st->reached = 0; st->pad = 0;
    }
}

__global__ __launch_bounds__(256) void k_sssp_relax(int64_t N, int64_t words, int round, const int64_t* __restrict__ colptr,
                                                    const int32_t* __restrict__ rowval, const double* __restrict__ nzval,
                                                    const uint64_t* __restrict__ efree, const uint64_t* __restrict__ F, double* C,
                                                    uint64_t* bm, sssp_state* st)
{
    const ring_idx r = ring_at(round);
    const double mlow = label_of_bits(st->slot[r.in].minbits);
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const uint64_t* bin;
    unsigned long long* bout;
    if (!ring_round(st->slot, &st->rounds, bm, words, r, gtid, nthreads, bin, bout)) return;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = nthreads >> 6;
    unsigned long long nrel = 0, nchg = 0;
    double lmin = INFINITY;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        const double cx = C[x];
        if (cx <= mlow) continue;
        if (F && !bit_of(F, x)) continue;
        const double best = column_fold<true, false>(colptr[x], colptr[x + 1], lane, rowval, nzval, efree, bin, C, nrel);
        if (best < cx) {
            if (lane == 0) {
                C[x] = best;
                atomicOr(&bout[x >> 6], 1ull << (x & 63));
                ++nchg;
                lmin = fmin(lmin, best);
            }
        }
    }
    nrel = wave_sum(nrel);
    if (lane == 0) {
        if (nrel) atomicAdd(&st->relax, nrel);
        if (nchg) {
            atomicAdd(&st->slot[r.out].changed, nchg);
            atomicMin(&st->slot[r.out].minbits, label_bits(lmin));
        }
    }
}

// A[x] = the usable y of lowest (C[y], y) with fl(C[y] + w) == C[x], 1-based; 0 for the source and for unreached samples
__global__ __launch_bounds__(256) void k_sssp_parents(int64_t N, int64_t src, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                      const double* __restrict__ nzval, const uint64_t* __restrict__ efree,
                                                      const double* __restrict__ C, int64_t* __restrict__ A, sssp_state* st)
{
    parents_body<false, false>(N, src, colptr, rowval, nzval, efree, C, nullptr, A, nullptr, &st->reached);
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
        band_ring_init(st->slot, 0);
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
    parents_body<true, false>(N, -1, colptr, rowval, nzval, efree, C, seed, A, nullptr, &st->reached);
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
    const unsigned nb = relax_wave_blocks(ctx, N);
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
        auto round = [&](int64_t t) {
            hipLaunchKernelGGL(k_sssp_relax, dim3(nb), dim3(256), 0, ctx->stream, N, words, ring_slot(t), ctx->colptr, ctx->rowval,
                               ctx->nzval, ctx->graph_free, d_F, ctx->sssp_C, ctx->sssp_bm, st);
        };
        if ((rc = relax_rounds(ctx, N, st, sh, sh->slot, round, "shortest-path relaxation did not settle within N rounds"))) return rc;
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
