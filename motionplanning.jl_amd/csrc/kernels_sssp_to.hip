// PRM* roadmap queries: the cost-to-go field of a target set over the resident free-edge graph (include/mpfmt.h, "cost-to-go";
// DESIGN.md 7i).  G[y] = the least fl(G[x] + w_yx) over usable edges y -> x, G = 0 on the targets: the policy "from every sample, the
// optimal cost to the goal set and the next sample on the way" on a DIRECTED graph.
//
// The device-native CSC gives a column x its in-edges (entry b, row y: the edge y -> x).  The forward field pulls along them; the
// cost-to-go pushes along the very same entries -- a label that dropped at x offers fl(G[x] + w) to every row y of column x -- so the
// graph, the mask and the point bitmap are read in place here too: no transpose, no copy, 64-bit entry indices throughout.
//
//   round t:  for every x of B[t % 3] (& F with checkpts): one wavefront loads G[x] once, its lanes stride over the entries of column x;
//             a free entry with row y: cand = fl(G[x] + w); a plain load of G[y] first (a stale value is only ever LARGER: labels only
//             decrease, so it can cost a wasted atomic, never a missed one), then a 64-bit atomicMin on the bit pattern (labels are
//             non-negative doubles: their bits order like their values); a returned old value above cand marks y in B[(t+1) % 3].
//
// * rounds are separate launches; three bitmaps in rotation, the ring of relax_core.h (its slots carry the count alone: the push has no
//   cost band); a fourth bitmap holds the targets for the successor passes;
// * the work unit of a wavefront is a quarter (16 bits) of a bitmap word: the unit is wave-uniform, so the column loop has no divergence;
// * the value of G[x] a round pushes may be the one of the kernel boundary or one lowered meanwhile by another wavefront: both are upper
//   bounds of the fixed point, and whoever lowered x marked it for the next round.  Nothing waits on another workgroup;
// * fl(a + w) is nondecreasing in a and >= a, a label only ever strictly decreases and is the fold of a simple path: the rounds end, at
//   the least fixed point, whose bits do not depend on the schedule (the argument of DESIGN.md 7c on the reversed graph);
// * unlike the pull, a round reads only the columns of the samples that changed: `columns` / `entries_read` / `atomics` record it;
// * successors are a function of the finished G alone, in two passes over the columns of reached x: pass 1 atomicMin of bits(G[x])
//   into best[y] among exact achievers, pass 2 atomicMin of x into S[y] among those with bits(G[x]) == best[y]: deterministic.
#include "relax_core.h"

struct sssp_to_state {
    count_slot slot[3];
    unsigned long long rounds, relax, atomics, entries, columns, reached;
};

__global__ __launch_bounds__(256) void k_sssp_to_init(int64_t N, int64_t words, double* __restrict__ G, uint64_t* __restrict__ bm,
                                                      sssp_to_state* __restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) G[i] = INFINITY;
    if (i < 4 * words) bm[i] = 0ull;
    if (i == 0) {
        st->slot[0].changed = st->slot[1].changed = st->slot[2].changed = 0;
        st->rounds = st->relax = st->atomics = st->entries = st->columns = st->reached = 0;
    }
}

// G = 0 on the targets (1-based, validated on the host; duplicates write the same values), their bits into B[0] and the target bitmap
__global__ __launch_bounds__(256) void k_sssp_to_targets(int64_t ntgt, int64_t words, const int64_t* __restrict__ tgt1, double* __restrict__ G,
                                                         uint64_t* bm, sssp_to_state* st)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < ntgt) {
        const int64_t t = tgt1[e] - 1;
        G[t] = 0.0;
        atomicOr((unsigned long long*)&bm[t >> 6], 1ull << (t & 63));
        atomicOr((unsigned long long*)&bm[3 * words + (t >> 6)], 1ull << (t & 63));
    }
    if (e == 0) st->slot[0].changed = 1;
}

__global__ __launch_bounds__(256) void k_sssp_to_push(int64_t N, int64_t words, int round, const int64_t* __restrict__ colptr,
                                                      const int32_t* __restrict__ rowval, const double* __restrict__ nzval,
                                                      const uint64_t* __restrict__ efree, const uint64_t* __restrict__ F, double* G,
                                                      uint64_t* bm, sssp_to_state* st)
{
    const ring_idx r = ring_at(round);
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    push_body(words, colptr, rowval, nzval, efree, F, G, bm, st->slot, &st->rounds, &st->relax, &st->atomics, &st->entries, &st->columns, r, gtid, nthreads);
}

__global__ __launch_bounds__(256) void k_sssp_to_succ_init(int64_t N, unsigned long long* __restrict__ best, unsigned long long* __restrict__ S)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) { best[i] = ~0ull; S[i] = ~0ull; }
}

// PASS 1: best[y] = min bits(G[x]) over usable x with fl(G[x] + w) == G[y];  PASS 2: S[y] = min (x + 1) among those with bits(G[x]) == best[y]
template <int PASS>
__global__ __launch_bounds__(256) void k_sssp_to_succ(int64_t N, int64_t words, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                      const double* __restrict__ nzval, const uint64_t* __restrict__ efree,
                                                      const uint64_t* __restrict__ F, const double* __restrict__ G, const uint64_t* __restrict__ bm,
                                                      unsigned long long* best, unsigned long long* S)
{
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    const uint64_t* tbm = bm + 3 * words;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        const double gx = G[x];
        if (!(gx < INFINITY)) continue;
        if (F && !((F[x >> 6] >> (x & 63)) & 1ull)) continue;
        const unsigned long long gxb = (unsigned long long)__double_as_longlong(gx);
        for (int64_t b = colptr[x] + lane; b < colptr[x + 1]; b += 64) {
            if (!((efree[b >> 6] >> (b & 63)) & 1ull)) continue;
            const int32_t y = rowval[b];
            if ((tbm[y >> 6] >> (y & 63)) & 1ull) continue;
            if (!(gx + nzval[b] == G[y])) continue;
            if (PASS == 1) { if (gxb < best[y]) atomicMin(&best[y], gxb); }
            else if (best[y] == gxb && (unsigned long long)(x + 1) < S[y]) atomicMin(&S[y], (unsigned long long)(x + 1));
        }
    }
}

// S = 0 where no successor was found (targets, unreached samples); reached = samples with G < +Inf
__global__ __launch_bounds__(256) void k_sssp_to_finish(int64_t N, const double* __restrict__ G, unsigned long long* __restrict__ S, int has_S,
                                                        sssp_to_state* st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool r = i < N && G[i] < INFINITY;
    if (has_S && i < N && S[i] == ~0ull) S[i] = 0ull;
    const unsigned long long m = __ballot(r);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st->reached, (unsigned long long)__popcll(m));
}

// The successor passes over a finished G on ctx->stream, for the one-shot field and for the tracked one (kernels_togo.hip): bm is four
// bitmaps of ceil(N / 64) words, the fourth the targets; best [N] is scratch; S [N] is left with ~0 where no successor was found.
void mpfmt_sssp_to_launch_successors(mpfmt_ctx* ctx, const uint64_t* d_F, const double* G, const uint64_t* bm, unsigned long long* best,
                                     unsigned long long* S)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    const unsigned nb_cols = relax_wave_blocks(ctx, N);                      // one wavefront per column
    const unsigned nb_n = (unsigned)((std::max<int64_t>(N, 1) + 255) / 256);
    hipLaunchKernelGGL(k_sssp_to_succ_init, dim3(nb_n), dim3(256), 0, ctx->stream, N, best, S);
    hipLaunchKernelGGL(k_sssp_to_succ<1>, dim3(nb_cols), dim3(256), 0, ctx->stream, N, words, ctx->colptr, ctx->rowval, ctx->nzval,
                       ctx->graph_free, d_F, G, bm, best, S);
    hipLaunchKernelGGL(k_sssp_to_succ<2>, dim3(nb_cols), dim3(256), 0, ctx->stream, N, words, ctx->colptr, ctx->rowval, ctx->nzval,
                       ctx->graph_free, d_F, G, bm, best, S);
}

// targets1: 1-based, on the host, validated by the caller; G_host [N]; S_host [N] or nullptr (then the successor passes do not run)
int32_t mpfmt_sssp_to_device(mpfmt_ctx* ctx, const int64_t* targets1, int64_t ntgt, const uint64_t* d_F, double* G_host, int64_t* S_host,
                             mpfmt_sssp_info* info)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = ctx->sssp_C.ensure(ctx, sizeof(double) * (size_t)N))) return rc;
    if (S_host && (rc = ctx->sssp_A.ensure(ctx, sizeof(int64_t) * (size_t)N))) return rc;
    if ((rc = ctx->sssp_bm.ensure(ctx, sizeof(uint64_t) * 4 * (size_t)words))) return rc;
    if (S_host && (rc = ctx->sssp_to_best.ensure(ctx, sizeof(unsigned long long) * (size_t)N))) return rc;
    if ((rc = ctx->sssp_to_tgt.ensure(ctx, sizeof(int64_t) * (size_t)std::max<int64_t>(ntgt, 1)))) return rc;
    if ((rc = ctx->sssp_to_state.ensure(ctx, sizeof(sssp_to_state)))) return rc;
    if ((rc = ctx->sssp_to_state_host.ensure(ctx, sizeof(sssp_to_state)))) return rc;
    for (int k = 0; k < 2; ++k) if (!ctx->sssp_ev[k]) HIPCHK(ctx, hipEventCreate(&ctx->sssp_ev[k]));
    sssp_to_state* st = (sssp_to_state*)ctx->sssp_to_state.get();
    sssp_to_state* sh = (sssp_to_state*)ctx->sssp_to_state_host.get();
    double* G = ctx->sssp_C;
    unsigned long long* S = (unsigned long long*)ctx->sssp_A.get();
    // one wavefront per quarter word of the changed-sample bitmap, grid-stride
    const unsigned nb = relax_wave_blocks(ctx, 4 * words);
    const unsigned nb_init = (unsigned)((std::max<int64_t>(N, 4 * words) + 255) / 256);
    const unsigned nb_n = (unsigned)((N + 255) / 256);
    if (ntgt > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->sssp_to_tgt, targets1, sizeof(int64_t) * (size_t)ntgt, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[0], ctx->stream));
    {
        mpfmt_timed tm(ctx);
        hipLaunchKernelGGL(k_sssp_to_init, dim3(nb_init), dim3(256), 0, ctx->stream, N, words, G, ctx->sssp_bm, st);
        if (ntgt > 0)
            hipLaunchKernelGGL(k_sssp_to_targets, dim3((unsigned)((ntgt + 255) / 256)), dim3(256), 0, ctx->stream, ntgt, words, ctx->sssp_to_tgt, G,
                               ctx->sssp_bm, st);
        auto round = [&](int64_t t) {
            hipLaunchKernelGGL(k_sssp_to_push, dim3(nb), dim3(256), 0, ctx->stream, N, words, ring_slot(t), ctx->colptr, ctx->rowval,
                               ctx->nzval, ctx->graph_free, d_F, G, ctx->sssp_bm, st);
        };
        if ((rc = relax_rounds(ctx, N, st, sh, sh->slot, round, "cost-to-go relaxation did not settle within N rounds"))) return rc;
        tm.end("sssp_to_push");
    }
    {
        mpfmt_timed tm(ctx);
        if (S_host) mpfmt_sssp_to_launch_successors(ctx, d_F, G, ctx->sssp_bm, ctx->sssp_to_best.get(), S);
        hipLaunchKernelGGL(k_sssp_to_finish, dim3(nb_n), dim3(256), 0, ctx->stream, N, G, S, S_host ? 1 : 0, st);
        tm.end("sssp_to_successors");
    }
    HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[1], ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sh, st, sizeof(sssp_to_state), hipMemcpyDeviceToHost, ctx->stream));
    if (G_host) HIPCHK(ctx, hipMemcpyAsync(G_host, G, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
    if (S_host) HIPCHK(ctx, hipMemcpyAsync(S_host, S, sizeof(int64_t) * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->sssp_ev[0], ctx->sssp_ev[1]));
    ctx->sssp_rounds = (int64_t)sh->rounds; ctx->sssp_relax = (int64_t)sh->relax; ctx->sssp_reached = (int64_t)sh->reached;
    ctx->sssp_to_atomics = (int64_t)sh->atomics; ctx->sssp_to_entries = (int64_t)sh->entries; ctx->sssp_to_columns = (int64_t)sh->columns;
    if (info) { info->reached = ctx->sssp_reached; info->rounds = ctx->sssp_rounds; info->relaxations = ctx->sssp_relax; info->ms_device = ms; }
    return MPFMT_OK;
}
