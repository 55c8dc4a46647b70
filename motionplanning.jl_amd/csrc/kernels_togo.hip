// A cost-to-go policy kept valid across in-place box edits (include/mpfmt.h, "a cost-to-go field kept valid across box edits";
// DESIGN.md 7j).  The field of one target set lives in buffers of its own -- labels G, successors S -- on whatever swept graph is
// resident (r-disc, imported, k-nearest, double integrator, Dubins, Reeds-Shepp), and after mpfmt_boxes_add / _remove it is REPAIRED:
//
//   dirty      mpfmt_togo_mark_dirty ORs the delta kernels' flagged-column list into this field's own bitmap D (k_field_dirty with
//              another target bitmap; the cost-to-come field of kernels_field.hip keeps its own);
//   invalidate k_togo_i0, lane per sample: I0 = the non-target y with a finite label whose successor edge y -> S[y] is no longer usable.
//              Only a y whose S[y] is dirty or has lost its point bit can be one; the entry of the edge is found by binary search of y in
//              the ascending column S[y] (every graph of the library has strictly ascending columns; an import is checked for it).  I0
//              also takes a y whose successor chain stays at y's own label for TOGO_EQUAL_HOPS hops (a circle of zero-length edges).  The
//              closure is k_field_close's form with S in the role of A: "a sample whose successor's label is +Inf takes +Inf" until a
//              pass changes nothing (an unreached sample is nobody's successor, so +Inf IS the mark); the host reads the pass counters
//              once per RELAX_BATCH passes.  The bitmap of I is kept: the seed reads it;
//   seed       ring slot 0 = D, plus the finite columns that hold a row of I:
//                form 0  (the library's own r-disc build: the rows of a column are its out-neighbours) one wavefront per y of I marks
//                        the finite rows of column y: the work follows I;
//                form 1  (k-nearest, imported, the three steering graphs: nothing rests on a symmetry the library does not guarantee)
//                        one wavefront per finite, unmarked column scans its rowval against the bitmap of I and marks itself on a hit
//                        (ballot): 4 bytes per entry, once;
//   push       the rounds of k_sssp_to_push (push_body of relax_core.h: the same ring, the same plain load then atomicMin on the label
//              bits, F applied to the pushing x) from slot 0 to a fixed point.  At the head of a round bin & F is ORed into `seen`
//              (one thread per word, grid-stride): the distinct columns read, counted once at the end;
//   successors the two passes of the one-shot field (the kernels of kernels_sssp_to.hip, launched by mpfmt_sssp_to_launch_successors: the
//              first four bitmaps of this field lie as that call's do) over the finished G: whole passes, a function of G alone.
//
// mpfmt_togo_begin, and an update whose delta history is gone, run the same push from the targets over labels of +Inf (path 0).
#include "relax_core.h"

struct togo_state {
    count_slot slot[3];                      // ring of the push rounds
    count_slot close[3];                     // ring of the closure's pass counters
    unsigned long long rounds, relax, atomics, entries, columns, reached, invalidated, dirty, distinct;
};

// bitmaps of tg_bm, `words` each: the ring of three | the targets (the layout of sssp_bm, which the successor kernels read) | D (dirty columns) | I (invalidated) | seen (columns read)
#define TOGO_BM_TARGETS 3
#define TOGO_BM_DIRTY 4
#define TOGO_BM_INV 5
#define TOGO_BM_SEEN 6
#define TOGO_BITMAPS 7
#define TOGO_EQUAL_HOPS MPFMT_TOGO_EQUAL_HOPS      // successor hops at one label after which a sample counts as unsupported (k_togo_i0)

__device__ __forceinline__ void togo_state_zero(togo_state* st)
{
    st->slot[0].changed = st->slot[1].changed = st->slot[2].changed = 0;
    st->close[0].changed = st->close[1].changed = st->close[2].changed = 0;
    st->rounds = st->relax = st->atomics = st->entries = st->columns = st->reached = st->invalidated = st->dirty = st->distinct = 0;
}

// the whole field from nothing: G = +Inf, every bitmap empty
__global__ __launch_bounds__(256) void k_togo_init(int64_t N, int64_t words, double* __restrict__ G, uint64_t* __restrict__ bm, togo_state* __restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) G[i] = INFINITY;
    if (i < TOGO_BITMAPS * words) bm[i] = 0ull;
    if (i == 0) togo_state_zero(st);
}

// G = 0 on the targets (1-based, validated on the host; duplicates write the same values), their bits into ring slot 0 and the target bitmap
__global__ __launch_bounds__(256) void k_togo_targets(int64_t ntgt, int64_t words, const int64_t* __restrict__ tgt1, double* __restrict__ G,
                                                      uint64_t* bm, togo_state* st)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < ntgt) {
        const int64_t t = tgt1[e] - 1;
        G[t] = 0.0;
        atomicOr((unsigned long long*)&bm[t >> 6], 1ull << (t & 63));
        atomicOr((unsigned long long*)&bm[TOGO_BM_TARGETS * words + (t >> 6)], 1ull << (t & 63));
    }
    if (e == 0) st->slot[0].changed = 1;
}

__global__ __launch_bounds__(64) void k_togo_state_init(togo_state* __restrict__ st)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) togo_state_zero(st);
}

// I0, lane per sample (a wavefront = one word of every bitmap); ring slot 0 = D, slots 1 and 2 = 0, the bitmap of I = I0, seen = 0
__global__ __launch_bounds__(256) void k_togo_i0(int64_t N, int64_t words, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                 const uint64_t* __restrict__ efree, const uint64_t* __restrict__ F, double* G,
                                                 const unsigned long long* __restrict__ S, uint64_t* __restrict__ bm, togo_state* st)
{
    const int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t w = y >> 6;
    const int lane = threadIdx.x & 63;
    if (w >= words) return;                                                    // (wave-uniform)
    const uint64_t* D = bm + TOGO_BM_DIRTY * words;
    bool inv = false;
    if (y < N && !((bm[TOGO_BM_TARGETS * words + w] >> lane) & 1ull) && G[y] < INFINITY) {
        const int64_t s = (int64_t)S[y] - 1;                                   // (a finite label off the targets has a successor)
        if (s >= 0 && s < N) {
            const bool fs = !F || bit_of(F, s);
            if (!fs) inv = true;
            else if (bit_of(D, s)) {
                // the entry of y -> s: y among the ascending rows of column s
                int64_t lo = colptr[s], hi = colptr[s + 1];
                const int64_t end = hi;
                while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((int64_t)rowval[mid] < y) lo = mid + 1; else hi = mid; }
                inv = !(lo < end && (int64_t)rowval[lo] == y && bit_of(efree, lo));
            }
        }
        // a chain of equal-label hops that does not leave its label (a group that hangs together by zero-length or absorbed edges only:
        // its successors may run in a circle and never show what supports it) cannot be vouched for: it joins I0, and the push gives
        // it its label back.  A label read here may already be the +Inf of another lane's I0: then the closure takes y.
        if (!inv && s >= 0 && s < N) {
            const unsigned long long gy = label_bits(G[y]);
            const uint64_t* tbm = bm + TOGO_BM_TARGETS * words;
            int64_t c = s;
            int hops = 0;
            while (hops < TOGO_EQUAL_HOPS && label_bits(G[c]) == gy && !bit_of(tbm, c)) {
                c = (int64_t)S[c] - 1;
                if (c < 0 || c >= N) break;
                ++hops;
            }
            inv = hops == TOGO_EQUAL_HOPS;
        }
        if (inv) G[y] = INFINITY;
    }
    const unsigned long long m = __ballot(inv);
    if (lane == 0) {
        const uint64_t dw = D[w];
        bm[w] = dw; bm[words + w] = 0ull; bm[2 * words + w] = 0ull;
        bm[TOGO_BM_INV * words + w] = m; bm[TOGO_BM_SEEN * words + w] = 0ull;
        if (dw) atomicAdd(&st->dirty, (unsigned long long)__popcll(dw));
        if (m) { atomicAdd(&st->invalidated, (unsigned long long)__popcll(m)); atomicAdd(&st->close[0].changed, (unsigned long long)__popcll(m)); }
    }
}

// one pass of the closure: a reached sample whose successor has lost its label loses its own (k_field_close with S in the role of A:
// pass p reads what pass p - 1 did; I0 is pass -1).  Labels are read in place: a pass may see the +Inf another lane wrote in the same
// pass, which only shortens the loop.  Targets have S = 0 and keep their 0.
__global__ __launch_bounds__(256) void k_togo_close(int64_t N, int pass, double* G, const unsigned long long* __restrict__ S, unsigned long long* Ibm,
                                                    togo_state* st)
{
    const ring_idx r = ring_at(pass);
    const int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ring_step(st->close, r, y) == 0) return;
    const int lane = threadIdx.x & 63;
    bool inv = false;
    if (y < N) {
        const int64_t s = (int64_t)S[y];
        if (s > 0 && s <= N && G[y] < INFINITY && !(G[s - 1] < INFINITY)) { G[y] = INFINITY; inv = true; }
    }
    const unsigned long long m = __ballot(inv);
    if (lane == 0 && m) {
        atomicOr(&Ibm[y >> 6], m);
        atomicAdd(&st->invalidated, (unsigned long long)__popcll(m));
        atomicAdd(&st->close[r.out].changed, (unsigned long long)__popcll(m));
    }
}

// seed, form 0 (symmetric structure): one wavefront per quarter word of the bitmap of I; the finite rows of a column y of I enter slot 0
__global__ __launch_bounds__(256) void k_togo_seed_rows(int64_t words, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                        const double* __restrict__ G, uint64_t* bm, const togo_state* __restrict__ st)
{
    if (st->invalidated == 0) return;
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    const uint64_t* Ibm = bm + TOGO_BM_INV * words;
    unsigned long long* P0 = (unsigned long long*)bm;
    for (int64_t u = gtid >> 6; u < 4 * words; u += nwaves) {
        const int64_t w = u >> 2;
        const int sh = (int)(u & 3) * 16;
        unsigned bits = __builtin_amdgcn_readfirstlane((unsigned)((Ibm[w] >> sh) & 0xffffull));
        while (bits) {
            const int64_t y = w * 64 + sh + __builtin_ctz(bits);
            bits &= bits - 1;
            for (int64_t b = colptr[y] + lane; b < colptr[y + 1]; b += 64) {
                const int32_t x = rowval[b];
                if (!(G[x] < INFINITY) || bit_of((const uint64_t*)bm, x)) continue;
                atomicOr(&P0[x >> 6], 1ull << (x & 63));
            }
        }
    }
}

// seed, form 1 (any graph): one wavefront per finite column that is not in slot 0 yet; a row in I marks the column
__global__ __launch_bounds__(256) void k_togo_seed_scan(int64_t N, int64_t words, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                        const double* __restrict__ G, uint64_t* bm, const togo_state* __restrict__ st)
{
    if (st->invalidated == 0) return;
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    const uint64_t* Ibm = bm + TOGO_BM_INV * words;
    unsigned long long* P0 = (unsigned long long*)bm;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        if (!(G[x] < INFINITY) || bit_of((const uint64_t*)bm, x)) continue;                     // (wave-uniform)
        const int64_t b1 = colptr[x + 1];
        for (int64_t base = colptr[x]; base < b1; base += 64) {
            const int64_t b = base + lane;
            const bool hit = b < b1 && bit_of(Ibm, rowval[b]);
            if (__ballot(hit)) {
                if (lane == 0) atomicOr(&P0[x >> 6], 1ull << (x & 63));
                break;
            }
        }
    }
}

// slot[0].changed = 1 when there is a pusher at all (the rounds return at once otherwise)
__global__ __launch_bounds__(64) void k_togo_arm(togo_state* st)
{
    if (threadIdx.x == 0) st->slot[0].changed = (st->dirty || st->invalidated) ? 1 : 0;
}

// a round of the push; before it, the columns it will read (the round's bitmap & F) enter `seen`, one thread per word
__global__ __launch_bounds__(256) void k_togo_push(int64_t N, int64_t words, int round, const int64_t* __restrict__ colptr,
                                                   const int32_t* __restrict__ rowval, const double* __restrict__ nzval,
                                                   const uint64_t* __restrict__ efree, const uint64_t* __restrict__ F, double* G,
                                                   uint64_t* bm, togo_state* st)
{
    const int rin = ring_slot(round);
    if (st->slot[rin].changed) {
        const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
        const uint64_t* bin = bm + (int64_t)rin * words;
        uint64_t* seen = bm + TOGO_BM_SEEN * words;
        for (int64_t w = gtid; w < words; w += nthreads) {
            uint64_t v = bin[w];
            if (F) v &= F[w];
            if (v) seen[w] |= v;
        }
    }
    const ring_idx r = ring_at(round);
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    push_body(words, colptr, rowval, nzval, efree, F, G, bm, st->slot, &st->rounds, &st->relax, &st->atomics, &st->entries, &st->columns, r, gtid, nthreads);
}

// S = 0 where no successor was found (targets, unreached samples); reached = samples with G < +Inf; distinct = the bits of `seen`
__global__ __launch_bounds__(256) void k_togo_finish(int64_t N, int64_t words, const double* __restrict__ G, unsigned long long* __restrict__ S,
                                                     const uint64_t* __restrict__ bm, togo_state* st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool r = i < N && G[i] < INFINITY;
    if (i < N && S[i] == ~0ull) S[i] = 0ull;
    const unsigned long long m = __ballot(r);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st->reached, (unsigned long long)__popcll(m));
    if (i < words) {
        const uint64_t v = bm[TOGO_BM_SEEN * words + i];
        if (v) atomicAdd(&st->distinct, (unsigned long long)__popcll(v));
    }
}

// The field follows a growth of the sample set (mpfmt_samples_add with option "samples_add_keeps_fields"), lane per sample
// of the grown set, out of the tracked buffers into the spare ones: old samples keep label and successor, new ones get +Inf and none and
// are no targets.  Threads [0, words) lay the seven bitmaps again for words = ceil(N / 64): the targets extended by zeros, dirty = the
// pending bits of earlier edits | the changed columns of the growth, everything else empty.  No invalidation rule of its own: k_togo_i0
// finds the successor edge of y by binary search in column S[y] whenever that column is dirty, and a column that lost the entry is.
__global__ __launch_bounds__(256) void k_togo_carry(int64_t n_old, int64_t N, int64_t words_old, int64_t words, const double* __restrict__ G,
                                                    const unsigned long long* __restrict__ S, const uint64_t* __restrict__ bm,
                                                    const uint64_t* __restrict__ changed, double* __restrict__ Gn, unsigned long long* __restrict__ Sn,
                                                    uint64_t* __restrict__ bmn)
{
    const int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (y < N) {
        Gn[y] = y < n_old ? G[y] : INFINITY;
        Sn[y] = y < n_old ? S[y] : 0ull;
    }
    if (y < words) {
        const bool old = y < words_old;
        bmn[y] = 0ull; bmn[words + y] = 0ull; bmn[2 * words + y] = 0ull;
        bmn[TOGO_BM_TARGETS * words + y] = old ? bm[TOGO_BM_TARGETS * words_old + y] : 0ull;
        bmn[TOGO_BM_DIRTY * words + y] = (old ? bm[TOGO_BM_DIRTY * words_old + y] : 0ull) | changed[y];
        bmn[TOGO_BM_INV * words + y] = 0ull; bmn[TOGO_BM_SEEN * words + y] = 0ull;
    }
}

// targets that join a tracked field (mpfmt_togo_targets_add; 1-based, validated on the host; duplicates and old targets write the same
// values): a label decrease -- G = 0, no successor, the target bit, and the dirty bit, so the sample pushes in round 0 of the next repair
__global__ __launch_bounds__(256) void k_togo_targets_add(int64_t ntgt, int64_t words, const int64_t* __restrict__ tgt1, double* __restrict__ G,
                                                          unsigned long long* __restrict__ S, uint64_t* bm)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ntgt) return;
    const int64_t t = tgt1[e] - 1;
    G[t] = 0.0; S[t] = 0ull;
    atomicOr((unsigned long long*)&bm[TOGO_BM_TARGETS * words + (t >> 6)], 1ull << (t & 63));
    atomicOr((unsigned long long*)&bm[TOGO_BM_DIRTY * words + (t >> 6)], 1ull << (t & 63));
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------

static int32_t togo_buffers(mpfmt_ctx* ctx)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = ctx->tg_state.ensure(ctx, sizeof(togo_state)))) return rc;
    if ((rc = ctx->tg_state_host.ensure(ctx, sizeof(togo_state)))) return rc;
    for (int k = 0; k < 2; ++k) if (!ctx->sssp_ev[k]) HIPCHK(ctx, hipEventCreate(&ctx->sssp_ev[k]));
    if (ctx->tg_N != N || !ctx->tg_G) {
        if ((rc = ctx->tg_G.ensure(ctx, sizeof(double) * (size_t)std::max<int64_t>(N, 1)))) return rc;
        if ((rc = ctx->tg_S.ensure(ctx, sizeof(unsigned long long) * (size_t)std::max<int64_t>(N, 1)))) return rc;
        if ((rc = ctx->tg_best.ensure(ctx, sizeof(unsigned long long) * (size_t)std::max<int64_t>(N, 1)))) return rc;
        if ((rc = ctx->tg_bm.ensure(ctx, sizeof(uint64_t) * TOGO_BITMAPS * (size_t)std::max<int64_t>(words, 1)))) return rc;
        ctx->tg_N = N;
    }
    return MPFMT_OK;
}

static void togo_stats(mpfmt_ctx* ctx, const togo_state* sh, int32_t path, float ms, mpfmt_togo_info* info)
{
    ctx->tg_path = path;
    ctx->tg_reached = (int64_t)sh->reached; ctx->tg_invalidated = (int64_t)sh->invalidated; ctx->tg_dirty_columns = (int64_t)sh->dirty;
    ctx->tg_columns_read = (int64_t)sh->distinct; ctx->tg_column_visits = (int64_t)sh->columns; ctx->tg_entries_read = (int64_t)sh->entries;
    ctx->tg_rounds = (int64_t)sh->rounds; ctx->tg_relax = (int64_t)sh->relax; ctx->tg_atomics = (int64_t)sh->atomics;
    if (info) {
        info->reached = ctx->tg_reached; info->invalidated = ctx->tg_invalidated; info->dirty_columns = ctx->tg_dirty_columns;
        info->columns_read = ctx->tg_columns_read; info->column_visits = ctx->tg_column_visits; info->entries_read = ctx->tg_entries_read;
        info->rounds = ctx->tg_rounds; info->relaxations = ctx->tg_relax; info->atomics = ctx->tg_atomics; info->ms_device = ms;
        info->path = path; info->pad_ = 0;
    }
}

// the push rounds from whatever ring slot 0 holds, then the successor passes and the counts; ends with the state in its host mirror
static int32_t togo_push_and_successors(mpfmt_ctx* ctx, const uint64_t* d_F)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    togo_state* st = (togo_state*)ctx->tg_state.get();
    togo_state* sh = (togo_state*)ctx->tg_state_host.get();
    double* G = ctx->tg_G;
    unsigned long long* S = ctx->tg_S;
    uint64_t* bm = ctx->tg_bm;
    const unsigned nb = relax_wave_blocks(ctx, 4 * words);                    // one wavefront per quarter word of the round's bitmap
    const unsigned nb_n = (unsigned)((std::max<int64_t>(N, 1) + 255) / 256);
    {
        mpfmt_timed tm(ctx);
        auto round = [&](int64_t t) {
            hipLaunchKernelGGL(k_togo_push, dim3(nb), dim3(256), 0, ctx->stream, N, words, ring_slot(t), ctx->colptr, ctx->rowval, ctx->nzval,
                               ctx->graph_free, d_F, G, bm, st);
        };
        if ((rc = relax_rounds(ctx, N, st, sh, sh->slot, round, "the cost-to-go push did not settle within N rounds"))) return rc;
        tm.end("togo_push");
    }
    {
        mpfmt_timed tm(ctx);
        mpfmt_sssp_to_launch_successors(ctx, d_F, G, bm, ctx->tg_best.get(), S);      // (the kernels of the one-shot field)
        hipLaunchKernelGGL(k_togo_finish, dim3(nb_n), dim3(256), 0, ctx->stream, N, words, G, S, bm, st);
        tm.end("togo_successors");
    }
    // the field is valid again: nothing is dirty
    HIPCHK(ctx, hipMemsetAsync(bm + TOGO_BM_DIRTY * words, 0, sizeof(uint64_t) * (size_t)words, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[1], ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sh, st, sizeof(togo_state), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

// what the field belongs to: the sample set, the resident graph and its parameters, and the builds and whole sweeps seen so far
static void togo_adopt(mpfmt_ctx* ctx)
{
    const bool steer = ctx->steer_filled;
    ctx->tg_tracked = true;
    ctx->tg_steer = steer;
    ctx->tg_samples_epoch = ctx->samples_epoch;
    ctx->tg_build_epoch = steer ? ctx->steer_epoch : ctx->graph_epoch;
    ctx->tg_sweep_epoch = steer ? ctx->steer_sweep_epoch : ctx->sweep_epoch;
    ctx->tg_graph_r = steer ? ctx->steer_r : ctx->graph_r;
    ctx->tg_knn_k = steer ? 0 : ctx->knn_k;
    ctx->tg_steer_kind = ctx->steer_kind;
    ctx->tg_steer_a = !steer ? 0.0 : ctx->steer_kind == MPFMT_STEER_DI ? ctx->di_rho : ctx->car_rt;
    ctx->tg_steer_b = !steer || ctx->steer_kind == MPFMT_STEER_DI ? 0.0 : ctx->car_sp;
    ctx->tg_dirty_any = false; ctx->tg_grown = false;
}

// The whole field of the target set into the tracked buffers (targets1: 1-based, on the host, validated by the caller; it may be the
// field's own list).  An earlier field is overwritten only after the buffers are there.
int32_t mpfmt_togo_compute(mpfmt_ctx* ctx, const int64_t* targets1, int64_t ntgt, int32_t checkpts, const uint64_t* d_F, mpfmt_togo_info* info)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = togo_buffers(ctx))) return rc;
    if ((rc = ctx->tg_tgt.ensure(ctx, sizeof(int64_t) * (size_t)std::max<int64_t>(ntgt, 1)))) return rc;
    if (targets1 != ctx->tg_targets.data()) ctx->tg_targets.assign(targets1, targets1 + ntgt);
    ctx->tg_checkpts = checkpts;
    ctx->tg_tracked = false;                                                   // (a computation cut short leaves no field)
    togo_state* st = (togo_state*)ctx->tg_state.get();
    togo_state* sh = (togo_state*)ctx->tg_state_host.get();
    const unsigned nb_init = (unsigned)((std::max<int64_t>(std::max<int64_t>(N, TOGO_BITMAPS * words), 1) + 255) / 256);
    if (ntgt > 0)
        HIPCHK(ctx, hipMemcpyAsync(ctx->tg_tgt, ctx->tg_targets.data(), sizeof(int64_t) * (size_t)ntgt, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[0], ctx->stream));
    hipLaunchKernelGGL(k_togo_init, dim3(nb_init), dim3(256), 0, ctx->stream, N, words, ctx->tg_G.get(), ctx->tg_bm.get(), st);
    if (ntgt > 0)
        hipLaunchKernelGGL(k_togo_targets, dim3((unsigned)((ntgt + 255) / 256)), dim3(256), 0, ctx->stream, ntgt, words, ctx->tg_tgt.get(),
                           ctx->tg_G.get(), ctx->tg_bm.get(), st);
    if ((rc = togo_push_and_successors(ctx, d_F))) return rc;
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->sssp_ev[0], ctx->sssp_ev[1]));
    togo_stats(ctx, sh, 0, ms, info);
    togo_adopt(ctx);
    return MPFMT_OK;
}

int32_t mpfmt_togo_mark_dirty(mpfmt_ctx* ctx)
{
    if (!ctx->tg_tracked || ctx->bd_columns <= 0 || !ctx->tg_bm || ctx->tg_N != ctx->N) return MPFMT_OK;
    const int64_t words = (ctx->N + 63) / 64;
    const int32_t rc = mpfmt_dirty_columns_into(ctx, (unsigned long long*)(ctx->tg_bm.get() + TOGO_BM_DIRTY * words));      // (k_field_dirty)
    if (rc) return rc;
    ctx->tg_dirty_any = true;
    return MPFMT_OK;
}

// steps 2-5 on the tracked buffers over the resident (edited) mask
int32_t mpfmt_togo_repair(mpfmt_ctx* ctx, const uint64_t* d_F, mpfmt_togo_info* info)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = togo_buffers(ctx))) return rc;
    togo_state* st = (togo_state*)ctx->tg_state.get();
    togo_state* sh = (togo_state*)ctx->tg_state_host.get();
    double* G = ctx->tg_G;
    unsigned long long* S = ctx->tg_S;
    uint64_t* bm = ctx->tg_bm;
    const unsigned nb_n = (unsigned)((std::max<int64_t>(N, 1) + 255) / 256);  // lane per sample: a wavefront = one word
    // the library's own r-disc build is symmetric by construction; every other graph is taken as directed
    const int form = (!ctx->steer_filled && ctx->knn_k == 0 && !ctx->graph_imported) ? 0 : 1;
    ctx->tg_seed_form = form;
    HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[0], ctx->stream));
    {
        mpfmt_timed tm(ctx);
        hipLaunchKernelGGL(k_togo_state_init, dim3(1), dim3(64), 0, ctx->stream, st);
        hipLaunchKernelGGL(k_togo_i0, dim3(nb_n), dim3(256), 0, ctx->stream, N, words, ctx->colptr, ctx->rowval, ctx->graph_free, d_F, G, S, bm, st);
        // (every pass that changes something gives +Inf to at least one more sample)
        auto pass = [&](int64_t p) {
            hipLaunchKernelGGL(k_togo_close, dim3(nb_n), dim3(256), 0, ctx->stream, N, ring_slot(p), G, S,
                               (unsigned long long*)(bm + TOGO_BM_INV * words), st);
        };
        if ((rc = relax_rounds(ctx, N, st, sh, sh->close, pass, "the closure of the invalidated set did not settle within N passes"))) return rc;
        tm.end("togo_invalidate");
    }
    const bool any = sh->dirty || sh->invalidated;                             // (the mirror is that of the closure's last batch)
    if (any) {
        mpfmt_timed tm(ctx);
        if (form == 0)
            hipLaunchKernelGGL(k_togo_seed_rows, dim3(relax_wave_blocks(ctx, 4 * words)), dim3(256), 0, ctx->stream, words, ctx->colptr, ctx->rowval,
                               G, bm, st);
        else
            hipLaunchKernelGGL(k_togo_seed_scan, dim3(relax_wave_blocks(ctx, N)), dim3(256), 0, ctx->stream, N, words, ctx->colptr, ctx->rowval,
                               G, bm, st);
        hipLaunchKernelGGL(k_togo_arm, dim3(1), dim3(64), 0, ctx->stream, st);
        tm.end("togo_seed");
    }
    if (any) {
        if ((rc = togo_push_and_successors(ctx, d_F))) return rc;
    } else {                                                                   // nothing flagged, nothing invalidated: the field stands
        HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[1], ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        sh->reached = (unsigned long long)ctx->tg_reached;
    }
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->sssp_ev[0], ctx->sssp_ev[1]));
    togo_stats(ctx, sh, 1, ms, info);
    ctx->tg_dirty_any = false; ctx->tg_grown = false;
    return MPFMT_OK;
}

// ctx->N is the grown size; the tracked buffers hold the field of the first n_old samples (tg_N == n_old, checked by the caller through
// mpfmt_togo_live before the sample set changed).  Nothing tracked is written: a failure leaves the field as it was.
int32_t mpfmt_togo_carry(mpfmt_ctx* ctx, int64_t n_old, const uint64_t* changed)
{
    const int64_t N = ctx->N, words = (N + 63) / 64, words_old = (n_old + 63) / 64;
    int32_t rc;
    if ((rc = ctx->tg_G_next.ensure(ctx, sizeof(double) * (size_t)N))) return rc;
    if ((rc = ctx->tg_S_next.ensure(ctx, sizeof(unsigned long long) * (size_t)N))) return rc;
    if ((rc = ctx->tg_bm_next.ensure(ctx, sizeof(uint64_t) * TOGO_BITMAPS * (size_t)words))) return rc;
    if ((rc = ctx->tg_best.ensure(ctx, sizeof(unsigned long long) * (size_t)N))) return rc;      // (scratch of the successor passes: nothing to keep)
    hipLaunchKernelGGL(k_togo_carry, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, n_old, N, words_old, words,
                       (const double*)ctx->tg_G.get(), (const unsigned long long*)ctx->tg_S.get(), (const uint64_t*)ctx->tg_bm.get(), changed,
                       ctx->tg_G_next.get(), ctx->tg_S_next.get(), ctx->tg_bm_next.get());
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

// after the growth has succeeded (the ctx's epochs are those of the grown graph): the field is the ctx's again, with columns pending
void mpfmt_togo_carry_commit(mpfmt_ctx* ctx)
{
    ctx->tg_G.swap(ctx->tg_G_next); ctx->tg_S.swap(ctx->tg_S_next); ctx->tg_bm.swap(ctx->tg_bm_next);
    ctx->tg_N = ctx->N;
    ctx->tg_samples_epoch = ctx->samples_epoch; ctx->tg_build_epoch = ctx->graph_epoch; ctx->tg_sweep_epoch = ctx->sweep_epoch;
    ctx->tg_graph_r = ctx->graph_r;
    ctx->tg_dirty_any = true; ctx->tg_grown = true;
}

// targets1: 1-based in 1 .. ctx->N, on the host (validated by the caller), ntgt > 0; the field is live
int32_t mpfmt_togo_add_targets(mpfmt_ctx* ctx, const int64_t* targets1, int64_t ntgt)
{
    const int64_t words = (ctx->N + 63) / 64;
    int32_t rc;
    mpfmt_dbuf<int64_t> d_t;                                                   // (tg_tgt holds the field's own list: a recomputation uploads into it)
    if ((rc = d_t.ensure(ctx, sizeof(int64_t) * (size_t)ntgt))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_t, targets1, sizeof(int64_t) * (size_t)ntgt, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_togo_targets_add, dim3((unsigned)((ntgt + 255) / 256)), dim3(256), 0, ctx->stream, ntgt, words, (const int64_t*)d_t.get(),
                       ctx->tg_G.get(), ctx->tg_S.get(), ctx->tg_bm.get());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tg_targets.insert(ctx->tg_targets.end(), targets1, targets1 + ntgt);
    ctx->tg_dirty_any = true;
    return MPFMT_OK;
}

void mpfmt_togo_drop_internal(mpfmt_ctx* ctx)
{
    ctx->tg_tracked = false;
    ctx->tg_dirty_any = false;
    ctx->tg_grown = false;
    ctx->tg_targets.clear();
}

bool mpfmt_togo_live(mpfmt_ctx* ctx)
{
    if (!ctx->tg_tracked) return false;
    const bool same_samples = ctx->world == 1 && ctx->tg_samples_epoch == ctx->samples_epoch && ctx->tg_N == ctx->N && ctx->tg_G;
    const bool filled = ctx->steer_filled || ctx->graph_filled;
    if (same_samples && !filled) return false;                                 // (between two builds: nothing to answer with, nothing to drop yet)
    if (same_samples && ctx->tg_steer && ctx->steer_filled && ctx->tg_steer_kind == ctx->steer_kind && ctx->tg_graph_r == ctx->steer_r &&
        (ctx->steer_kind == MPFMT_STEER_DI ? ctx->tg_steer_a == ctx->di_rho : (ctx->tg_steer_a == ctx->car_rt && ctx->tg_steer_b == ctx->car_sp)))
        return true;
    if (same_samples && !ctx->tg_steer && !ctx->steer_filled && ctx->graph_filled && ctx->tg_graph_r == ctx->graph_r && ctx->tg_knn_k == ctx->knn_k)
        return true;
    mpfmt_togo_drop_internal(ctx);                                             // (new samples, another graph: the field belongs to neither)
    return false;
}

bool mpfmt_togo_history(const mpfmt_ctx* ctx)
{
    return ctx->tg_steer ? (ctx->tg_build_epoch == ctx->steer_epoch && ctx->tg_sweep_epoch == ctx->steer_sweep_epoch)
                         : (ctx->tg_build_epoch == ctx->graph_epoch && ctx->tg_sweep_epoch == ctx->sweep_epoch);
}
