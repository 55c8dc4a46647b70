// A cost-to-come field kept valid across in-place box edits (include/mpfmt.h, "a cost-to-come field kept valid across box edits";
// DESIGN.md "a tracked field").  The field of one source lives in buffers of its own -- labels C, parents A, and Ab[x] = the entry
// index of the parent edge A[x] -> x -- and after mpfmt_boxes_add / _remove it is REPAIRED with work that follows the edit:
//
//   dirty      the delta kernels' flagged-column list is ORed into a bitmap D of N bits (k_field_dirty);
//   invalidate I0 = the dirty x != s with a finite label whose parent edge lost its bit (one load through Ab) or whose point bit is
//              clear; their labels become +Inf and their bits enter the round-0 candidates (k_field_i0).  The closure over the
//              descendants is "a sample whose parent's label is +Inf takes +Inf" until a pass changes nothing (k_field_close, lane per
//              sample, N-sized; an unreached sample has no children, so +Inf IS the mark); the host reads the pass counters once per
//              RELAX_BATCH passes and a pass whose predecessor changed nothing returns at once;
//   relax      k_field_relax: one wavefront per column, lanes over entries, the fold and the aligned 8-byte label loads and stores of
//              k_sssp_relax, and its cost band (a column with C[x] <= mlow = the lowest label written in the round before cannot
//              improve).  One ring of three bitmaps drives it, the ring of relax_core.h:
//                round 0      the slot holds the candidates I u D; a candidate looks at all its usable rows with finite labels, mlow = 0;
//                symmetric    (the library's own r-disc build: the rows of a column are its out-neighbours) a column that lowers its
//                             label marks its ROWS: the slot holds the next round's candidates and only they are read;
//                otherwise    (k-nearest, imported) a column that lowers its label marks ITSELF and rounds >= 1 are those of
//                             k_sssp_relax: every column is a candidate and looks at the rows of the slot.  Nothing rests on a symmetry
//                             the library does not guarantee;
//              while the rounds run, the dirty bitmap's storage holds the set of columns read so far (the stat counts them once);
//   parents    k_field_parents: the parent pass of k_sssp_parents (parents_body of relax_core.h) over the finished labels, which also
//              writes Ab and counts the reached samples.
//
// Why the band holds without a row filter (symmetric mode): a label written in round t >= 1 is fl(C[y] + w) for a row y of a candidate
// x.  If y has not changed since x last looked at it, x holds min(..., fl(C[y] + w)) already.  If it has, it changed in round t - 1 or
// in round t itself, and by induction over the writes every such label is >= mlow(t); so the value is >= mlow(t) and a column at or
// below mlow(t) cannot improve.
#include "relax_core.h"

struct field_state {
    band_slot slot[3];
    count_slot close[3];                     // ring of the closure's pass counters
    unsigned long long relax, rounds, reached, invalidated, dirty, distinct, visits, entries;
};

// the flagged columns of a delta call into the dirty bitmap (words are shared between wavefronts: atomicOr)
__global__ __launch_bounds__(256) void k_field_dirty(const int32_t* __restrict__ cols, int64_t n, int64_t N, unsigned long long* __restrict__ D)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t x = cols[i];
    if (x < 0 || x >= N) return;
    atomicOr(&D[x >> 6], 1ull << (x & 63));
}

__global__ __launch_bounds__(256) void k_field_state_init(field_state* __restrict__ st)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        band_ring_init(st->slot, 0);
        st->close[0].changed = st->close[1].changed = st->close[2].changed = 0;
        st->relax = st->rounds = st->reached = st->invalidated = st->dirty = st->distinct = st->visits = st->entries = 0;
    }
}

// I0 on the dirty columns, lane per sample (a wavefront = one word of every bitmap); ring slot 0 = D | I0, slots 1 and 2 = 0
__global__ __launch_bounds__(256) void k_field_i0(int64_t N, int64_t words, int64_t src, const uint64_t* __restrict__ efree, const uint64_t* __restrict__ F,
                                                  double* __restrict__ C, const int64_t* __restrict__ Ab, const uint64_t* __restrict__ D,
                                                  uint64_t* __restrict__ ring, field_state* st)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t w = x >> 6;
    const int lane = threadIdx.x & 63;
    if (w >= words) return;                                                    // (wave-uniform)
    const uint64_t dw = D[w];
    bool inv = false;
    if (x < N && ((dw >> lane) & 1ull) && x != src && C[x] < INFINITY) {
        const int64_t b = Ab[x];                                               // (FIELD_AB_GONE: the radius rule of a growth dropped the parent edge)
        inv = b < 0 || !((efree[b >> 6] >> (b & 63)) & 1ull);
        if (F && !((F[w] >> lane) & 1ull)) inv = true;
        if (inv) C[x] = INFINITY;
    }
    const unsigned long long m = __ballot(inv);
    if (lane == 0) {
        ring[w] = dw | m; ring[words + w] = 0ull; ring[2 * words + w] = 0ull;
        if (dw) atomicAdd(&st->dirty, (unsigned long long)__popcll(dw));
        if (m) { atomicAdd(&st->invalidated, (unsigned long long)__popcll(m)); atomicAdd(&st->close[0].changed, (unsigned long long)__popcll(m)); }
    }
}

// one pass of the closure: a reached sample whose parent has lost its label loses its own.  The pass counters are a ring of
// relax_core.h (pass p reads what pass p - 1 did; I0 is pass -1).  Labels are read in place: a pass may see the +Inf another lane wrote
// in the same pass, which only shortens the loop.
__global__ __launch_bounds__(256) void k_field_close(int64_t N, int64_t src, int pass, double* C, const int64_t* __restrict__ A,
                                                     unsigned long long* ring0, field_state* st)
{
    const ring_idx r = ring_at(pass);
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ring_step(st->close, r, x) == 0) return;
    const int lane = threadIdx.x & 63;
    bool inv = false;
    if (x < N && x != src) {
        const int64_t p = A[x];
        if (p > 0 && C[x] < INFINITY && !(C[p - 1] < INFINITY)) { C[x] = INFINITY; inv = true; }
    }
    const unsigned long long m = __ballot(inv);
    if (lane == 0 && m) {
        atomicOr(&ring0[x >> 6], m);
        atomicAdd(&st->invalidated, (unsigned long long)__popcll(m));
        atomicAdd(&st->close[r.out].changed, (unsigned long long)__popcll(m));
    }
}

// slot[0].changed = 1 when there is a candidate at all (the rounds return at once otherwise)
__global__ __launch_bounds__(64) void k_field_arm(field_state* st)
{
    if (threadIdx.x == 0) st->slot[0].changed = (st->dirty || st->invalidated) ? 1 : 0;
}

// sym != 0: the slot of the round holds candidate COLUMNS (rounds >= 0); sym == 0: it does so in round 0 and holds the changed ROWS after
__global__ __launch_bounds__(256) void k_field_relax(int64_t N, int64_t words, int round, int first, int sym, const int64_t* __restrict__ colptr,
                                                     const int32_t* __restrict__ rowval, const double* __restrict__ nzval,
                                                     const uint64_t* __restrict__ efree, const uint64_t* __restrict__ F, double* C,
                                                     uint64_t* ring, unsigned long long* seen, field_state* st)
{
    const ring_idx r = ring_at(round);
    const double mlow = label_of_bits(st->slot[r.in].minbits);
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const uint64_t* bin;
    unsigned long long* bout;
    if (!ring_round(st->slot, &st->rounds, ring, words, r, gtid, nthreads, bin, bout)) return;
    const bool by_column = sym || first;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = nthreads >> 6;
    unsigned long long nrel = 0, nchg = 0, nvis = 0, ndis = 0, nent = 0;
    double lmin = INFINITY;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        if (by_column && !bit_of(bin, x)) continue;
        const double cx = C[x];
        if (cx <= mlow) continue;                                             // (the source, C = 0, always: its exemption from F)
        if (F && !bit_of(F, x)) continue;
        const int64_t b0 = colptr[x], b1 = colptr[x + 1];
        if (lane == 0) {
            const unsigned long long bit = 1ull << (x & 63);
            const unsigned long long old = atomicOr(&seen[x >> 6], bit);
            ++nvis; nent += (unsigned long long)(b1 - b0);
            if (!(old & bit)) ++ndis;
        }
        const double best = by_column ? column_fold<false, true>(b0, b1, lane, rowval, nzval, efree, bin, C, nrel)
                                      : column_fold<true, true>(b0, b1, lane, rowval, nzval, efree, bin, C, nrel);
        if (best < cx) {
            if (lane == 0) {
                C[x] = best;
                ++nchg;
                lmin = fmin(lmin, best);
                if (!sym) atomicOr(&bout[x >> 6], 1ull << (x & 63));
            }
            if (sym)                                                          // the rows of x are its out-neighbours: they look next round
                for (int64_t b = b0 + lane; b < b1; b += 64) {
                    const int32_t y = rowval[b];
                    atomicOr(&bout[y >> 6], 1ull << (y & 63));
                }
        }
    }
    nrel = wave_sum(nrel);
    if (lane == 0) {
        if (nrel) atomicAdd(&st->relax, nrel);
        if (nvis) { atomicAdd(&st->visits, nvis); atomicAdd(&st->entries, nent); }
        if (ndis) atomicAdd(&st->distinct, ndis);
        if (nchg) {
            atomicAdd(&st->slot[r.out].changed, nchg);
            atomicMin(&st->slot[r.out].minbits, label_bits(lmin));
        }
    }
}

// k_sssp_parents, which also writes the entry index of the parent edge
__global__ __launch_bounds__(256) void k_field_parents(int64_t N, int64_t src, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                       const double* __restrict__ nzval, const uint64_t* __restrict__ efree,
                                                       const double* __restrict__ C, int64_t* __restrict__ A, int64_t* __restrict__ Ab, field_state* st)
{
    parents_body<false, true>(N, src, colptr, rowval, nzval, efree, C, nullptr, A, Ab, &st->reached);
}

// The field follows a growth of the sample set (mpfmt_samples_add with option "samples_add_keeps_fields"), lane per sample
// of the grown set, out of the tracked buffers into the spare ones.  Old samples keep label and parent; the entry index of the parent
// edge is found again by binary search of row A[x] - 1 in the GROWN column x (strictly ascending rows; every entry index has moved), and
// is FIELD_AB_GONE when the smaller radius dropped the entry -- column x lost an entry, so it is in `changed` and k_field_i0 takes it.
// New samples: +Inf, no parent.  Threads [0, words) also lay the bitmaps again for words = ceil(N / 64): dirty = the pending bits of
// earlier edits | the changed columns of the growth, the ring slots empty.
#define FIELD_AB_GONE ((int64_t)-1)
__global__ __launch_bounds__(256) void k_field_carry(int64_t n_old, int64_t N, int64_t words_old, int64_t words, const int64_t* __restrict__ colptr,
                                                     const int32_t* __restrict__ rowval, const double* __restrict__ C, const int64_t* __restrict__ A,
                                                     const uint64_t* __restrict__ D, const uint64_t* __restrict__ changed, double* __restrict__ Cn,
                                                     int64_t* __restrict__ An, int64_t* __restrict__ Abn, uint64_t* __restrict__ bmn)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < N) {
        double c = INFINITY;
        int64_t p = 0, b = FIELD_AB_GONE;
        if (x < n_old) {
            c = C[x]; p = A[x];
            if (p > 0 && p <= n_old) {
                int64_t lo = colptr[x], hi = colptr[x + 1];
                const int64_t end = hi, y = p - 1;
                while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((int64_t)rowval[mid] < y) lo = mid + 1; else hi = mid; }
                if (lo < end && (int64_t)rowval[lo] == y) b = lo;
            }
        }
        Cn[x] = c; An[x] = p; Abn[x] = b;
    }
    if (x < words) {
        bmn[x] = (x < words_old ? D[x] : 0ull) | changed[x];
        bmn[words + x] = 0ull; bmn[2 * words + x] = 0ull; bmn[3 * words + x] = 0ull;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------

static int32_t field_buffers(mpfmt_ctx* ctx)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = ctx->fld_state.ensure(ctx, sizeof(field_state)))) return rc;
    if ((rc = ctx->fld_state_host.ensure(ctx, sizeof(field_state)))) return rc;
    if (ctx->fld_N != N || !ctx->fld_C) {
        if ((rc = ctx->fld_C.ensure(ctx, sizeof(double) * (size_t)N))) return rc;
        if ((rc = ctx->fld_A.ensure(ctx, sizeof(int64_t) * (size_t)N))) return rc;
        if ((rc = ctx->fld_Ab.ensure(ctx, sizeof(int64_t) * (size_t)N))) return rc;
        if ((rc = ctx->fld_bm.ensure(ctx, sizeof(uint64_t) * 4 * (size_t)words))) return rc;
        ctx->fld_N = N;
    }
    return MPFMT_OK;
}

static void field_stats(mpfmt_ctx* ctx, const field_state* sh, int32_t path, float ms, mpfmt_field_info* info)
{
    ctx->fld_path = path;
    ctx->fld_reached = (int64_t)sh->reached; ctx->fld_invalidated = (int64_t)sh->invalidated; ctx->fld_dirty_columns = (int64_t)sh->dirty;
    ctx->fld_columns_read = (int64_t)sh->distinct; ctx->fld_column_visits = (int64_t)sh->visits; ctx->fld_entries_read = (int64_t)sh->entries;
    ctx->fld_rounds = (int64_t)sh->rounds; ctx->fld_relax = (int64_t)sh->relax;
    if (info) {
        info->reached = ctx->fld_reached; info->invalidated = ctx->fld_invalidated; info->dirty_columns = ctx->fld_dirty_columns;
        info->columns_read = ctx->fld_columns_read; info->column_visits = ctx->fld_column_visits; info->entries_read = ctx->fld_entries_read;
        info->rounds = ctx->fld_rounds; info->relaxations = ctx->fld_relax; info->ms_device = ms; info->path = path; info->pad_ = 0;
    }
}

// The whole field of source0 into the tracked buffers: the relaxation of mpfmt_graph_sssp (its scratch labels are copied), then the
// parents pass that also writes Ab.  The tracked buffers are written only after the relaxation has succeeded.
int32_t mpfmt_field_compute(mpfmt_ctx* ctx, int64_t source0, int32_t checkpts, const uint64_t* d_F, mpfmt_field_info* info)
{
    const int64_t N = ctx->N, words = (N + 63) / 64;
    int32_t rc;
    if ((rc = field_buffers(ctx))) return rc;
    mpfmt_sssp_info si;
    if ((rc = mpfmt_sssp_device(ctx, source0, d_F, nullptr, nullptr, &si))) return rc;
    field_state* st = (field_state*)ctx->fld_state.get();
    field_state* sh = (field_state*)ctx->fld_state_host.get();
    HIPCHK(ctx, hipMemcpyAsync(ctx->fld_C, ctx->sssp_C, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->fld_bm, 0, sizeof(uint64_t) * 4 * (size_t)words, ctx->stream));
    hipLaunchKernelGGL(k_field_state_init, dim3(1), dim3(64), 0, ctx->stream, st);
    {
        mpfmt_timed tm(ctx);
        hipLaunchKernelGGL(k_field_parents, dim3(relax_wave_blocks(ctx, N)), dim3(256), 0, ctx->stream, N, source0, ctx->colptr, ctx->rowval, ctx->nzval,
                           ctx->graph_free, ctx->fld_C, ctx->fld_A, ctx->fld_Ab, st);
        tm.end("field_parents");
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(sh, st, sizeof(field_state), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    sh->rounds = (unsigned long long)si.rounds; sh->relax = (unsigned long long)si.relaxations;
    field_stats(ctx, sh, 0, si.ms_device, info);
    ctx->fld_tracked = true;
    ctx->fld_source0 = source0; ctx->fld_checkpts = checkpts;
    ctx->fld_samples_epoch = ctx->samples_epoch; ctx->fld_graph_epoch = ctx->graph_epoch; ctx->fld_sweep_epoch = ctx->sweep_epoch;
    ctx->fld_graph_r = ctx->graph_r; ctx->fld_knn_k = ctx->knn_k;
    ctx->fld_dirty_any = false; ctx->fld_grown = false;
    return MPFMT_OK;
}

// the flagged columns of the last delta call, ctx->bd_cols[0 .. bd_columns), ORed into the dirty bitmap D (N bits) on ctx->stream: each
// tracked field passes its own
int32_t mpfmt_dirty_columns_into(mpfmt_ctx* ctx, unsigned long long* D)
{
    const int64_t n = ctx->bd_columns;
    if (n <= 0) return MPFMT_OK;
    hipLaunchKernelGGL(k_field_dirty, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->bd_cols, n, ctx->N, D);
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

int32_t mpfmt_field_mark_dirty(mpfmt_ctx* ctx)
{
    if (!ctx->fld_tracked || ctx->bd_columns <= 0 || !ctx->fld_bm || ctx->fld_N != ctx->N) return MPFMT_OK;
    const int32_t rc = mpfmt_dirty_columns_into(ctx, (unsigned long long*)ctx->fld_bm.get());
    if (rc) return rc;
    ctx->fld_dirty_any = true;
    return MPFMT_OK;
}

// steps 2-4 on the tracked buffers over the resident (edited) mask
int32_t mpfmt_field_repair(mpfmt_ctx* ctx, const uint64_t* d_F, mpfmt_field_info* info)
{
    const int64_t N = ctx->N, words = (N + 63) / 64, src = ctx->fld_source0;
    int32_t rc;
    if ((rc = field_buffers(ctx))) return rc;
    for (int k = 0; k < 2; ++k) if (!ctx->sssp_ev[k]) HIPCHK(ctx, hipEventCreate(&ctx->sssp_ev[k]));
    field_state* st = (field_state*)ctx->fld_state.get();
    field_state* sh = (field_state*)ctx->fld_state_host.get();
    uint64_t* D = ctx->fld_bm.get();
    uint64_t* ring = D + words;
    const unsigned nb_n = (unsigned)((std::max<int64_t>(N, 1) + 255) / 256);  // lane per sample: a wavefront = one word
    const unsigned nb = relax_wave_blocks(ctx, N);
    // the library's own r-disc build is symmetric by construction; a k-nearest graph is directed and an imported one is the caller's
    const int sym = (ctx->knn_k == 0 && !ctx->graph_imported) ? 1 : 0;
    HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[0], ctx->stream));
    {
        mpfmt_timed tm(ctx);
        hipLaunchKernelGGL(k_field_state_init, dim3(1), dim3(64), 0, ctx->stream, st);
        hipLaunchKernelGGL(k_field_i0, dim3(nb_n), dim3(256), 0, ctx->stream, N, words, src, ctx->graph_free, d_F, ctx->fld_C, ctx->fld_Ab, D, ring, st);
        // (every pass that changes something gives +Inf to at least one more sample)
        auto pass = [&](int64_t p) {
            hipLaunchKernelGGL(k_field_close, dim3(nb_n), dim3(256), 0, ctx->stream, N, src, ring_slot(p), ctx->fld_C, ctx->fld_A,
                               (unsigned long long*)ring, st);
        };
        if ((rc = relax_rounds(ctx, N, st, sh, sh->close, pass, "the closure of the invalidated set did not settle within N passes"))) return rc;
        // the dirty set has entered ring slot 0: its storage now collects the columns read
        HIPCHK(ctx, hipMemsetAsync(D, 0, sizeof(uint64_t) * (size_t)words, ctx->stream));
        hipLaunchKernelGGL(k_field_arm, dim3(1), dim3(64), 0, ctx->stream, st);
        tm.end("field_invalidate");
    }
    {
        mpfmt_timed tm(ctx);
        auto round = [&](int64_t t) {
            hipLaunchKernelGGL(k_field_relax, dim3(nb), dim3(256), 0, ctx->stream, N, words, ring_slot(t), t == 0 ? 1 : 0, sym,
                               ctx->colptr, ctx->rowval, ctx->nzval, ctx->graph_free, d_F, ctx->fld_C, ring,
                               (unsigned long long*)D, st);
        };
        if ((rc = relax_rounds(ctx, N, st, sh, sh->slot, round, "the field repair did not settle within N rounds"))) return rc;
        HIPCHK(ctx, hipMemsetAsync(D, 0, sizeof(uint64_t) * (size_t)words, ctx->stream));      // the field is valid again: nothing is dirty
        tm.end("field_relax");
    }
    {
        mpfmt_timed tm(ctx);
        hipLaunchKernelGGL(k_field_parents, dim3(nb), dim3(256), 0, ctx->stream, N, src, ctx->colptr, ctx->rowval, ctx->nzval, ctx->graph_free,
                           ctx->fld_C, ctx->fld_A, ctx->fld_Ab, st);
        tm.end("field_parents");
    }
    HIPCHK(ctx, hipEventRecord(ctx->sssp_ev[1], ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sh, st, sizeof(field_state), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->sssp_ev[0], ctx->sssp_ev[1]));
    field_stats(ctx, sh, 1, ms, info);
    ctx->fld_dirty_any = false; ctx->fld_grown = false;
    return MPFMT_OK;
}

// ctx->N is the grown size; the tracked buffers hold the field of the first n_old samples (fld_N == n_old, checked by the caller through
// mpfmt_field_live before the sample set changed).  Nothing tracked is written: a failure leaves the field as it was.
int32_t mpfmt_field_carry(mpfmt_ctx* ctx, int64_t n_old, const int64_t* colptr_new, const int32_t* rowval_new, const uint64_t* changed)
{
    const int64_t N = ctx->N, words = (N + 63) / 64, words_old = (n_old + 63) / 64;
    int32_t rc;
    if ((rc = ctx->fld_C_next.ensure(ctx, sizeof(double) * (size_t)N))) return rc;
    if ((rc = ctx->fld_A_next.ensure(ctx, sizeof(int64_t) * (size_t)N))) return rc;
    if ((rc = ctx->fld_Ab_next.ensure(ctx, sizeof(int64_t) * (size_t)N))) return rc;
    if ((rc = ctx->fld_bm_next.ensure(ctx, sizeof(uint64_t) * 4 * (size_t)words))) return rc;
    hipLaunchKernelGGL(k_field_carry, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, n_old, N, words_old, words, colptr_new, rowval_new,
                       (const double*)ctx->fld_C.get(), (const int64_t*)ctx->fld_A.get(), (const uint64_t*)ctx->fld_bm.get(), changed,
                       ctx->fld_C_next.get(), ctx->fld_A_next.get(), ctx->fld_Ab_next.get(), ctx->fld_bm_next.get());
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

// after the growth has succeeded (the ctx's epochs are those of the grown graph): the field is the ctx's again, with columns pending
void mpfmt_field_carry_commit(mpfmt_ctx* ctx)
{
    ctx->fld_C.swap(ctx->fld_C_next); ctx->fld_A.swap(ctx->fld_A_next); ctx->fld_Ab.swap(ctx->fld_Ab_next); ctx->fld_bm.swap(ctx->fld_bm_next);
    ctx->fld_N = ctx->N;
    ctx->fld_samples_epoch = ctx->samples_epoch; ctx->fld_graph_epoch = ctx->graph_epoch; ctx->fld_sweep_epoch = ctx->sweep_epoch;
    ctx->fld_graph_r = ctx->graph_r;
    ctx->fld_dirty_any = true; ctx->fld_grown = true;
}

void mpfmt_field_drop_internal(mpfmt_ctx* ctx)
{
    ctx->fld_tracked = false;
    ctx->fld_dirty_any = false;
    ctx->fld_grown = false;
    ctx->fld_source0 = -1;
}

bool mpfmt_field_live(mpfmt_ctx* ctx)
{
    if (!ctx->fld_tracked) return false;
    const bool same_samples = ctx->world == 1 && ctx->fld_samples_epoch == ctx->samples_epoch && ctx->fld_N == ctx->N && ctx->fld_C;
    if (same_samples && !ctx->graph_filled) return false;                      // (between two builds: nothing to answer with, nothing to drop yet)
    if (same_samples && ctx->graph_filled && ctx->fld_graph_r == ctx->graph_r && ctx->fld_knn_k == ctx->knn_k) return true;
    mpfmt_field_drop_internal(ctx);                                            // (new samples, another r or k: the field belongs to neither)
    return false;
}

bool mpfmt_field_history(const mpfmt_ctx* ctx)
{
    return ctx->fld_graph_epoch == ctx->graph_epoch && ctx->fld_sweep_epoch == ctx->sweep_epoch;
}
