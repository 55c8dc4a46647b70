// The relaxation core of the roadmap fields: what kernels_sssp.hip, kernels_sssp_multi.hip, kernels_field.hip,
// kernels_sssp_to.hip and kernels_togo.hip share -- the ring of three changed-sample bitmaps with its round state, the column fold of
// the pull, the parent rule, the push of the cost-to-go, and the host loop that issues the rounds.  Everything here is __forceinline__
// or a host template: each kernel stays a kernel of its own and inlines the blocks it uses.
//
// * three sample bitmaps in rotation: round t reads B[t % 3], marks B[(t+1) % 3] and clears B[(t+2) % 3] (last read by round t-1),
//   so no round needs a memset of its own;
// * the per-round state lives in a ring of three slots like the bitmaps; the host reads it once per RELAX_BATCH rounds, and a round
//   whose predecessor changed nothing returns at once, so the tail of a batch costs empty launches only;
// * the cost band: mlow(t) = the lowest label written in round t-1.  Every label written in round t is fl(C[y] + w) >= C[y] >= mlow(t)
//   for a y of the bitmap (by induction over the writes of the round), so a column with C[x] <= mlow(t) cannot improve and is skipped
//   before any of its entries is read: the settled interior stops costing bandwidth.  (The source, C = 0, is always skipped: that is
//   its exemption from F.)
// * labels are read and written in place while the round runs (plain aligned 8-byte loads and stores, never torn).  A reader may see
//   the label of this round or the one before -- the L2 of another XCD may hold the older one -- both are upper bounds of the fixed
//   point that only ever decrease, and the writer's bit in B[(t+1) % 3] makes the reader look again next round: values are
//   independent of the schedule, `rounds` and `relaxations` are not;
// * parents come from a separate pass over the finished labels, a function of C alone.
#pragma once
#include "mpfmt_internal.h"
#include <cmath>
#include <algorithm>

#define RELAX_BATCH 8                        // rounds (or closure passes) issued between two reads of the round state
#define LABEL_INF_BITS 0x7FF0000000000000ull

// labels are >= 0: their bit patterns order like the values
__device__ __forceinline__ unsigned long long label_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double label_of_bits(unsigned long long b) { return __longlong_as_double((long long)b); }

__device__ __forceinline__ double wave_min(double v)
{
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- the ring ---------------------------------------------------------------------------------------------------------------------------

// step t reads slot `in` (what step t-1 marked), marks slot `out` and clears slot `clr` (the slot step t+1 will mark: nobody reads or
// writes it during this step)
struct ring_idx { int in, out, clr; };
__host__ __device__ __forceinline__ int ring_slot(int64_t t) { return (int)(t % 3); }
__device__ __forceinline__ ring_idx ring_at(int t) { return {ring_slot(t), ring_slot(t + 1), ring_slot(t + 2)}; }

// What a slot carries besides the count of what its step marked is the slot type's own business: clear(gtid) resets it, spread over
// the first threads of the grid.
struct count_slot {                          // no payload: the cost-to-go push, the closure of the invalidated set
    unsigned long long changed;
    __device__ __forceinline__ void clear(int64_t gtid) { if (gtid == 0) changed = 0; }
};
struct band_slot {                           // one band minimum: the bits of the lowest label the step wrote
    unsigned long long changed, minbits;
    __device__ __forceinline__ void clear(int64_t gtid) { if (gtid == 0) { changed = 0; minbits = LABEL_INF_BITS; } }
};

// the band ring before round 0: slot 0 holds the count of the start set and mlow(0) = 0 (every label is >= 0)
__device__ __forceinline__ void band_ring_init(band_slot* slot, unsigned long long changed0)
{
    slot[0].changed = changed0; slot[0].minbits = 0ull;
    slot[1].changed = 0; slot[1].minbits = LABEL_INF_BITS;
    slot[2].changed = 0; slot[2].minbits = LABEL_INF_BITS;
}

// the counter part: what step t-1 marked, and the reset of the slot step t+1 will mark
template <class Slot>
__device__ __forceinline__ unsigned long long ring_step(Slot* slot, const ring_idx& r, int64_t gtid)
{
    const unsigned long long cin = slot[r.in].changed;
    slot[r.clr].clear(gtid);
    return cin;
}

// The header of a round kernel.  False: the predecessor changed nothing and the round returns at once.  Otherwise the round is counted,
// the bitmap of slot `clr` is cleared grid-stride, and bin / bout are the bitmaps the round reads and marks.
template <class Slot>
__device__ __forceinline__ bool ring_round(Slot* slot, unsigned long long* rounds, uint64_t* bm, int64_t words, const ring_idx& r, int64_t gtid,
                                           int64_t nthreads, const uint64_t*& bin, unsigned long long*& bout)
{
    const unsigned long long cin = ring_step(slot, r, gtid);
    if (gtid == 0 && cin) *rounds += 1;
    if (cin == 0) return false;
    uint64_t* bclr = bm + (int64_t)r.clr * words;
    for (int64_t w = gtid; w < words; w += nthreads) bclr[w] = 0ull;
    bin = bm + (int64_t)r.in * words;
    bout = (unsigned long long*)(bm + (int64_t)r.out * words);
    return true;
}

// bit i of a bitmap; the index keeps its own width (a row index is 32 bits wide: its word index is one 32-bit shift)
template <class Index>
__device__ __forceinline__ bool bit_of(const uint64_t* bm, Index i) { return (bm[i >> 6] >> (i & 63)) & 1ull; }

// ---- the column fold of the pull ----------------------------------------------------------------------------------------------------------

// One wavefront per column: fmin of fl(C[y] + w) over the usable entries [b0, b1) of the column, lanes over entries, then the
// xor-shuffle minimum.  MARKED_ROWS: only the rows of the bitmap `bin` (those that changed in the round before) are looked at;
// FINITE_ROWS: a row without a label is no candidate (and is not counted).  nrel counts the candidates this lane evaluated.
template <bool MARKED_ROWS, bool FINITE_ROWS>
__device__ __forceinline__ double column_fold(int64_t b0, int64_t b1, int lane, const int32_t* __restrict__ rowval, const double* __restrict__ nzval,
                                              const uint64_t* __restrict__ efree, const uint64_t* bin, const double* C, unsigned long long& nrel)
{
    double best = INFINITY;
    for (int64_t b = b0 + lane; b < b1; b += 64) {
        const int32_t y = rowval[b];
        if (MARKED_ROWS && !bit_of(bin, y)) continue;
        if (!bit_of(efree, b)) continue;
        const double cy = C[y];
        if (FINITE_ROWS && !(cy < INFINITY)) continue;
        const double c = cy + nzval[b];
        ++nrel;
        best = fmin(best, c);
    }
    return wave_min(best);
}

// ---- the parent rule -------------------------------------------------------------------------------------------------------

// (c, y) before (cb, yb) in the order of the parent rule: the lower label, then the lower index
__device__ __forceinline__ bool parent_before(double c, int32_t y, double cb, int32_t yb) { return c < cb || (c == cb && y < yb); }

#define PARENT_NONE 0x7fffffff

// The parent of column x with label cx: the usable y of lowest (C[y], y) with fl(C[y] + w) == C[x], and the entry eb of the edge
// y -> x; yb = PARENT_NONE when no entry achieves cx.  One wavefront per column; every lane returns the same pair.
__device__ __forceinline__ void parent_scan(int64_t b0, int64_t b1, int lane, const int32_t* __restrict__ rowval, const double* __restrict__ nzval,
                                            const uint64_t* __restrict__ efree, const double* __restrict__ C, double cx, int32_t& yb, int64_t& eb)
{
    double cb = INFINITY;
    yb = PARENT_NONE; eb = 0;
    for (int64_t b = b0 + lane; b < b1; b += 64) {
        if (!bit_of(efree, b)) continue;
        const int32_t y = rowval[b];
        const double cy = C[y];
        if (!(cy + nzval[b] == cx)) continue;
        if (parent_before(cy, y, cb, yb)) { cb = cy; yb = y; eb = b; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double oc = __shfl_xor(cb, off);
        const int32_t oy = __shfl_xor(yb, off);
        const int64_t oe = __shfl_xor(eb, off);
        if (parent_before(oc, oy, cb, yb)) { cb = oc; yb = oy; eb = oe; }
    }
}

// The body of the single-source parent kernels: A[x] = the parent of x by the rule above, 1-based; 0 for the source and for unreached
// samples; *reached counts the samples with a label.  SEEDED: the source is an external start that entered as seed labels, index 0 of
// label 0 -- seed[x] == C[x] makes it the parent of lowest (C, index), A[x] = -1 -- and no sample is the source (src is not read).
// WITH_ENTRY: Ab[x] = the entry index of the parent edge A[x] -> x (0 where A[x] = 0).
template <bool SEEDED, bool WITH_ENTRY>
__device__ __forceinline__ void parents_body(int64_t N, int64_t src, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                             const double* __restrict__ nzval, const uint64_t* __restrict__ efree, const double* __restrict__ C,
                                             const double* __restrict__ seed, int64_t* __restrict__ A, int64_t* __restrict__ Ab,
                                             unsigned long long* reached)
{
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    unsigned long long nreach = 0;
    for (int64_t x = gtid >> 6; x < N; x += nwaves) {
        const double cx = C[x];
        int64_t a = 0, e = 0;
        bool scan = cx < INFINITY;
        if (scan) {
            ++nreach;
            if (SEEDED) { if (seed[x] == cx) { a = -1; scan = false; } }
            else if (x == src) scan = false;
        }
        if (scan) {
            int32_t yb;
            parent_scan(colptr[x], colptr[x + 1], lane, rowval, nzval, efree, C, cx, yb, e);
            a = yb == PARENT_NONE ? 0 : (int64_t)yb + 1;
        }
        if (lane == 0) { A[x] = a; if (WITH_ENTRY) Ab[x] = e; }
    }
    if (lane == 0 && nreach) atomicAdd(reached, nreach);
}

// ---- the push of the cost-to-go ---------------------------------------------------------------------------------------

// The body of a push round, shared by k_sssp_to_push (the one-shot field) and k_togo_push (the tracked one): the ring header, then one
// wavefront per quarter word of the round's bitmap (& F with checkpts).  A column x of it loads G[x] once and offers fl(G[x] + w) to
// every row y of a free entry: a plain load of G[y] first, then a 64-bit atomicMin on the label bits; a returned old value above the
// candidate marks y for the next round.  The counters are those of the caller's state.  r = ring_at(round), gtid and nthreads (the
// global thread index and the grid size) come from the kernel, which computes them in this order.
__device__ __forceinline__ void push_body(int64_t words, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                          const double* __restrict__ nzval, const uint64_t* __restrict__ efree, const uint64_t* __restrict__ F,
                                          double* G, uint64_t* bm, count_slot* slot, unsigned long long* rounds, unsigned long long* relax,
                                          unsigned long long* atomics, unsigned long long* entries, unsigned long long* columns,
                                          const ring_idx& r, int64_t gtid, int64_t nthreads)
{
    const uint64_t* bin;
    unsigned long long* bout;
    if (!ring_round(slot, rounds, bm, words, r, gtid, nthreads, bin, bout)) return;
    unsigned long long* Gb = (unsigned long long*)G;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = nthreads >> 6;
    unsigned long long nrel = 0, natom = 0, nchg = 0, nent = 0, ncol = 0;
    for (int64_t u = gtid >> 6; u < 4 * words; u += nwaves) {
        const int64_t w = u >> 2;
        const int sh = (int)(u & 3) * 16;
        uint64_t word = bin[w];
        if (F) word &= F[w];
        unsigned bits = __builtin_amdgcn_readfirstlane((unsigned)((word >> sh) & 0xffffull));        // (the same in every lane: say so)
        while (bits) {
            const int64_t x = w * 64 + sh + __builtin_ctz(bits);
            bits &= bits - 1;
            const double gx = G[x];
            const int64_t b0 = colptr[x], b1 = colptr[x + 1];
            if (lane == 0) { ++ncol; nent += (unsigned long long)(b1 - b0); }
            for (int64_t b = b0 + lane; b < b1; b += 64) {
                if (!bit_of(efree, b)) continue;
                const int32_t y = rowval[b];
                const double cand = gx + nzval[b];
                ++nrel;
                if (!(cand < G[y])) continue;
                const unsigned long long cb = label_bits(cand);
                const unsigned long long old = atomicMin(&Gb[y], cb);
                ++natom;
                if (old > cb) { atomicOr(&bout[y >> 6], 1ull << (y & 63)); ++nchg; }
            }
        }
    }
    nrel = wave_sum(nrel); natom = wave_sum(natom); nchg = wave_sum(nchg);
    if (lane == 0) {
        if (nrel) atomicAdd(relax, nrel);
        if (natom) atomicAdd(atomics, natom);
        if (nchg) atomicAdd(&slot[r.out].changed, nchg);
        if (ncol) { atomicAdd(columns, ncol); atomicAdd(entries, nent); }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------

// one wavefront per unit of work (a column, or a quarter word of a bitmap), grid-stride, in blocks of 256: enough waves to fill the
// chip several times over (a skipped column costs one load)
static inline unsigned relax_wave_blocks(const mpfmt_ctx* ctx, int64_t units)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((units + 3) / 4, (int64_t)ctx->num_cus * 16));
}

// The rounds of a relaxation (or the passes of a closure): launch(t) issues step t on ctx->stream; after every RELAX_BATCH steps the
// device state `st` is copied to its pinned mirror `sh`, and the loop ends when the mirror's ring `slots` shows that the batch's last
// step marked nothing for the next one.  Every non-final step of the callers changes at least one of N samples for good (a label that is the fold of a simple
// path drops; a sample loses its label), so N steps bound the loop: past them the call fails with `unsettled`.
template <class State, class Slot, class Launch>
static int32_t relax_rounds(mpfmt_ctx* ctx, int64_t N, State* st, State* sh, const Slot* slots, Launch launch, const char* unsettled)
{
    int64_t t = 0;
    bool done = false;
    while (!done) {
        if (t > N + RELAX_BATCH) return mpfmt_fail(ctx, MPFMT_ERR_HIP, "%s", unsettled);
        for (int q = 0; q < RELAX_BATCH; ++q, ++t) launch(t);
        HIPCHK(ctx, hipMemcpyAsync(sh, st, sizeof(State), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        done = slots[ring_slot(t)].changed == 0;
    }
    return MPFMT_OK;
}
