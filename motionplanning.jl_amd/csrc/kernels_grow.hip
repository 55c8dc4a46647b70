// Growing the sample set of a resident, swept r-disc graph (include/mpfmt.h, "growing the sample set"; DESIGN.md has the section of the
// same name).  A neighbour relation, a distance and a free bit are pure functions of one ordered pair: the old entries of the graph ARE
// entries of the grown graph, what is new is the pairs that involve a new sample, and the rest is a merge of arrays.
//
//   k_grow_near    : one workgroup per new sample q = V[v], in the manner of k_roadmap (kernels_roadmap.hip); its four wavefronts each
//                    take every fourth row of the cells of the GROWN set's grid that meet q's r-box (a refinement adds few samples: with
//                    one wavefront each, 100 of them leave nine SIMDs in ten idle and the pass is the latency of one walk).  The bounds of
//                    64 rows are fetched at once, lane = row; lanes then run over the candidates of a row, exact fp64 distances in the
//                    canonical fold; members (d2 <= r2, index != v) are queued in LDS and tested 64 at a time against the boxes that meet
//                    q's r-box with the predicates of sweep_predicates.h, in BOTH directions: bit 0 = is_free_motion(V[y], q) (the entry
//                    of row y in column v), bit 1 = is_free_motion(q, V[y]) (the entry of row v in column y).  MODE 0 counts per (sample,
//                    part), MODE 1 fills the parts' consecutive segments at the scanned offsets, in cell order.
//   k_grow_sort    : a new column's list into ascending index order (rank by counting: the indices are distinct), and the number of new
//                    rows every old column gains (an atomic COUNT: its value does not depend on the scheduling).
//   k_grow_scatter : the transposition.  The entries (row y old, column v) of the new columns land in column y's segment at an atomic
//                    cursor -- in scheduling order -- and
//   k_grow_tsort   : puts every old column's segment into ascending row order, so the lists are the same whatever the scheduling.
//   k_grow_count / k_grow_fill : the merge, one wavefront per grown column: the old entries that stay (all of them at the graph's own
//                    radius; below it by the stored distance, an entry ON the tie by its recomputed d2), then the added ones.  The fill
//                    also writes one BYTE per grown entry: its free bit (old bit, or the near pass's).  The count leaves the CHANGED
//                    COLUMNS as a bitmap over the grown set -- every new column, every old column that lost an entry to the radius
//                    rule or gained a row -- which is what a tracked field has to look at again (kernels_field.hip, kernels_togo.hip:
//                    the carry).  A bit is a function of the column alone, set by atomicOr: the bitmap does not depend on scheduling.
//   k_grow_repack  : the mask.  Every bit position has shifted, so the words are assembled again: a wavefront owns 64 consecutive output
//                    words, each word is the ballot of 64 bytes, written once by that wavefront alone (no atomics, no read-modify-write);
//                    the bits behind the last entry are zero.
#include "mpfmt_internal.h"
#include "sweep_predicates.h"
#include <cmath>
#include <algorithm>

#define GW_WAVES 4               // wavefronts per workgroup = parts of ONE new sample's walk (a refinement adds few samples: the chip is filled by parts)
#define GW_QCAP 128              // members queued per wavefront (a round adds at most 64 to fewer than 64)
#define GW_CULL 512              // boxes a wavefront lists after the cull (a larger set is walked whole)
#define GW_LDS_BOXES (40 * 1024) // the box set is staged when it fits
#define GW_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

struct gw_near_args {
    const double* Xo; int64_t n_old, n_add; int mode;
    const double* Xt; const int32_t* perm; const int32_t* cellstart;
    double r2, rpad;
    const double* boxes; int M, stage;
    int64_t* cnt;                                          // [n_add][GW_WAVES] members per new sample and part
    const int64_t* ptr; int32_t* idx; double* dist; uint8_t* bits;      // mode 1 (ptr: [n_add * GW_WAVES + 1])
    unsigned long long* ncand;
};

template <int D, int MODE>
__global__ __launch_bounds__(GW_WAVES * 64) void k_grow_near(gw_near_args a, mpfmt_grid G, mpfmt_ss ss)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int32_t s_qp[MODE ? GW_WAVES : 1][GW_QCAP];
    __shared__ double s_qd[MODE ? GW_WAVES : 1][GW_QCAP];
    __shared__ int32_t s_cull[MODE ? GW_WAVES : 1][GW_CULL];
    double* sbox = (double*)smem;
    if (a.stage && MODE != 0) stage_boxes<D>(sbox, a.boxes, 0, a.M);
    __syncthreads();                                         // (the only workgroup barrier: the wavefronts are on their own from here)
    const double* bx = (a.stage && MODE != 0) ? (const double*)sbox : a.boxes;
    const int lane = threadIdx.x & 63, wv = MODE ? (int)(threadIdx.x >> 6) : 0, part = threadIdx.x >> 6;
    const int64_t qi = blockIdx.x, vq = qi * GW_WAVES + part;       // part: this wavefront walks the rows of cells row % GW_WAVES == part
    const int32_t v = (int32_t)(a.n_old + qi);
    const unsigned long long lt = (1ull << lane) - 1ull;
    double q[D];
    int clo[D], chi[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        q[i] = a.Xo[(int64_t)v * D + i];
        clo[i] = mpfmt_cell_of(q[i] - a.rpad, G.lo[i], G.inv_w[i], G.g[i]);
        chi[i] = mpfmt_cell_of(q[i] + a.rpad, G.lo[i], G.inv_w[i], G.g[i]);
    }
    // the boxes that meet q's r-box: every segment between q and a member lies inside it
    int nsurv = a.M;
    bool listed = false;
    if (MODE != 0 && a.M > 0 && a.M <= GW_CULL) {
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
        GW_FENCE();
    }
    const bool q_in = in_state_space_sl<D>(q, ss);
    int64_t nnear = 0, nwritten = 0;
    unsigned long long ncand = 0;
    int qn = 0;
    const int64_t base = MODE == 1 ? a.ptr[vq] : 0, lim = MODE == 1 ? a.ptr[vq + 1] : 0;

    // the first n queued members, lane = member: both segment tests, then the list entry
    auto process = [&](int n) {
        const bool on = lane < n;
        const int32_t p = s_qp[wv][on ? lane : 0];
        const double d2 = s_qd[wv][on ? lane : 0];
        const int32_t y = a.perm[p];
        double c[D];
#pragma unroll
        for (int i = 0; i < D; ++i) c[i] = a.Xt[(((int64_t)p >> 6) * D + i) * 64 + (p & 63)];
        bool fin = on && in_state_space_sl<D>(c, ss);        // y -> q: the first point is the member
        bool fout = on && q_in;                              // q -> y
        double l[D], h[D];
        seg_bbox<D>(c, q, l, h);                             // (min / max: the same box for both directions)
        for (int j = 0; j < nsurv; ++j) {
            const int k = listed ? s_cull[wv][j] : j;
            const box_regs<D> b = load_box<D>(bx, k);        // wave-uniform k: broadcast reads
            const bool pend = (fin | fout) & !broadphase_free_sl<D>(l, h, b);
            if (__ballot(pend)) {
                if (pend) {
                    if (fin) fin = narrow_free_sl<D>(c, q, b);
                    if (fout) fout = narrow_free_sl<D>(q, c, b);
                }
            }
        }
        const int64_t slot = base + nwritten + lane;
        if (on && slot < lim) { a.idx[slot] = y; a.dist[slot] = sqrt(d2); a.bits[slot] = (uint8_t)((fin ? 1 : 0) | (fout ? 2 : 0)); }
        nwritten += n;
    };

    constexpr int L = D - 1;
    int64_t rows = 1;
#pragma unroll
    for (int i = 0; i < L; ++i) rows *= (chi[i] - clo[i] + 1);
    const int64_t myrows = rows > part ? (rows - part + GW_WAVES - 1) / GW_WAVES : 0;
    for (int64_t rb0 = 0; rb0 < myrows; rb0 += 64) {
        // the bounds of 64 rows at once, lane = row: the two dependent loads of a row are out of the serial chain
        int32_t ra_l = 0, rb_l = 0;
        if (rb0 + lane < myrows) {
            int64_t rem = (rb0 + lane) * GW_WAVES + part, cbase = 0;
#pragma unroll
            for (int i = L - 1; i >= 0; --i) {
                const int span = chi[i] - clo[i] + 1;
                cbase += mpfmt_cell_term(G, i, clo[i] + (int)(rem % span));
                rem /= span;
            }
            ra_l = a.cellstart[cbase + clo[L]]; rb_l = a.cellstart[cbase + chi[L] + 1];
        }
        const int nr = (int)min((int64_t)64, myrows - rb0);
        for (int j = 0; j < nr; ++j) {
            const int64_t ra = __shfl(ra_l, j), rb = __shfl(rb_l, j);
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
                bool member = valid && d2 <= a.r2;
                if (member) member = a.perm[p] != v;         // self is excluded by index, not by distance
                const unsigned long long m = __ballot(member);
                if (!m) continue;
                nnear += __popcll(m);
                if (MODE == 0) continue;
                if (member) { const int slot = qn + __popcll(m & lt); s_qp[wv][slot] = (int32_t)p; s_qd[wv][slot] = d2; }
                qn += __popcll(m);
                GW_FENCE();
                if (qn >= 64) {
                    process(64);
                    const int rest = qn - 64;
                    int32_t tp = 0; double td = 0.0;
                    if (lane < rest) { tp = s_qp[wv][64 + lane]; td = s_qd[wv][64 + lane]; }
                    GW_FENCE();
                    if (lane < rest) { s_qp[wv][lane] = tp; s_qd[wv][lane] = td; }
                    GW_FENCE();
                    qn = rest;
                }
            }
        }
    }
    if (MODE != 0 && qn > 0) process(qn);
    if (lane == 0) {
        if (MODE == 0) a.cnt[vq] = nnear;
        if (ncand) atomicAdd(a.ncand, ncand);                // (distances evaluated: the sample's own among them)
    }
}

// a new column's list from cell order into ascending index order; tcnt[y] += 1 for every old row y.  One wavefront per new column.
// Quadratic in the list, as k_roadmap_sort.
__global__ __launch_bounds__(256) void k_grow_sort(int64_t n_add, int64_t n_old, const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx_in,
                                                   const double* __restrict__ dist_in, const uint8_t* __restrict__ bits_in,
                                                   int32_t* __restrict__ idx_out, double* __restrict__ dist_out, uint8_t* __restrict__ bits_out,
                                                   unsigned long long* __restrict__ tcnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= n_add) return;
    const int64_t b0 = ptr[qi * GW_WAVES], b1 = ptr[(qi + 1) * GW_WAVES];      // (the parts' segments are consecutive)
    for (int64_t e = b0 + lane; e < b1; e += 64) {
        const int32_t mine = idx_in[e];
        int64_t rank = 0;
        for (int64_t j = b0; j < b1; ++j) rank += (idx_in[j] < mine) ? 1 : 0;
        idx_out[b0 + rank] = mine; dist_out[b0 + rank] = dist_in[e]; bits_out[b0 + rank] = bits_in[e];
        if (mine < n_old) atomicAdd(&tcnt[mine], 1ull);
    }
}

// the transposition: entry (row y < n_old, column v) of a new column becomes (row v, column y), in column y's segment of the transposed
// lists at an atomic cursor
__global__ __launch_bounds__(256) void k_grow_scatter(int64_t n_add, int64_t n_old, const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                      const double* __restrict__ dist, const uint8_t* __restrict__ bits,
                                                      const int64_t* __restrict__ tptr, unsigned long long* __restrict__ tcur,
                                                      int32_t* __restrict__ trow, double* __restrict__ tdist, uint8_t* __restrict__ tbit)
{
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= n_add) return;
    const int64_t b0 = ptr[qi * GW_WAVES], b1 = ptr[(qi + 1) * GW_WAVES];
    for (int64_t e = b0 + lane; e < b1; e += 64) {
        const int32_t y = idx[e];
        if (y >= n_old) continue;
        const int64_t slot = tptr[y] + (int64_t)atomicAdd(&tcur[y], 1ull);
        if (slot < tptr[y + 1]) { trow[slot] = (int32_t)(n_old + qi); tdist[slot] = dist[e]; tbit[slot] = (uint8_t)((bits[e] >> 1) & 1); }
    }
}

// an old column's new rows into ascending order (insertion sort by one lane: a column gains n_add / N of its degree)
__global__ __launch_bounds__(256) void k_grow_tsort(int64_t n_old, const int64_t* __restrict__ tptr, int32_t* __restrict__ trow, double* __restrict__ tdist,
                                                    uint8_t* __restrict__ tbit)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_old) return;
    const int64_t b0 = tptr[x], b1 = tptr[x + 1];
    for (int64_t i = b0 + 1; i < b1; ++i) {
        const int32_t r = trow[i]; const double dd = tdist[i]; const uint8_t bb = tbit[i];
        int64_t j = i;
        while (j > b0 && trow[j - 1] > r) { trow[j] = trow[j - 1]; tdist[j] = tdist[j - 1]; tbit[j] = tbit[j - 1]; --j; }
        trow[j] = r; tdist[j] = dd; tbit[j] = bb;
    }
}

struct gw_merge_args {
    int64_t n_old, n_all; int d, check;
    const double* Xo; double r2, s;                        // s = fl(sqrt(r2)): the tie of the stored distances
    const int64_t* colptr; const int32_t* rowval; const double* nzval; const uint64_t* efree;      // the old graph
    const int64_t* nptr; const int32_t* nidx; const double* ndist; const uint8_t* nbits;           // the new columns, ascending
    const int64_t* tptr; const int32_t* trow; const double* tdist; const uint8_t* tbit;            // the old columns' new rows, ascending
    int64_t* cnt;                                          // count: [n_all + 1] entries per grown column
    const int64_t* optr; int32_t* orow; double* oval; uint8_t* obyte;                              // fill
    unsigned long long* dropped;
    unsigned long long* changed; unsigned long long* flagged;      // count: bitmap of the changed columns [ceil(n_all / 64)], its population
};

// does old entry e of column x stay at the new radius?  The stored distance decides unless it sits on the tie
__device__ __forceinline__ bool gw_kept(const gw_merge_args& a, int64_t x, int64_t e)
{
    const double nz = a.nzval[e];
    if (nz < a.s) return true;
    if (nz > a.s) return false;
    const double* px = a.Xo + x * a.d;
    const double* py = a.Xo + (int64_t)a.rowval[e] * a.d;
    double d2 = 0.0;
    for (int i = 0; i < a.d; ++i) {
        const double t = px[i] - py[i];
        const double tt = t * t;
        d2 = (i == 0) ? tt : d2 + tt;
    }
    return d2 <= a.r2;
}

// one wavefront per grown column; FILL = false counts, true writes rowval / nzval and one byte per entry
template <bool FILL>
__global__ __launch_bounds__(256) void k_grow_merge(gw_merge_args a)
{
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= a.n_all) return;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int64_t o = FILL ? a.optr[x] : 0;
    const int64_t o_end = FILL ? a.optr[x + 1] : 0;
    int64_t kept = 0, nadd;
    const int32_t* arow; const double* adist; const uint8_t* abit;
    int64_t ab;
    if (x < a.n_old) {
        const int64_t e0 = a.colptr[x], e1 = a.colptr[x + 1];
        if (!FILL && !a.check) kept = e1 - e0;
        else
            for (int64_t eb = e0; eb < e1; eb += 64) {
                const int64_t e = eb + lane;
                const bool valid = e < e1;
                const bool keep = valid && (!a.check || gw_kept(a, x, e));
                const unsigned long long m = __ballot(keep);
                if (FILL) {
                    const int64_t pos = o + kept + __popcll(m & lt);
                    if (keep && pos < o_end) {
                        a.orow[pos] = a.rowval[e]; a.oval[pos] = a.nzval[e];
                        a.obyte[pos] = (uint8_t)((a.efree[e >> 6] >> (e & 63)) & 1ull);
                    }
                }
                kept += __popcll(m);
            }
        if (!FILL && a.check && lane == 0 && kept < e1 - e0) atomicAdd(a.dropped, (unsigned long long)(e1 - e0 - kept));
        ab = a.tptr[x]; nadd = a.tptr[x + 1] - ab;
        arow = a.trow; adist = a.tdist; abit = a.tbit;
    } else {
        ab = a.nptr[(x - a.n_old) * GW_WAVES]; nadd = a.nptr[(x - a.n_old + 1) * GW_WAVES] - ab;
        arow = a.nidx; adist = a.ndist; abit = a.nbits;
    }
    if (!FILL) {
        if (lane == 0) {
            a.cnt[x] = kept + nadd;
            const bool chg = x >= a.n_old || nadd > 0 || kept < a.colptr[x + 1] - a.colptr[x];
            if (chg) { atomicOr(&a.changed[x >> 6], 1ull << (x & 63)); atomicAdd(a.flagged, 1ull); }
        }
        return;
    }
    for (int64_t t = lane; t < nadd; t += 64) {
        const int64_t pos = o + kept + t;
        if (pos < o_end) { a.orow[pos] = arow[ab + t]; a.oval[pos] = adist[ab + t]; a.obyte[pos] = (uint8_t)(abit[ab + t] & 1); }
    }
}

// the mask out of the bytes: a wavefront owns the 64 output words [w0, w0 + 64), word w0 + k is the ballot of bytes [64 (w0 + k), + 64)
__global__ __launch_bounds__(256) void k_grow_repack(const uint8_t* __restrict__ byte, int64_t nnz, int64_t words, uint64_t* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t w0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (w0 >= words) return;
    unsigned long long mine = 0ull;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) {
        const int64_t e = (w0 + k) * 64 + lane;
        const bool on = e < nnz && byte[e] != 0;             // (behind the last entry: zero)
        const unsigned long long m = __ballot(on);
        if (lane == k) mine = m;
    }
    if (w0 + lane < words) out[w0 + lane] = mine;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------

static int32_t gw_near_launch(mpfmt_ctx* ctx, gw_near_args& a, double r)
{
    a.Xo = ctx->Xo; a.Xt = ctx->Xt; a.perm = ctx->perm; a.cellstart = ctx->cellstart;
    a.r2 = r * r; a.rpad = r * (1.0 + 1e-9) + 1e-300;
    a.boxes = ctx->boxes; a.M = ctx->M;
    const size_t box_bytes = (size_t)ctx->M * 2 * ctx->d * sizeof(double);
    a.stage = (ctx->M > 0 && box_bytes <= GW_LDS_BOXES) ? 1 : 0;
    const size_t lds = (a.stage && a.mode != 0) ? box_bytes : 0;
    const unsigned nb = (unsigned)a.n_add;
    if (a.mode == 0) { DISPATCH_D(ctx->d, hipLaunchKernelGGL((k_grow_near<DD, 0>), dim3(nb), dim3(GW_WAVES * 64), lds, ctx->stream, a, ctx->grid, ctx->ss)); }
    else { DISPATCH_D(ctx->d, hipLaunchKernelGGL((k_grow_near<DD, 1>), dim3(nb), dim3(GW_WAVES * 64), lds, ctx->stream, a, ctx->grid, ctx->ss)); }
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

int32_t mpfmt_grow_apply(mpfmt_ctx* ctx, int64_t n_old, double r_new, int32_t carry)
{
    int32_t rc;
    const int64_t N = ctx->N, n_add = N - n_old, nnz_old = ctx->nnz;
    const int d = ctx->d;
    const bool check = r_new < ctx->graph_r || ctx->graph_imported;      // (a built graph at its own radius keeps every entry)
    // the grid of the grown set at r_new: rewrites the cell order and nothing of the graph, whose flags mpfmt_build_grid clears
    {
        const double gr = ctx->graph_r;
        const bool counted = ctx->graph_counted, filled = ctx->graph_filled, swept = ctx->graph_swept;
        ctx->grid_r = -1.0;
        rc = mpfmt_build_grid(ctx, r_new, true);
        ctx->graph_r = gr; ctx->graph_counted = counted; ctx->graph_filled = filled; ctx->graph_swept = swept; ctx->knn_k = 0;
        ctx->rowpos_valid = false; ctx->pend_valid = false; ctx->pool_valid = false; ctx->spec_ready = false; ctx->tptr_valid = false;
        ctx->wf_seen_epoch = -1;
        if (rc) return rc;
    }
    // ---- near pass ----
    // the call's temporaries live in three grow-only buffers of the ctx (no allocation on a repeated call): the counters, whose sizes
    // N and n_add give; the lists, sized by the near pass's total; one byte per grown entry, sized by the merge's count
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const int64_t nvq = n_add * GW_WAVES;                     // (new sample, part) pairs: the near pass's units
    const size_t o_ncnt = 0, o_nptr = o_ncnt + up(sizeof(int64_t) * (size_t)(nvq + 1)), o_ctr = o_nptr + up(sizeof(int64_t) * (size_t)(nvq + 1)),
                 o_tcnt = o_ctr + up(sizeof(unsigned long long) * 3), o_tcur = o_tcnt + up(sizeof(int64_t) * (size_t)(n_old + 1)),
                 o_tptr = o_tcur + up(sizeof(int64_t) * (size_t)(n_old + 1)), o_mcnt = o_tptr + up(sizeof(int64_t) * (size_t)(n_old + 1)),
                 o_chg = o_mcnt + up(sizeof(int64_t) * (size_t)(N + 1)), a_bytes = o_chg + up(sizeof(uint64_t) * (size_t)((N + 63) / 64));
    if ((rc = ctx->grow_counts.ensure(ctx, a_bytes))) return rc;
    char* ca = (char*)ctx->grow_counts.get();
    int64_t* ncnt = (int64_t*)(ca + o_ncnt); int64_t* nptr = (int64_t*)(ca + o_nptr);
    unsigned long long* ctr = (unsigned long long*)(ca + o_ctr);      // [0] candidates, [1] dropped, [2] changed columns (the 256 bytes hold them)
    unsigned long long* chg = (unsigned long long*)(ca + o_chg);      // bitmap of the changed columns over the grown set
    unsigned long long* tcnt = (unsigned long long*)(ca + o_tcnt); unsigned long long* tcur = (unsigned long long*)(ca + o_tcur);
    int64_t* tptr = (int64_t*)(ca + o_tptr); int64_t* mcnt = (int64_t*)(ca + o_mcnt);
    HIPCHK(ctx, hipMemsetAsync(ca, 0, a_bytes, ctx->stream));
    mpfmt_timed tn(ctx);
    gw_near_args na{};
    na.n_old = n_old; na.n_add = n_add; na.mode = 0; na.cnt = ncnt; na.ncand = ctr;
    if ((rc = gw_near_launch(ctx, na, r_new))) return rc;
    if ((rc = mpfmt_scan_i64(ctx, ncnt, nptr, (size_t)(nvq + 1)))) return rc;
    int64_t total = 0;
    HIPCHK(ctx, hipMemcpyAsync(&total, nptr + nvq, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t l4 = up(sizeof(int32_t) * (size_t)total), l8 = up(sizeof(double) * (size_t)total), l1 = up((size_t)total);
    if ((rc = ctx->grow_lists.ensure(ctx, 3 * (l4 + l8 + l1)))) return rc;
    char* cl = (char*)ctx->grow_lists.get();
    int32_t *idx_c = (int32_t*)cl, *nidx = (int32_t*)(cl + l4), *trow = (int32_t*)(cl + 2 * l4);
    double *dist_c = (double*)(cl + 3 * l4), *ndist = (double*)(cl + 3 * l4 + l8), *tdist = (double*)(cl + 3 * l4 + 2 * l8);
    uint8_t *bits_c = (uint8_t*)(cl + 3 * (l4 + l8)), *nbits = bits_c + l1, *tbit = bits_c + 2 * l1;
    const unsigned nb4 = (unsigned)((n_add + 3) / 4);
    if (total > 0) {
        HIPCHK(ctx, hipMemsetAsync(ctr, 0, sizeof(unsigned long long), ctx->stream));      // (the fill counts its candidates again)
        na.mode = 1; na.ptr = nptr; na.idx = idx_c; na.dist = dist_c; na.bits = bits_c;
        if ((rc = gw_near_launch(ctx, na, r_new))) return rc;
        hipLaunchKernelGGL(k_grow_sort, dim3(nb4), dim3(256), 0, ctx->stream, n_add, n_old, (const int64_t*)nptr, (const int32_t*)idx_c, (const double*)dist_c,
                           (const uint8_t*)bits_c, nidx, ndist, nbits, tcnt);
        HIPCHK(ctx, hipGetLastError());
    }
    // ---- transposition ----
    if ((rc = mpfmt_scan_i64(ctx, (const int64_t*)tcnt, tptr, (size_t)(n_old + 1)))) return rc;
    if (total > 0) {
        hipLaunchKernelGGL(k_grow_scatter, dim3(nb4), dim3(256), 0, ctx->stream, n_add, n_old, (const int64_t*)nptr, (const int32_t*)nidx, (const double*)ndist,
                           (const uint8_t*)nbits, (const int64_t*)tptr, tcur, trow, tdist, tbit);
        if (n_old > 0)
            hipLaunchKernelGGL(k_grow_tsort, dim3((unsigned)((n_old + 255) / 256)), dim3(256), 0, ctx->stream, n_old, (const int64_t*)tptr, trow, tdist, tbit);
        HIPCHK(ctx, hipGetLastError());
    }
    tn.end("samples_add_near");
    // ---- merge ----
    mpfmt_timed tg(ctx);
    if ((rc = ctx->colptr_next.ensure(ctx, sizeof(int64_t) * (size_t)(N + 1)))) return rc;
    gw_merge_args ma{};
    ma.n_old = n_old; ma.n_all = N; ma.d = d; ma.check = check ? 1 : 0;
    ma.Xo = ctx->Xo; ma.r2 = r_new * r_new; ma.s = std::sqrt(ma.r2);
    ma.colptr = ctx->colptr; ma.rowval = ctx->rowval; ma.nzval = ctx->nzval; ma.efree = ctx->graph_free;
    ma.nptr = nptr; ma.nidx = nidx; ma.ndist = ndist; ma.nbits = nbits;
    ma.tptr = tptr; ma.trow = trow; ma.tdist = tdist; ma.tbit = tbit;
    ma.cnt = mcnt; ma.dropped = ctr + 1; ma.changed = chg; ma.flagged = ctr + 2;
    const unsigned nbm = (unsigned)((N + 3) / 4);
    hipLaunchKernelGGL(k_grow_merge<false>, dim3(nbm), dim3(256), 0, ctx->stream, ma);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = mpfmt_scan_i64(ctx, mcnt, ctx->colptr_next, (size_t)(N + 1)))) return rc;
    int64_t nnz_new = 0;
    unsigned long long hctr[3] = {0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(&nnz_new, ctx->colptr_next.get() + N, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hctr, ctr, sizeof(hctr), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t words = (nnz_new + 63) / 64;
    if ((rc = ctx->grow_bytes.ensure(ctx, (size_t)nnz_new))) return rc;
    uint8_t* obyte = (uint8_t*)ctx->grow_bytes.get();
    if ((rc = ctx->rowval_next.ensure(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(nnz_new, 1)))) return rc;
    if ((rc = ctx->nzval_next.ensure(ctx, sizeof(double) * (size_t)std::max<int64_t>(nnz_new, 1)))) return rc;
    if ((rc = ctx->free_next.ensure(ctx, sizeof(uint64_t) * (size_t)std::max<int64_t>(words, 1)))) return rc;
    if (nnz_new > 0) {
        ma.optr = ctx->colptr_next; ma.orow = ctx->rowval_next; ma.oval = ctx->nzval_next; ma.obyte = obyte;
        hipLaunchKernelGGL(k_grow_merge<true>, dim3(nbm), dim3(256), 0, ctx->stream, ma);
        hipLaunchKernelGGL(k_grow_repack, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, ctx->stream, (const uint8_t*)obyte, nnz_new, words,
                           ctx->free_next.get());
        HIPCHK(ctx, hipGetLastError());
    }
    tg.end("samples_add_merge");
    // ---- the tracked fields follow (option "samples_add_keeps_fields"): into spare buffers of their own, over the grown arrays ----
    if (carry) {
        mpfmt_timed tc(ctx);
        if ((carry & 1) && (rc = mpfmt_field_carry(ctx, n_old, ctx->colptr_next, ctx->rowval_next, (const uint64_t*)chg))) return rc;
        if ((carry & 2) && (rc = mpfmt_togo_carry(ctx, n_old, (const uint64_t*)chg))) return rc;
        tc.end("samples_add_carry");
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // ---- everything has succeeded: the grown arrays change places with the ctx's own ----
    ctx->colptr.swap(ctx->colptr_next); ctx->rowval.swap(ctx->rowval_next); ctx->nzval.swap(ctx->nzval_next);
    ctx->graph_free.swap(ctx->free_next);
    ctx->nnz = nnz_new; ctx->nnz_cap = 0;
    ctx->graph_r = r_new; ctx->graph_counted = ctx->graph_filled = true; ctx->graph_swept = true; ctx->knn_k = 0;
    ctx->graph_epoch += 1; ctx->sweep_epoch += 1;
    ctx->sweep_in_order = false; ctx->sweep_pending_used = false; ctx->bits_in_records = false;
    ctx->grow_candidates = (int64_t)hctr[0];
    ctx->grow_dropped = (int64_t)hctr[1];
    ctx->grow_flagged = (int64_t)hctr[2];
    ctx->grow_entries = nnz_new - (nnz_old - ctx->grow_dropped);
    return MPFMT_OK;
}
