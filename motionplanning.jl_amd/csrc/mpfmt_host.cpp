// Host-only part of libmpfmt.so: the sequential dynamic-programming recursion of the reference (src/planners/fmt.jl:43-101)
// over GPU-built arrays, its priority queue, the goal predicates and the validation of imported graphs.  Plain C++17, no HIP:
// this file is compiled into the library by hipcc and, unchanged, into the sanitizer test binary of tests/asan/ by g++
// (-fsanitize=address,undefined).
#include "mpfmt_host.h"
#include "discretize_core.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

// binary min-heap on (cost, index): Base.Collections.PriorityQueue of fmt.jl:51,66,78,86.  Ties on cost are
// broken by the lowest sample index (the reference leaves the order of equal priorities unspecified).
struct Heap {
    std::vector<double> pri; std::vector<int64_t> idx;
    bool less(size_t a, size_t b) const { return pri[a] < pri[b] || (pri[a] == pri[b] && idx[a] < idx[b]); }
    void push(int64_t i, double p)
    {
        pri.push_back(p); idx.push_back(i);
        size_t c = pri.size() - 1;
        while (c > 0) { size_t par = (c - 1) / 2; if (less(c, par)) { std::swap(pri[c], pri[par]); std::swap(idx[c], idx[par]); c = par; } else break; }
    }
    int64_t pop()
    {
        int64_t top = idx[0];
        pri[0] = pri.back(); idx[0] = idx.back(); pri.pop_back(); idx.pop_back();
        size_t n = pri.size(), c = 0;
        for (;;) {
            size_t l = 2 * c + 1, r = l + 1, m = c;
            if (l < n && less(l, m)) m = l;
            if (r < n && less(r, m)) m = r;
            if (m == c) break;
            std::swap(pri[c], pri[m]); std::swap(idx[c], idx[m]); c = m;
        }
        return top;
    }
    bool empty() const { return pri.empty(); }
};

// goal predicates, src/goals.jl:96 (Rectangle), :100 (Ball), :111-114 (Point), Identity state2workspace
}  // namespace

bool mpfmt_is_goal_pt(const double* v, int d, int kind, const double* g)
{
    if (kind == MPFMT_GOAL_RECT) {
        for (int i = 0; i < d; ++i) if (!(g[i] <= v[i] && v[i] <= g[d + i])) return false;
        return true;
    }
    if (kind == MPFMT_GOAL_BALL) {
        double s = 0.0;
        for (int i = 0; i < d; ++i) { double t = v[i] - g[i]; double tt = t * t; s = (i == 0) ? tt : s + tt; }
        return std::sqrt(s) <= g[d];
    }
    for (int i = 0; i < d; ++i) if (!(v[i] == g[i])) return false;
    return true;
}


// The sequential recursion of fmt.jl:43-101 on a finished r-disc graph: CSC (0-based colptr / int32 rows, ascending
// rows = the order the reference's neighbourhood scans run in), per-entry free bits (row -> column motions) and the
// optional checkpts bitmap F.  Pure host code, no device use -- the GPU's job ends where this starts.
//   - W and H are bit sets (125 KB each at N = 1e6, cache resident): the inner scan touches C[y] / nzval only for the
//     few open neighbours;
//   - the candidates x in near(z) & W are collected first, so the adjacency rows of the NEXT candidates can be
//     prefetched while the current one is scanned (each row is a random ~400-byte read from a GB-sized array).
// gd = coordinates the goal predicate reads (d for Euclidean spaces; 2 = workspace (x, y) / 3 = whole state for SE2 cars);
// nseg != NULL: per-entry count of the segment tests the reference would make (car spaces), else one test per edge check
int32_t mpfmt_host_fmt_recursion_impl(int64_t N, int32_t d, const double* X, const int64_t* colptr, const int32_t* rowval,
                                       const double* nzval, const uint64_t* efree, const uint64_t* F, const double* ss_lo,
                                       const double* ss_hi, int64_t init_idx, int32_t goal_kind, const double* goal_params, int32_t gd,
                                       const uint8_t* nseg, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);

int32_t mpfmt_host_fmt_recursion(int64_t N, int32_t d, const double* X, const int64_t* colptr, const int32_t* rowval,
                                 const double* nzval, const uint64_t* efree, const uint64_t* F, const double* ss_lo,
                                 const double* ss_hi, int64_t init_idx, int32_t goal_kind, const double* goal_params,
                                 int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{
    return mpfmt_host_fmt_recursion_impl(N, d, X, colptr, rowval, nzval, efree, F, ss_lo, ss_hi, init_idx, goal_kind, goal_params, d, nullptr,
                                   A, C, path, res);
}

int32_t mpfmt_host_fmt_recursion_impl(int64_t N, int32_t d, const double* X, const int64_t* colptr, const int32_t* rowval,
                                       const double* nzval, const uint64_t* efree, const uint64_t* F, const double* ss_lo,
                                       const double* ss_hi, int64_t init_idx, int32_t goal_kind, const double* goal_params, int32_t gd,
                                       const uint8_t* nseg, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{
    if (!X || !colptr || !rowval || !nzval || !efree || !goal_params || !A || !C || !path || !res) return MPFMT_ERR_ARG;
    if (N < 1 || d < 1 || d > MPFMT_MAX_DIM || init_idx < 1 || init_idx > N || goal_kind < 0 || goal_kind > 2) return MPFMT_ERR_ARG;
    if ((ss_lo == nullptr) != (ss_hi == nullptr)) return MPFMT_ERR_ARG;
    const auto t_begin = std::chrono::steady_clock::now();
    const int64_t words = (N + 63) / 64;
    std::vector<uint64_t> Wb((size_t)words, ~0ull), Hb((size_t)words, 0ull);
    auto getb = [](const uint64_t* m, int64_t i) { return (m[(size_t)(i >> 6)] >> (i & 63)) & 1ull; };
    auto setb = [](std::vector<uint64_t>& m, int64_t i) { m[(size_t)(i >> 6)] |= 1ull << (i & 63); };
    auto clrb = [](std::vector<uint64_t>& m, int64_t i) { m[(size_t)(i >> 6)] &= ~(1ull << (i & 63)); };
    std::vector<int64_t> Hnew, cand;
    for (int64_t i = 0; i < N; ++i) { A[i] = 0; C[i] = 0.0; }
    Heap heap;
    const int64_t i0 = init_idx - 1;
    clrb(Wb, i0); setb(Hb, i0);
    heap.push(i0, 0.0);
    int64_t z = heap.pop();
    int64_t count = 0;
    auto prefetch_row = [&](int64_t x) {
        const char* p = (const char*)(rowval + colptr[x]);
        const char* e = (const char*)(rowval + colptr[x + 1]);
        for (int q = 0; q < 8 && p < e; ++q, p += 64) __builtin_prefetch(p, 0, 1);
    };
    while (!mpfmt_is_goal_pt(&X[(size_t)z * d], gd, goal_kind, goal_params)) {
        Hnew.clear();
        cand.clear();
        for (int64_t a = colptr[z]; a < colptr[z + 1]; ++a) {                 // fmt.jl:70-71
            const int64_t x = rowval[a];
            if (getb(Wb.data(), x) && (!F || getb(F, x))) cand.push_back(x);
        }
        const size_t nc = cand.size();
        for (size_t q = 0; q < nc && q < 3; ++q) prefetch_row(cand[q]);
        for (size_t q = 0; q < nc; ++q) {
            if (q + 3 < nc) prefetch_row(cand[q + 3]);
            const int64_t x = cand[q];
            int64_t y_min = -1, e_min = -1; double c_min = 0.0;
            for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) {             // fmt.jl:72-74
                const int64_t y = rowval[b];
                if (!getb(Hb.data(), y)) continue;
                const double c = C[y] + nzval[b];
                if (y_min < 0 || c < c_min) { y_min = y; c_min = c; e_min = b; }
            }
            if (y_min < 0) continue;
            if (nseg) {
                count += nseg[e_min];
            } else {   // boxesND.jl:26 is only reached when in_state_space(V[y_min]) held (statespaces.jl:155-157)
                bool inb = true;
                if (ss_lo) for (int k = 0; k < d; ++k) inb = inb && (ss_lo[k] <= X[(size_t)y_min * d + k]) && (X[(size_t)y_min * d + k] <= ss_hi[k]);
                if (inb) ++count;
            }
            if (getb(efree, e_min)) {                                         // fmt.jl:75
                A[x] = y_min + 1; C[x] = c_min;
                heap.push(x, c_min);
                Hnew.push_back(x);
                clrb(Wb, x);
            }
        }
        for (int64_t x : Hnew) setb(Hb, x);                                   // fmt.jl:83
        clrb(Hb, z);                                                          // fmt.jl:84
        if (!heap.empty()) z = heap.pop(); else break;                        // fmt.jl:85-89
    }
    // path back-trace, fmt.jl:92-101 (walks until sample 1)
    std::vector<int64_t> rev;
    int64_t cur = z;
    rev.push_back(cur + 1);
    while (cur != 0) {
        const int64_t p = A[cur];
        if (p == 0) break;
        cur = p - 1;
        rev.push_back(cur + 1);
    }
    for (size_t i = 0; i < rev.size(); ++i) path[i] = rev[rev.size() - 1 - i];
    res->status = mpfmt_is_goal_pt(&X[(size_t)z * d], gd, goal_kind, goal_params) ? 1 : 0;
    res->cost = C[z];
    res->z = z + 1;
    res->collision_checks = count;
    res->path_len = (int64_t)rev.size();
    res->nnz = colptr[N];
    res->ms_host_loop = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return MPFMT_OK;
}


// fmt.jl:43-101 over a DIRECTED cost graph (quasi-metric spaces: double integrator, Dubins car): forward sets = rows of the
// cost matrix (DSF = Dmat', linearquadratic.jl:73), backward sets = its columns (the CSC given).  efree / nseg are per CSC
// entry (row -> column motion free; segment tests the reference would have counted; nseg NULL: one each), F the checkpts bitmap
// (may be NULL).  fwd_mask (per CSC entry, may be NULL: all) restricts the FORWARD sets: the examination loop (fmt.jl:70) walks an
// entry (row z in column x) only when its bit is set -- the k-nearest graph's mutualknnF(z) = { x : z in knn(x) and x in knn(z) } --
// while the backward sets stay whole columns: an open y in column x is a candidate parent of x whatever its bit, so the incremental
// relaxation of open_node and the rescan both ignore the mask.
void mpfmt_directed_fmt_recursion(int64_t N, const int64_t* colptr_, const int32_t* rowval_, const double* nzval_, const uint64_t* efree_,
                                  const uint8_t* nseg_, const uint64_t* F_, int64_t init_idx, const std::function<bool(int64_t)>& goal_hit,
                                  int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res, const mpfmt_csr_view* pre,
                                  const uint64_t* fwd_mask)
{
    const int64_t nnz = colptr_[N];
    struct view64 { const int64_t* p; int64_t operator[](int64_t i) const { return p[i]; } };
    struct view32 { const int32_t* p; int32_t operator[](int64_t i) const { return p[i]; } };
    struct viewd { const double* p; double operator[](int64_t i) const { return p[i]; } };
    struct view8 { const uint8_t* p; uint8_t operator[](int64_t i) const { return p[i]; } };
    const view64 colptr{colptr_}; const view32 rowval{rowval_}; const viewd nzval{nzval_}; const view8 nseg{nseg_};
    const bool checkpts = F_ != nullptr;
    auto bitp = [](const uint64_t* m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1ull; };
    // forward sets: CSR of the cost matrix (DSF = Dmat', linearquadratic.jl:73), rows ascending in target index -- taken from
    // the device transpose when the caller has one (mpfmt_csc_transpose_device), else built here
    std::vector<int64_t> rowptr_own, centry_own;
    std::vector<int32_t> colidx_own;
    const int64_t* rowptr;
    const int32_t* colidx;
    const uint32_t* centry32 = nullptr;
    if (pre) {
        rowptr = pre->rowptr; colidx = pre->colidx; centry32 = pre->centry;
    } else {
        rowptr_own.assign((size_t)N + 1, 0); colidx_own.resize((size_t)std::max<int64_t>(nnz, 1)); centry_own.resize((size_t)std::max<int64_t>(nnz, 1));
        std::vector<int64_t> cur((size_t)N);
        for (int64_t e = 0; e < nnz; ++e) rowptr_own[rowval[e] + 1]++;
        for (int64_t i = 0; i < N; ++i) rowptr_own[i + 1] += rowptr_own[i];
        for (int64_t i = 0; i < N; ++i) cur[i] = rowptr_own[i];
        for (int64_t j = 0; j < N; ++j)
            for (int64_t e = colptr[j]; e < colptr[j + 1]; ++e) { const int64_t a = cur[rowval[e]]++; colidx_own[a] = (int32_t)j; centry_own[a] = e; }
        rowptr = rowptr_own.data(); colidx = colidx_own.data();
    }
    auto centry_at = [&](int64_t a) -> int64_t { return centry32 ? (int64_t)centry32[a] : centry_own[a]; };
    // The recursion of fmt.jl:43-90.  DI neighbourhoods are large (hundreds of entries) and arcs are often blocked, so a
    // sample can be examined by many expanding neighbours; rescanning nearB(x) & H each time is what the reference does
    // and is O(N deg^2).  Here the argmin over the OPEN backward neighbours is maintained instead: when y opens it
    // relaxes best[x] of its forward neighbours still in W; when the best itself has closed, x is rescanned once.  The
    // order is the reference's (lowest cost, then lowest index = first minimum of its scan), so A, C, the path and the
    // collision count are unchanged.
    std::vector<uint8_t> Wm(N, 1), Hm(N, 0);
    std::vector<int64_t> Hnew;
    std::vector<int64_t> by(N, -1), be(N, -1);       // best open parent of x and its CSC entry (-1 none, -2 rescan)
    std::vector<double> bc(N, 0.0);
    for (int64_t i = 0; i < N; ++i) { A[i] = 0; C[i] = 0.0; }
    auto open_node = [&](int64_t y) {                 // y has just entered H: offer it to its forward neighbours
        Hm[y] = 1;
        const double cy = C[y];
        for (int64_t a = rowptr[y]; a < rowptr[y + 1]; ++a) {
            const int64_t x = colidx[a];
            if (!Wm[x] || by[x] == -2) continue;
            if (by[x] >= 0 && !Hm[by[x]]) { by[x] = -2; continue; }           // its best has closed: rescan when examined
            const int64_t e = centry_at(a);
            const double c = cy + nzval[e];
            if (by[x] < 0 || c < bc[x] || (c == bc[x] && y < by[x])) { by[x] = y; bc[x] = c; be[x] = e; }
        }
    };
    Heap heap;
    const int64_t i0 = init_idx - 1;
    Wm[i0] = 0;
    open_node(i0);
    heap.push(i0, 0.0);
    int64_t z = heap.pop();
    int64_t count = 0;
    while (!goal_hit(z)) {
        Hnew.clear();
        for (int64_t a = rowptr[z]; a < rowptr[z + 1]; ++a) {                  // nearF(V, z, r, W), fmt.jl:70
            const int64_t x = colidx[a];
            if (!Wm[x]) continue;
            if (fwd_mask && !bitp(fwd_mask, centry_at(a))) continue;             // not a forward neighbour of z (mutualknnF)
            if (checkpts && !bitp(F_, x)) continue;
            if (by[x] == -2 || (by[x] >= 0 && !Hm[by[x]])) {                   // nearB(V, x, r, H), fmt.jl:72-74
                int64_t y_min = -1, e_min = -1; double c_min = 0.0;
                for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) {
                    const int64_t y = rowval[b];
                    if (!Hm[y]) continue;
                    const double c = C[y] + nzval[b];
                    if (y_min < 0 || c < c_min) { y_min = y; c_min = c; e_min = b; }
                }
                by[x] = y_min; bc[x] = c_min; be[x] = e_min;
            }
            if (by[x] < 0) continue;
            const int64_t y_min = by[x], e_min = be[x];
            count += nseg_ ? nseg[e_min] : 1;                                             // boxesND.jl:26 per tested segment
            if (bitp(efree_, e_min)) {
                A[x] = y_min + 1; C[x] = bc[x];
                heap.push(x, bc[x]);
                Hnew.push_back(x);
                Wm[x] = 0;
            }
        }
        Hm[z] = 0;                                                             // fmt.jl:84 (before 83: same final sets)
        for (int64_t x : Hnew) open_node(x);                                   // fmt.jl:83
        if (!heap.empty()) z = heap.pop(); else break;
    }
    std::vector<int64_t> rev;
    int64_t cu = z;
    rev.push_back(cu + 1);
    while (cu != 0) { const int64_t p = A[cu]; if (p == 0) break; cu = p - 1; rev.push_back(cu + 1); }
    for (size_t i = 0; i < rev.size(); ++i) path[i] = rev[rev.size() - 1 - i];
    res->status = goal_hit(z) ? 1 : 0;
    res->cost = C[z]; res->z = z + 1; res->collision_checks = count; res->path_len = (int64_t)rev.size(); res->nnz = nnz;
}

// The goal node of the roadmap planners over a finished field C (+Inf = unreached): the reached sample inside the goal region of lowest
// (C, index), 0-based, or -1.  X holds N states of d coordinates; the goal reads the first gd of them (d in a Euclidean space; in a steering
// space the workspace coordinates, and the whole state for a POINT goal: StateGoal is exact state equality, goals.jl:128-131).
int64_t mpfmt_goal_pick(int64_t N, int d, int gd, const double* X, const double* C, int goal_kind, const double* goal_params)
{
    int64_t z = -1;
    for (int64_t i = 0; i < N; ++i)
        if (C[i] < INFINITY && (z < 0 || C[i] < C[z]) && mpfmt_is_goal_pt(&X[(size_t)i * d], gd, goal_kind, goal_params)) z = i;
    return z;
}

// The goal walk of the roadmap planners over a finished field: labels C, parents A (1-based, 0 = none), the source init_idx (1-based)
// and the goal node z the caller picked (0-based; -1: no reached sample is a goal).  path = init_idx ... z + 1 by the parents, or
// [init_idx] without a goal node.  A walk stops at the source, at a parent of 0, and after N hops whatever A holds: path has N slots.
void mpfmt_walk_back(int64_t N, const double* C, const int64_t* A, int64_t init_idx, int64_t z, int64_t* path, mpfmt_fmt_result* res)
{
    std::vector<int64_t> rev;
    if (z >= 0) {
        int64_t cur = z;
        rev.push_back(cur + 1);
        while (cur != init_idx - 1 && (int64_t)rev.size() <= N) {
            const int64_t p = A[cur];
            if (p == 0) break;
            cur = p - 1;
            rev.push_back(cur + 1);
        }
        res->status = 1; res->cost = C[z]; res->z = z + 1;
    } else {
        rev.push_back(init_idx);
        res->status = 0; res->cost = INFINITY; res->z = init_idx;
    }
    for (size_t i = 0; i < rev.size() && i < (size_t)N; ++i) path[i] = rev[rev.size() - 1 - i];
    res->path_len = (int64_t)std::min<size_t>(rev.size(), (size_t)N);
    res->collision_checks = 0;
}

// PRM* cost-to-come field over the free-edge graph (include/mpfmt.h, "roadmap queries"): a binary-heap Dijkstra from one source
// over the device-native CSC.  Entry b of column x with row y is the edge y -> x, so the scan of a settled y needs its out-edges:
// the CSR transpose is built here.  A label is the left-to-right fp64 fold of the weights along a path, fl(C[y] + w); fl(a + w) is
// nondecreasing in a and w >= 0, so the order in which Dijkstra settles does not matter for the values: they are the least fixed
// point of C[x] = min_y fl(C[y] + w_yx), the same one the device's chaotic relaxation reaches (csrc/kernels_sssp.hip).  Parents are
// not taken from the relaxation: the final pass below picks, per reached x, the usable y of lowest (C[y], y) with
// fl(C[y] + w) == C[x] -- the rule of the device's parent kernel, a function of C alone.
int32_t mpfmt_host_graph_sssp(int64_t N, const int64_t* colptr, const int32_t* rowval, const double* nzval, const uint64_t* efree,
                              const uint64_t* F, int64_t source, double* C, int64_t* A)
{
    if (!colptr || !efree || !C || N < 1 || source < 1 || source > N) return MPFMT_ERR_ARG;
    if (colptr[0] != 0) return MPFMT_ERR_ARG;
    for (int64_t j = 0; j < N; ++j) if (colptr[j + 1] < colptr[j]) return MPFMT_ERR_ARG;
    const int64_t nnz = colptr[N];
    if (nnz > 0 && (!rowval || !nzval)) return MPFMT_ERR_ARG;
    for (int64_t e = 0; e < nnz; ++e) if (rowval[e] < 0 || rowval[e] >= N || !(nzval[e] >= 0.0)) return MPFMT_ERR_ARG;
    auto bitp = [](const uint64_t* m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1ull; };
    const int64_t s = source - 1;
    // out-edges of every sample: the usable entries only (free bit set, target allowed by F)
    std::vector<int64_t> rowptr((size_t)N + 1, 0);
    for (int64_t x = 0; x < N; ++x) {
        if (F && !bitp(F, x)) continue;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) if (bitp(efree, b)) rowptr[rowval[b] + 1]++;
    }
    for (int64_t i = 0; i < N; ++i) rowptr[i + 1] += rowptr[i];
    std::vector<int64_t> cur(rowptr.begin(), rowptr.end() - 1);
    std::vector<int32_t> tgt((size_t)std::max<int64_t>(rowptr[N], 1));
    std::vector<double> wgt((size_t)std::max<int64_t>(rowptr[N], 1));
    for (int64_t x = 0; x < N; ++x) {
        if (F && !bitp(F, x)) continue;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b)
            if (bitp(efree, b)) { const int64_t a = cur[rowval[b]]++; tgt[a] = (int32_t)x; wgt[a] = nzval[b]; }
    }
    for (int64_t i = 0; i < N; ++i) C[i] = INFINITY;
    C[s] = 0.0;
    Heap heap;
    heap.push(s, 0.0);
    while (!heap.empty()) {
        const double cy = heap.pri[0];
        const int64_t y = heap.pop();
        if (cy > C[y]) continue;                                               // a stale entry: y was settled at a lower label
        for (int64_t a = rowptr[y]; a < rowptr[y + 1]; ++a) {
            const int64_t x = tgt[a];
            const double c = cy + wgt[a];
            if (c < C[x]) { C[x] = c; heap.push(x, c); }
        }
    }
    if (!A) return MPFMT_OK;
    for (int64_t x = 0; x < N; ++x) {
        A[x] = 0;
        if (x == s || !(C[x] < INFINITY)) continue;
        int64_t yb = -1; double cb = 0.0;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) {
            if (!bitp(efree, b)) continue;
            const int64_t y = rowval[b];
            const double cy = C[y];
            if (!(cy + nzval[b] == C[x])) continue;
            if (yb < 0 || cy < cb || (cy == cb && y < yb)) { yb = y; cb = cy; }
        }
        A[x] = yb + 1;
    }
    return MPFMT_OK;
}

// PRM* cost-to-go field of a target set (include/mpfmt.h, "cost-to-go"): a binary-heap Dijkstra over the REVERSED edges.  Entry b of
// column x with row y is the edge y -> x; a settled x offers fl(G[x] + w) to the rows of its own column, so the reversed graph IS the
// CSC and the scan reads the columns in place (usable: free bit set, F[x] set; no exemption).  The values are the least fixed point of
// G[y] = min(G0[y], min_x fl(G[x] + w_yx)), the one the device's push reaches (csrc/kernels_sssp_to.hip).  Successors come from a
// final pass over the finished G: per reached non-target y the usable x of lowest (G[x], x) with fl(G[x] + w) == G[y]; the pass walks
// the columns, so the candidates of a y arrive in no particular order and the minimum is kept per y.
int32_t mpfmt_host_graph_sssp_to(int64_t N, const int64_t* colptr, const int32_t* rowval, const double* nzval, const uint64_t* efree,
                                 const uint64_t* F, const int64_t* targets, int64_t ntgt, double* G, int64_t* S)
{
    if (!colptr || !efree || !G || N < 1 || ntgt < 0 || (ntgt > 0 && !targets)) return MPFMT_ERR_ARG;
    if (colptr[0] != 0) return MPFMT_ERR_ARG;
    for (int64_t j = 0; j < N; ++j) if (colptr[j + 1] < colptr[j]) return MPFMT_ERR_ARG;
    const int64_t nnz = colptr[N];
    if (nnz > 0 && (!rowval || !nzval)) return MPFMT_ERR_ARG;
    for (int64_t e = 0; e < nnz; ++e) if (rowval[e] < 0 || rowval[e] >= N || !(nzval[e] >= 0.0)) return MPFMT_ERR_ARG;
    for (int64_t q = 0; q < ntgt; ++q) if (targets[q] < 1 || targets[q] > N) return MPFMT_ERR_ARG;
    auto bitp = [](const uint64_t* m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1ull; };
    std::vector<uint8_t> is_tgt((size_t)N, 0);
    for (int64_t i = 0; i < N; ++i) G[i] = INFINITY;
    Heap heap;
    for (int64_t q = 0; q < ntgt; ++q) {
        const int64_t t = targets[q] - 1;
        if (!is_tgt[t]) { is_tgt[t] = 1; G[t] = 0.0; heap.push(t, 0.0); }
    }
    while (!heap.empty()) {
        const double gx = heap.pri[0];
        const int64_t x = heap.pop();
        if (gx > G[x]) continue;                                               // a stale entry: x was settled at a lower label
        if (F && !bitp(F, x)) continue;                                        // no usable edge into x
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) {
            if (!bitp(efree, b)) continue;
            const int64_t y = rowval[b];
            const double c = gx + nzval[b];
            if (c < G[y]) { G[y] = c; heap.push(y, c); }
        }
    }
    if (!S) return MPFMT_OK;
    std::vector<double> best((size_t)N, INFINITY);
    for (int64_t i = 0; i < N; ++i) S[i] = 0;
    for (int64_t x = 0; x < N; ++x) {
        const double gx = G[x];
        if (!(gx < INFINITY) || (F && !bitp(F, x))) continue;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) {
            if (!bitp(efree, b)) continue;
            const int64_t y = rowval[b];
            if (is_tgt[y] || !(gx + nzval[b] == G[y])) continue;
            if (S[y] == 0 || gx < best[y]) { S[y] = x + 1; best[y] = gx; }     // (x ascends: an equal G[x] keeps the lower index)
        }
    }
    return MPFMT_OK;
}

// The repair of a tracked field on the host (include/mpfmt.h, "a cost-to-come field kept valid across box edits"): steps 2-4 over the
// device-native arrays.  C / A hold the old field; efree / F are the new mask and point bitmap; dirty marks the columns the edits
// flagged.  I0 is tested on the dirty columns through the parent's entry (rows are distinct inside a column: the entry of A[x] is the
// one whose row is A[x]); the closure walks the children lists of the parent forest; the heap is seeded from the boundary -- every
// column of I u D looks at all its usable rows with finite labels -- and then corrects labels in key order.  Parents are those of
// mpfmt_host_graph_sssp, from the final labels alone.
int32_t mpfmt_host_field_repair(int64_t N, const int64_t* colptr, const int32_t* rowval, const double* nzval, const uint64_t* efree,
                                const uint64_t* F, const uint64_t* dirty, int64_t source, double* C, int64_t* A, int64_t* invalidated)
{
    if (!colptr || !efree || !dirty || !C || !A || N < 1 || source < 1 || source > N) return MPFMT_ERR_ARG;
    if (colptr[0] != 0) return MPFMT_ERR_ARG;
    for (int64_t j = 0; j < N; ++j) if (colptr[j + 1] < colptr[j]) return MPFMT_ERR_ARG;
    const int64_t nnz = colptr[N];
    if (nnz > 0 && (!rowval || !nzval)) return MPFMT_ERR_ARG;
    for (int64_t e = 0; e < nnz; ++e) if (rowval[e] < 0 || rowval[e] >= N || !(nzval[e] >= 0.0)) return MPFMT_ERR_ARG;
    for (int64_t x = 0; x < N; ++x) if (A[x] < 0 || A[x] > N || !(C[x] >= 0.0)) return MPFMT_ERR_ARG;
    auto bitp = [](const uint64_t* m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1ull; };
    const int64_t s = source - 1;
    // step 2: I0 on the dirty columns, then its descendants
    std::vector<char> inI((size_t)N, 0);
    std::vector<int64_t> stack;
    for (int64_t x = 0; x < N; ++x) {
        if (!bitp(dirty, x) || x == s || !(C[x] < INFINITY)) continue;
        bool lost = F && !bitp(F, x);
        if (!lost) {
            lost = true;                                                       // (no entry with the parent's row: the edge is gone)
            for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b)
                if (rowval[b] == A[x] - 1) { lost = !bitp(efree, b); break; }
        }
        if (lost) { inI[x] = 1; stack.push_back(x); }
    }
    std::vector<int64_t> cptr((size_t)N + 1, 0);
    for (int64_t x = 0; x < N; ++x) if (x != s && C[x] < INFINITY && A[x] > 0) cptr[A[x]]++;
    for (int64_t i = 0; i < N; ++i) cptr[i + 1] += cptr[i];
    std::vector<int64_t> ccur(cptr.begin(), cptr.end() - 1), child((size_t)std::max<int64_t>(cptr[N], 1));
    for (int64_t x = 0; x < N; ++x) if (x != s && C[x] < INFINITY && A[x] > 0) child[ccur[A[x] - 1]++] = x;
    int64_t nI = (int64_t)stack.size();
    while (!stack.empty()) {
        const int64_t p = stack.back(); stack.pop_back();
        for (int64_t a = cptr[p]; a < cptr[p + 1]; ++a) {
            const int64_t x = child[a];
            if (!inI[x]) { inI[x] = 1; ++nI; stack.push_back(x); }
        }
    }
    for (int64_t x = 0; x < N; ++x) if (inI[x]) C[x] = INFINITY;
    if (invalidated) *invalidated = nI;
    // out-edges of every sample: the usable entries only (free bit set, target allowed by F)
    std::vector<int64_t> rowptr((size_t)N + 1, 0);
    for (int64_t x = 0; x < N; ++x) {
        if (F && !bitp(F, x)) continue;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) if (bitp(efree, b)) rowptr[rowval[b] + 1]++;
    }
    for (int64_t i = 0; i < N; ++i) rowptr[i + 1] += rowptr[i];
    std::vector<int64_t> cur(rowptr.begin(), rowptr.end() - 1);
    std::vector<int32_t> tgt((size_t)std::max<int64_t>(rowptr[N], 1));
    std::vector<double> wgt((size_t)std::max<int64_t>(rowptr[N], 1));
    for (int64_t x = 0; x < N; ++x) {
        if (F && !bitp(F, x)) continue;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b)
            if (bitp(efree, b)) { const int64_t a = cur[rowval[b]]++; tgt[a] = (int32_t)x; wgt[a] = nzval[b]; }
    }
    // step 3: the boundary seeds the heap, then labels are corrected in key order
    Heap heap;
    for (int64_t x = 0; x < N; ++x) {
        if (!(inI[x] || bitp(dirty, x)) || x == s) continue;
        if (F && !bitp(F, x)) continue;
        double best = C[x];
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) {
            if (!bitp(efree, b)) continue;
            const double cy = C[rowval[b]];
            if (!(cy < INFINITY) || inI[rowval[b]]) continue;
            const double c = cy + nzval[b];
            if (c < best) best = c;
        }
        if (best < C[x]) { C[x] = best; heap.push(x, best); }
    }
    while (!heap.empty()) {
        const double cy = heap.pri[0];
        const int64_t y = heap.pop();
        if (cy > C[y]) continue;
        for (int64_t a = rowptr[y]; a < rowptr[y + 1]; ++a) {
            const int64_t x = tgt[a];
            if (x == s) continue;
            const double c = cy + wgt[a];
            if (c < C[x]) { C[x] = c; heap.push(x, c); }
        }
    }
    // step 4
    for (int64_t x = 0; x < N; ++x) {
        A[x] = 0;
        if (x == s || !(C[x] < INFINITY)) continue;
        int64_t yb = -1; double cb = 0.0;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) {
            if (!bitp(efree, b)) continue;
            const int64_t y = rowval[b];
            const double cy = C[y];
            if (!(cy + nzval[b] == C[x])) continue;
            if (yb < 0 || cy < cb || (cy == cb && y < yb)) { yb = y; cb = cy; }
        }
        A[x] = yb + 1;
    }
    return MPFMT_OK;
}

// ImmutableNNC(D, r) handed in from outside (mpfmt_graph_import; nearneighbors.jl:23-28): 1-based CSC, monotone colptr,
// rows in range, strictly ascending inside a column, no self loops.  Returns 0, or the 1-based column at fault (negative:
// -1 colptr[1] != 1, -2 colptr decreases) with a message in err.
int64_t mpfmt_validate_csc(int64_t N, const int64_t* colptr, const int64_t* rowval, char* err, size_t errlen)
{
    if (colptr[0] != 1) { snprintf(err, errlen, "colptr[1] must be 1 (1-based CSC)"); return -1; }
    for (int64_t j = 0; j < N; ++j)
        if (colptr[j + 1] < colptr[j]) { snprintf(err, errlen, "colptr decreases at column %lld", (long long)(j + 1)); return -2; }
    for (int64_t j = 0; j < N; ++j)
        for (int64_t e = colptr[j] - 1; e < colptr[j + 1] - 1; ++e) {
            const int64_t y = rowval[e];
            if (y < 1 || y > N || y == j + 1) { snprintf(err, errlen, "column %lld: row %lld out of range or a self loop", (long long)(j + 1), (long long)y); return j + 1; }
            if (e > colptr[j] - 1 && rowval[e - 1] >= y) { snprintf(err, errlen, "column %lld: rows are not strictly ascending", (long long)(j + 1)); return j + 1; }
        }
    return 0;
}

// ---- adaptive shortcutting of one path (src/postprocessors.jl:6-39) against the AABB checker: the CPU baseline and the checker of
// mpfmt_adaptive_shortcut_batch (kernels_shortcut.hip).  The recursion is the reference's, on index ranges of the working path instead
// of copies; the scalar predicates restate boxesND.jl:42-56 in the operation order of sweep_predicates.h.
namespace {

struct ShortcutWorld {
    int d; const double* lohi; int M; const double* ss_lo; const double* ss_hi;
    int64_t checks = 0, tests = 0;

    // free(v, w) = in_state_space(v) && is_free_motion(v, w, boxes) (statespaces.jl:153-158); the checker -- and its count, boxesND.jl:26
    // -- is reached only when the first point lies inside the bounds
    bool free(const double* v, const double* w)
    {
        ++tests;
        if (ss_lo) {
            bool in = true;
            for (int i = 0; i < d; ++i) in = in && (ss_lo[i] <= v[i]) && (v[i] <= ss_hi[i]);
            if (!in) return false;
        }
        ++checks;
        double l[MPFMT_MAX_DIM], h[MPFMT_MAX_DIM], v_to_w[MPFMT_MAX_DIM];
        for (int i = 0; i < d; ++i) {
            l[i] = (w[i] < v[i]) ? w[i] : v[i];                                  // map(min, v, w)
            h[i] = (v[i] < w[i]) ? w[i] : v[i];                                  // map(max, v, w)
            v_to_w[i] = w[i] - v[i];
        }
        for (int k = 0; k < M; ++k) {
            const double* lo = lohi + (size_t)k * 2 * d;
            const double* hi = lo + d;
            bool sep = false;                                                    // boxesND.jl:44-45
            for (int i = 0; i < d; ++i) sep = sep || (hi[i] < l[i]) || (lo[i] > h[i]);
            if (sep) continue;
            for (int i = 0; i < d; ++i) {                                        // boxesND.jl:46-51
                const double corner = (v[i] < lo[i]) ? lo[i] : hi[i];            // blend(v .< lo, lo, hi)
                const double lambda = (corner - v[i]) / v_to_w[i];               // IEEE: may be +-Inf / NaN
                bool all = true;
                for (int j = 0; j < d; ++j) {
                    if (j == i) continue;
                    const double prod = v_to_w[j] * lambda;
                    const double x = v[j] + prod;                                // unfused
                    all = all && (lo[j] <= x) && (x <= hi[j]);
                }
                if (all) return false;
            }
        }
        return true;
    }

    // shortcut(path[lo..hi]) (postprocessors.jl:6-16): appends the kept states after path[lo] to `keep`
    void shortcut(const std::vector<double>& p, int64_t lo, int64_t hi, std::vector<int64_t>& keep)
    {
        const int64_t N = hi - lo + 1;
        if (N == 2) { keep.push_back(hi); return; }
        if (free(&p[(size_t)lo * d], &p[(size_t)hi * d])) { keep.push_back(hi); return; }
        const int64_t mid = lo + (N + 1) / 2 - 1;                                // ceil(Int, N/2), 1-based inside the range
        shortcut(p, lo, mid, keep);
        shortcut(p, mid, hi, keep);
    }

    // `while (short_path = shortcut(path, CC)) != path` (:29-31, :34-36)
    void shortcut_fixed_point(std::vector<double>& p)
    {
        std::vector<int64_t> keep;
        std::vector<double> q;
        for (;;) {
            const int64_t n = (int64_t)(p.size() / d);
            keep.clear();
            keep.push_back(0);
            shortcut(p, 0, n - 1, keep);
            if ((int64_t)keep.size() == n) return;
            q.resize(keep.size() * d);
            for (size_t a = 0; a < keep.size(); ++a) memcpy(&q[a * d], &p[(size_t)keep[a] * d], sizeof(double) * d);
            p.swap(q);
        }
    }
};

}  // namespace

int32_t mpfmt_host_adaptive_shortcut(const double* P, int64_t n, int32_t d, const double* lohi, int32_t M, const double* ss_lo,
                                     const double* ss_hi, int32_t iterations, int64_t max_states, double* out_P, int64_t out_cap,
                                     double* cumcost, mpfmt_shortcut_info* info)
{
    if (!P || !out_P || !cumcost || !info || (M > 0 && !lohi)) return MPFMT_ERR_ARG;
    if (n < 2 || d < 1 || d > MPFMT_MAX_DIM || M < 0 || iterations < 0 || max_states < n || max_states > (1 << 20)) return MPFMT_ERR_ARG;
    if ((ss_lo == nullptr) != (ss_hi == nullptr)) return MPFMT_ERR_ARG;
    for (int64_t i = 0; i < n * d; ++i) if (!std::isfinite(P[i])) return MPFMT_ERR_ARG;
    ShortcutWorld W{d, lohi, M, ss_lo, ss_hi};
    std::vector<double> path(P, P + (size_t)n * d), next;
    memset(info, 0, sizeof *info);
    info->max_working_len = n;
    W.shortcut_fixed_point(path);
    double a[MPFMT_MAX_DIM], b[MPFMT_MAX_DIM], na[MPFMT_MAX_DIM], nb[MPFMT_MAX_DIM];
    for (int32_t it = 0; it < iterations; ++it) {
        const int64_t m = (int64_t)(path.size() / d);
        if (2 * m - 2 > max_states) { info->status = MPFMT_SHORTCUT_TRUNCATED; break; }
        next.assign(path.begin(), path.begin() + d);                             // path[1:1]
        bool stuck = false;
        for (int64_t j = 1; j + 1 < m && !stuck; ++j) {                          // cut_corner(path[j-1:j+1]..., CC)[2:3]
            const double *v1 = &path[(size_t)(j - 1) * d], *v2 = &path[(size_t)j * d], *v3 = &path[(size_t)(j + 1) * d];
            for (int i = 0; i < d; ++i) { const double s = v1[i] + v2[i]; a[i] = s / 2; const double t = v3[i] + v2[i]; b[i] = t / 2; }
            int64_t halvings = 0;
            while (!W.free(a, b)) {
                bool same = true;
                for (int i = 0; i < d; ++i) {
                    const double s = a[i] + v2[i]; na[i] = s / 2;
                    const double t = b[i] + v2[i]; nb[i] = t / 2;
                    same = same && na[i] == a[i] && nb[i] == b[i];
                }
                ++halvings;
                if (same) { stuck = true; break; }
                memcpy(a, na, sizeof(double) * d); memcpy(b, nb, sizeof(double) * d);
            }
            if (halvings > info->max_halvings) info->max_halvings = halvings;
            next.insert(next.end(), a, a + d);
            next.insert(next.end(), b, b + d);
        }
        if (stuck) { info->status = MPFMT_SHORTCUT_STUCK; break; }
        next.insert(next.end(), path.end() - d, path.end());                     // path[end:end]
        path.swap(next);
        if ((int64_t)(path.size() / d) > info->max_working_len) info->max_working_len = (int64_t)(path.size() / d);
        W.shortcut_fixed_point(path);
        ++info->iterations_done;
    }
    const int64_t n_out = (int64_t)(path.size() / d);
    info->n_out = n_out;
    info->collision_checks = W.checks;
    info->tests_evaluated = W.tests;
    if (n_out > out_cap) return MPFMT_ERR_CAPACITY;
    memcpy(out_P, path.data(), sizeof(double) * path.size());
    cumcost[0] = 0.0;
    for (int64_t i = 1; i < n_out; ++i) {                                        // cumsum([0; map(norm, diff(path))])
        double s = 0.0;
        for (int c = 0; c < d; ++c) { const double t = path[(size_t)i * d + c] - path[(size_t)(i - 1) * d + c]; const double tt = t * t; s = (c == 0) ? tt : s + tt; }
        cumcost[i] = cumcost[i - 1] + std::sqrt(s);
    }
    return MPFMT_OK;
}

// ---- roadmap query for one external pair (s, g) on the host (include/mpfmt.h, "roadmap queries for external states"): the checker of
// mpfmt_roadmap_query (kernels_roadmap.hip, kernels_sssp.hip), bit-equal to it.  Near sets by a scan of all samples, the free-motion test
// above, a binary-heap Dijkstra from the usable seeds, then the parent rule with s as index 0 of label 0.
int32_t mpfmt_host_roadmap_query(int64_t N, int32_t d, const double* X, const int64_t* colptr, const int32_t* rowval, const double* nzval,
                                 const uint64_t* efree, const uint64_t* F, const double* lohi, int32_t M, const double* ss_lo,
                                 const double* ss_hi, double r, const double* s, const double* g, double* cost, int64_t* path, int64_t cap,
                                 mpfmt_roadmap_info* info)
{
    if (!X || !colptr || !efree || !s || !g || !cost || !info || N < 1 || d < 1 || d > MPFMT_MAX_DIM || M < 0 || cap < 0) return MPFMT_ERR_ARG;
    if ((M > 0 && !lohi) || (cap > 0 && !path) || (ss_lo == nullptr) != (ss_hi == nullptr) || !(r >= 0.0) || !std::isfinite(r)) return MPFMT_ERR_ARG;
    if (colptr[0] != 0) return MPFMT_ERR_ARG;
    for (int64_t j = 0; j < N; ++j) if (colptr[j + 1] < colptr[j]) return MPFMT_ERR_ARG;
    const int64_t nnz = colptr[N];
    if (nnz > 0 && (!rowval || !nzval)) return MPFMT_ERR_ARG;
    for (int64_t e = 0; e < nnz; ++e) if (rowval[e] < 0 || rowval[e] >= N || !(nzval[e] >= 0.0)) return MPFMT_ERR_ARG;
    for (int i = 0; i < d; ++i) if (!std::isfinite(s[i]) || !std::isfinite(g[i])) return MPFMT_ERR_ARG;
    auto bitp = [](const uint64_t* m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1ull; };
    ShortcutWorld W{d, lohi, M, ss_lo, ss_hi};
    auto state_free = [&](const double* v) {                                     // is_free_state (statespaces.jl:151-152, boxesND.jl:42-43)
        if (ss_lo) for (int i = 0; i < d; ++i) if (!((ss_lo[i] <= v[i]) && (v[i] <= ss_hi[i]))) return false;
        for (int k = 0; k < M; ++k) {
            const double* lo = lohi + (size_t)k * 2 * d;
            const double* hi = lo + d;
            bool out = false;
            for (int i = 0; i < d; ++i) out = out || !((lo[i] <= v[i]) && (v[i] <= hi[i]));
            if (!out) return false;
        }
        return true;
    };
    auto dist2 = [&](const double* a, const double* b) {
        double s2 = 0.0;
        for (int i = 0; i < d; ++i) { const double t = a[i] - b[i]; const double tt = t * t; s2 = (i == 0) ? tt : s2 + tt; }
        return s2;
    };
    memset(info, 0, sizeof *info);
    *cost = INFINITY;
    const double r2 = r * r;
    // near sets: seeds (tail direction, s -> y) and the goal's entries (head direction, y -> g)
    std::vector<double> seed((size_t)N, INFINITY);
    std::vector<int64_t> gy; std::vector<double> gd;
    for (int64_t y = 0; y < N; ++y) {
        const double* v = X + (size_t)y * d;
        const double ds2 = dist2(s, v);
        if (ds2 <= r2) {
            ++info->near_s;
            if (W.free(s, v) && (!F || bitp(F, y))) { ++info->usable_s; seed[(size_t)y] = 0.0 + std::sqrt(ds2); }
        }
        const double dg2 = dist2(g, v);
        if (dg2 <= r2) {
            ++info->near_g;
            if (W.free(v, g)) { ++info->usable_g; gy.push_back(y); gd.push_back(std::sqrt(dg2)); }
        }
    }
    if (!state_free(s)) { info->status = 2; return MPFMT_OK; }
    if (!state_free(g)) { info->status = 3; return MPFMT_OK; }
    const double dsg2 = dist2(s, g);
    const bool direct = dsg2 <= r2 && W.free(s, g);
    // out-edges of every sample: the usable entries only (free bit set, target allowed by F)
    std::vector<int64_t> rowptr((size_t)N + 1, 0);
    for (int64_t x = 0; x < N; ++x) {
        if (F && !bitp(F, x)) continue;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) if (bitp(efree, b)) rowptr[rowval[b] + 1]++;
    }
    for (int64_t i = 0; i < N; ++i) rowptr[i + 1] += rowptr[i];
    std::vector<int64_t> cur(rowptr.begin(), rowptr.end() - 1);
    std::vector<int32_t> tgt((size_t)std::max<int64_t>(rowptr[N], 1));
    std::vector<double> wgt((size_t)std::max<int64_t>(rowptr[N], 1));
    for (int64_t x = 0; x < N; ++x) {
        if (F && !bitp(F, x)) continue;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b)
            if (bitp(efree, b)) { const int64_t a = cur[rowval[b]]++; tgt[a] = (int32_t)x; wgt[a] = nzval[b]; }
    }
    std::vector<double> C(seed);
    Heap heap;
    for (int64_t y = 0; y < N; ++y) if (C[(size_t)y] < INFINITY) heap.push(y, C[(size_t)y]);
    while (!heap.empty()) {
        const double cy = heap.pri[0];
        const int64_t y = heap.pop();
        if (cy > C[(size_t)y]) continue;
        for (int64_t a = rowptr[y]; a < rowptr[y + 1]; ++a) {
            const int64_t x = tgt[a];
            const double c = cy + wgt[a];
            if (c < C[(size_t)x]) { C[(size_t)x] = c; heap.push(x, c); }
        }
    }
    // the last hop: lowest (fl(C[y] + d(y, g)), C[y], y); the direct edge is (d(s, g), 0, index 0)
    double best = INFINITY, bcy = INFINITY; int64_t by = -1;
    for (size_t k = 0; k < gy.size(); ++k) {
        const int64_t y = gy[k];
        const double cy = C[(size_t)y];
        if (!(cy < INFINITY)) continue;
        const double c = cy + gd[k];
        if (c < best || (c == best && (cy < bcy || (cy == bcy && y < by)))) { best = c; bcy = cy; by = y; }
    }
    if (direct) {
        const double dsg = std::sqrt(dsg2);
        if (by < 0 || dsg <= best) { *cost = dsg; info->status = 0; info->path_len = 0; return MPFMT_OK; }
    }
    if (by < 0) { info->status = 1; return MPFMT_OK; }
    *cost = best;
    std::vector<int64_t> rev;
    int64_t x = by;
    for (;;) {
        rev.push_back(x + 1);
        if ((int64_t)rev.size() > N) break;
        if (seed[(size_t)x] == C[(size_t)x]) break;                              // parent s
        int64_t yb = -1; double cb = 0.0;
        for (int64_t b = colptr[x]; b < colptr[x + 1]; ++b) {
            if (!bitp(efree, b)) continue;
            const int64_t y = rowval[b];
            const double cy = C[(size_t)y];
            if (!(cy + nzval[b] == C[(size_t)x])) continue;
            if (yb < 0 || cy < cb || (cy == cb && y < yb)) { yb = y; cb = cy; }
        }
        if (yb < 0) break;
        x = yb;
    }
    info->path_len = (int64_t)rev.size();
    if ((int64_t)rev.size() > cap) return MPFMT_ERR_CAPACITY;
    for (size_t i = 0; i < rev.size(); ++i) path[i] = rev[rev.size() - 1 - i];
    return MPFMT_OK;
}

// ---- time discretisation of one solution path (include/mpfmt.h, "time discretisation"): steering_control(SS, path...)
// (statespaces.jl:147), duration(::ControlSequence) and propagate(d, v, us, times) (statespaces.jl:104-119) statement for statement --
// the running (v, t0, i) of the reference's loop, not a search.  The CPU baseline and the checker of mpfmt_discretize_batch
// (kernels_discretize.hip), which shares the per-step arithmetic of discretize_core.h with this loop.
namespace {

template <class SP>
int32_t disc_host(const double* prm, const double* P, int64_t n, int32_t mode, double dt, int64_t n_samples, int32_t append_end, double* out_X,
                  double* out_T, int32_t* out_seg, int64_t out_cap, mpfmt_disc_info* info)
{
    constexpr int d = SP::d, nc = SP::nc, maxs = SP::maxs;
    std::vector<double> st, sc;                                          // us: durations, controls
    std::vector<int64_t> sp;                                             // the pair a step came from (0-based)
    for (int64_t i = 0; i + 1 < n; ++i) {                                // vcat([steering_control(SS.dist, V[i], V[i+1]) ...]...)
        double t[maxs], c[maxs * nc];
        const int L = SP::steer(P + i * d, P + (i + 1) * d, prm, t, c);
        for (int q = 0; q < L; ++q) { st.push_back(t[q]); sp.push_back(i); sc.insert(sc.end(), c + q * nc, c + (q + 1) * nc); }
    }
    const int64_t K = (int64_t)st.size();
    double tf = 0.0;
    for (int64_t j = 0; j < K; ++j) tf = tf + st[(size_t)j];             // duration(us)
    info->steps = K; info->duration = tf;
    int64_t n_grid = 0, n_out = 0;
    const bool ok = disc_counts(mode, tf, dt, n_samples, append_end, &n_grid, &n_out);
    info->n_out = n_out;
    if (!ok) return MPFMT_ERR_ARG;
    if (out_cap == 0) return MPFMT_OK;                                   // the size query
    if (n_out > out_cap) return MPFMT_ERR_CAPACITY;
    double v[d], nv[d];
    for (int c = 0; c < d; ++c) v[c] = P[c];
    double t0 = 0.0;
    int64_t i = 0;
    for (int64_t k = 0; k < n_out; ++k) {                                // for t in s
        const double t = disc_time(mode, k, n_grid, tf, dt, n_samples);
        while (t >= t0 + st[(size_t)i] && i < K - 1) {
            const int64_t pr = sp[(size_t)i];
            SP::full(v, P + pr * d, P + (pr + 1) * d, st[(size_t)i], &sc[(size_t)i * nc], nv);
            for (int c = 0; c < d; ++c) v[c] = nv[c];
            t0 = t0 + st[(size_t)i];
            ++i;
        }
        const int64_t pr = sp[(size_t)i];
        const double s = t - t0, ti = st[(size_t)i];
        double* o = out_X + k * d;
        if (s <= 0) { for (int c = 0; c < d; ++c) o[c] = v[c]; }
        else if (s >= ti) SP::full(v, P + pr * d, P + (pr + 1) * d, ti, &sc[(size_t)i * nc], o);
        else SP::part(v, P + pr * d, P + (pr + 1) * d, ti, &sc[(size_t)i * nc], s, o);
        out_T[k] = t;
        if (out_seg) out_seg[k] = (int32_t)(pr + 1);
    }
    return MPFMT_OK;
}

}  // namespace

const char* mpfmt_disc_check(int32_t space, int32_t d, const double* params, int32_t mode, double dt, int64_t n_samples)
{
    if (space == MPFMT_SPACE_EUCLID) { if (d < 1 || d > MPFMT_MAX_DIM) return "d does not fit the Euclidean space"; }
    else if (space == MPFMT_SPACE_DI) { if (d < 2 || d > 12 || (d & 1)) return "the double integrator has d = 2 m, m = 1 .. 6"; }
    else if (space == MPFMT_SPACE_DUBINS || space == MPFMT_SPACE_REEDSSHEPP) { if (d != 3) return "the car spaces have d = 3"; }
    else return "unknown space";
    if (space != MPFMT_SPACE_EUCLID) {
        if (!params) return "params is NULL";
        if (!std::isfinite(params[0]) || !std::isfinite(params[1]) || !(params[0] > 0) || !(params[1] > 0)) return "params must be finite and > 0";
    }
    if (mode == MPFMT_DISC_DT) { if (!std::isfinite(dt) || !(dt > 0)) return "dt must be finite and > 0"; }
    else if (mode == MPFMT_DISC_N) { if (n_samples < 2 || n_samples > 2147483647LL) return "n_samples must lie in [2, 2^31 - 1]"; }
    else return "unknown mode";
    return nullptr;
}

int32_t mpfmt_host_discretize(int32_t space, int32_t d, const double* params, const double* P, int64_t n, int32_t mode, double dt,
                              int64_t n_samples, int32_t append_end, double* out_X, double* out_T, int32_t* out_seg, int64_t out_cap,
                              mpfmt_disc_info* info)
{
    if (!P || !info || out_cap < 0 || (out_cap > 0 && (!out_X || !out_T))) return MPFMT_ERR_ARG;
    if (mpfmt_disc_check(space, d, params, mode, dt, n_samples)) return MPFMT_ERR_ARG;
    if (n < 2) return MPFMT_ERR_ARG;
    for (int64_t i = 0; i < n * d; ++i) if (!std::isfinite(P[i])) return MPFMT_ERR_ARG;
    memset(info, 0, sizeof *info);
#define DISC_GO(SP) return disc_host<SP>(params, P, n, mode, dt, n_samples, append_end, out_X, out_T, out_seg, out_cap, info)
    if (space == MPFMT_SPACE_DUBINS) DISC_GO(disc_car<1>);
    if (space == MPFMT_SPACE_REEDSSHEPP) DISC_GO(disc_car<2>);
    if (space == MPFMT_SPACE_DI) {
        switch (d / 2) {
            case 1: DISC_GO(disc_di<1>); case 2: DISC_GO(disc_di<2>); case 3: DISC_GO(disc_di<3>);
            case 4: DISC_GO(disc_di<4>); case 5: DISC_GO(disc_di<5>); default: DISC_GO(disc_di<6>);
        }
    }
    switch (d) {
        case 1: DISC_GO(disc_euclid<1>); case 2: DISC_GO(disc_euclid<2>); case 3: DISC_GO(disc_euclid<3>); case 4: DISC_GO(disc_euclid<4>);
        case 5: DISC_GO(disc_euclid<5>); case 6: DISC_GO(disc_euclid<6>); case 7: DISC_GO(disc_euclid<7>); case 8: DISC_GO(disc_euclid<8>);
        case 9: DISC_GO(disc_euclid<9>); case 10: DISC_GO(disc_euclid<10>); case 11: DISC_GO(disc_euclid<11>); case 12: DISC_GO(disc_euclid<12>);
        case 13: DISC_GO(disc_euclid<13>); case 14: DISC_GO(disc_euclid<14>); case 15: DISC_GO(disc_euclid<15>); default: DISC_GO(disc_euclid<16>);
    }
#undef DISC_GO
}

// ---- growth of an r-disc graph by appended samples on the host (include/mpfmt.h, "growing the sample set"): the normative statement of
// what mpfmt_samples_add leaves, and its checker.  Near sets by a scan of all samples, the free-motion test above; old entries are kept by
// their stored distance, an entry that sits on the tie (nzval == fl(sqrt(fl(r_new * r_new)))) by its recomputed squared distance.
int32_t mpfmt_host_graph_grow(int64_t N, int64_t n_add, int32_t d, const double* X, const int64_t* colptr, const int32_t* rowval,
                              const double* nzval, const uint64_t* efree, const double* lohi, int32_t M, const double* ss_lo,
                              const double* ss_hi, double r_new, int64_t* out_colptr, int32_t* out_rowval, double* out_nzval,
                              uint64_t* out_efree, int64_t cap, int64_t* nnz_out, mpfmt_grow_info* info)
{
    if (!X || !colptr || !out_colptr || !nnz_out || !info || N < 0 || n_add < 0 || d < 1 || d > MPFMT_MAX_DIM || M < 0 || cap < 0) return MPFMT_ERR_ARG;
    if ((M > 0 && !lohi) || (ss_lo == nullptr) != (ss_hi == nullptr) || !(r_new > 0.0) || !std::isfinite(r_new)) return MPFMT_ERR_ARG;
    if (N + n_add >= ((int64_t)1 << 31) - 64) return MPFMT_ERR_ARG;
    if (cap > 0 && (!out_rowval || !out_nzval || !out_efree)) return MPFMT_ERR_ARG;
    if (colptr[0] != 0) return MPFMT_ERR_ARG;
    for (int64_t j = 0; j < N; ++j) if (colptr[j + 1] < colptr[j]) return MPFMT_ERR_ARG;
    const int64_t nnz = colptr[N];
    if (nnz > 0 && (!rowval || !nzval || !efree)) return MPFMT_ERR_ARG;
    for (int64_t e = 0; e < nnz; ++e) if (rowval[e] < 0 || rowval[e] >= N || !(nzval[e] >= 0.0)) return MPFMT_ERR_ARG;
    const int64_t NN = N + n_add;
    for (int64_t i = 0; i < NN * d; ++i) if (!std::isfinite(X[i])) return MPFMT_ERR_ARG;
    auto bitp = [](const uint64_t* m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1ull; };
    auto dist2 = [&](const double* a, const double* b) {
        double s2 = 0.0;
        for (int i = 0; i < d; ++i) { const double t = a[i] - b[i]; const double tt = t * t; s2 = (i == 0) ? tt : s2 + tt; }
        return s2;
    };
    ShortcutWorld W{d, lohi, M, ss_lo, ss_hi};
    memset(info, 0, sizeof *info);
    const double r2 = r_new * r_new, s = std::sqrt(r2);
    // which old entries stay: a stored distance below the rounded root of r2 is a member, above it is not, on it decides nothing
    auto kept = [&](int64_t x, int64_t e) {
        if (nzval[e] < s) return true;
        if (nzval[e] > s) return false;
        return dist2(X + (size_t)x * d, X + (size_t)rowval[e] * d) <= r2;
    };
    // the near sets of the new samples among ALL samples, ascending, self excluded by index
    struct ent { int32_t y; double d2; };
    std::vector<std::vector<ent>> nn((size_t)n_add);
    std::vector<int64_t> addcnt((size_t)N, 0);
    for (int64_t j = 0; j < n_add; ++j) {
        const int64_t v = N + j;
        const double* q = X + (size_t)v * d;
        for (int64_t y = 0; y < NN; ++y) {
            if (y == v) continue;
            ++info->candidates;
            const double d2 = dist2(q, X + (size_t)y * d);
            if (d2 <= r2) { nn[(size_t)j].push_back({(int32_t)y, d2}); if (y < N) addcnt[(size_t)y]++; }
        }
    }
    out_colptr[0] = 0;
    for (int64_t x = 0; x < NN; ++x) {
        int64_t c;
        if (x < N) {
            c = addcnt[(size_t)x];
            for (int64_t e = colptr[x]; e < colptr[x + 1]; ++e) { if (kept(x, e)) ++c; else ++info->dropped; }
        } else c = (int64_t)nn[(size_t)(x - N)].size();
        out_colptr[x + 1] = out_colptr[x] + c;
    }
    const int64_t nnz_new = out_colptr[NN];
    *nnz_out = nnz_new;
    for (int64_t j = 0; j < n_add; ++j) info->entries += (int64_t)nn[(size_t)j].size();
    for (int64_t x = 0; x < N; ++x) info->entries += addcnt[(size_t)x];
    if (cap == 0) return MPFMT_OK;                                       // the size query
    if (nnz_new > cap) return MPFMT_ERR_CAPACITY;
    for (int64_t w = 0; w < (nnz_new + 63) / 64; ++w) out_efree[w] = 0;
    auto put = [&](int64_t o, int32_t y, double dist, bool fr) {
        out_rowval[o] = y; out_nzval[o] = dist;
        if (fr) out_efree[o >> 6] |= 1ull << (o & 63);
    };
    std::vector<int64_t> cur((size_t)N);
    for (int64_t x = 0; x < N; ++x) {
        int64_t o = out_colptr[x];
        for (int64_t e = colptr[x]; e < colptr[x + 1]; ++e) if (kept(x, e)) put(o++, rowval[e], nzval[e], bitp(efree, e) != 0);
        cur[(size_t)x] = o;
    }
    // new samples in ascending order: the rows appended to an old column ascend
    for (int64_t j = 0; j < n_add; ++j) {
        const int64_t v = N + j;
        const double* q = X + (size_t)v * d;
        int64_t o = out_colptr[v];
        for (const ent& t : nn[(size_t)j]) {
            const double* py = X + (size_t)t.y * d;
            const double dist = std::sqrt(t.d2);
            put(o++, t.y, dist, W.free(py, q));                          // entry (row y, column v): the motion y -> v
            if (t.y < N) put(cur[(size_t)t.y]++, (int32_t)v, dist, W.free(q, py));
        }
    }
    return MPFMT_OK;
}
