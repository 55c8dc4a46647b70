/*
 * mpfmt.h -- C ABI of libmpfmt.so: the MI355X (gfx950) implementation of the FMT* batch-expand
 * hot path of schmrlng/MotionPlanning.jl (r-disc neighbour graph, segment-vs-AABB sweep,
 * per-edge cost, FMT* expansion).
 *
 * The reference has no FFI: its plugin surface is Julia multiple dispatch on the abstract types
 * SampleSet / DistanceDataStructure / CollisionChecker / StateSpace held in the abstract fields of
 * MPProblem (src/problems.jl:12-30).  Each export below names the reference method it stands behind
 * (paths relative to the reference repository); INTEGRATION.md shows the Julia `ccall` glue.
 *
 * Conventions
 *   - every call returns int32 status: 0 = MPFMT_OK, negative = error; mpfmt_last_error(ctx) has text.
 *     No exception crosses the ABI.
 *   - the caller (Julia) owns every host array passed in; the library owns device memory inside ctx.
 *   - sample / edge INDICES ARE 1-BASED Int64 at this ABI (Julia `Int`), like every index the
 *     reference stores (rowval of SparseMatrixCSC, A = parents, path).  colptr is 1-based too.
 *   - samples: const double* X = d x N column-major, i.e. the memory of Vector{SVector{d,Float64}}
 *     (zero-copy view `statevec2mat`, src/primitivetypes.jl:21-24).
 *   - boxes:   const double* lohi = (2*dw) x M column-major: lo(dw) then hi(dw) per box, the memory of
 *     Vector{BoxBounds{dw,Float64}} (src/collisioncheckers/boxesND.jl:5-13).
 *   - bit masks: uint64 words, bit e of word e>>6, LSB first == BitVector.chunks.
 *   - calls are blocking and must come from one host thread per ctx (the reference is single-threaded).
 *   - arithmetic that decides a mask bit is IEEE binary64, unfused, in the reference's written order;
 *     masks and indices are bit-exact against the CPU oracle, costs within 1e-6 relative.
 */
#ifndef MPFMT_H
#define MPFMT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* every export carries default visibility; the library itself is built with -fvisibility=hidden, so nothing else (C++ helpers,
 * kernel launch stubs) is visible to a process that loads it beside other HIP libraries */
#define MPFMT_API __attribute__((visibility("default")))

#define MPFMT_OK              0
#define MPFMT_ERR_ARG        -1   /* bad argument (null pointer, dimension out of range, index out of range) */
#define MPFMT_ERR_STATE      -2   /* call out of order (e.g. fill before count, sweep before boxes) */
#define MPFMT_ERR_HIP        -3   /* HIP runtime error (text in mpfmt_last_error) */
#define MPFMT_ERR_NODEVICE   -4   /* no gfx950 device visible: the library has NO CPU fallback */
#define MPFMT_ERR_CAPACITY   -5   /* caller buffer too small */
#define MPFMT_ERR_INFEASIBLE -6   /* fmtstar: initial state infeasible (src/planners/fmt.jl:24-29) */
#define MPFMT_RETRY            1   /* not an error: mpfmt_allgather_free_mask_finish on a ctx driven inside mpfmt_group_begin / _end -- a shard
                                      outgrew the agreed capacity; call _relaunch for every ctx (in a group), then _finish again */

#define MPFMT_MAX_DIM 16

typedef struct mpfmt_ctx mpfmt_ctx;

/* goal kinds for mpfmt_fmtstar (src/goals.jl): params = [lo(d),hi(d)] | [center(d),radius] | [pt(d)] */
#define MPFMT_GOAL_RECT  0   /* RectangleGoal   src/goals.jl:8-12,96  */
#define MPFMT_GOAL_BALL  1   /* BallGoal        src/goals.jl:17-21,100 */
#define MPFMT_GOAL_POINT 2   /* PointGoal       src/goals.jl:45,111-114 */

/* ---- context ------------------------------------------------------------------------------------- */

/* device = HIP device ordinal (one ctx per GPU; one process per GPU in multi-GPU runs). */
MPFMT_API int32_t mpfmt_ctx_create(int32_t device, mpfmt_ctx** out);
MPFMT_API int32_t mpfmt_ctx_destroy(mpfmt_ctx* ctx);
MPFMT_API const char* mpfmt_last_error(const mpfmt_ctx* ctx);
/* Version string of the library build ("mpfmt <semver> gfx950"). */
MPFMT_API const char* mpfmt_version(void);
/* Launch on a caller-provided hipStream_t (e.g. torch's current stream); NULL = the ctx's own stream. */
MPFMT_API int32_t mpfmt_set_stream(mpfmt_ctx* ctx, void* hip_stream);
/* Multi-GPU: this ctx owns shard `rank` of `world` (contiguous ranges of the library's cell-sorted
 * sample order).  Graph build / sweep then only produce the columns of the shard.  Default (0,1). */
MPFMT_API int32_t mpfmt_set_shard(mpfmt_ctx* ctx, int32_t rank, int32_t world);

/* ---- index build: helper_data_structures(V, dist) (src/nearneighbors.jl:95-100,
 *      src/statespaces/geometric.jl:14) called by MetricNN(V, dist, init) (src/nearneighbors.jl:70-74)
 *      every time addpoints runs (src/sampling.jl:43). --------------------------------------------- */
/* X: d x N column-major host doubles (Julia's Vector{SVector{d,Float64}} as it lies in memory).  One PCIe copy; the set's bounding
 * box and the finiteness check run on the device beside it (one reduction over the uploaded copy -- a host loop over the coordinates
 * would cost more than the copy).  A non-finite coordinate returns MPFMT_ERR_ARG naming the first such sample (1-based) and leaves
 * the ctx as it was -- the sample set it had, its index, graph and capacity hints (the copy lands in a second buffer that changes
 * places with the ctx's only once the set has been accepted). */
MPFMT_API int32_t mpfmt_upload_samples(mpfmt_ctx* ctx, const double* X, int64_t N, int32_t d);
/* The same for a sample set that already lives in HBM of ctx's device (dX = device pointer, same d x N column-major layout): a batch
 * produced on the device -- the library's sampler (mpfmt_sample_free leaves its set in ctx already), a ROCArray -- becomes the
 * SampleSet of the next index build (addpoints, src/nearneighbors.jl:108-109) without crossing PCIe.  One device-to-device copy;
 * the set's bounding box and the finiteness check run on the device.
 * Ordering: dX is read on ctx's stream.  Whatever produced it must be complete on that stream -- hand the producer's stream to
 * mpfmt_set_stream first, or synchronise it before the call.  On return the copy is complete (dX may be reused).
 * A non-finite coordinate returns MPFMT_ERR_ARG and leaves the ctx as it was, as for mpfmt_upload_samples. */
MPFMT_API int32_t mpfmt_upload_samples_device(mpfmt_ctx* ctx, const double* dX, int64_t N, int32_t d);

/* ---- collision checker: PointRobotNDBoxes(boxes) (src/collisioncheckers/boxesND.jl:15-23) and the
 *      BoundedStateSpace bounds used by in_state_space (src/statespaces.jl:29-34,150).
 *      ss_lo/ss_hi: d_state doubles each, or both NULL (no bounds test).
 *      dw = workspace dimension (Identity s2w: dw == d). ------------------------------------------- */
MPFMT_API int32_t mpfmt_upload_boxes(mpfmt_ctx* ctx, const double* lohi, int32_t M, int32_t dw,
                           const double* ss_lo, const double* ss_hi, int32_t d_state);
/* addobstacle / addblocker (boxesND.jl, robots2D.jl:23-24) on the ctx's PointRobotNDBoxes set, in place.  After either call the
 * ctx is what mpfmt_upload_boxes with the resulting list (same dw, same state-space bounds) leaves, except that the free-edge
 * mask of a swept, unsharded resident graph (r-disc, imported or k-nearest) is brought up to date on the ctx's stream instead
 * of being thrown away: adding boxes only clears bits (new = old AND free against the added boxes), removing one only sets
 * bits of blocked entries whose segment box meets it (tested again against what remains).  The mask is the one a whole sweep
 * of the resulting list writes, bit for bit.
 * A resident, swept steering graph (double integrator, Dubins, Reeds-Shepp) of an unsharded ctx follows in place too, mask AND
 * per-entry segment counts (nseg), when dw is what the space's sweep requires (d / 2; 2 for the cars) and the resulting list is
 * one the whole sweep accepts (the double integrator's box limit): with F(list) = (free, nseg) of an entry,
 *   add:    free = old free AND free(added alone), nseg = min(old nseg, nseg(added alone)) -- the count of a blocked entry can drop;
 *   remove: a blocked entry that is not free against the removed boxes alone is evaluated again against what remains (free and
 *           nseg); every other entry keeps both.
 * Mask and counts are byte for byte those of a whole sweep of the resulting list; the graph stays swept ("steer_swept" stays 1)
 * and the next mpfmt_*_fmtstar_wavefront on the same parameters sweeps nothing.  If the update itself fails, the edited list
 * stands and the graph is swept again.
 * In every other state (no swept mask, a sharded ctx, a list beyond the sweep's limit) the list is edited and the mask
 * invalidated, as mpfmt_upload_boxes does.
 *   mpfmt_boxes_add:    lohi [M_add][2][dw] (the ctx's dw), appended behind the current boxes.
 *   mpfmt_boxes_remove: ids 1-based, distinct; the remaining boxes keep their order.
 * Refused, leaving the ctx as it was: NULL with a positive count, an id out of range or repeated (MPFMT_ERR_ARG); no box set
 * uploaded, or the 2-D SAT world (MPFMT_ERR_STATE).  A count of 0 succeeds and does nothing.
 * mpfmt_get_stat: "boxes_delta_path" (1 in place, 0 invalidated), "boxes_delta_columns" (columns whose entries were read),
 * "boxes_delta_entries" (Euclidean graphs: entries that reached an exact test; steering graphs: entries evaluated against the
 * delta boxes), "steer_swept" (1: a swept steering graph is resident); timing keys "boxes_delta" / "steer_delta". */
MPFMT_API int32_t mpfmt_boxes_add(mpfmt_ctx* ctx, const double* lohi, int32_t M_add);
MPFMT_API int32_t mpfmt_boxes_remove(mpfmt_ctx* ctx, const int64_t* ids, int32_t n_ids);
/* The resident, swept steering mask (ceil(nnz / 64) words, bit e = entry e free) and segment counts (nnz bytes; nseg may be NULL)
 * copied to the host as they are -- after in-place edits, what a whole sweep of the current list writes.  Nothing is swept
 * (mpfmt_*_graph_edges_free always sweep again).  nnz: mpfmt_get_stat "nnz".  MPFMT_ERR_STATE when no swept steering graph is
 * resident (mpfmt_get_stat "steer_swept" == 0); MPFMT_ERR_ARG when mask is NULL and nnz > 0. */
MPFMT_API int32_t mpfmt_steer_mask_read(mpfmt_ctx* ctx, uint64_t* mask, uint8_t* nseg);

/* ---- r-disc neighbour graph = ImmutableNNC(D::SparseMatrixCSC, r) (src/nearneighbors.jl:23-27):
 *      column v = inball(V, dist, DS, v, r) (src/nearneighbors.jl:179-183) for every v.
 *      Two-phase so Julia allocates exact sizes:
 *        count: colptr[N+1] (1-based, colptr[1] == 1), *nnz = colptr[N+1]-1
 *        fill : rowval[nnz] (1-based, strictly ascending inside a column, self excluded), nzval[nnz].
 *      With a shard set, only the shard's columns are non-empty. ------------------------------------ */
MPFMT_API int32_t mpfmt_rdisc_count(mpfmt_ctx* ctx, double r, int64_t* colptr, int64_t* nnz);
MPFMT_API int32_t mpfmt_rdisc_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval);

/* One query = inball(V, dist, DS, v, r, forwards) (src/nearneighbors.jl:179-183), the MutableNNC
 * cache-miss path (src/nearneighbors.jl:129-135).  v 1-based.  *k = neighbour count; at most cap
 * entries are written (MPFMT_ERR_CAPACITY if k > cap, *k still set). */
MPFMT_API int32_t mpfmt_rdisc_query(mpfmt_ctx* ctx, int64_t v, double r, int64_t* inds, double* ds, int64_t cap, int64_t* k);

/* ---- batch validity ------------------------------------------------------------------------------
 * points_free: bit e = is_free_state(V[idx[e]], CC, SS) (src/statespaces.jl:151-152,
 *              src/collisioncheckers/boxesND.jl:42-43); idx NULL = all N samples in order
 *              (the checkpts sweep, src/planners/fmt.jl:31-36).
 * edges_free : bit e = is_free_motion(V[src[e]], V[dst[e]], CC, SS) (src/statespaces.jl:153-158,
 *              src/collisioncheckers/boxesND.jl:26,44-56); src = parent first (src/planners/fmt.jl:75).
 * graph_edges_free: the same over every stored graph entry, CSC order: entry e in column x with
 *              row y  <->  is_free_motion(V[y], V[x]).  mask has ceil(nnz/64) words. */
MPFMT_API int32_t mpfmt_points_free(mpfmt_ctx* ctx, const int64_t* idx, int64_t n, uint64_t* mask);
MPFMT_API int32_t mpfmt_edges_free(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, uint64_t* mask);
MPFMT_API int32_t mpfmt_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask);
/* Same three on explicit points (not sample indices): P = d x n column-major; Q likewise (segment ends).
 * is_free_state(v, CC, SS) / is_free_motion(v, w, CC, SS) for states that are not samples
 * (sampler candidates src/sampling.jl:25, shortcut segments src/postprocessors.jl:6-39). */
MPFMT_API int32_t mpfmt_states_free(mpfmt_ctx* ctx, const double* P, int64_t n, uint64_t* mask);
MPFMT_API int32_t mpfmt_motions_free(mpfmt_ctx* ctx, const double* P, const double* Q, int64_t n, uint64_t* mask);
/* is_free_path(p, CC, SS) = @all [is_free_motion(p[i], p[i+1], CC, SS)] (src/statespaces.jl:159-160) for a path of n states
 * P = d x n column-major: *free_out = 1 / 0; seg_mask (may be NULL) gets the n-1 segment bits.  (The reference's box-list
 * method iterates 1:length(BL)-1 instead of the path length, src/collisioncheckers/boxesND.jl:57 -- a bug that is not
 * reproduced: every segment is tested.)  A path of fewer than 2 states is free. */
MPFMT_API int32_t mpfmt_path_free(mpfmt_ctx* ctx, const double* P, int64_t n, int32_t* free_out, uint64_t* seg_mask);

/* ---- Euclidean per-edge steer, src/statespaces/geometric.jl:18-19, batched over E edges src[e] -> dst[e]
 *      (1-based sample indices):
 *        euclid_steer     : steering_control(M::Euclidean, v, w) = StepControl(evaluate(M, v, w), normalize(w - v)):
 *                           t[e] = |w - v| (the graph's edge cost, bit for bit), u[e][d] = unit direction = inv(|w - v|) * (w - v)
 *                           (a zero-length edge gives t = 0 and NaN directions, as in the reference).
 *        euclid_propagate : propagate(M::Euclidean, v, u::StepControl) = v + u.t * u.u from v = V[src[e]]; with s != NULL the
 *                           partial form of src/statespaces.jl:79-81: s[e] <= 0 -> v, s[e] >= t[e] -> full step, else v + s[e] * u.
 *      collision_waypoints(::Euclidean, v, w) = (v, w) (geometric.jl:20) is what mpfmt_edges_free sweeps. */
MPFMT_API int32_t mpfmt_euclid_steer(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, double* t, double* u);
MPFMT_API int32_t mpfmt_euclid_propagate(mpfmt_ctx* ctx, const int64_t* src, int64_t E, const double* t, const double* u, const double* s,
                               double* out);

/* ---- batch expand: the body of the FMT* loop (src/planners/fmt.jl:70-82) for a set of z.
 *      For every unvisited (W) and valid (F, may be NULL) sample x with a forward neighbour in zs:
 *        y_min = first argmin over open (H) backward neighbours y of C[y] + d(y,x)   (fmt.jl:72-74)
 *        free  = is_free_motion(V[y_min], V[x], CC, SS)                              (fmt.jl:75)
 *      Results are reported sorted by x ascending.  W,H,F: N-bit masks; C: N doubles; zs 1-based.
 *      Requires a built graph (mpfmt_rdisc_count).  xs/ymin/cmin/free_out need capacity cap. */
MPFMT_API int32_t mpfmt_expand(mpfmt_ctx* ctx, const uint64_t* W, const uint64_t* H, const uint64_t* F, const double* C,
                     const int64_t* zs, int64_t nz,
                     int64_t* xs, int64_t* ymin, double* cmin, uint8_t* free_out, int64_t cap, int64_t* nx);

/* ---- whole solve: fmtstar!(P, N; r, init_idx, checkpts) with connections = :R
 *      (src/planners/fmt.jl:3-119).  The GPU builds the r-disc graph, the checkpts bitmap and the
 *      per-edge free mask; the sequential dynamic-programming recursion (fmt.jl:68-90) then runs on the
 *      host over those arrays, so tree, costs and path equal the lazy reference loop's.
 *      A (parents, 1-based, 0 = none), C (cost-to-come): N entries.  path: capacity N.
 *      collision_checks counts the edge checks the loop ASKED for (P.CC.count, boxesND.jl:26). */
typedef struct {
    int32_t status;            /* 1 = :solved, 0 = :failed                      (fmt.jl:103) */
    double  cost;              /* C[z]                                          (fmt.jl:107) */
    int64_t z;                 /* last dequeued sample, 1-based */
    int64_t collision_checks;  /* metadata["collision_checks"]                  (fmt.jl:106) */
    int64_t path_len;          /* metadata["path"] length                       (fmt.jl:92-101) */
    int64_t nnz;               /* directed edges in the r-disc graph */
    double  ms_graph;          /* device time: r-disc graph build */
    double  ms_sweep;          /* device time: point + edge validity sweeps */
    double  ms_host_loop;      /* host time: sequential FMT* recursion */
} mpfmt_fmt_result;

MPFMT_API int32_t mpfmt_fmtstar(mpfmt_ctx* ctx, double r, int64_t init_idx, int32_t checkpts,
                      int32_t goal_kind, const double* goal_params,
                      int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);

/* ---- k-nearest connections: fmtstar!(...; connections = :K, k) (src/planners/fmt.jl:6,17-19).  The reference exports the
 *      names mutualknnF! / knnB! (src/nearneighbors.jl:9-11) and defines neither; the semantics here are this library's:
 *      d2(v, i) in the canonical arithmetic of the r-disc graph; k_eff = min(k, N - 1); knn(v) = the k_eff samples i != v
 *      smallest under the total order (d2(v, i), i) -- selection on d2, equal d2 to the lower index.  The graph is a CSC over
 *      ALL samples: column v = knn(v), rows ascending, nzval = sqrt(d2), colptr[v] = 1 + (v - 1) k_eff (1-based like every
 *      other graph).  knnB(x) = column x.  mutualknnF(z) = { x in knn(z) : z in knn(x) }: per entry e (row y in column x) the
 *      mutual bit says x in knn(y), and the forward set of z is the set of columns that hold z with the bit set.
 * knn_count : builds the graph on the device (exact for every sample distribution; candidate rounds at growing radii, the
 *             last one a scan of all samples) and leaves it resident like an r-disc graph; colptr has N + 1 entries.
 * knn_fill  : rowval[nnz], nzval[nnz], mutual[ceil(nnz/64)] (mutual may be NULL).
 * knn_graph_edges_free : bit e = is_free_motion(V[row], V[col]) over the resident k-nearest graph (the sweep of
 *             mpfmt_graph_edges_free).
 * knn_fmtstar : fmt.jl:43-101 with nearF = mutualknnF, nearB = knnB (fmt.jl:17-19): outputs as mpfmt_fmtstar; res->nnz =
 *             N k_eff.  AABB / 2-D SAT checkers on Euclidean samples, unsharded ctx; k < 1 is MPFMT_ERR_ARG.
 * A later mpfmt_fmtstar(r) / mpfmt_graph_step_device(r) on the ctx builds its r-disc graph anew.  The graph occupies the ctx's one
 * graph slot: while it is resident, the accessors that read that slot without a radius (mpfmt_rdisc_fill, mpfmt_graph_edges_free,
 * mpfmt_graph_sweep_device, mpfmt_graph_device_ptrs, mpfmt_graph_export, mpfmt_expand) hand out the k-nearest graph (0-based /
 * 1-based as they document); the knn accessors refuse an r-disc graph (MPFMT_ERR_STATE). */
MPFMT_API int32_t mpfmt_knn_count(mpfmt_ctx* ctx, int64_t k, int64_t* colptr, int64_t* nnz);
MPFMT_API int32_t mpfmt_knn_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval, uint64_t* mutual);
MPFMT_API int32_t mpfmt_knn_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask);
MPFMT_API int32_t mpfmt_knn_fmtstar(mpfmt_ctx* ctx, int64_t k, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                          int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);

/* The sequential part of fmtstar! on its own (src/planners/fmt.jl:43-101): host code, no ctx and no device.  Input is
 * the finished r-disc graph in the device-native format -- colptr[N+1] 0-based offsets, rowval[nnz] 0-based int32 rows
 * (ascending per column), nzval[nnz] distances, efree = one bit per entry (row -> column motion free), F = checkpts
 * bitmap over samples (NULL: checkpts = false), ss_lo/ss_hi = state-space bounds (both NULL: none).  init_idx is 1-based;
 * A / path are 1-based like mpfmt_fmtstar's; res gets status, cost, z, collision_checks, path_len, nnz.
 * mpfmt_fmtstar = graph_build_device + graph_sweep_device + this. */
MPFMT_API int32_t mpfmt_host_fmt_recursion(int64_t N, int32_t d, const double* X, const int64_t* colptr, const int32_t* rowval,
                                 const double* nzval, const uint64_t* efree, const uint64_t* F, const double* ss_lo,
                                 const double* ss_hi, int64_t init_idx, int32_t goal_kind, const double* goal_params,
                                 int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);

/* ---- roadmap queries (PRM*): exact shortest paths over the free-edge graph.  The reference names the graph planner and never
 *      built it (src/problems.jl:57, "# TODO: graph (PRM)"); the semantics here are this library's.
 *      The graph is the ctx's resident graph slot -- r-disc, k-nearest, or a filled and swept steering graph (double integrator,
 *      Dubins, Reeds-Shepp: the same device slots and the same direction convention) -- in the device-native CSC: entry b of column x with row y
 *      is the DIRECTED edge y -> x of weight nzval[b]; its free bit is mask bit b = is_free_motion(V[y], V[x]) (the reading of
 *      mpfmt_host_fmt_recursion).  An edge is USABLE iff its bit is set and, with checkpts != 0, the point bit F[x] of its target is
 *      set (fmt.jl:71); the source itself is exempt from F.
 *      Costs for a source s: C[s] = 0; C[x] = the least value of the left-to-right fp64 fold (((0 + w1) + w2) + ...) over all usable
 *      paths s -> x; C[x] = +Inf when there is none (FMT* writes 0 for unvisited samples; these calls do not).  fl(a + w) is
 *      nondecreasing in a and w >= 0, so Dijkstra and any chaotic relaxation started from +Inf reach the same least fixed point of
 *      C[x] = min_y fl(C[y] + w_yx): the values are unique, independent of scheduling, and bit-identical between
 *      mpfmt_graph_sssp and mpfmt_host_graph_sssp (DESIGN.md "PRM* roadmap queries" has the argument and what it asks of the device).
 *      Parents: A[x] (1-based; 0 for the source and for unreached samples) = the usable y of lowest (C[y], y) among those with
 *      fl(C[y] + w_yx) == C[x], found by a final pass over the finished C -- never during relaxation -- so fl(C[A[x]] + w) == C[x]
 *      holds exactly.  Following A from a reached x arrives at s in fewer than N hops whenever every reached x != s has such a y
 *      with C[y] < C[x] (always, unless a whole group of equal-cost samples hangs together by zero-length or absorbed edges only).
 * mpfmt_host_graph_sssp : a binary-heap Dijkstra on the host over the device-native arrays (colptr[N+1] 0-based offsets, rowval
 *      0-based int32, efree one bit per entry, F the point bitmap or NULL for checkpts = false; source 1-based; A may be NULL).
 *      No ctx, no device.  MPFMT_ERR_ARG on malformed arrays (colptr[0] != 0, decreasing colptr, a row out of range, a negative or
 *      NaN weight).
 * mpfmt_graph_sssp : the same field on the device for nsrc sources (1-based), one after another (mpfmt_graph_sssp_multi below runs 64 per
 *      pass), over the resident graph and mask
 *      WITHOUT copying or transposing them.  C / A are nsrc x N, source-major (A may be NULL); info[nsrc] (may be NULL).
 *      checkpts != 0 sweeps the point bitmap on the device first (on a steering ctx: the bitmap of the steering planners,
 *      is_free_state = the state-space bounds on all d coordinates and the point test on the first dw).  MPFMT_ERR_STATE: no
 *      resident r-disc / k-nearest / steering graph, no mask
 *      for the current graph and obstacle set (a mask goes stale with mpfmt_upload_boxes / mpfmt_upload_shapes2d /
 *      mpfmt_set_state_bounds: sweep again -- this call never sweeps edges on its own), or a sharded ctx; MPFMT_ERR_ARG: a source
 *      out of range.  A refused call leaves the ctx as it was.  A steering mask stays valid across mpfmt_boxes_add / _remove (they
 *      bring it up to date in place) and goes stale like the Euclidean one.
 * mpfmt_prmstar / mpfmt_knn_prmstar : the planner: mpfmt_graph_step_device(r) (k-nearest: the build + sweep of mpfmt_knn_fmtstar)
 *      -- graph and mask are reused when they are resident for this r (k) and obstacle set, a stale mask is swept again --, the
 *      checkpts sweep, the field from init_idx and goal extraction: the goal node is the reached sample inside the goal region of
 *      lowest (C, index).  A, C (N entries, C = +Inf for unreached) and path as mpfmt_fmtstar; res->status / cost / z / path_len /
 *      nnz mean what they mean there (no goal sample reached: status 0, z = init_idx, cost = +Inf, path = (init_idx));
 *      res->ms_host_loop = the field and the extraction.  res->collision_checks = 0: the planner consults a mask that the step
 *      swept whole, it asks for no lazy edge test of its own (there is no counterpart of P.CC.count, boxesND.jl:26).
 *      An infeasible init is MPFMT_ERR_INFEASIBLE as in mpfmt_fmtstar.  Euclidean samples, unsharded ctx.
 *      Timers: "sssp_relax" (all rounds of one source), "sssp_parents"; stats "sssp_rounds", "sssp_relaxations", "sssp_reached"
 *      (last source). */
typedef struct {
    int64_t reached;           /* samples with C < +Inf, the source included */
    int64_t rounds;            /* relaxation rounds that ran (the last one changes nothing) */
    int64_t relaxations;       /* fl(C[y] + w) evaluated, all rounds; scheduling-dependent, unlike C and A */
    double  ms_device;         /* device time of the source: init, rounds, parent pass */
} mpfmt_sssp_info;
MPFMT_API int32_t mpfmt_host_graph_sssp(int64_t N, const int64_t* colptr, const int32_t* rowval, const double* nzval, const uint64_t* efree,
                              const uint64_t* F, int64_t source, double* C, int64_t* A);
MPFMT_API int32_t mpfmt_graph_sssp(mpfmt_ctx* ctx, const int64_t* sources, int64_t nsrc, int32_t checkpts, double* C, int64_t* A,
                         mpfmt_sssp_info* info);
MPFMT_API int32_t mpfmt_prmstar(mpfmt_ctx* ctx, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                      int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);
MPFMT_API int32_t mpfmt_knn_prmstar(mpfmt_ctx* ctx, int64_t k, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                          int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);

/* ---- cost-to-go: the field of a target set, and the PRM* planners of the steering spaces.
 *      Notation of the roadmap queries above: entry b of column x with row y is the DIRECTED edge y -> x of weight w_yx = nzval[b].
 *      It is USABLE iff mask bit b is set and, with checkpts, F[x] is set.  There is no exemption: a target t with F[t] clear keeps
 *      G[t] = 0 and simply has no usable edge into it.
 *      Costs for a target set T (1-based, duplicates allowed; ntgt = 0 is legal: all +Inf, reached = 0): G[t] = 0 for every t in T,
 *      whatever F[t] is; otherwise G[y] = the least value of fl(G[x] + w_yx) over usable edges, i.e. the least fixed point of
 *      G[y] = min(G0[y], min_x fl(G[x] + w_yx)); +Inf when no target is reachable from y.  This is the fold of a path from the
 *      target BACKWARDS, (((0 + w_last) + ...) + w_first): it is NOT bit-equal to the forward fold of the same path that
 *      mpfmt_graph_sssp computes, and on a quasi-metric graph (double integrator, Dubins, k-nearest) the two fields differ by more
 *      than rounding.  fl(a + w) is nondecreasing in a and >= a, so any relaxation order that runs until nothing changes gives the
 *      bits of Dijkstra on the reversed graph: mpfmt_graph_sssp_to and mpfmt_host_graph_sssp_to agree bit for bit, no tolerance.
 *      Successors: S[y] (1-based; 0 for targets and for unreached samples) = the usable x of lowest (G[x], x) among those with
 *      fl(G[x] + w_yx) == G[y]: a function of the finished G alone.  S may be NULL.  Following S from a reached y arrives at a
 *      target in fewer than N hops under the condition stated for the parents above.
 * mpfmt_host_graph_sssp_to : a binary-heap Dijkstra over the reversed edges on the host (the arrays and the argument checks of
 *      mpfmt_host_graph_sssp, plus MPFMT_ERR_ARG for a target out of range or ntgt < 0).  No ctx, no device.
 * mpfmt_graph_sssp_to : the same field on the device over whatever swept graph is resident (r-disc, k-nearest, steering), read in
 *      place: a push along the entries of the columns whose label changed, 64-bit atomic minima on the labels, rounds as separate
 *      launches.  info (may be NULL) has the fields of mpfmt_sssp_info: reached counts G < +Inf, targets included; relaxations
 *      counts fl(G[x] + w) evaluated.  The refusals of mpfmt_graph_sssp (MPFMT_ERR_ARG: a target out of range); a refused call
 *      leaves the ctx as it was.  It shares the buffers of mpfmt_graph_sssp (the parent buffer only when S is asked for) and adds 8 N bytes of its own, with S only.
 *      Timers: "sssp_to_push" (all rounds), "sssp_to_successors"; stats "sssp_rounds", "sssp_relaxations", "sssp_reached", and
 *      "sssp_to_columns" / "sssp_to_entries_read" (columns walked and their entries, all rounds: a round reads only the columns of
 *      samples that changed), "sssp_to_atomics" (atomic minima issued).
 * mpfmt_di_prmstar / mpfmt_dubins_prmstar / mpfmt_reedsshepp_prmstar : mpfmt_prmstar in the steering spaces: the prelude of the
 *      steering FMT* planners (MPFMT_ERR_INFEASIBLE for a blocked init), the graph of the space -- a resident graph of the same
 *      space and parameters is reused, and its sweep while it is valid, which includes after mpfmt_boxes_add / _remove --, the
 *      cost-to-come field from init_idx and the goal extraction of mpfmt_prmstar: the reached sample in the region of lowest
 *      (C, index).  The goal predicate is that of the steering FMT* planners: POINT = the exact state, RECT / BALL on the first dw
 *      coordinates.  res as in mpfmt_prmstar; collision_checks = 0.
 * Tracked fields (mpfmt_field_*) and the Euclidean calls on external states (mpfmt_roadmap_*) stay refused on a steering graph:
 *      MPFMT_ERR_STATE, "Euclidean graphs only".  External states on a steering graph have entry points of their own:
 *      mpfmt_steer_roadmap_* ("roadmap queries for external states, steering spaces", below). */
MPFMT_API int32_t mpfmt_host_graph_sssp_to(int64_t N, const int64_t* colptr, const int32_t* rowval, const double* nzval,
                                           const uint64_t* efree, const uint64_t* F, const int64_t* targets, int64_t ntgt,
                                           double* G, int64_t* S);
MPFMT_API int32_t mpfmt_graph_sssp_to(mpfmt_ctx* ctx, const int64_t* targets, int64_t ntgt, int32_t checkpts,
                                      double* G, int64_t* S, mpfmt_sssp_info* info);
MPFMT_API int32_t mpfmt_di_prmstar(mpfmt_ctx* ctx, double rho, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind,
                                   const double* goal_params, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);
MPFMT_API int32_t mpfmt_dubins_prmstar(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                                       int32_t goal_kind, const double* goal_params, int64_t* A, double* C, int64_t* path,
                                       mpfmt_fmt_result* res);
MPFMT_API int32_t mpfmt_reedsshepp_prmstar(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                                           int32_t goal_kind, const double* goal_params, int64_t* A, double* C, int64_t* path,
                                           mpfmt_fmt_result* res);

/* ---- a cost-to-come field kept valid across box edits: repair, not recompute (DESIGN.md "a tracked field").
 *      Notation of the roadmap queries above: entry b of column x with row y is the edge y -> x; it is usable iff mask bit b is set
 *      and, with checkpts, F[x] is set; the source is exempt from F; C* is the least fixed point of C[x] = min_y fl(C[y] + w_yx)
 *      with C[s] = 0.
 *      A TRACKED FIELD is (s, checkpts, C, A, Ab), held in buffers of its own that no other call writes: C and A are exactly what
 *      mpfmt_graph_sssp returns for s; Ab[x] is the entry index b of the parent edge A[x] -> x (undefined for the source and for
 *      unreached samples).
 *      The REPAIR runs after any sequence of in-place edits (mpfmt_boxes_add / _remove, mpfmt_shapes2d_add / _remove, mixed):
 *        1. F is recomputed when checkpts is set.
 *        2. Invalidate.  I0 = the x != s with C[x] < Inf for which mask bit Ab[x] is now clear, or checkpts is set and F[x] is clear.
 *           I = I0 plus every descendant of I0 in the parent forest A; C[x] = +Inf on I.  I is exactly this closure.
 *        3. Relax to a fixed point with C[x] <- min(C[x], fl(C[y] + w)) over usable entries.  Round 0 lets every column of I u D look
 *           at all its usable rows with finite labels (D = the dirty columns: those the delta kernels flagged since the field was
 *           last valid); later rounds are driven by which labels changed.
 *        4. Parents by the rule of the roadmap queries (lowest (C[y], y) among achievers), a function of the final C alone; Ab is
 *           refreshed.
 *      The result is bit-identical to a fresh field over the edited mask (DESIGN.md has the argument).
 * mpfmt_field_begin  : computes the field of `source` (1-based) over the resident swept graph into the tracked buffers.  The refusals of
 *      mpfmt_graph_sssp; a refused call leaves an earlier tracked field as it was.
 * mpfmt_field_update : the repair.  A field that lost its delta history while a swept mask exists (a box edit took the fall-back of
 *      mpfmt_boxes_add and the mask was swept whole since) is recomputed in full: info->path = 0.  No swept mask for the current graph
 *      and box set: MPFMT_ERR_STATE.  With nothing dirty it returns at once with zero rounds.
 * mpfmt_field_read   : host copies of C[N] and A[N]; either pointer may be NULL.
 * mpfmt_field_goal   : the goal extraction and walk-back of mpfmt_prmstar on the tracked field: the same res fields (status, cost, z,
 *      path_len, nnz), collision_checks = 0; path has capacity N.  While box edits are pending (no mpfmt_field_update since) the
 *      field is that of the previous box set: MPFMT_ERR_STATE (mpfmt_field_read hands out the field as it was last valid).
 * mpfmt_field_drop   : forgets the field (always succeeds).
 * The field is dropped by new samples (mpfmt_samples_add carries it across an in-place growth once the ctx's option
 * "samples_add_keeps_fields" is 1: "growing the sample set" below), a new graph (another r or k, an import), mpfmt_upload_boxes, mpfmt_upload_shapes2d,
 * mpfmt_set_state_bounds, mpfmt_set_shard and by destroying the ctx; mpfmt_field_update / _read / _goal then return MPFMT_ERR_STATE
 * until mpfmt_field_begin.  mpfmt_graph_sssp, mpfmt_prmstar and the roadmap queries keep scratch buffers of their own and leave it alone.
 * Unsharded ctx, Euclidean samples; the in-place edits are those of the AABB checker (mpfmt_boxes_add / _remove) and of the 2-D SAT
 * world (mpfmt_shapes2d_add / _remove, which flag their columns for the repair in the same way).
 * mpfmt_get_stat: "field_tracked", "field_update_path" (1 repaired, 0 recomputed), "field_invalidated" (|I|), "field_dirty_columns"
 * (|D|), "field_columns_read" (distinct columns whose entries the relaxation read, over all rounds), "field_column_visits" (the same
 * counted once per round), "field_entries_read", "field_rounds", "field_relaxations", "field_reached".
 * Timers: "field_invalidate", "field_relax", "field_parents".
 * mpfmt_host_field_repair : steps 2-4 on the host over the device-native arrays (as mpfmt_host_graph_sssp), no ctx and no device:
 *      C / A hold the old field on entry and the repaired one on return; efree / F are the NEW mask and point bitmap (F NULL:
 *      checkpts = false), dirty the bitmap of D over samples; *invalidated receives |I| (may be NULL).  It returns what
 *      mpfmt_host_graph_sssp returns on the new mask. */
typedef struct {
    int64_t reached;           /* samples with C < +Inf, the source included */
    int64_t invalidated;       /* |I| */
    int64_t dirty_columns;     /* |D| */
    int64_t columns_read;      /* distinct columns whose entries the relaxation read */
    int64_t column_visits;     /* columns read, counted once per round */
    int64_t entries_read;      /* entries of the columns read, counted once per round (rowval + nzval: 12 bytes each) */
    int64_t rounds;            /* relaxation rounds that ran */
    int64_t relaxations;       /* fl(C[y] + w) evaluated; scheduling-dependent */
    double  ms_device;         /* device time of the call */
    int32_t path;              /* 1 repaired, 0 computed in full */
    int32_t pad_;
} mpfmt_field_info;
MPFMT_API int32_t mpfmt_field_begin(mpfmt_ctx* ctx, int64_t source, int32_t checkpts, mpfmt_field_info* info);
MPFMT_API int32_t mpfmt_field_update(mpfmt_ctx* ctx, mpfmt_field_info* info);
MPFMT_API int32_t mpfmt_field_read(mpfmt_ctx* ctx, double* C, int64_t* A);
MPFMT_API int32_t mpfmt_field_goal(mpfmt_ctx* ctx, int32_t goal_kind, const double* goal_params, int64_t* path, mpfmt_fmt_result* res);
MPFMT_API int32_t mpfmt_field_drop(mpfmt_ctx* ctx);
MPFMT_API int32_t mpfmt_host_field_repair(int64_t N, const int64_t* colptr, const int32_t* rowval, const double* nzval, const uint64_t* efree,
                                const uint64_t* F, const uint64_t* dirty, int64_t source, double* C, int64_t* A, int64_t* invalidated);

/* ---- a cost-to-go field kept valid across box edits, on any resident swept graph.
 *      Notation of the cost-to-go above: entry b of column x with row y is the edge y -> x; it is usable iff mask bit b is set and,
 *      with checkpts, F[x] is set; G = 0 on the targets whatever their F; G* is the least fixed point; S[y] = the usable x of lowest
 *      (G[x], x) among those with fl(G[x] + w_yx) == G[y].
 *      A TRACKED COST-TO-GO FIELD is (targets, checkpts, G, S), held in buffers of its own that no other call writes: G and S are
 *      exactly what mpfmt_graph_sssp_to returns for the targets.  It is admitted wherever mpfmt_graph_sssp_to is: r-disc, imported,
 *      k-nearest, double integrator, Dubins, Reeds-Shepp; unsharded ctx; under the AABB checker or, on the Euclidean graphs, the 2-D
 *      SAT world.
 *      The REPAIR runs after any sequence of in-place edits (mpfmt_boxes_add / _remove, mpfmt_shapes2d_add / _remove, mixed):
 *        1. F is recomputed when checkpts is set (on a steering graph: the bitmap of the steering planners).
 *        2. Invalidate.  I0 = the non-target y with G[y] < Inf whose successor edge y -> S[y] is no longer usable: its mask bit is now
 *           clear, or checkpts is set and F[S[y]] is clear.  I = I0 plus every y whose successor chain passes through I0; G = +Inf on
 *           I.  (Only a y whose S[y] is a flagged column or has lost its point bit is looked at for this; the entry of the edge is
 *           found by binary search of y in the ascending column S[y].)
 *           I0 also takes every non-target y with G[y] < Inf whose successor chain S[y], S[S[y]], ... stays at the label of y for
 *           MPFMT_TOGO_EQUAL_HOPS = 64 hops without arriving at a target.  Where a group of equal-cost samples hangs together by
 *           zero-length or absorbed edges only (the case excluded above for walks along S) the successors may run in a circle, and
 *           no chain then shows what supports the group's labels; such a y loses its label at every repair that runs and gets it
 *           back from the push.  A chain of more than 64 legitimate equal-label hops is treated the same way: more work, same result.
 *           I is exactly the closure of this I0, and "togo_invalidated" reports |I|: it counts these samples too.
 *        3. Seed.  The pushers of round 0 are a set P0 with
 *             P0 >= {x : G[x] < Inf, (no checkpts or F[x]), x in D or column x has a row in I}  and  P0 <= D u Nout(I),
 *           D = the columns the delta kernels flagged since the field was last valid, Nout(I) = the columns holding an entry whose
 *           row is in I, usable or not.  On the library's own r-disc graph (rows of a column = its out-neighbours) the finite rows of
 *           the columns of I are marked ("togo_seed_form" 0); on every other graph each finite, unmarked column scans its rows
 *           against the bitmap of I (form 1: one pass over rowval).
 *        4. Push.  The rounds of mpfmt_graph_sssp_to from P0 to a fixed point: fl(G[x] + w) offered to the rows of the columns whose
 *           label changed, a plain load then a 64-bit atomic minimum on the label bits, F applied to the pushing x.
 *        5. Successors from the final G alone, by the rule above: two whole passes over the reached columns.
 *      With D and I both empty nothing runs: no rounds, no successor pass, the same bytes.
 *      The result is byte-identical to a fresh mpfmt_graph_sssp_to over the edited mask (DESIGN.md 7j has the argument).
 * mpfmt_togo_begin  : computes the field of the target set (1-based, duplicates allowed, ntgt = 0 legal) into the tracked buffers.
 *      The refusals of mpfmt_graph_sssp_to; a refused call leaves an earlier tracked field as it was.  info->path = 0.
 * mpfmt_togo_update : the repair, info->path = 1.  The delta history is valid while no graph build and no whole sweep (Euclidean or
 *      steering) has happened since the field was last valid; otherwise, with a swept mask resident, the field is recomputed in full:
 *      info->path = 0.  No swept mask for the resident graph and the current box set: MPFMT_ERR_STATE, the field stays tracked.
 * mpfmt_togo_read   : host copies of G[N] and S[N] (S may be NULL, and so may G): the field as it was last valid.
 * mpfmt_togo_drop   : forgets the field (always succeeds).
 * mpfmt_togo_targets_add : 1-based targets join the tracked set (duplicates and old targets allowed, ntgt = 0 legal and does
 *      nothing).  Each is a label decrease: target bit, G = 0, S = 0, and the sample joins D, so it pushes in round 0 of the next
 *      repair; the field's target list is extended (a recomputation, path = 0, starts from it).  Legal while box edits or a carried
 *      growth are pending; the next mpfmt_togo_update yields the bytes of mpfmt_graph_sssp_to for the union of the targets.  An index
 *      outside 1 .. N: MPFMT_ERR_ARG; no tracked field: MPFMT_ERR_STATE; a refusal leaves the field untouched.
 * The field is dropped by new samples (mpfmt_samples_add carries it across an in-place growth of an r-disc graph once the ctx's option
 * "samples_add_keeps_fields" is 1: "growing the sample set" below), another graph (another radius, k, steering space or steering parameters; an import),
 * mpfmt_upload_shapes2d, mpfmt_set_state_bounds, mpfmt_set_shard and by destroying the ctx: mpfmt_togo_update / _read then return
 * MPFMT_ERR_STATE until mpfmt_togo_begin.  mpfmt_upload_boxes replaces the list whole: the labels lose their history but the targets
 * stay, and after the whole sweep that such an upload needs mpfmt_togo_update recomputes (path = 0).  mpfmt_field_*,
 * mpfmt_graph_sssp, mpfmt_graph_sssp_to and the roadmap queries keep buffers of their own and leave it alone; it and the tracked
 * cost-to-come field may be live at once, each with its own dirty bitmap.
 * mpfmt_get_stat: "togo_tracked", "togo_path" (1 repaired, 0 computed in full), "togo_seed_form", "togo_reached",
 * "togo_invalidated" (|I|), "togo_dirty_columns" (|D|), "togo_columns_read" (distinct columns whose entries the push read, all
 * rounds), "togo_column_visits" (the same counted once per round), "togo_entries_read", "togo_rounds", "togo_relaxations",
 * "togo_atomics".  Timers: "togo_invalidate", "togo_seed", "togo_push", "togo_successors". */
#define MPFMT_TOGO_EQUAL_HOPS 64
typedef struct {
    int64_t reached;           /* samples with G < +Inf, the targets included */
    int64_t invalidated;       /* |I| */
    int64_t dirty_columns;     /* |D| */
    int64_t columns_read;      /* distinct columns whose entries the push read */
    int64_t column_visits;     /* columns read, counted once per round */
    int64_t entries_read;      /* entries of the columns read, counted once per round */
    int64_t rounds;            /* push rounds that ran */
    int64_t relaxations;       /* fl(G[x] + w) evaluated; scheduling-dependent */
    int64_t atomics;           /* atomic minima issued; scheduling-dependent */
    double  ms_device;         /* device time of the call */
    int32_t path;              /* 1 repaired, 0 computed in full */
    int32_t pad_;
} mpfmt_togo_info;
MPFMT_API int32_t mpfmt_togo_begin(mpfmt_ctx* ctx, const int64_t* targets, int64_t ntgt, int32_t checkpts, mpfmt_togo_info* info);
MPFMT_API int32_t mpfmt_togo_update(mpfmt_ctx* ctx, mpfmt_togo_info* info);
MPFMT_API int32_t mpfmt_togo_read(mpfmt_ctx* ctx, double* G, int64_t* S);
MPFMT_API int32_t mpfmt_togo_targets_add(mpfmt_ctx* ctx, const int64_t* targets, int64_t ntgt);
MPFMT_API int32_t mpfmt_togo_drop(mpfmt_ctx* ctx);

/* ---- roadmap queries for external states: start and goal states that are NOT samples (the robot's present pose, a batch of candidate
 *      goals) are attached to the resident roadmap instead of being appended to the sample set (which would rebuild graph and mask).
 *      The ctx holds an unsharded, swept r-disc graph of radius r = its graph radius (built or imported); the checker is the N-D AABB
 *      checker in the state space's own coordinates (identity workspace).  For an external state q (d finite doubles):
 *        near(q) = the samples y with d2(q, y) <= r * r, d2 = the left-to-right unfused fp64 fold of squared differences (the membership
 *                  test of mpfmt_rdisc_query, same arithmetic), distance = sqrt(d2) (the graph costs' canon); indices ascend.  A q that is
 *                  bit-equal to sample v gets column v of the resident graph plus v itself at distance 0.
 *        tail direction (q -> y): the free bit is what mpfmt_motions_free returns for (P = q, Q = V[y]), first-point bounds test included;
 *        head direction (y -> q): the free bit is what mpfmt_motions_free returns for (P = V[y], Q = q).
 *      A pair query (s, g) is the PRM* field of the section above on the graph augmented by two nodes:
 *        edges s -> y, y in near(s), usable iff free and, with checkpts != 0, F[y] set; edges y -> g, y in near(g), usable iff free;
 *        the direct edge s -> g exists iff d2(s, g) <= r * r and free(s, g);
 *        C = the least fixed point of C[x] = min(seed[x], min_y fl(C[y] + w_yx)), seed[y] = fl(0 + d(s, y)) on usable seeds, +Inf elsewhere
 *        (seeds are further upper bounds only: the uniqueness argument above carries over, host and device results are bit-identical and
 *        independent of scheduling; DESIGN.md "Roadmap queries for external states");
 *        cost = min(d(s, g) if direct, min_y fl(C[y] + d(y, g)) over usable y), +Inf when there is none.
 *      Path: s counts as index 0 with C = 0 in the parent rule above (lowest (C[y], y) with fl(C[y] + w) == C[x]): a sample whose seed
 *        equals its label has parent s; the last hop to g follows the same rule, the direct edge wins when d(s, g) == cost.  The result
 *        is the list of 1-based sample indices between s and g (empty when the edge is direct).
 *      Per-query status is a field, not an error: 0 solved, 1 no usable path, 2 s is not a free state, 3 g is not a free state
 *        (mpfmt_states_free semantics; s is looked at first).  Statuses 1-3 give cost = +Inf and an empty path.  near_s / usable_s /
 *        near_g / usable_g (sizes of the near sets and their usable parts) are filled for every status.
 * mpfmt_roadmap_near : the list form for nq states Q (d x nq column-major); direction 0 = tail, 1 = head.  CSR: ptr[nq + 1] 0-based
 *      offsets (always written), idx 1-based ascending, dist, free_mask bit e = free bit of entry e (ceil(cap / 64) words), *total = ptr[nq].
 *      *total > cap: MPFMT_ERR_CAPACITY with *total and ptr written, like mpfmt_closeR.  cap == 0 is the size query: only the count pass runs.
 *      The lists are put in index order by a counting rank, quadratic in a list's length: meant for roadmap radii (lists up to about a
 *      thousand entries), not for an r that spans a sizeable part of the sample cloud.
 * mpfmt_roadmap_attach : the reduce form over a host field C[N] (e.g. a row of mpfmt_graph_sssp): per state the head-direction minimum
 *      cost[q] = min over free y in near(q) with C[y] < +Inf of fl(C[y] + d(y, q)), parent[q] = that y of lowest (C[y], y), 1-based; none:
 *      parent 0, cost +Inf.  No list is stored: one field, many goals.
 * mpfmt_roadmap_query : nq pairs S / G (d x nq).  cost[nq]; path_ptr[nq + 1] 0-based offsets into path (1-based samples, room for
 *      path_cap; beyond it: MPFMT_ERR_CAPACITY with cost, info and path_ptr written); info[nq] (may be NULL).  All 2 nq attachments run in one
 *      launch each way, the seeded fields one after another.  info.rounds and ms_device depend on scheduling, nothing else does.
 * mpfmt_host_roadmap_query : one pair on the host over the device-native arrays (as mpfmt_host_graph_sssp; X d x N, lohi (2 d) x M,
 *      ss_lo / ss_hi or both NULL, F NULL: checkpts = false): all samples scanned for the near sets, the free-motion test of
 *      mpfmt_host_adaptive_shortcut, a binary-heap Dijkstra with seeds.  No ctx, no device.  path has room for cap indices
 *      (MPFMT_ERR_CAPACITY with info written otherwise).
 * Refusals leave the ctx as it was.  MPFMT_ERR_STATE: no resident r-disc graph, a k-nearest graph in the slot, a stale or missing mask, a
 *      sharded ctx, the 2-D SAT world, a non-identity workspace; MPFMT_ERR_ARG: NULL arrays, a non-finite query coordinate.  nq == 0
 *      succeeds and does nothing.  Timers "roadmap_near", "roadmap_attach"; stats "roadmap_candidates" (distances evaluated by the last
 *      call), "roadmap_near_total" (near-set entries it found).
 * Out of scope: k-nearest graphs (an external state has no radius there), the SAT world, sharded contexts, and repairing
 *      a field after mpfmt_boxes_add / _remove (the mask stays current: ask again).  A resident steering graph is refused here and
 *      served by mpfmt_steer_roadmap_* (after the cost matrices below). */
typedef struct {
    int32_t status;            /* 0 solved, 1 no usable path, 2 s not a free state, 3 g not a free state */
    int32_t pad_;
    int64_t near_s, usable_s;
    int64_t near_g, usable_g;
    int64_t rounds;            /* relaxation rounds of the seeded field (0 on the host) */
    int64_t path_len;          /* samples between s and g */
    double  ms_device;
} mpfmt_roadmap_info;
MPFMT_API int32_t mpfmt_roadmap_near(mpfmt_ctx* ctx, const double* Q, int64_t nq, int32_t direction, int64_t* ptr, int64_t cap, int64_t* idx,
                           double* dist, uint64_t* free_mask, int64_t* total);
MPFMT_API int32_t mpfmt_roadmap_attach(mpfmt_ctx* ctx, const double* Q, int64_t nq, const double* C, int64_t* parent, double* cost);
MPFMT_API int32_t mpfmt_roadmap_query(mpfmt_ctx* ctx, const double* S, const double* G, int64_t nq, int32_t checkpts, double* cost,
                            int64_t* path_ptr, int64_t* path, int64_t path_cap, mpfmt_roadmap_info* info);
MPFMT_API int32_t mpfmt_host_roadmap_query(int64_t N, int32_t d, const double* X, const int64_t* colptr, const int32_t* rowval, const double* nzval,
                                 const uint64_t* efree, const uint64_t* F, const double* lohi, int32_t M, const double* ss_lo,
                                 const double* ss_hi, double r, const double* s, const double* g, double* cost, int64_t* path, int64_t cap,
                                 mpfmt_roadmap_info* info);

/* ---- growing the sample set of a resident roadmap: addpoints (src/nearneighbors.jl:108) behind fmtstar!(P, N)'s incremental sampling
 *      (src/planners/fmt.jl:30, src/sampling.jl:43) without the rebuild (DESIGN.md "Growing the sample set").
 * mpfmt_samples_add : X_add d x n_add column-major host doubles (the ctx's d), appended behind the ctx's samples: new sample j becomes
 *      index N + j (1-based N + 1 ... N + n_add).  mpfmt_samples_add_device: the same for a batch in HBM of the ctx's device, read on
 *      the ctx's stream (ordering as for mpfmt_upload_samples_device).
 *      IN PLACE when the ctx is unsharded, uses the N-D AABB checker with an identity workspace (dw == d), holds a resident r-disc graph
 *      (built or imported) whose mask is swept and current, and 0 < r_new <= the graph's radius (its own radius keeps it).  After the
 *      call the ctx holds N + n_add samples, and colptr / rowval / nzval / the free mask (padding bits of the last word included) are
 *      byte for byte what mpfmt_upload_samples of the concatenated set and mpfmt_graph_step_device(r_new) leave:
 *        membership  i != v and d2 <= r_new * r_new (d2 the left-to-right unfused fp64 fold), distance sqrt(d2);
 *        old column  keeps its entries (radius rule below) and gains the new samples within r_new behind them;
 *        new column  old and new neighbours ascending, self excluded BY INDEX (a bit-copy of another sample is a neighbour at 0);
 *        free bit    of (row y, column x) is is_free_motion(V[y], V[x]), first-point bounds test included -- both directions of a
 *                    new pair are tested; old entries keep their bits.
 *      r_new below the graph's radius: an old entry stays iff its d2 <= fl(r_new * r_new).  Only fl(sqrt(d2)) is stored; with
 *      s = fl(sqrt(fl(r_new * r_new))) a stored distance < s is a member, > s is not, == s decides nothing and the entry's d2 is
 *      computed again from the coordinates.  An imported graph's distances are taken as given.
 *      Afterwards the ctx is in the state mpfmt_graph_import leaves plus a current swept mask: the radius is r_new, the cell grid
 *      is that of the grown set, a resident steering graph is dropped, and so are a tracked field and a tracked cost-to-go (as new
 *      samples drop them) unless the ctx opted in to carrying them -- option "samples_add_keeps_fields", below;
 *      mpfmt_prmstar / mpfmt_fmtstar at r_new run without pair phase or sweep, mpfmt_boxes_add / _remove stay in place.
 *      TRACKED FIELDS.  With mpfmt_set_option(ctx, "samples_add_keeps_fields", 1) (default 0) an in-place call CARRIES a
 *      live tracked cost-to-come field and a live tracked cost-to-go field whose delta history stands (one that the next update would
 *      recompute anyway is dropped): labels, parents and successors of the old samples are kept, the new samples get +Inf and none and
 *      are no targets, the entry index of every parent edge is found again in the grown column, and the CHANGED COLUMNS -- every new
 *      column, every old column that lost an entry to the radius rule or gained a row -- join the field's dirty set beside the
 *      pending columns of earlier box or shape edits.  A parent edge that the smaller radius dropped counts as an edge that lost its
 *      bit.  The field stays tracked, and mpfmt_field_update / mpfmt_togo_update then run the repair as after a box edit (path = 1):
 *      C / A are byte for byte mpfmt_graph_sssp(source) on the grown graph, G / S byte for byte mpfmt_graph_sssp_to(targets), for any
 *      interleaving of growths (radius kept or shrunk) with mpfmt_boxes_add / _remove, with or without checkpts.  Between a carried
 *      growth and the next update mpfmt_field_read, mpfmt_field_goal and mpfmt_togo_read return MPFMT_ERR_STATE: the last valid
 *      field has another length.  The carry writes spare buffers that change places with the tracked ones only when the whole call
 *      has succeeded (footprint: each carried field twice at the peak); a refused call leaves both fields as they were.  On the
 *      invalidating path both are dropped whatever the option.  New goal samples join a carried cost-to-go field through
 *      mpfmt_togo_targets_add.
 *      Measured on one MI355X (profiles/growfield_mi355x.json): at N = 1e6 in R^6, 100 new samples change 1 % of the
 *      columns and mpfmt_samples_add + mpfmt_field_update cost 4.2 ms against 15.3 ms for mpfmt_samples_add + mpfmt_field_begin (3.7x;
 *      the cost-to-go field of a ball of targets: 5.2 against 10.9 ms, 2.1x), at the radius kept or shrunk by the default rule
 *      (3.1x / 1.9x); 1e4 new samples change 65-84 % of the columns and the two ways are level (1.04-1.18x); at n_add / N = 10 %
 *      (N = 1e5) the repair is slower than the recomputation (0.87-0.99x).  Carrying pays up to n_add / N of about 0.1 % and is level at
 *      1 %: the range in which growth itself pays; beyond that, leave the option at 0 and begin the fields again.
 *      ALL OR NOTHING: the grown arrays are built in spare buffers that change places with the ctx's own only when everything has
 *      succeeded.  Footprint: at the peak the ctx holds the graph twice (old and grown colptr / rowval / nzval / mask) plus one
 *      byte per grown entry and the new samples' lists (about 2 x 21 bytes per added entry); the spare buffers stay with the ctx.
 *      Refused, leaving samples, graph, mask and tracked state as they were: NULL with a positive count, a non-finite coordinate, an
 *      r_new that is not finite and positive, N + n_add beyond the sample limit (MPFMT_ERR_ARG); a failed allocation
 *      (MPFMT_ERR_HIP).  n_add == 0 succeeds and does nothing.
 *      EVERY OTHER STATE (no resident graph, a k-nearest graph, an unswept or stale mask, a sharded ctx, the 2-D SAT world, a
 *      non-identity workspace, r_new above the graph's radius): the samples are appended on the device and the ctx is what
 *      mpfmt_upload_samples of the concatenated set leaves.
 *      mpfmt_get_stat: "samples_add_path" (1 in place, 0 invalidated), "samples_add_candidates" (distances evaluated),
 *      "samples_add_entries" (entries added, both directions), "samples_add_dropped" (old entries the smaller radius removed),
 *      "samples_add_flagged_columns" (the changed columns of an in-place call: a function of the two graphs alone),
 *      "samples_add_fields_carried" (bit 0: the cost-to-come field, bit 1: the cost-to-go field was carried by the last call),
 *      "samples_add_keeps_fields" (the option, read back);
 *      timing keys "samples_add_near", "samples_add_merge", "samples_add_carry", "samples_add".
 *      Meant for n_add well below N (a refinement step).  The merge moves the whole CSC once whatever n_add is; every new sample walks
 *      its 3^d cells of the grid on its own.  Measured on one MI355X (profiles/grow_mi355x.json): at N = 1e6 in R^6
 *      (nnz 1.1e8) 100 new samples cost 1.5 ms against 3.4 ms for the upload and step of the concatenated set, 1e4 cost the same as
 *      the rebuild, 1e5 five times more; in R^12 100 samples cost 7 ms against 35 ms and 1e4 six times the rebuild.  Growth pays up
 *      to n_add / N of about 1 % in R^6 and about 0.05 % in R^12; beyond that, upload the concatenated set.
 * mpfmt_host_graph_grow : the same on the host over the device-native arrays (X d x (N + n_add), all samples; 0-based colptr / rowval,
 *      nzval and efree of the old graph; lohi (2 d) x M, bounds or both NULL).  No ctx, no device.  cap == 0 is the size query
 *      (out_colptr, *nnz_out and info are written); *nnz_out > cap: MPFMT_ERR_CAPACITY.  The normative statement of the contract. */
typedef struct {
    int64_t candidates;        /* distances evaluated */
    int64_t entries;           /* entries added, both directions */
    int64_t dropped;           /* old entries the smaller radius removed */
} mpfmt_grow_info;
/* the radius of the resident r-disc graph (built, imported or grown); MPFMT_ERR_STATE when none is resident (a k-nearest or steering graph
 * is none) */
MPFMT_API int32_t mpfmt_graph_radius(mpfmt_ctx* ctx, double* r);
MPFMT_API int32_t mpfmt_samples_add(mpfmt_ctx* ctx, const double* X_add, int64_t n_add, double r_new);
MPFMT_API int32_t mpfmt_samples_add_device(mpfmt_ctx* ctx, const double* dX_add, int64_t n_add, double r_new);
MPFMT_API int32_t mpfmt_host_graph_grow(int64_t N, int64_t n_add, int32_t d, const double* X, const int64_t* colptr, const int32_t* rowval,
                              const double* nzval, const uint64_t* efree, const double* lohi, int32_t M, const double* ss_lo,
                              const double* ss_hi, double r_new, int64_t* out_colptr, int32_t* out_rowval, double* out_nzval,
                              uint64_t* out_efree, int64_t cap, int64_t* nnz_out, mpfmt_grow_info* info);

/* ---- many-source fields and cost matrices: up to 64 sources per pass over the graph (DESIGN.md "Many sources per pass").
 *      mpfmt_graph_sssp and mpfmt_roadmap_query compute one field per pass over rowval / nzval / the mask.  The two calls here keep the
 *      labels as L[sample][source], 64 doubles per sample, one wavefront lane per source: one visit of an entry serves 64 fields with one
 *      512-byte row read.  The least fixed point is unique and independent of the schedule (the roadmap queries above), so every value is
 *      BIT-IDENTICAL to what the one-field calls return; only rounds, relaxations and times differ.
 * mpfmt_graph_sssp_multi : the argument and result contract of mpfmt_graph_sssp -- sources 1-based (duplicates allowed), C / A nsrc x N
 *      source-major (A may be NULL: no parent pass runs and no parent buffer is held), info[nsrc] (may be NULL), the same resident graphs,
 *      the same refusals and codes, and it never sweeps edges on its own.  Sources run in groups of up to 64, one group per pass; nsrc == 0
 *      succeeds and does nothing.  C and A equal those of mpfmt_graph_sssp for the same source, bit for bit.  info[q].reached is exact per
 *      source; info[q].rounds, .relaxations and .ms_device are the GROUP's values, repeated for each of its members, and relaxations counts
 *      the entry visits whose 512-byte label row was read (one per entry and round, whatever the number of sources), not lane evaluations.
 * mpfmt_roadmap_matrix : S is d x ns, G is d x ng (column-major: state i at S + i * d).  cost[i * ng + j] and status[i * ng + j] (status may
 *      be NULL) are exactly the cost and info.status that mpfmt_roadmap_query gives for the pair (S_i, G_j): 0 solved, 1 no usable path,
 *      2 start not free, 3 goal not free (the start is looked at first); cost = +Inf unless solved.  ns fields are computed, 64 per pass,
 *      and every goal's head list is reduced over a whole group at once; the ns * ng direct edges go through the motion test of
 *      mpfmt_motions_free.  No paths are returned: ask mpfmt_roadmap_query for the pair of a chosen cell.  The refusals of
 *      mpfmt_roadmap_query (no resident r-disc graph, a k-nearest graph in the slot, a stale mask, a sharded ctx, the SAT world, a
 *      non-identity workspace: MPFMT_ERR_STATE; NULL arrays, a non-finite coordinate: MPFMT_ERR_ARG); a refused call leaves the ctx as it
 *      was.  ns == 0 or ng == 0 succeeds and does nothing.  info (may be NULL) is per call; the per-start sizes near_s / usable_s are NOT
 *      reported (an array inside an info struct would make it an in/out argument: mpfmt_roadmap_near with direction 0 gives them).
 * Both calls keep device buffers of their own in the ctx (grow-only, freed with it): 512 N bytes of labels per group, another 512 N bytes of
 *      parents once mpfmt_graph_sssp_multi was asked for A, 32 MiB of transposed staging for its copy-out; the matrix needs no parents, no
 *      seed array and no staging.  Neither touches the tracked field, the scratch of mpfmt_graph_sssp, the graph or the mask.  A failed
 *      allocation returns MPFMT_ERR_HIP and leaves the ctx usable.
 *      Stats (last call): "sssp_multi_groups", "sssp_multi_rounds" (summed over groups), "sssp_multi_rows_read" (512-byte label rows read by
 *      the relaxation, all rounds: times 512 a lower bound of its traffic), "sssp_multi_bytes" (device bytes these buffers hold).
 *      Timers: "sssp_multi_relax" (all rounds of one group), "sssp_multi_parents", "roadmap_matrix" (seeds, rounds and goal reduction). */
typedef struct {
    int64_t groups;            /* passes over the graph: ceil(ns / 64) */
    int64_t rounds;            /* relaxation rounds, summed over the groups */
    int64_t near_s, usable_s;  /* near-set entries of all starts (tail direction) and their usable part */
    int64_t near_g, usable_g;  /* near-set entries of all goals (head direction) and their free part */
    double  ms_device;         /* device time of the groups: seeds, rounds, goal reduction */
} mpfmt_roadmap_matrix_info;
MPFMT_API int32_t mpfmt_graph_sssp_multi(mpfmt_ctx* ctx, const int64_t* sources, int64_t nsrc, int32_t checkpts, double* C, int64_t* A,
                               mpfmt_sssp_info* info);
MPFMT_API int32_t mpfmt_roadmap_matrix(mpfmt_ctx* ctx, const double* S, int64_t ns, const double* G, int64_t ng, int32_t checkpts, double* cost,
                             int32_t* status, mpfmt_roadmap_matrix_info* info);

/* ---- roadmap queries for external states, steering spaces: the calls of "roadmap queries for external states" on a
 *      resident double-integrator, Dubins or Reeds-Shepp graph.  The ctx holds an unsharded, filled and swept steering graph and an
 *      N-D box set; callers pass no space parameters: the resident graph's (rho or turning radius and speed, the cost radius r) are used.
 *      GOVERNING RULE.  An external state q (d finite doubles) gets the entries it would have had, had it been a sample when the graph
 *      was built and swept: the same arithmetic, the same direction convention (entry of column x with row y = the edge y -> x), and
 *      no self-exclusion, because q has no index.
 *      Head list of q (direction 1, edges y -> q, q in the role of a column); cost <= r is required in every space:
 *        double integrator : member iff dcost(V[y], q; r) > 0 (the build's candidate test) and cost <= r from steer(V[y], q);
 *                            weight = that cost; free bit = the sweep's 5-waypoint motion test V[y] -> q with the t* of that steer.
 *        Dubins            : member iff the positions are within r (the canonical 2-D fold d2 <= r * r of the candidate graph) and
 *                            cost <= r from dubins(V[y], q); weight = that cost; free bit = the sweep's motion test V[y] -> q.
 *        Reeds-Shepp       : member iff positions within r and reedsshepp cost (q, V[y]) <= r -- the cost-only evaluation in the
 *                            direction the build stores for column q, row y; weight = that cost; free bit = motion test V[y] -> q.
 *      Tail list of q (direction 0, edges q -> y, q as a row of column y): the mirror image.  Double integrator and Dubins: steer
 *        and motion q -> V[y].  Reeds-Shepp: weight = cost (V[y], q), motion test q -> V[y].
 *      Consequences: indices ascend.  A sample bit-equal to q is a member like any duplicate sample is today (cost 0, t* = 0, and
 *        whatever bit the motion test returns at t = 0).  For q bit-equal to sample v the head list is column v of the resident graph
 *        plus v itself, the tail list every entry with row v plus v; weights and bits are the resident ones, bit for bit.
 *      A pair query (s, g) reads as mpfmt_roadmap_query with these lists substituted: seeds fl(0 + w(s, y)) on tail entries that are
 *        free and, with checkpts, have F[y] set (F = the bitmap of the steering planners: bounds on all d coordinates, the point test
 *        on the first dw); the direct edge exists iff g passes the tail-list membership of s (g treated as a sample) and the motion
 *        s -> g is free, its weight is that entry's weight; C = the least fixed point of C[x] = min(seed[x], min_y fl(C[y] + w_yx));
 *        cost = min(direct, min_y fl(C[y] + w(y, g))) over free head entries; parents by the rule above with s as index 0 and
 *        label 0, the direct edge wins ties.  The uniqueness argument needs only w >= 0 and monotone fl(a + w): it holds for these
 *        quasi-metric weights.  Status 0 solved, 1 no usable path, 2 s not a free state, 3 g not a free state (the steering planners'
 *        predicate: bounds on all d coordinates, point test on the first dw; s is looked at first).  near_* and usable_* are filled for
 *        every status; info is mpfmt_roadmap_info.
 * mpfmt_steer_roadmap_near / _attach / _query : arguments, CSR layout, the cap == 0 size query and MPFMT_ERR_CAPACITY exactly as
 *      mpfmt_roadmap_near / _attach / _query.  Lists leave the kernel in ascending order (no ordering pass).
 * Refusals leave the ctx as it was.  MPFMT_ERR_STATE: no resident steering graph (a Euclidean or k-nearest graph: use
 *      mpfmt_roadmap_*), an unswept graph or no mask, a sharded ctx, the 2-D SAT world, no box set.  MPFMT_ERR_ARG: NULL arrays, a
 *      bad direction, negative counts, a non-finite coordinate.  nq == 0 succeeds and does nothing.  The calls touch neither graph,
 *      mask, segment counts, a tracked cost-to-go field nor the samples.
 *      Timers "steer_roadmap_near", "steer_roadmap_attach"; stats "roadmap_candidates" (pairs pre-tested by the last call),
 *      "roadmap_near_total" (entries found), "steer_roadmap_steered" (exact steers run).
 * Out of scope: a matrix form and a host twin (the product has no host restatement of the steering sweeps), k-nearest graphs, the
 *      SAT world, sharded contexts, the controls of the attachment edges (mpfmt_di_steer / _dubins_steer / _reedsshepp_steer give
 *      them for any state pair). */
MPFMT_API int32_t mpfmt_steer_roadmap_near(mpfmt_ctx* ctx, const double* Q, int64_t nq, int32_t direction, int64_t* ptr, int64_t cap,
                                           int64_t* idx, double* dist, uint64_t* free_mask, int64_t* total);
MPFMT_API int32_t mpfmt_steer_roadmap_attach(mpfmt_ctx* ctx, const double* Q, int64_t nq, const double* C, int64_t* parent, double* cost);
MPFMT_API int32_t mpfmt_steer_roadmap_query(mpfmt_ctx* ctx, const double* S, const double* G, int64_t nq, int32_t checkpts, double* cost,
                                            int64_t* path_ptr, int64_t* path, int64_t path_cap, mpfmt_roadmap_info* info);

/* ---- adaptive shortcutting of solution paths (Hsu 2000): shortcut / cut_corner / adaptive_shortcut(!) of src/postprocessors.jl:6-50,
 *      statement for statement, for ONE path on the host and for a BATCH of paths on the device (one wavefront per path; the tree paths
 *      that mpfmt_prmstar / mpfmt_graph_sssp leave to every reached sample are the batch).
 *      free(v, w) is the bit mpfmt_motions_free returns under the ctx's resident checker (N-D AABBs or 2-D SAT shapes), the first-point
 *      bounds test of statespaces.jl:153-158 included.
 *        shortcut(p)     : n == 2 -> p; free(p[1], p[n]) -> the two ends; else mid = ceil(n / 2) and
 *                          shortcut(p[1:mid])[1:end-1] ++ shortcut(p[mid:n])                                    (postprocessors.jl:6-16)
 *        cut_corner      : m1 = (v1 + v2) / 2, m2 = (v3 + v2) / 2; while !free(m1, m2): both <- their midpoints with v2 (fp64, one add and
 *                          one halving per coordinate, unfused); the result is the FIRST free level              (:18-26)
 *        adaptive_shortcut(p, iterations): shortcut to a fixed point (equal length = equal path: shortcut only removes states), then
 *                          `iterations` times: every interior vertex becomes its two cut points, shortcut to a fixed point   (:28-39)
 *        cumcost         = cumsum([0; norm.(diff(path))]), norm = sqrt of the left-to-right fold of squares (the graph costs' canon),
 *                          summed left to right.
 *      Two guards the reference lacks, identical on host and device:
 *        max_states : an expansion that would make the working path longer than max_states (2 n - 2 > max_states) stops the path: it
 *                     returns as it stood after the last completed iteration, status TRUNCATED.
 *        stuck      : a halving that changes neither m1 nor m2 while the segment is not free (an interior vertex inside an obstacle) would
 *                     loop forever: the path returns as it stood after the last completed iteration, status STUCK.  Corners are cut in
 *                     order, so the counts cover the corners before the stuck one, its own tests, and nothing after it.
 *      info: iterations_done = completed iterations; max_working_len = longest working path (the input and every completed expansion);
 *      max_halvings = most halvings of one cut_corner loop; collision_checks = the tests the SEQUENTIAL loop asks for whose first point
 *      lies inside the state bounds (what P.CC.count gains: boxesND.jl:26 behind statespaces.jl:155) -- a function of the resolved
 *      recursion, not of scheduling; tests_evaluated = tests actually run (the device tests the whole split tree and blocks of
 *      cut_corner levels speculatively; on the host: every test asked).
 *      Paths: d x n column-major; a batch is the concatenation with offsets[B + 1] (0-based state offsets, offsets[0] = 0).  out_P /
 *      cumcost have room for out_cap states (sum of n_out > out_cap: MPFMT_ERR_CAPACITY, info and out_offsets are still written; B *
 *      max_states always suffices); out_offsets[B + 1] as offsets.
 *      MPFMT_ERR_ARG: a path of fewer than 2 states, a non-finite coordinate, iterations < 0, max_states below a path's length (or above
 *      2^20); MPFMT_ERR_STATE: no resident checker, a sharded ctx.  A refused call leaves the ctx as it was.  A path of 2 states comes
 *      back unchanged with 0 checks.  Timer "shortcut_batch"; stats "shortcut_tests_evaluated", "shortcut_checks" (last batch).
 *      mpfmt_host_adaptive_shortcut: one path against the AABB checker given as arrays (lohi (2 d) x M as mpfmt_upload_boxes, ss_lo /
 *      ss_hi or both NULL); no ctx, no device: the CPU baseline and the checker of the device result (bit-equal). */
#define MPFMT_SHORTCUT_DONE      0
#define MPFMT_SHORTCUT_TRUNCATED 1
#define MPFMT_SHORTCUT_STUCK     2
typedef struct {
    int32_t status;            /* MPFMT_SHORTCUT_DONE / _TRUNCATED / _STUCK */
    int32_t iterations_done;
    int64_t n_out;             /* states of the returned path */
    int64_t max_working_len;
    int64_t max_halvings;
    int64_t collision_checks;
    int64_t tests_evaluated;
} mpfmt_shortcut_info;
MPFMT_API int32_t mpfmt_host_adaptive_shortcut(const double* P, int64_t n, int32_t d, const double* lohi, int32_t M, const double* ss_lo,
                                     const double* ss_hi, int32_t iterations, int64_t max_states, double* out_P, int64_t out_cap,
                                     double* cumcost, mpfmt_shortcut_info* info);
MPFMT_API int32_t mpfmt_adaptive_shortcut_batch(mpfmt_ctx* ctx, const double* P, const int64_t* offsets, int64_t B, int32_t iterations,
                                      int64_t max_states, double* out_P, int64_t* out_offsets, int64_t out_cap, double* cumcost,
                                      mpfmt_shortcut_info* info);
MPFMT_API int32_t mpfmt_adaptive_shortcut(mpfmt_ctx* ctx, const double* P, int64_t n, int32_t iterations, int64_t max_states, double* out_P,
                                int64_t out_cap, double* cumcost, mpfmt_shortcut_info* info);

/* ---- time discretisation of solution paths: time_discretize_solution! / time_space_solution! of src/postprocessors.jl:61-83, i.e.
 *      steering_control(SS, path...) (statespaces.jl:147) followed by propagate(d, v, us, times) (statespaces.jl:104-119), for ONE path on
 *      the host and for a BATCH of paths on the device (lane = output sample).
 *      A path is n >= 2 states p_1 .. p_n (d doubles each, all finite) in one of four spaces:
 *        MPFMT_SPACE_EUCLID      d as mpfmt_euclid_steer accepts (1 .. MPFMT_MAX_DIM)   params NULL
 *        MPFMT_SPACE_DI          d = 2 m, m = 1 .. 6                                    params {rho, r}  (r: the Newton bracket tm of steer,
 *                                                                                       linearquadratic.jl:191-195); both > 0
 *        MPFMT_SPACE_DUBINS      d = 3                                                  params {turn_radius, speed}, both > 0
 *        MPFMT_SPACE_REEDSSHEPP  d = 3                                                  params {turn_radius, speed}, both > 0
 *      Control steps: every consecutive pair (p_i, p_i+1) is steered on its own, from the GIVEN states: Euclidean one step (t, u) with the
 *        arithmetic of mpfmt_euclid_steer; double integrator one step (t*, target p_i+1), t* of mpfmt_di_steer; Dubins 3 steps (duration,
 *        speed, curvature) as mpfmt_dubins_steer returns them; Reeds-Shepp nsegs <= 5 steps as mpfmt_reedsshepp_steer returns them.  The
 *        steps of a path are numbered j = 1 .. K in order.  A Euclidean pair of equal states gives one step of duration 0 with u = 0 (the
 *        reference would produce NaN there: a declared guard).
 *      Chain: S_1 = p_1, S_j+1 = propagate(S_j, c_j), the full step: Euclidean S_j + t_j * u_j (unfused); cars: the propagate of
 *        simplecars.jl:55-67, mod 2 pi included; double integrator: the target p_i+1 exactly (linearquadratic.jl:80).  T0_1 = 0, T0_j+1 =
 *        fl(T0_j + t_j), tf = T0_K+1: the left-to-right fold of duration(::ControlSequence) (primitivetypes.jl:132).
 *      Times: mode MPFMT_DISC_DT (time_discretize_solution!), dt > 0 finite: n_out = floor(fl(tf / dt)) + 1, t_k = min(fl(k * dt), tf) for
 *        k = 0 .. n_out - 1; with append_end != 0 and the last t_k < tf one more sample at tf follows (the [0:dt:t; t] of waypoints,
 *        statespaces.jl:127-131).  Mode MPFMT_DISC_N (time_space_solution!), n_out = n_samples >= 2: t_k = fl(fl(k / (n_samples - 1)) * tf),
 *        so the last time is tf exactly.  Both are DECLARED forms: Julia's FloatRange and LinSpace can differ from them in the last bit,
 *        and in the count where tf / dt lies within an ulp of an integer.
 *      Sample at t_k: j = the first step with t_k < T0_j+1, or K if there is none -- what the reference's loop `while t >= t0 +
 *        duration(u[i]) && i < length(u)` (statespaces.jl:111) arrives at, T0 being that loop's own running sum; steps of duration 0 are
 *        passed over unless one is the last step.  With s = t_k - T0_j the state is propagate(S_j, c_j, s) (statespaces.jl:79-81,
 *        linearquadratic.jl:81-82): s <= 0 gives S_j, s >= t_j the full step, otherwise Euclidean S_j + s * u_j, cars the car propagate
 *        with duration s, double integrator the closed-form state x(p_i, p_i+1, t*, s) of the collision waypoints.
 *      Per sample: the state (out_X, d doubles), T = t_k (out_T), seg = the 1-based index i of the pair the step j belongs to (out_seg,
 *        may be NULL).  Per path: mpfmt_disc_info {n_out, steps = K, duration = tf}.
 *      Layout as mpfmt_adaptive_shortcut_batch: paths d x n column-major, offsets[B + 1] 0-based with offsets[0] = 0; out_offsets[B + 1]
 *        likewise.  out_cap == 0 is the size query (only the steer and the chain run; out_offsets and info are written; out_X / out_T
 *        may be NULL); a total above out_cap returns MPFMT_ERR_CAPACITY with out_offsets and info written.
 *      MPFMT_ERR_ARG: a path of fewer than 2 states, a non-finite coordinate or parameter (or one <= 0), dt <= 0 or not finite in DT
 *        mode, n_samples < 2 in N mode, a d that does not fit the space, a total above 2^31 - 1 samples; MPFMT_ERR_STATE: a sharded ctx.
 *      Nothing resident is needed or touched: no samples, no graph, no obstacle set; a fresh ctx serves.  Timer "discretize_batch" (also
 *        "discretize_steer", "discretize_chain", "discretize_sample" by launch); stats "discretize_steps", "discretize_samples" (last
 *        batch).  Every loop on the device is bounded by an array length or by K; the only iterative arithmetic is the Newton search of
 *        mpfmt_di_steer, unchanged.
 *      mpfmt_host_discretize: one path, no ctx, no device: the sequential loop of statespaces.jl:104-119 statement for statement; the CPU
 *        baseline and the checker of the device result, which is bit-equal in all four spaces (same operations, same mp_math.h
 *        trigonometry, unfused, correctly rounded / and sqrt). */
#define MPFMT_SPACE_EUCLID     0
#define MPFMT_SPACE_DI         1
#define MPFMT_SPACE_DUBINS     2
#define MPFMT_SPACE_REEDSSHEPP 3
#define MPFMT_DISC_DT 0
#define MPFMT_DISC_N  1
typedef struct {
    int64_t n_out;             /* samples of the path */
    int64_t steps;             /* K */
    double duration;           /* tf */
} mpfmt_disc_info;
MPFMT_API int32_t mpfmt_host_discretize(int32_t space, int32_t d, const double* params, const double* P, int64_t n, int32_t mode, double dt,
                              int64_t n_samples, int32_t append_end, double* out_X, double* out_T, int32_t* out_seg, int64_t out_cap,
                              mpfmt_disc_info* info);
MPFMT_API int32_t mpfmt_discretize_batch(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const int64_t* offsets,
                               int64_t B, int32_t mode, double dt, int64_t n_samples, int32_t append_end, double* out_X, double* out_T,
                               int32_t* out_seg, int64_t* out_offsets, int64_t out_cap, mpfmt_disc_info* info);
MPFMT_API int32_t mpfmt_discretize(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, int64_t n, int32_t mode,
                         double dt, int64_t n_samples, int32_t append_end, double* out_X, double* out_T, int32_t* out_seg, int64_t out_cap,
                         mpfmt_disc_info* info);

/* ---- steering shortcut: shortcutting of solution paths in the double-integrator, Dubins and Reeds-Shepp spaces, for a BATCH of paths on
 *      the device (one wavefront per path), and the pair primitive it is made of.  The reference refuses these spaces
 *      (adaptive_shortcut: "requires Euclidean SS", postprocessors.jl:41-50); the procedure below is this library's own statement.
 *      space / d / params as mpfmt_discretize: MPFMT_SPACE_DI (d = 2 m, m = 1 .. 6, params {rho, tmax}: tmax the Newton bracket of the
 *      steer), MPFMT_SPACE_DUBINS / _REEDSSHEPP (d = 3, params {turn_radius, speed}).
 *      The checker is the ctx's resident one, bound as the space's graph sweep binds it: the workspace boxes of mpfmt_upload_boxes (dw = m
 *      for the double integrator, dw = 2 for the cars) with the d state bounds, or the 2-D shape world (mpfmt_upload_shapes2d; cars, and
 *      the double integrator with m = 2; its d state bounds through mpfmt_set_state_bounds).  No sample set and no graph is needed:
 *      mpfmt_upload_boxes takes the number of state bounds as an argument, so a fresh ctx with a checker serves.
 *
 *   mpfmt_steer_motions_free: n pairs (P_e, Q_e), P and Q d x n column-major.  Per pair: cost[e] = the steer's cost (mpfmt_di_steer,
 *      mpfmt_dubins_steer, mpfmt_reedsshepp_steer); dur[e] = t* for the double integrator, the left-to-right sum of the step durations for
 *      the cars; bit e of mask = is_free_motion(P_e, Q_e, CC, SS) exactly as the space's graph sweep computes it, with the same device
 *      functions: 5 waypoints at the steer's t*, or arc waypoints every pi / 12, the bounds test of each segment's first waypoint
 *      included; nseg[e] = the segment tests counted (what CC.count gains).  cost, dur and nseg may be NULL; mask has ceil(n / 64) words.
 *      Errors as mpfmt_discretize (MPFMT_ERR_ARG: NULL P / Q / mask with n > 0, n < 0, a non-finite coordinate or parameter, a d that does
 *      not fit the space), plus MPFMT_ERR_STATE: no checker, a checker whose workspace or bounds do not fit the space, a sharded ctx.
 *      n == 0 succeeds and does nothing.  Timer "steer_motions_free".
 *
 *   mpfmt_steer_shortcut_batch / mpfmt_steer_shortcut: with (cost, dur, bit, nseg)(v, w) the primitive's results for the pair,
 *      Working path and leg costs: the working path is p_1 .. p_n with leg costs c_i (and leg durations); cum_1 = 0 and cum_i+1 =
 *        fl(cum_i + c_i), a left-to-right fold.  Input legs are steered and tested once; legs_blocked counts input legs whose own test
 *        fails: they are reported, not altered.
 *      Acceptance: ok(i, j), for j > i + 1, holds iff bit(p_i, p_j) is set and cost(p_i, p_j) <= fl(SLACK * fl(cum_j - cum_i)), SLACK =
 *        1 + 2^-30 (exact in fp64): a reconnection that IS the replaced trajectory ties on the accepting side, not on rounding noise.
 *        The cost condition also covers a double-integrator steer clamped at its bracket tmax: a valid trajectory, not an improvement.
 *        Every ok asked evaluates the pair test (its nseg counts) whatever the cost comparison gives.
 *      shortcut(p): postprocessors.jl:6-16 with is_free_motion replaced by ok: n == 2 -> p; ok(1, n) -> the two ends; else mid =
 *        ceil(n / 2) and shortcut(p[1:mid])[1:end-1] ++ shortcut(p[mid:n]); cum is the fold of the path the pass began with.  An accepted
 *        node's leg cost (and duration) is its steer's.  Applied to a fixed point: the length strictly decreases until it stops.
 *      refine(p): every leg of duration T > 0 proposes the state m at fl(T / 2) along its own steered trajectory: the double integrator's
 *        closed-form waypoint state, the cars' partial propagate through the control steps, both exactly as mpfmt_discretize samples a
 *        two-state path at 3 samples.  m is inserted iff bit(p_i, m), bit(m, p_i+1) and fl(c' + c'') <= fl(SLACK * c_i) for the two
 *        re-steered costs; both halves are always asked.  Invariant: every leg of the working path is an input leg or has passed the
 *        motion test.
 *      Driver: shortcut to a fixed point; then `iterations` times: refine, then shortcut to a fixed point.  An iteration that returns the
 *        bit-identical states it began with ends the loop (later ones would repeat it); it still counts in iterations_done.  Guard: a
 *        refine that would make the working path longer than max_states returns the path of the last completed iteration, status
 *        MPFMT_SHORTCUT_TRUNCATED (the tests of that refine were asked and are counted); MPFMT_SHORTCUT_STUCK cannot occur.
 *      Outputs: out_P, out_offsets and cumcost laid out as mpfmt_adaptive_shortcut_batch (cumcost = the cum fold of the result);
 *        out_origin (may be NULL): int32 per output state, the 1-based index of the input state, 0 for an inserted one; per path an
 *        mpfmt_steer_shortcut_info: inserted = states the completed refines inserted; collision_checks = the nseg of the tests the
 *        SEQUENTIAL procedure asks for (input legs, asked nodes, both halves of every proposing leg); tests_evaluated = pair tests
 *        actually run (the device tests the whole split tree speculatively); cost_in / cost_out = cum_n of the input and of the result;
 *        max_working_len = the longest working path (the input and every completed refine).
 *      A path of 2 states is shortcut to itself: with iterations == 0 it comes back unchanged with only its one leg test.
 *      MPFMT_ERR_ARG: as the primitive, plus a path of fewer than 2 states, iterations < 0, max_states below a path's length or above 2^16;
 *        MPFMT_ERR_STATE as the primitive.  sum of n_out > out_cap: MPFMT_ERR_CAPACITY with info and out_offsets written (out_cap == 0 with
 *        NULL outputs is the size query; B * max_states always suffices).  A refused call leaves the ctx as it was.  There is no host
 *        twin: the library has no host restatement of the steering sweeps.  Timer "steer_shortcut_batch"; stats
 *        "steer_shortcut_tests_evaluated", "steer_shortcut_checks" (last batch). */
typedef struct {
    int32_t status;            /* MPFMT_SHORTCUT_DONE / _TRUNCATED */
    int32_t iterations_done;
    int64_t n_out;             /* states of the returned path */
    int64_t max_working_len;
    int64_t inserted;
    int64_t legs_blocked;
    int64_t collision_checks;
    int64_t tests_evaluated;
    double cost_in, cost_out;
} mpfmt_steer_shortcut_info;
MPFMT_API int32_t mpfmt_steer_motions_free(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const double* Q,
                                 int64_t n, uint64_t* mask, double* cost, double* dur, int32_t* nseg);
MPFMT_API int32_t mpfmt_steer_shortcut_batch(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P,
                                   const int64_t* offsets, int64_t B, int32_t iterations, int64_t max_states, double* out_P,
                                   int64_t* out_offsets, int64_t out_cap, double* cumcost, int32_t* out_origin,
                                   mpfmt_steer_shortcut_info* info);
MPFMT_API int32_t mpfmt_steer_shortcut(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, int64_t n,
                             int32_t iterations, int64_t max_states, double* out_P, int64_t out_cap, double* cumcost, int32_t* out_origin,
                             mpfmt_steer_shortcut_info* info);

/* ---- Monte-Carlo collision probability of candidate edges (BASELINE.json configs[4]).  The reference
 *      has no implementation (README.md:9-10 cites the papers only); the workload is the one SURVEY 8d defines: per edge
 *      (src[e] -> dst[e], 1-based sample indices) `rollouts` perturbed copies of the 2-point trajectory, each put through
 *      is_free_motion(v', w', CC, SS) (statespaces.jl:153-158, boxesND.jl:44-56).  v' = v + sigma z with z a standardised
 *      Irwin-Hall(8) variate built from the halfwords of Philox4x32-10(key = seed, counter = (rollout, edge, coordinate, 2))
 *      -- integer sums and unfused fp64 only, so a scalar loop reproduces hits[e] (colliding rollouts) exactly.
 *      Needs the AABB checker; E and rollouts < 2^32. */
MPFMT_API int32_t mpfmt_mc_edges_collision(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, double sigma, int64_t rollouts,
                                 uint64_t seed, int64_t* hits);
/*      Importance-sampling estimator of the same probability (the approach of the papers README.md:9-10 cites): rollouts are drawn from
 *      a mixture -- half of them from the nominal noise, the rest from the noise shifted (both end points alike, at most 3 sigma per
 *      coordinate) towards the closest points of the up to three obstacles nearest to the nominal segment (closest(p, BB, I) of
 *      boxesND.jl:61-86 with W = I -- a clamp -- at five points of the segment); a colliding rollout counts with weight
 *      f(y) / (0.5 f(y) + sum_j (0.5 / K) f(y - s_j)), f the product of Irwin-Hall(8) densities.  Weights are quantised to 2^-40 and
 *      summed as integers: estimate = wsum[e] / (rollouts * 2^40), which a scalar loop reproduces exactly (the arithmetic is spelled out
 *      at k_mc_is_edges, csrc/kernels_sweep.hip).  rollouts < 2^22; the whole obstacle set must fit one LDS stage (M <= 256 at d <= 8). */
MPFMT_API int32_t mpfmt_mc_edges_collision_is(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, double sigma, int64_t rollouts,
                                    uint64_t seed, uint64_t* wsum);
/*      The ADAPTIVE estimator (BASELINE configs[4]: "adaptive-importance-sampling"): per edge a pilot of 4096 rollouts with the noise
 *      inflated by 1.625 finds colliding perturbations; their likelihood-ratio-weighted mean -- the mean of the nominal noise GIVEN a
 *      collision, one cross-entropy update of the proposal's mean in all 2 d noise coordinates -- becomes the shift of a two-component
 *      mixture (half nominal, half shifted); weights f(y) / (0.5 f(y) + 0.5 f(y - mu)) as above.  An edge whose pilot sees no collision
 *      is estimated by plain Monte Carlo (mu = 0, every weight 1).  shifts (may be NULL): E x 2 d doubles, the mu of every edge in
 *      noise units.  Spelled out: pilot rollout k, coordinate c < 2 d: Irwin-Hall integer S from Philox(key = seed, counter = (k, e,
 *      64 + c, 2)), Z = S - 262140, z = Z / 53509.92, y = 1.625 z; a colliding rollout's likelihood ratio lr = prod g(x(y_c)) /
 *      prod g(x(z_c)) (g, x as above), Wq = (uint64)(lr 2^30); SW = sum Wq, A_c = sum Wq Z_c over the hits; mu_c = clip(1.625 (A_c /
 *      53509.92) / SW, -3, 3).  Main rollouts: noise as in mpfmt_mc_edges_collision, shifted by mu when word 0 of Philox(counter = (k,
 *      e, 2 d, 3)) is odd.  Integer sums throughout: a scalar loop reproduces wsum and shifts exactly; same limits as above. */
MPFMT_API int32_t mpfmt_mc_edges_collision_ais(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, double sigma, int64_t rollouts,
                                     uint64_t seed, uint64_t* wsum, double* shifts);

/* ---- Dubins car: DubinsQuasiMetricSpace(r_turn, s, lo, hi) of src/statespaces/simplecars.jl:32-38.
 *      Samples are SE2 states (x, y, theta) (upload_samples with d = 3); obstacles live in the workspace (x, y)
 *      (VectorView(1:2)): upload_boxes with dw = 2 and the 3 state bounds (lo_x, lo_y, 0; hi_x, hi_y, 2pi).
 *      dubins_graph_count/fill : the chopped backward sets (nearneighbors.jl:185-198) as a sparse cost matrix in CSC,
 *             column j = sources i (ascending, 1-based) with |xy_i - xy_j| <= r and dubins(i -> j) <= r
 *             (simplecars.jl:106-215), nzval = cost; the forward sets are its transpose.
 *      dubins_graph_edges_free : entry e (row y -> column x): is_free_motion(V[y], V[x], CC, SS) over the reference's
 *             collision waypoints (arcs every pi/12, :68-83; statespaces.jl:127-135,153-158); nseg[e] = workspace
 *             segment tests the reference would have counted (may be NULL).
 *      dubins_steer : batch steer on explicit pairs; controls[i][3][3] = (duration, speed, signed curvature) per segment.
 *      dubins_fmtstar : fmtstar! in this space (forward / backward neighbour sets like the double integrator's).
 *      sin / cos / atan2 / acos are the library's own (csrc/mp_math.h: fixed reductions and polynomials from + - * / sqrt), the
 *      same header the CPU oracle compiles: graphs, masks and costs are bit-identical to the oracle's; against a libm-based
 *      host (Julia) costs agree to ~1e-15 relative. */
MPFMT_API int32_t mpfmt_dubins_graph_count(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t* colptr, int64_t* nnz);
MPFMT_API int32_t mpfmt_dubins_graph_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval);
MPFMT_API int32_t mpfmt_dubins_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask, uint8_t* nseg);
MPFMT_API int32_t mpfmt_dubins_steer(mpfmt_ctx* ctx, const double* X0, const double* X1, int64_t n, double turn_radius, double speed,
                           double* cost, double* controls);
MPFMT_API int32_t mpfmt_dubins_fmtstar(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                             int32_t goal_kind, const double* goal_params, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);

/* ---- Reeds-Shepp car: ReedsSheppMetricSpace(r_turn, s, lo, hi) of src/statespaces/simplecars.jl:29-34 --
 *      the car that may reverse; a symmetric (chopped) metric, so forward and backward neighbour sets coincide
 *      (nearneighbors.jl:200-203).  Same world set-up as the Dubins car above.
 *      reedsshepp_graph_count/fill : column v = { w : |xy_w - xy_v| <= r and reedsshepp(v, w) <= r } (simplecars.jl:266-364
 *             with the word families :367-553), rows ascending 1-based, nzval = reedsshepp(v, w) -- evaluated in that
 *             argument order: the two directions can differ in the last bits, and the reference's inball(v) holds d(v, w).
 *      reedsshepp_graph_edges_free : entry e (row w of column v): is_free_motion(V[w], V[v], CC, SS) -- the motion
 *             fmtstar! tests when it connects v to the open parent w (fmt.jl:75) -- over the waypoints of
 *             steering_control(V[w], V[v]) (:68, :70-82); nseg[e] as above.
 *      reedsshepp_steer : batch steer; controls[i][5][3] = (duration, speed, signed curvature), segments >= nsegs[i]
 *             are zero (nsegs may be NULL).
 *      reedsshepp_fmtstar : fmtstar! in this space (the symmetric recursion of fmt.jl:36-100); workspace goals act on
 *             (x, y), MPFMT_GOAL_POINT takes a whole state (3 doubles). */
MPFMT_API int32_t mpfmt_reedsshepp_graph_count(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t* colptr, int64_t* nnz);
MPFMT_API int32_t mpfmt_reedsshepp_graph_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval);
MPFMT_API int32_t mpfmt_reedsshepp_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask, uint8_t* nseg);
MPFMT_API int32_t mpfmt_reedsshepp_steer(mpfmt_ctx* ctx, const double* X0, const double* X1, int64_t n, double turn_radius, double speed,
                               double* cost, double* controls, int32_t* nsegs);
MPFMT_API int32_t mpfmt_reedsshepp_fmtstar(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                                 int32_t goal_kind, const double* goal_params, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);

/* ---- Closest obstacle points in a Mahalanobis metric: closest(p, CC, W) / closeR(p, CC, W, r2) of
 *      src/collisioncheckers/boxesND.jl:33-34,61-86 (boxes, through bvls of src/collisioncheckers/bvls.jl:19-218) and
 *      src/collisioncheckers/robots2D.jl:25-26 + SAT2D.jl:208-285 (circles / convex polygons / compounds), batched over n
 *      query points P [n][dw] against the ctx's current obstacle set (mpfmt_upload_boxes or mpfmt_upload_shapes2d).
 *      W [dw][dw] symmetric positive definite; W = NULL selects the Euclidean SAT2D methods (:208-211, :239, :260-269) and
 *      is an error for boxes (the reference has no such method).
 *      mpfmt_closest : d2min[i], vmin[i][dw] and kmin[i] (1-based obstacle, 0 = none) = the minimum over the obstacles
 *             with strict < (first minimum wins); no obstacle: (Inf, p) for boxes, (Inf, 0) for shapes, as the reference.
 *      mpfmt_closeR  : per point the obstacles with d2 < r2 in ascending d2 (ties in obstacle order: the reference's
 *             sort! is stable): ptr [n+1] 1-based offsets (always written), then obstacle / d2 / v [*total][dw];
 *             MPFMT_ERR_CAPACITY with *total set when *total > cap (nothing else written).
 *      *failures (may be NULL) counts the (point, box) pairs on which the reference's bvls exhausts its 10n iterations and
 *             returns `nothing` (closest() then throws a MethodError) -- the same pairs are detected here, reported and
 *             left out of the minimum / the lists; for circles, pairs whose multiplier iteration (SAT2D.jl:222-235,
 *             unbounded in the reference) has not ended after 200 Newton steps.
 *      Values agree with the reference's LAPACK route (QR least squares, eigfact) to rounding, not bit for bit. */
MPFMT_API int32_t mpfmt_closest(mpfmt_ctx* ctx, const double* P, int64_t n, const double* W, double* d2min, double* vmin, int64_t* kmin,
                      int64_t* failures);
MPFMT_API int32_t mpfmt_closeR(mpfmt_ctx* ctx, const double* P, int64_t n, const double* W, double r2, int64_t* ptr, int64_t cap,
                     int64_t* obstacle, double* d2, double* v, int64_t* total, int64_t* failures);

/* ---- 2-D SAT world: PointRobot2D(Compound2D(parts)) of src/collisioncheckers/robots2D.jl:12-14 and
 *      SAT2D.jl -- parts are Circle(c, r) (:14-28) and convex Polygon(points) (:32-58; Box2D = 4-point polygon, :59-62).
 *      Switches the ctx's collision checker: afterwards mpfmt_points_free / _states_free = is_free_state (point vs
 *      shapes, SAT2D.jl:121-133), mpfmt_edges_free / _motions_free / _graph_edges_free / graph sweep / expand / fmtstar =
 *      is_free_motion = !colliding(Line(v, w), obstacles) (SAT2D.jl:154-178), both wrapped in the state-space checks of
 *      statespaces.jl:150-158.  mpfmt_upload_boxes switches back.  Samples must be 2-D.
 *      kinds[i]: 0 = circle, data = (cx, cy, r); 1 = polygon with nverts[i] (3..16) vertices, data = (x1, y1, x2, y2, ...);
 *      data is the concatenation in shape order (nverts is ignored for circles).  The library runs the reference's
 *      constructors (orientation, unit normals, extrema per normal, AABBs; non-convex polygons are refused like :49).
 *      Nested Compound2D parts are not represented: flatten them (every basic test starts with its own AABB check). */
#define MPFMT_SHAPE_CIRCLE  0
#define MPFMT_SHAPE_POLYGON 1
MPFMT_API int32_t mpfmt_upload_shapes2d(mpfmt_ctx* ctx, int32_t n_shapes, const int32_t* kinds, const int32_t* nverts, const double* data,
                              const double* ss_lo, const double* ss_hi);
/* ---- in-place edits of the 2-D SAT world's shape list (the counterpart of mpfmt_boxes_add / _remove, and what the
 *      reference's addobstacle / addblocker(p, r) = Circle(p, r) of robots2D.jl:23-24 become on a resident roadmap).
 *   mpfmt_shapes2d_add:    n_add shapes encoded as for mpfmt_upload_shapes2d and validated by the same constructors, appended behind
 *                          the current list.
 *   mpfmt_shapes2d_remove: ids 1-based, distinct; the remaining shapes keep their order.
 * After either call the ctx is what mpfmt_upload_shapes2d(resulting list, same bounds) leaves -- the compound box recomputed from the
 * resulting list -- except that a resident swept mask may follow in place (the table) and that the tracked fields (mpfmt_field_*,
 * mpfmt_togo_*) are NOT dropped: on the in-place path they learn the columns the edit read and their update repairs; on the other
 * path their delta history is lost and their update recomputes (path = 0) once the mask has been swept again.
 * The bit of entry e (row y in column x, segment (v, w)) under list L with compound box B(L) is
 *   in_ss(v) && ( gate(e, B(L)) || no S in L hits (v, w) ),   gate = the segment's box does not overlap B(L)
 * and the gate is not inert in floating point (a circle can "hit" an endpoint one ulp outside its own box), so
 *   add:    a free entry keeps its bit when gate(e, B') holds; else it is cleared when an added shape hits; else, when the compound
 *           box changed and the old list was not empty, when gate(e, B) held and a shape of the old list hits.  Blocked entries stay.
 *   remove: a blocked entry with in_ss(v) is set when gate(e, B') holds; else, when a removed shape hits it, it is evaluated again
 *           against all that remains.  Free entries stay.  (An empty list: the gate always holds and nothing hits.)
 * The mask is the one a whole sweep of the resulting list writes, bit for bit.
 *   state at the call                                                                      | mask                 | "boxes_delta_path"
 *   unsharded ctx, Euclidean graph (r-disc, imported, k-nearest) filled and swept, nnz > 0, | updated in place,    | 1
 *   mask resident, no speculative step in flight                                           | "graph_swept" stays  |
 *   option "steer_shapes_delta" = 1, unsharded ctx, steering graph (double integrator in    | mask and segment     | 1
 *   R^4, Dubins, Reeds-Shepp) filled and swept, nnz > 0, mask and counts resident, state    | counts updated in    |
 *   bounds unset or of the state's dimension (what the whole sweep accepts)                 | place, "steer_swept" |
 *                                                                                          | stays                |
 *   anything else: no graph, unswept, nnz == 0, sharded, a step in flight, a steering graph | graph_swept = false, | 0
 *   resident without the option                                                            | steer_swept = false  |
 * If the update itself fails, the edited list stands and the graph is swept again.
 * Under a steering graph an entry is walked over the segments between its collision waypoints, the state bounds checked
 * before each; the walk is the whole sweep's own with a delta predicate in the place of the segment test:
 *   add:    P_add(s) = gate(s, B') || ( no added shape hits s && !( the compound box changed, the old list was not empty, gate(s, B)
 *           holds and a shape of the old list hits s ) );  free' = free && free under P_add, count' = min(count, count under P_add).
 *           Every entry of a flagged column is walked: a blocked entry keeps its bit, but its count can drop.
 *   remove: P_rem(s) = gate(s, B) || ( no removed shape hits s && !( the compound box changed or nothing remains, and nothing remains
 *           or gate(s, B') holds ) );  a blocked entry whose walk under P_rem is not free is evaluated again from nothing against
 *           what remains; nothing else changes.
 * Mask words (the padding bits of the last word included) and segment counts are byte for byte those of the whole sweep of the
 * resulting list; mpfmt_steer_mask_read reads them, the next mpfmt_*_fmtstar_wavefront on the same parameters builds and sweeps
 * nothing, and a tracked cost-to-go field learns the flagged columns (mpfmt_togo_update repairs).  Flagged columns: the workspace
 * position within the column's reach (double integrator: r (|v1| + r / sqrt(rho)) (1 + 1e-9) with v1 the column's velocity; cars:
 * r (1 + 1e-6)) of a delta shape's box on both axes, or -- when the compound box changed
 * and the smaller side's list is not empty -- not inside the smaller compound box shrunk by the reach on every side.
 * "boxes_delta_entries" then counts the entries walked under the delta predicate; the timing key is "steer_delta".
 * Refused, leaving the ctx as it was: NULL with a positive count, an id out of range or repeated, an invalid shape (radius, convexity,
 * more than 16 vertices) (MPFMT_ERR_ARG); no shape world resident -- the AABB checker, or nothing uploaded
 * (MPFMT_ERR_STATE).  A count of 0 succeeds and does nothing.
 * mpfmt_get_stat: "boxes_delta_path", "boxes_delta_columns" (columns whose entries were read: sample within graph_r (1 + 1e-9) of a
 * delta shape's box, or -- when the compound box changed -- outside the compound box of the smaller list; all columns of a k-nearest
 * graph), "boxes_delta_entries" (entries that reached a shape test), "boxes" (the list length); timing key "shapes_delta". */
MPFMT_API int32_t mpfmt_shapes2d_add(mpfmt_ctx* ctx, int32_t n_add, const int32_t* kinds, const int32_t* nverts, const double* data);
MPFMT_API int32_t mpfmt_shapes2d_remove(mpfmt_ctx* ctx, const int64_t* ids, int32_t n_ids);
/* The 2-D SAT world under a steering space (the notebook's double-integrator and Dubins examples, docs/MotionPlanning.ipynb cells 7-11:
 * PointRobot2D with DoubleIntegrator(2) / DubinsQuasiMetricSpace): upload the shapes (workspace bounds), then the state-space
 * bounds of the steering space (4 for the double integrator, 3 for SE2; src/statespaces.jl:29-34, in_state_space :150).  The
 * steering sweeps (mpfmt_di_graph_edges_free, mpfmt_dubins_ / mpfmt_reedsshepp_graph_edges_free, the *_fmtstar calls) then test
 * their workspace segments with is_free_motion(v, w, CC::PointRobot2D) (robots2D.jl:13-14). */
MPFMT_API int32_t mpfmt_set_state_bounds(mpfmt_ctx* ctx, const double* ss_lo, const double* ss_hi, int32_t d_state);

/* ---- graph persistence: install a graph exported earlier by mpfmt_rdisc_count / mpfmt_rdisc_fill (same
 *      1-based CSC: colptr[N+1], rowval[nnz] strictly ascending per column, nzval[nnz]) for the samples now uploaded --
 *      the reference's ImmutableNNC(D, r) (src/nearneighbors.jl:23-28; its saveNN / loadNN! are commented out, :114-116).
 *      Afterwards mpfmt_graph_edges_free / mpfmt_graph_sweep_device / mpfmt_expand / mpfmt_fmtstar(r) use it without
 *      running the pair phase (mpfmt_fmtstar reuses any filled graph of the same radius).  The arrays are validated
 *      (monotone colptr, rows in range, ascending, no self loops); distances are taken as given. */
MPFMT_API int32_t mpfmt_graph_import(mpfmt_ctx* ctx, double r, const int64_t* colptr, const int64_t* rowval, const double* nzval);

/* ---- batch free-space sampler: sample_free!(P, N, true; ensure_goal_ct) of src/sampling.jl:11-45 with
 *      the rejection loop (sample_space, statespaces.jl:40; is_free_state, statespaces.jl:151-152) run in batches on the
 *      device.  Needs mpfmt_upload_boxes with state-space bounds (the BoundedStateSpace lo / hi) and an Identity
 *      state2workspace (d_state == dw).  The reference draws from Julia's unseeded global RNG; here candidates come from
 *      a counter-based stream (Philox4x32-10, key = seed, counter = candidate index), tested IN ORDER like the reference's
 *      loop, so the result is a pure function of (seed, N, bounds, obstacles, goal) -- independent of batching and
 *      reproducible by a scalar loop.  V[1] = init when init != NULL (sampling.jl:15-20); the last min(goal_ct, N-1)
 *      samples are free goal samples, V[N+1-i] = the i-th one (sampling.jl:37-41; sample_goal, goals.jl:97,101-108,115).
 *      The set is left uploaded in ctx (as by mpfmt_upload_samples); X_out (N*d, may be NULL) receives a copy;
 *      attempts = sample_space candidates the sequential loop would have consumed.
 *      sample_free_biased adds the goal_bias keyword (sampling.jl:11,28-30): each accepted sample is replaced by a free goal
 *      sample with probability goal_bias -- the decision for the k-th accepted sample is the uniform (seed, k) of a third
 *      stream, the replacements take free goal samples in stream order, before the ensure_goal tail does. */
MPFMT_API int32_t mpfmt_sample_free(mpfmt_ctx* ctx, uint64_t seed, int64_t N, const double* init, int32_t goal_kind,
                          const double* goal_params, int32_t goal_ct, double* X_out, int64_t* attempts);
MPFMT_API int32_t mpfmt_sample_free_biased(mpfmt_ctx* ctx, uint64_t seed, int64_t N, const double* init, int32_t goal_kind,
                                 const double* goal_params, int32_t goal_ct, double goal_bias, double* X_out, int64_t* attempts);

/* ---- double-integrator (LinearQuadratic quasi-metric) space: DoubleIntegrator(m; vmax, r=rho)
 *      (src/statespaces/linearquadratic.jl:46-53).  Samples are states (p, v) in R^{2m} (upload_samples with
 *      d = 2m); obstacles live in the workspace (first m coordinates, OutputMatrix C = [I 0], :51-52), so
 *      upload_boxes takes dw = m and the 2m state-space bounds (lo, -vmax..; hi, +vmax..).
 *      di_graph_count/fill : helper_data_structures(V, M::LinearQuadratic) = all-pairs steer_pairwise
 *             (:68-77,196-225): sparse cost matrix Dmat, entry (i -> j) kept when cost(i -> j) <= r.
 *             CSC: column j lists the sources i (ascending, 1-based) = DSB (backward sets, nearB);
 *             DSF (forward sets) is its transpose.  nzval = cost, tval = optimal time t* (the duration of the
 *             DurationAndTargetControl of :222-224; pass NULL to skip).
 *      di_graph_edges_free : entry e (row y -> column x): is_free_motion(V[y], V[x], CC, SS) with the 5
 *             collision waypoints x(v, w, t*, s), s = linspace(0, t*, 5) (:85-88; src/statespaces.jl:153-158).
 *             nseg[e] (may be NULL) = workspace segment tests the reference would have made for that edge
 *             (its CC.count increments, boxesND.jl:26), so collision_checks can be reproduced.
 *      di_steer : batch steer(L, x0, x1, r) -> (cost, t*) (:191-195) on explicit pairs, X0/X1 = 2m x n col-major.
 *      di_fmtstar : fmtstar! (src/planners/fmt.jl:3-119) over that graph; POINT goal = StateGoal (exact state,
 *             src/goals.jl:128-131), RECT/BALL act on the workspace coordinates. */
MPFMT_API int32_t mpfmt_di_graph_count(mpfmt_ctx* ctx, double rho, double r, int64_t* colptr, int64_t* nnz);
MPFMT_API int32_t mpfmt_di_graph_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval, double* tval);
MPFMT_API int32_t mpfmt_di_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask, uint8_t* nseg);
MPFMT_API int32_t mpfmt_di_steer(mpfmt_ctx* ctx, const double* X0, const double* X1, int64_t n, int32_t m, double rho, double r,
                       double* cost, double* topt);
/* The same graph and edge bits with every output left in HBM (the device-resident form of helper_data_structures,
 * linearquadratic.jl:68-77,196-225, + the per-edge is_free_motion of src/statespaces.jl:153-158): count, fill and -- when an obstacle
 * set is uploaded -- the 5-waypoint sweep, one host synchronisation at the end.  Pointers (device addresses, valid until the next
 * build on the ctx): colptr int64[N+1] 0-based, rowval int32[nnz] 0-based ascending per column, nzval / tval double[nnz],
 * free_mask uint64[ceil(nnz/64)] and nseg uint8[nnz] (NULL without a sweep). */
MPFMT_API int32_t mpfmt_di_graph_step_device(mpfmt_ctx* ctx, double rho, double r, int64_t* nnz);
MPFMT_API int32_t mpfmt_di_graph_device_ptrs(mpfmt_ctx* ctx, void** colptr, void** rowval, void** nzval, void** tval, void** free_mask, void** nseg);
MPFMT_API int32_t mpfmt_di_fmtstar(mpfmt_ctx* ctx, double rho, double r, int64_t init_idx, int32_t checkpts,
                         int32_t goal_kind, const double* goal_params,
                         int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);
/* DIAGNOSTIC, for tests of the matrix-core candidate test of the double-integrator build (option "di_path"); no planner needs it.
 * On the resident samples (64 <= N <= 1024, state dimension 2 or 4) it computes the threshold and builds the fp16 operands exactly as
 * the build does, forms the fragments and the matrix-core instructions of the pair kernel through the kernel's own helpers, and
 * returns every accumulator: acc float[npad][npad], row = target, column = source, npad = N rounded up to 64 (rows / columns >= N are
 * pad states), entry = Q(source -> target) - T as the matrix core delivered it (the pair kernel keeps a pair when its entry is
 * negative).  opsT / opsS: uint16[npad][16], the fp16 bit patterns of the target- and source-role operands.  terms:
 * double[MPFMT_DI_MF_PROBE_TERMS] = sp, sv, pc[0], pc[1], split term, accumulation term, E, T, negT, usable (0 / 1), Pm, Vm, F, G, N0,
 * guards (bit 0 arguments, 1 finite box, 2 fp16 range, 3 E small against 1 / rho) -- written even when the call then fails with
 * MPFMT_ERR_ARG because the prefilter does not apply.  A resident steering graph is dropped (the operand buffer is rewritten). */
#define MPFMT_DI_MF_PROBE_TERMS 16
MPFMT_API int32_t mpfmt_di_mf_probe(mpfmt_ctx* ctx, double rho, double r, float* acc, uint16_t* opsT, uint16_t* opsS, double* terms,
                                    int64_t* npad);


/* ---- device-resident forms (bench / multi-GPU: no PCIe in the timed region) -----------------------
 * graph_build_device: count+fill on the device only; outputs stay in HBM.  Returns nnz.
 * graph_sweep_device: per-edge free mask of the resident graph into HBM.
 * Pointers to the resident arrays (device addresses, valid until the next build / ctx destroy):
 *   colptr int64[N+1] 0-based offsets, rowval int32[nnz] 0-based, nzval double[nnz], free uint64[ceil(nnz/64)]. */
MPFMT_API int32_t mpfmt_graph_build_device(mpfmt_ctx* ctx, double r, int64_t* nnz);
MPFMT_API int32_t mpfmt_graph_sweep_device(mpfmt_ctx* ctx);
/* graph_step_device: graph_build_device + graph_sweep_device as ONE call with one host synchronisation -- the planner's
 * whole step (fmt.jl:70-75's neighbour sets and edge checks for every sample).  The two-call form needs the host between
 * its kernels (nnz sizes the CSC and the mask).  When the previous step of the same (N, r, shard) took the single-pass
 * path, this call trusts its sizes, issues every kernel back to back, lets a device flag void the kernels after a capacity
 * that did not hold, validates after the synchronisation and transparently redoes the step the careful way if needed.
 * Results are identical to the two-call form and complete in HBM when the call returns (graph_sweep_device, by contrast,
 * only enqueues its kernel on the ctx's stream). */
MPFMT_API int32_t mpfmt_graph_step_device(mpfmt_ctx* ctx, double r, int64_t* nnz);
/* The same step in two calls, for ONE host thread that drives several ctxs (a Julia process holding one ctx per GPU, SURVEY
 * 8e): _launch issues the step's kernels and returns without waiting when the previous step's sizes can be trusted (otherwise
 * it runs the careful form to completion), _finish makes the one synchronisation, validates and repairs.  graph_step_device
 * = _launch + _finish. */
MPFMT_API int32_t mpfmt_graph_step_launch(mpfmt_ctx* ctx, double r);
MPFMT_API int32_t mpfmt_graph_step_finish(mpfmt_ctx* ctx, int64_t* nnz);
MPFMT_API int32_t mpfmt_graph_device_ptrs(mpfmt_ctx* ctx, void** colptr, void** rowval, void** nzval, void** free_mask);
/* The graph and mask a step left resident, to the host in the format of mpfmt_rdisc_count / _fill / mpfmt_graph_edges_free -- colptr[N+1]
 * and rowval[nnz] 1-based Int64, nzval[nnz], mask[(nnz+63)/64] BitVector chunks (mask may be NULL) -- WITHOUT rebuilding or re-sweeping:
 * the drop-in precompute! of julia/MPFmtHIP.jl is mpfmt_graph_step_device + this call, after which the unmodified fmtstar!
 * (src/planners/fmt.jl:68-90) reads ImmutableNNC columns (src/nearneighbors.jl:23-27,128) and answers is_free_motion from the mask.
 * Index conversion runs on the device ahead of two copy streams; *gb_per_s (may be NULL) reports the rate.  The copies run at link
 * speed when the destinations are page-locked: mpfmt_pinned_alloc hands out such memory (Julia wraps it with unsafe_wrap /
 * pointer_to_array, own = false, and returns it with mpfmt_pinned_free). */
MPFMT_API int32_t mpfmt_graph_export(mpfmt_ctx* ctx, int64_t* colptr, int64_t* rowval, double* nzval, uint64_t* mask, double* gb_per_s);
MPFMT_API int32_t mpfmt_pinned_alloc(int64_t bytes, void** out);
MPFMT_API int32_t mpfmt_pinned_free(void* p);
/* Page-locking is the expensive part of a page-locked export (hipHostMalloc: ~0.2 s per GB, several times the copy it speeds up), so the
 * ctx keeps ONE page-locked arena for it: grow-only, valid until it has to grow or the ctx is destroyed (mpfmt_ctx_destroy frees it).
 * mpfmt_export_arena returns at least `bytes` of it.  mpfmt_graph_export_pinned is mpfmt_graph_export into that arena: it returns the
 * four arrays (64-byte aligned; *mask may be asked for or NULL; *nnz_out their length) -- the memory behind the SparseMatrixCSC of
 * ImmutableNNC(D, r) (src/nearneighbors.jl:23-28) and the BitVector of free edges in julia/MPFmtHIP.jl hip_precompute_step!, which
 * every later call of the same ctx reuses: the second graph of a problem costs the copy alone.  The arrays are overwritten by the
 * next export of this ctx -- and FREED by one that needs a larger arena (a graph with more entries): pointers of an earlier export
 * must be dropped before the call (julia/MPFmtHIP.jl re-wraps them after every export).  A call that fails on the ctx's state (no
 * resident graph, mask asked for but not swept) leaves the arena and the earlier export untouched. */
MPFMT_API int32_t mpfmt_export_arena(mpfmt_ctx* ctx, int64_t bytes, void** out);
MPFMT_API int32_t mpfmt_graph_export_pinned(mpfmt_ctx* ctx, int64_t** colptr, int64_t** rowval, double** nzval, uint64_t** mask,
                                            int64_t* nnz_out, double* gb_per_s);

/* ---- streaming r-disc: per-column reductions WITHOUT the stored graph.  BASELINE configs[2] at the radius of src/planners/fmt.jl:39
 *      (R^12, N = 1e6: ~4 700 neighbours per sample, 57 GB of CSC) cannot keep ImmutableNNC resident; what the loop body
 *      src/planners/fmt.jl:70-82 needs of column x is a reduction over inball(x) (src/nearneighbors.jl:179-183):
 *        deg[x]      = |inball(x)|                                        (PRM*-style degree; *nnz = their sum)
 *        parent[x]   = argmin over y in inball(x), y in H, of C[y] + d(y, x), FIRST minimum in ascending y (findmin, fmt.jl:73),
 *                      1-based, 0 when no open neighbour; cost[x] = that minimum (Inf when none) -- C = NULL skips both;
 *                      H = NULL: every sample is open.  The caller then makes the ONE lazy edge test of fmt.jl:75 (mpfmt_edges_free).
 *        free_deg[x] = number of y in inball(x) with is_free_motion(V[y], V[x]) (src/statespaces.jl:153-158) when want_free != 0
 *      C: N doubles by sample index; H: BitVector chunks over the samples.  Outputs: N entries each, caller-owned.  Needs an
 *      unsharded ctx, d <= 12 and a radius the fp16 filter can take (the MFMA pair kernel does the work); membership and costs are
 *      the canonical fp64 arithmetic of every other entry point. ---------------------------------------------------------------- */
MPFMT_API int32_t mpfmt_rdisc_stream(mpfmt_ctx* ctx, double r, const double* C, const uint64_t* H, int32_t want_free,
                                     int64_t* deg, int64_t* free_deg, int64_t* parent, double* cost, int64_t* nnz);
/* Shard bookkeeping for the all-gather: column range (in the library's sorted order) and the number
 * of edges this shard produced. */
MPFMT_API int32_t mpfmt_shard_info(mpfmt_ctx* ctx, int64_t* col_begin, int64_t* col_end, int64_t* shard_nnz);

/* ---- wavefront solve: fmtstar! (src/planners/fmt.jl:3-119) with the dynamic-programming recursion ON THE DEVICE.
 *      mpfmt_fmtstar runs the loop fmt.jl:68-90 on one host core over GPU-built arrays; here W / H / C / A live in HBM and
 *      one step expands a whole cost band of open nodes Z = { z in H : C[z] <= min_H C + band } with the loop body
 *      fmt.jl:70-82 evaluated for every z of the batch against the same (W, H, C), the deferred H update fmt.jl:83-84 per
 *      batch, and the stop test fmt.jl:68 on the batch (answer = goal node of lowest (cost, index)).  Edge checks are lazy
 *      like the reference's (is_free_motion only for the y_min of an examined x, fmt.jl:75); collision_checks counts them.
 *        flags & MPFMT_WF_SINGLE : the batch is the ONE lowest (cost, index) open node: every step is one iteration of the
 *              reference loop -- tree, costs, path, collision_checks identical to mpfmt_fmtstar / the sequential recursion.
 *        band > 0 : every step equals mpfmt_expand (the batch form of the loop body) on the same sets; the tree is a valid
 *              FMT* tree of the same graph whose cost can exceed the sequential one slightly (reported by the tests / bench).
 *        flags & MPFMT_WF_EAGER  : answer edge tests from the swept graph mask (mpfmt_graph_step_device) instead of testing
 *              lazily; forced for checkers without a lane-per-obstacle form here (2-D SAT world, non-identity workspace).
 *              Without the flag the mask is still USED when a step left one for this graph and obstacle set (an edge's bit is a
 *              pure function of the edge: tree, costs and collision_checks are the lazy loop's) -- never computed for the solve.
 *        flags & MPFMT_WF_LAZY   : test every asked-for edge against the obstacle set even when a mask is resident (measurements).
 *      mpfmt_fmtstar_wavefront = begin + steps until done + finish.  A / C / path may be NULL (skips the 12 N-byte copy).
 *      Step-wise form (tests, drivers that interleave other work): wf_begin, wf_step ... until info.done, wf_finish;
 *      wf_state copies the sets out (W, H as the next step will see them; A 1-based, 0 = none), wf_batch the z of the
 *      last step (1-based).
 *      Sharded ctx (mpfmt_set_shard / mpfmt_comm_create): every rank holds the whole (W, H, C, A) and the columns
 *      of its own samples; a step examines the rank's own unvisited samples and ONE all-gather per wavefront carries every
 *      rank's (x, y_min, c_min) connections (counts ride in the slot headers).  Without a communicator the same exchange is
 *      made by the caller: wf_step on every ctx, wf_triples from each, wf_commit of all of them to each. */
#define MPFMT_WF_SINGLE 1
#define MPFMT_WF_EAGER  2
#define MPFMT_WF_LAZY   4
typedef struct {
    int32_t done;              /* 0 running, 1 goal reached (:solved), 2 open set exhausted (:failed) */
    int32_t nz;                /* batch size of the last step */
    int32_t nx;                /* samples examined (fmt.jl:70-74) */
    int32_t nconn;             /* samples connected (fmt.jl:76-80), all ranks */
    int32_t ntrip;             /* connections found by this rank (sharded) */
    int64_t iters;             /* steps so far */
    int64_t checks;            /* edge checks so far (this rank) */
    double  cmin;              /* lowest open cost at the last step */
    int64_t tot_z, tot_x, tot_conn;   /* sums over the steps */
} mpfmt_wf_info;
MPFMT_API int32_t mpfmt_fmtstar_wavefront(mpfmt_ctx* ctx, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                                double band, int32_t flags, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res, mpfmt_wf_info* info);
MPFMT_API int32_t mpfmt_wf_begin(mpfmt_ctx* ctx, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                       double band, int32_t flags);
MPFMT_API int32_t mpfmt_wf_step(mpfmt_ctx* ctx, mpfmt_wf_info* info);
MPFMT_API int32_t mpfmt_wf_state(mpfmt_ctx* ctx, uint64_t* W, uint64_t* H, double* C, int64_t* A);
MPFMT_API int32_t mpfmt_wf_batch(mpfmt_ctx* ctx, int64_t* zs, int64_t cap, int64_t* nz);
MPFMT_API int32_t mpfmt_wf_triples(mpfmt_ctx* ctx, int64_t cap, int64_t* x, int64_t* y, double* c, int64_t* n);
MPFMT_API int32_t mpfmt_wf_commit(mpfmt_ctx* ctx, int64_t n, const int64_t* x, const int64_t* y, const double* c);
MPFMT_API int32_t mpfmt_wf_finish(mpfmt_ctx* ctx, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res);
/* mpfmt_dubins_fmtstar_wavefront / mpfmt_reedsshepp_fmtstar_wavefront : the car planners (simplecars.jl spaces) the same way. */
MPFMT_API int32_t mpfmt_dubins_fmtstar_wavefront(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                                       int32_t goal_kind, const double* goal_params, double band, int32_t flags, int64_t* A, double* C,
                                       int64_t* path, mpfmt_fmt_result* res, mpfmt_wf_info* info);
MPFMT_API int32_t mpfmt_reedsshepp_fmtstar_wavefront(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                                           int32_t goal_kind, const double* goal_params, double band, int32_t flags, int64_t* A, double* C,
                                           int64_t* path, mpfmt_fmt_result* res, mpfmt_wf_info* info);
/* mpfmt_di_fmtstar_wavefront : mpfmt_di_fmtstar with the recursion on the device: the double-integrator graph is directed, so
 *        the forward sets nearF (rows of the cost matrix, linearquadratic.jl:73) are transposed on the device and the edge
 *        answers come from the 5-waypoint sweep's mask and segment counts.  MPFMT_WF_SINGLE reproduces mpfmt_di_fmtstar exactly;
 *        A / C / path may be NULL. */
MPFMT_API int32_t mpfmt_di_fmtstar_wavefront(mpfmt_ctx* ctx, double rho, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind,
                                   const double* goal_params, double band, int32_t flags, int64_t* A, double* C, int64_t* path,
                                   mpfmt_fmt_result* res, mpfmt_wf_info* info);

/* ---- multi-GPU exchange: RCCL over xGMI behind the ABI.  The reference has no analogue (single thread,
 *      src/planners/fmt.jl); the exchange assembles on every GPU what the single process of the reference holds in one
 *      address space: the free bit of every graph edge (is_free_motion results, statespaces.jl:153-158) and, in the
 *      wavefront solve below, the connections of every wavefront (fmt.jl:76-80).
 *      comm_unique_id : 128-byte RCCL id; rank 0 obtains it, the host hands it to every rank (file, socket, Julia array).
 *      comm_create    : ncclCommInitRank on the ctx's device + mpfmt_set_shard(rank, world).  world = 1 is allowed.
 *      group_begin/end: ncclGroupStart / ncclGroupEnd, for ONE host thread that drives several ctxs (a Julia process
 *                       holding G handles): bracket the comm_create calls, and each round of *_launch calls, with them.
 *      allgather_free_mask : after mpfmt_graph_step_device on every rank -- one all-gather of the per-shard free-edge masks.
 *                       *gathered = device address of [world][*stride_words] uint64: per rank (mask words, nnz, then the
 *                       mask, zero padded); words_each / nnz_each [world] on the host (may be NULL).  Steady state is ONE
 *                       collective: the lengths ride in front of the payload and every rank derives the next capacity
 *                       from the lengths it saw (a shard that outgrew it makes every rank repeat at the exact size).
 *                       _launch / _finish split the call: the gather runs on the ctx's communication stream and overlaps
 *                       whatever is enqueued next (the following step's index build); cap_hint > 0 = capacity in words
 *                       the caller guarantees to be identical on all ranks (needed by a single-thread driver on the
 *                       first step, when the blocking lengths exchange would wait on a peer it has yet to launch).
 *                       _launch snapshots the rank's mask, so the next step may overwrite the ctx's mask before _finish.
 *                       Calls that may sit inside mpfmt_group_begin / _end: mpfmt_comm_create, mpfmt_allgather_free_mask_launch
 *                       (with cap_hint > 0 the first time) and _relaunch; _finish must come after mpfmt_group_end.  A ctx
 *                       launched inside a group never repeats a gather on its own (its peers hang off the same thread): _finish
 *                       returns MPFMT_RETRY on every ctx instead, the driver calls _relaunch for all of them in a group and
 *                       _finish again.  (Verified with the tests' RCCL stand-in, which defers collectives to the end of
 *                       the group like RCCL does; a multi-GPU box has not been available.)
 *                       MPFMT_RCCL_LIB (tests: a stand-in library) is honoured only with MPFMT_ALLOW_RCCL_OVERRIDE=1. */
#define MPFMT_COMM_ID_BYTES 128
MPFMT_API int32_t mpfmt_comm_unique_id(uint8_t* id128);
MPFMT_API int32_t mpfmt_comm_create(mpfmt_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id128);
MPFMT_API int32_t mpfmt_comm_destroy(mpfmt_ctx* ctx);
MPFMT_API int32_t mpfmt_group_begin(void);
MPFMT_API int32_t mpfmt_group_end(void);
MPFMT_API int32_t mpfmt_allgather_free_mask(mpfmt_ctx* ctx, void** gathered, int64_t* stride_words, int64_t* words_each, int64_t* nnz_each);
MPFMT_API int32_t mpfmt_allgather_free_mask_launch(mpfmt_ctx* ctx, int64_t cap_hint);
MPFMT_API int32_t mpfmt_allgather_free_mask_finish(mpfmt_ctx* ctx, void** gathered, int64_t* stride_words, int64_t* words_each, int64_t* nnz_each);
MPFMT_API int32_t mpfmt_allgather_free_mask_relaunch(mpfmt_ctx* ctx);

/* ---- measurement: average device milliseconds per launch of a named kernel group since the last
 *      reset, measured with HIP events on the launch stream.  names: "rdisc_count", "rdisc_fill",
 *      "rdisc_sort", "grid", "sweep_graph" (mask preset + round table + kernel), "sweep_kernel" (the round-table sweep kernel alone),
 *      "pair_kernel" (the pair kernel alone), "exact_pairs" (k_exact_pairs, edge-test form 2),
 *      "sweep_points", "sweep_edges", "expand". */
MPFMT_API int32_t mpfmt_timing_reset(mpfmt_ctx* ctx);
MPFMT_API int32_t mpfmt_timing_get(mpfmt_ctx* ctx, const char* name, double* avg_ms, int64_t* launches);
/* Tuning / test knobs.  "rdisc_path": 0 = auto, 1 = exact fp64 VALU pair kernel, 2 = fp16 MFMA distance-matrix
 * filter + exact fp64 refine (both give bit-identical graphs).  "timing": 0/1 event timing off/on.
 * "sweep_rounds" (default 1): round-table sweep kernel where it applies
 * (d <= 8, at most 256 boxes), 0 = the task-header kernel everywhere.  Same mask bits either way.
 * "rdisc_half" (default 1): the single-pass build tests every pair of the ctx's own samples once and writes the hit records
 * of both columns (same CSC bit for bit; a build that overflows its logs is counted again whole).
 * "fuse_broad" (default 2): in mpfmt_graph_step* on such a build (AABB checker in the state space's own coordinates, d <= 6,
 * <= 256 boxes, every sample inside the state space) the edge tests ride in the graph kernels: 2 = broad phase in the pair
 * kernel, slab tests of the flagged pairs before the columns are ordered, the ordering pass writes the mask; 1 = flagged entries
 * tested after the ordering; 0 = the separate sweep kernel.  Same graph and mask bits in every combination; a sweep called on
 * its own (mpfmt_graph_sweep_device, mpfmt_graph_edges_free) is always the whole sweep.
 * "di_path" (default 0 = auto): the double-integrator build's candidate test on the vector ALUs (1) or as an fp16 bilinear form on the
 * matrix cores in front of the same fp64 tests (2; workspace dim <= 2 and a threshold the fp16 error bound leaves meaningful); same graph.
 * "wf_graphs" (default 0): a measured alternative kept for the record (LABNOTES.md).
 * "mf_target_items" (default 40000): work items (tile x slice of its chunk list, one wavefront each) the MFMA pair kernel aims for; the
 * slice count is made odd.  "mf_xcd_mode" (default -1 = by launch size): items reach the XCDs in interleaved groups of this many
 * (0 = one contiguous range per XCD, 1 = round robin).  "cell_fb_max" (default 8): position bits inside a cell that the cell sort's key
 * carries.
 * "overlap" (default 1): the step runs its per-sample obstacle masks and the counter fill beside the chunk lists, and the degree count,
 * its scan, the mask preset and the capacity check beside the exact pair tests, on a second (lowest-priority) stream of the ctx forked
 * and joined with events -- from 65536 samples on (smaller steps are shorter than the events' latencies); 2 = always; 0 = every kernel
 * on the ctx's stream.  "ord_draw" (default 1): the ordering kernel's workgroups draw their
 * quarter tiles from per-XCD counters when a quarter holds >= 1536 records on average; 2 = always; 0 = every nb-th quarter each.  "mf_tail_slices" / "mf_tail_permille" / "mf_tail_min_items"
 * (defaults 9 / 80 / 32768): the last permille of a single-pass launch's tiles are cut into that many (odd) slices instead of the
 * launch's own, in launches of at least that many items.  "index_halo" / "shard_blocks" (default 1 / 1, sharded ctxs): the index is
 * built for the shard's tiles and their neighbour cells only; cell ids are block-major so that a shard is a compact block.
 * "wf_pos_space" (default 1): the device solve keeps its sets a second time by cell-sorted position from the SECOND solve on a graph on
 * (2: from the first, 0: never).
 * "steer_shapes_delta" (default 0): 1 = mpfmt_shapes2d_add / _remove under a filled and swept steering graph bring its mask and
 * segment counts up to date in place (the table at mpfmt_shapes2d_add) instead of invalidating them; the mask and counts
 * any later sweep writes are the same whatever its value.  mpfmt_get_stat "steer_shapes_delta" reads it back.
 * "samples_add_keeps_fields" (default 0): 1 = an in-place mpfmt_samples_add / _device carries the tracked cost-to-come and cost-to-go
 * fields instead of dropping them ("growing the sample set"); graph and mask are the same whatever its value.
 * Tuning knobs only: the graph and the masks are the same bit for bit whatever their values.
 * "debug_small_lists": test knob, shrinks the pending lists of the fused edge tests so that their overflow path runs. */
MPFMT_API int32_t mpfmt_set_option(mpfmt_ctx* ctx, const char* name, int64_t value);
/* Counters of the last graph build: "rdisc_path_used", "pairs_tested", "survivors" (pairs that passed the
 * MFMA filter), "nnz", "slices", "cells", "rdisc_half_used", "pool_used", "drains" / "drain_boxes" (drains of the pair kernel that
 * ran the broad phase's box walk, and the boxes they walked in all; 0 where the drain held no broad phase); of the last step's edge tests: "sweep_form"
 * (0 / 1 / 2 as "fuse_broad"), "pair_items" (pairs listed for the exact tests; a synchronising read); diagnostics: "redo_count" /
 * "redo_reason" (builds redone since the ctx was made and why: 1 a chunk list was cut, 2 a log overflowed, 4 a column too long for the
 * ordering pass, 8 more entries than allocated, 16 the pending-pair list was cut), "qcap" (records a quarter log holds), "ord_per_cu"
 * (ordering-pass workgroups per CU), "filter_valu" (1: the last single-pass build filtered with the exact fp64 test on the vector ALUs),
 * "wf_pos_space_used" (1: the last device solve gathered by cell-sorted position), "list_cap" / "list_max" / "list_q<permille>" / "list_argmax" / "list_sum" (chunk-list lengths of
 * the last list build; synchronising reads); of the last k-nearest build: "knn_pairs_tested" (sample pairs distance-tested, counted once
 * per column and round -- the passes of the selection evaluate them again), "knn_rounds" (candidate rounds run, the first included),
 * "knn_short_columns" (columns the first round left to a later one), "knn_scan_columns" (columns answered by the scan of all samples).
 * Timers of that build (mpfmt_timing_get): "knn_candidates" (cell-sorted index + tile boxes), "knn_select" (the rounds), "knn_mutual". */
MPFMT_API int32_t mpfmt_get_stat(mpfmt_ctx* ctx, const char* name, int64_t* value);
/* work counters of the last graph build: candidate pairs distance-tested, tiles, slices. */
MPFMT_API int32_t mpfmt_graph_stats(mpfmt_ctx* ctx, int64_t* pairs_tested, int64_t* tiles, int64_t* slices, int64_t* cells);

#ifdef __cplusplus
}
#endif
#endif /* MPFMT_H */
