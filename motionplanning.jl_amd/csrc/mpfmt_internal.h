// Internal declarations shared by the translation units of libmpfmt.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <functional>
#include <string>
#include <map>
#include <utility>
#include <vector>
#include "../../include/mpfmt.h"
#include "mpfmt_host.h"

#define MPFMT_WAVE 64           // CDNA wavefront width; tile of samples = one wavefront of queries
#define MPFMT_MAXS 16           // max candidate slices per tile

struct mpfmt_timer {
    double total_ms = 0.0;
    int64_t launches = 0;
};

// Geometry of the uniform cell grid that bins the samples for one radius (host copy; passed by value
// to kernels).  Cells are at least r wide in every gridded dimension, so the neighbours of a point in
// cell c lie in cells c-1..c+1.
// Cell ids.  Unsharded: row-major with the LAST dimension fastest, so a run of cells along that dimension is a contiguous
// range of the cell-sorted sample array.  Sharded (world > 1): BLOCK-MAJOR -- the leading nsplit axes are cut in two at a cell
// boundary (cells [0, split) | [split, g)), the id's most significant digits say which half of each cut axis a cell lies in
// (axis 0 first), and inside such a half-block the order is the row-major one above.  An index range of the cell-sorted order
// is then a compact block of space (0.5^3 x 1^3 at 8 shards in R^6) instead of a slab thinner than r, which is what decides
// how many edges join two shards.  The last axis is never cut (runs along it stay contiguous); a cut axis with an odd cell
// count leaves holes in the id range (ids of cells that do not exist: empty).
struct mpfmt_grid {
    int32_t gd;                          // dims are all gridded; g[i] == 1 means "not split"
    int32_t g[MPFMT_MAX_DIM];            // cells per dimension
    double  lo[MPFMT_MAX_DIM];           // lower corner of the sample bounding box
    double  w[MPFMT_MAX_DIM];            // cell width
    double  inv_w[MPFMT_MAX_DIM];
    int64_t stride[MPFMT_MAX_DIM];       // id stride per dimension inside a half-block
    int32_t split[MPFMT_MAX_DIM];        // 0: the axis is not cut; else the first cell of its upper half
    int32_t ext[MPFMT_MAX_DIM];          // cells per dimension of a half-block's id range (split, or g when not cut)
    int64_t hstride[MPFMT_MAX_DIM];      // id offset of the upper half of a cut axis
    int32_t nsplit;                      // cut axes (the leading ones: 0 .. nsplit-1)
    int64_t inner;                       // ids per half-block
    int64_t ncells;                      // id range = inner << nsplit
};
// cell coordinate of x along one axis, clamped to [0, g - 1]: THE binning rule -- the cell sort and every kernel that looks for a sample's
// cell (pair kernels, single queries, external states) share this one definition
__host__ __device__ __forceinline__ int mpfmt_cell_of(double x, double lo, double inv_w, int g)
{
    double f = floor((x - lo) * inv_w);
    int c = (int)f;
    if (!(f >= 0.0)) c = 0;
    if (f >= (double)g) c = g - 1;
    return c;
}
// contribution of cell coordinate c of axis i to the cell id
__host__ __device__ __forceinline__ int64_t mpfmt_cell_term(const mpfmt_grid& G, int i, int c)
{
    const int s = G.split[i];
    return (s > 0 && c >= s) ? G.hstride[i] + (int64_t)(c - s) * G.stride[i] : (int64_t)c * G.stride[i];
}
// cell coordinate of axis i out of a cell id (may be >= g[i] for a hole of the block-major id range)
__host__ __device__ __forceinline__ int mpfmt_cell_coord(const mpfmt_grid& G, int i, int64_t id)
{
    const int64_t in = id % G.inner;
    int c = (int)((in / G.stride[i]) % G.ext[i]);
    if (G.split[i] > 0 && ((id / G.hstride[i]) & 1)) c += G.split[i];
    return c;
}

struct mpfmt_boxes_dev {                 // obstacle set in HBM: [M][2][dw] (lo then hi per box)
    const double* lohi;
    int32_t M;
    int32_t dw;
};

struct mpfmt_ss {                        // BoundedStateSpace bounds (statespaces.jl:29-34)
    int32_t has;
    int32_t d;
    double lo[MPFMT_MAX_DIM];
    double hi[MPFMT_MAX_DIM];
};

// 2-D SAT world (kernels_sat2d.hip): a Circle or a convex Polygon with the fields the predicates read
#define MPFMT_MAX_POLY 16
struct mpfmt_shape2d {
    int32_t kind, n;
    double c[2], r;
    double xr[2], yr[2];
    double pts[MPFMT_MAX_POLY][2], normals[MPFMT_MAX_POLY][2], nex[MPFMT_MAX_POLY][2];
};
struct mpfmt_aabb2d { double xr[2], yr[2]; };

struct mpfmt_ctx;
struct mpfmt_wf;                         // kernels_wavefront.hip
struct mpfmt_comm;                       // mpfmt_comm.hip
struct mpfmt_timer_state;                    // mpfmt_capi.hip
int32_t mpfmt_fail(mpfmt_ctx* ctx, int32_t code, const char* fmt, ...);

// An owning buffer: one pointer, its capacity in bytes, and a destructor.  PINNED = false: device memory; true: page-locked host
// memory.  Whoever holds one of these owns the allocation; a raw pointer member is a view into somebody else's.
template <class T, bool PINNED> struct mpfmt_buf {
    mpfmt_buf() = default;
    mpfmt_buf(const mpfmt_buf&) = delete;
    mpfmt_buf& operator=(const mpfmt_buf&) = delete;
    mpfmt_buf(mpfmt_buf&& o) noexcept { swap(o); }
    mpfmt_buf& operator=(mpfmt_buf&& o) noexcept { swap(o); return *this; }
    ~mpfmt_buf() { reset(); }
    void swap(mpfmt_buf& o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); }
    void reset()
    {
        if (p_) { if (PINNED) hipHostFree(p_); else hipFree(p_); }
        p_ = nullptr; bytes_ = 0;
    }
    // grow-only, exact size (no slack), contents NOT kept across a reallocation; 0 bytes asks for 16.  A failed allocation leaves
    // the buffer empty.
    int32_t ensure(mpfmt_ctx* ctx, size_t bytes)
    {
        if (bytes == 0) bytes = 16;
        if (p_ && bytes_ >= bytes) return MPFMT_OK;
        reset();
        void* q = nullptr;
        const hipError_t e = PINNED ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
        if (e != hipSuccess)
            return mpfmt_fail(ctx, MPFMT_ERR_HIP, "%s of %zu bytes failed: %s", PINNED ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
        p_ = (T*)q; bytes_ = bytes;
        return MPFMT_OK;
    }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};
template <class T> using mpfmt_dbuf = mpfmt_buf<T, false>;      // device
template <class T> using mpfmt_hbuf = mpfmt_buf<T, true>;       // page-locked host

// temporaries of one ABI call: device buffers freed on every exit path
struct mpfmt_tmp {
    std::vector<void*> p;
    mpfmt_tmp() = default;
    mpfmt_tmp(const mpfmt_tmp&) = delete;
    mpfmt_tmp& operator=(const mpfmt_tmp&) = delete;
    ~mpfmt_tmp() { for (void* q : p) hipFree(q); }
    template <class T> hipError_t get(T** out, size_t bytes)
    {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
        if (e == hipSuccess) { p.push_back(q); *out = (T*)q; }
        return e;
    }
};

// the steering graph resident in a ctx (kernels_di.hip, kernels_car.hip)
enum mpfmt_steer : int32_t { MPFMT_STEER_DI = 1, MPFMT_STEER_DUBINS = 2, MPFMT_STEER_REEDSSHEPP = 3 };

struct mpfmt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    // A second stream for the two kernels of a step that have nothing to wait for on the first but one predecessor: the per-sample obstacle
    // masks (beside the chunk lists) and the flagged pairs' exact tests (beside the logs' degree count and its scans).  Forked and joined
    // with events; side_pending: work is in flight there that ctx->stream has not waited for yet.
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool side_pending = false;
    int64_t preset_entries = -1;         // speculative step: the mask's trusted capacity, for the preset beside the exact pair tests
    int64_t mask_preset_words = -1;      // words of graph_free preset to ones ahead of mpfmt_order_logs (-1: none)
    bool masks_early = false;            // this build's sample masks were launched beside its chunk lists
    int32_t overlap = 1;                 // option: 1 = the side stream from 65536 samples on, 2 = always, 0 = every kernel of the step on ctx->stream
    hipStream_t copy_stream[2] = {nullptr, nullptr};      // mpfmt_graph_export: two device-to-host streams and their hand-over events
    hipEvent_t ev_conv[2] = {nullptr, nullptr}, ev_copy[2] = {nullptr, nullptr};
    mpfmt_hbuf<void> export_arena;        // page-locked host memory of mpfmt_graph_export_pinned (grow-only, lives as long as the ctx)
    std::string err;
    int rank = 0, world = 1;

    // ---- samples -------------------------------------------------------------------------------
    int64_t N = 0;
    int32_t d = 0;
    mpfmt_dbuf<double> Xo;                // [N][d] original order (AoS = the caller's layout)
    mpfmt_dbuf<double> Xo_next;           // where an upload lands: changes places with Xo once the set has been accepted (a refused set leaves the ctx as it was)
    double bb_lo[MPFMT_MAX_DIM], bb_hi[MPFMT_MAX_DIM];
    mpfmt_dbuf<void> bb_dev;              // mpfmt_upload_samples_device: per-block partial boxes, and their pinned host mirror
    mpfmt_hbuf<void> bb_host;

    // ---- cell grid for radius grid_r --------------------------------------------------------------
    double grid_r = -1.0;
    mpfmt_grid grid;
    int64_t ntiles = 0;                  // ceil(N/64)
    mpfmt_dbuf<int32_t> perm;             // [ntiles*64] sorted position -> original index (pad = -1)
    mpfmt_dbuf<int32_t> iperm;            // [N] original index -> sorted position
    mpfmt_dbuf<uint32_t> cellkey;         // [N] cell id of each sorted position
    // one arena, one fill per index build: cellstart [ncells + 1] (the cells' counters, scanned in place) | list_max (longest chunk list,
    // k_chunk_lists) | tileneed [ntiles] bytes
    mpfmt_dbuf<void> idx_arena;
    int32_t* cellstart = nullptr;        // view: [ncells+1] (inside idx_arena)
    int32_t* list_max = nullptr;         // view: (inside idx_arena)
    mpfmt_dbuf<int32_t> cellcnt_pad;      // block-major ids (sharded ctx): the cell counters of the count pass, one per 64-byte line (kernels_rdisc.hip)
    bool list_max_clean = false;         // zeroed by the index build's fill and not written since
    // sharded ctx on the matrix-core path: only the tiles this rank reads are built -- its own and the halo (the tiles of the cells next
    // to its own cells); tileneed [ntiles] marks them (nullptr: the index is whole)
    uint8_t* tileneed = nullptr;         // view: tileneed_buf or nullptr
    uint8_t* tileneed_buf = nullptr;     // view: (inside idx_arena)
    int32_t index_halo = 1;              // option: allow the shard + halo index
    int32_t shard_blocks = 1;            // option: block-major cell ids on a sharded ctx (0: row-major -- shards are slabs; measurements)
    int index_rank = 0, index_world = 1; // the shard the index was built for
    std::vector<double> cut_frac;        // shard boundaries as fractions of the cell-sorted order (cut_key: the geometry they belong to)
    std::vector<int64_t> cut_key;
    mpfmt_dbuf<double> Xt;                // [ntiles][d][64] tiled SoA, cell-sorted, NaN padded
    mpfmt_dbuf<double> tile_lo;           // [ntiles][d] tight bounding box of each tile
    mpfmt_dbuf<double> tile_hi;
    mpfmt_dbuf<double> tile_sub;          // [ntiles][4][d] two sub-boxes per tile (k_tile_bbox)
    mpfmt_dbuf<float> tile_sub32;         // the same boxes in fp32, rounded outward: the candidate side of the chunk-list test (half the bytes)

    // ---- r-disc graph (device resident) ------------------------------------------------------------
    double graph_r = -1.0;
    bool graph_counted = false, graph_filled = false;
    int32_t S = 1;                       // candidate slices per tile
    int64_t tile_begin = 0, tile_end = 0;  // shard tile range
    mpfmt_dbuf<int32_t> slice_cnt;        // [S][ntiles*64] hits per (slice, sorted query)
    mpfmt_dbuf<int64_t> deg;              // [N+1] degree by original index
    mpfmt_dbuf<int64_t> degs;             // [npad+1] degree by sorted position
    mpfmt_dbuf<int64_t> tptr;             // [npad+1] offsets of the sorted-order staging CSC (rowtmp/valtmp)
    bool tptr_valid = false;             // tptr holds the scan of the counted graph's degs (the single-pass build leaves it undone)
    // MFMA filter path (kernels_rdisc_mfma.hip)
    mpfmt_dbuf<double> Xs;                // [npad][d] cell-sorted AoS fp64 (NaN padded): exact refine gathers
    mpfmt_dbuf<void> ops;                 // [npad] 16 fp16 slots (32 B) per sorted sample: MFMA operands
    double mf_scale = 1.0;
    double ops_r = -1.0;                 // grid radius the operands were built for
    int32_t rdisc_path = 0;              // 0 auto, 1 exact fp64 VALU kernel, 2 MFMA filter + exact refine
    int32_t rdisc_path_used = 0;
    bool filter_valu = false;            // the counted graph's pair kernel ran the exact fp64 filter on the vector ALUs (k_rdisc_vf_w4) instead of the fp16 matrix-core one
    int32_t cell_fb_max = 8;             // position bits inside a cell that the sort key carries (k_cellkey)
    int64_t mf_tail_min_items = 32768;   // ... in launches of at least this many items (smaller ones do not fill the chip: nothing to even out)
    int32_t ord_draw = 1;                // option: 1 = the ordering kernel's workgroups draw their quarters when those are long (>= 1536 records on average), 2 = always, 0 = every nb-th quarter each
    int32_t mf_tail_permille = 80, mf_tail_slices = 9;      // options: the last tiles of a single-pass pair-kernel launch are cut into this many slices (0: off)
    int32_t mf_xcd_mode = -1;            // work items go to the XCDs in interleaved groups of this many; -1: 256 for launches of >= 32768 items, else 64
                                         // (north star: groups of 64 2.02 ms / 5.6 GB of counter traffic, 256 2.04 / 4.6, 512 2.05 / 4.4; one range per XCD 2.41 ms)
    int32_t num_cus = 256;               // compute units of the device (persistent-grid sizing)
    int ord_per_cu = 0;          // k_order_logs: resident workgroups per CU on THIS ctx's device
    mpfmt_dbuf<int> sweep_ctr;            // graph sweep: one task counter per obstacle chunk
    int32_t sweep_rounds = 1;            // option: round-table sweep (k_graph_sweep_rt) where it applies (d <= 8, M <= 256)
    mpfmt_dbuf<int64_t> rt_cnt;           // [columns visited + 1] rounds per column, then (scan) first round of each column
    mpfmt_dbuf<int64_t> rt_off;
    mpfmt_dbuf<void> rt_tmp;              // scan temporary
    mpfmt_dbuf<void> rt_table;            // [rounds] (column, entries | first << 31, first entry) in visiting order
    mpfmt_dbuf<int64_t> rt_total;         // device: number of rounds
    mpfmt_dbuf<double> rt_ss;             // device copy of the state-space bounds (lo[MAX_DIM], hi[MAX_DIM]) for scalar loads
    mpfmt_ss rt_ss_host;                 // what rt_ss holds
    bool rt_ss_valid = false;
    // "every sample lies in the state space" for (samples_epoch, ss): the sweep then skips the per-row in_state_space test
    int64_t samples_epoch = 0, ssflag_epoch = -1;
    mpfmt_ss ssflag_ss;
    bool ssflag_all_in = false;
    mpfmt_dbuf<int32_t> ssflag_dev;
    int64_t mf_target_items = 40000;     // work items (tile x slice) the MFMA path aims for (tools/run_shard_sweep_items.py: flat from 40k up at 1 shard, best at 2 and 4)
    float mf_negT = 0.f;
    mpfmt_dbuf<void> lists;               // [shard tiles][list_cap] candidate chunk ids per tile
    mpfmt_dbuf<int32_t> list_len;         // [shard tiles + 1] lengths, last = max
    mpfmt_dbuf<void> lists_stage;         // small shards with long lists: [tiles][4][list_cap] staging of the 4-wavefront list kernel
    int64_t list_cap = 0;
    double lists_r = -1.0; int64_t lists_begin = -1, lists_end = -1;
    // single-pass hit pool (MFMA path): hits found by the count pass are kept, so the fill pass is a scatter
    int32_t use_pool = 1;                // option "rdisc_pool"
    int64_t qcap = 0;                    // capacity of one quarter log, in records (a multiple of 16)
    mpfmt_dbuf<uint32_t> qkey;            // [quarter tiles of the shard][qcap] record keys: row sample index | column within the quarter << 26 | flags
    mpfmt_dbuf<double> qd2;               // [quarter tiles of the shard][qcap] squared distances
    const double* st_C = nullptr; const uint64_t* st_H = nullptr; int st_free = 0;      // streaming mode (mpfmt_rdisc_stream): inputs of the launch in flight
    mpfmt_dbuf<void> st_best; mpfmt_dbuf<int32_t> st_besti, st_nfree;                    //   and its per-slice partials [S][npad]
    mpfmt_dbuf<void> smask;               // [npad] per-sample obstacle masks (k_sample_masks: the boxes within r of the sample, Euclidean -- drain_cull.h): the drain's broad phase walks the boxes in (mask_q & mask_c) only
    int64_t pool_hint_qmax = 0;          // records in the fullest quarter (16 consecutive cell-sorted columns) of the last build: sizes the next one's logs
    // half build of the single-pass r-disc graph (kernels_rdisc_mfma.hip: every pair found once, the other column's record goes
    // to a foreign log of that column's tile)
    int use_half = 1;                    // option rdisc_half
    int fuse_broad = 2;                  // option: broad phase of the edge tests in the half build's drain (step APIs only)
    mpfmt_dbuf<void> pend_items;          // [segments][pend_wcap] (entry, column sample, row position) of the entries that need an exact test
    int64_t pend_wcap = 0;
    mpfmt_dbuf<int32_t> pend_cnt;         // [segments] items per segment, then the overflow flag
    int32_t* pend_over = nullptr;        // view: behind pend_cnt's segments
    int pend_nseg = 0;
    bool sweep_pending_used = false;     // the last graph sweep visited the pending list only
    bool pend_overflowed = false;        // read back behind the speculative step's synchronisation
    bool pend_valid = false;             // the resident graph has its pending list (made by this step's ordering pass)
    mpfmt_dbuf<void> pair_items;          // fuse_broad = 2: [items][pair_icap] 32-byte pending-pair items (k_exact_pairs)
    int64_t pair_icap = 0;
    int pair_slack = 1;                  // doubled (to 8) by a step whose pending-pair list overflowed
    bool sweep_in_order = false;         // the mask of the resident graph was written by the ordering pass (form 2)
    bool bits_in_records = false;        // this count's blocked edges are marked in the records (bit 31 of the row index)
    int debug_small_lists = 0;           // option (tests): pending lists of 8 items, so that their overflow path runs
    bool want_broad = false;             // set by the step APIs around their count
    bool broad_in_drain = false;         // this count's records carry the broad-phase flag (bit 30 of the row index)
    bool half_used = false;              // the counted graph was built that way
    int64_t redo_count = 0; int32_t redo_reason = 0;      // stats: builds redone because a capacity did not hold (1 chunk list cut, 2 log overflow, 4 column too long, 8 nnz beyond the allocation, 16 pending list cut)
    bool pool_skip_once = false;         // the next count runs in the two-pass form (a log of the single pass overflowed, or a column was too long)
    bool lists_half = false;             // the cached chunk lists hold only chunks >= the tile
    int cell_fb = 0;                     // position bits below the cell id in cellkey (k_cellkey)
    int64_t max_deg = 0;                 // longest column of the counted graph (k_degree)
    int32_t pool_slack = 1;              // doubled after a build whose slot lists overflowed
    bool pool_valid = false;             // pool holds exactly the nnz hits of the counted graph
    // speculative single-sync step (mpfmt_graph_step): capacities of the previous identical build are trusted, every kernel
    // after the count bails out on the device flag spec_fail, and the host validates once at the end
    bool spec_ready = false;             // the previous build of the same (N, r, shard) went through the single-pass pool path
    bool spec_lists = false;             // chunk lists of the pending count were built without reading back their maximum
    bool cnt_pool = false, cnt_mf = false;   // the pending count used the pool / the MFMA pair kernel
    mpfmt_dbuf<int32_t> spec_fail;        // device flag: pool overflow, truncated chunk list or nnz beyond the trusted capacity
    int64_t nnz_cap = 0;                 // entries rowval / nzval / the mask are sized for
    mpfmt_dbuf<void> rb_dev;              // count read-back block (device) and its pinned host mirror
    mpfmt_hbuf<void> rb_host;
    int64_t lists_cap_trusted = -1;      // list capacity that a verified build found sufficient
    int64_t pool_hint_N = -1; double pool_hint_r = -1.0; int64_t pool_hint_nnz = 0; int64_t pool_hint_maxdeg = 0; int pool_hint_rank = -1, pool_hint_world = -1;   // capacity hint from the last build
    int64_t survivors = 0;
    mpfmt_dbuf<int64_t> colptr;           // [N+1] 0-based offsets by original index
    int64_t nnz = 0;
    mpfmt_dbuf<int32_t> rowtmp;           // [nnz] unsorted fill
    mpfmt_dbuf<double> valtmp;
    mpfmt_dbuf<int32_t> rowval;           // [nnz] 0-based, ascending per column
    mpfmt_dbuf<double> nzval;
    mpfmt_dbuf<int32_t> rowpos;           // [nnz] cell-sorted position of each entry's row (single-pass build): the sweep gathers rows from Xs
    bool rowpos_valid = false;
    mpfmt_dbuf<uint64_t> graph_free;      // [ceil(nnz/64)]
    bool graph_swept = false;
    bool deg_zero_valid = false;         // sharded ctx: deg[] is all zeros (the ordering pass cleared what the last step wrote)
    // The small per-build counters.  Each is a VIEW: into zarena (one arena, one fill per build) when the ctx has one, else into the
    // _own buffer beside it (a ctx whose counters were first allocated one by one -- by the steering spaces' builds -- keeps them
    // and their separate fills).  Views are never freed; zarena and the _own buffers always are.
    mpfmt_dbuf<void> zarena;
    mpfmt_dbuf<unsigned long long> d_pairs_own;
    mpfmt_dbuf<int32_t> pool_flag_own, pair_cnt_own, qlen_own;
    unsigned long long* d_pairs = nullptr;   // view: [514] candidate pairs tested (512 sharded counters), longest column, fullest quarter
    int32_t* pool_flag = nullptr;        // view: the logs' overflow flag
    int32_t* pair_cnt = nullptr;         // view: [items] pending pairs per item, then the overflow flag
    int32_t* pair_over = nullptr;        // view: pair_cnt + 1024
    int32_t* qlen = nullptr;             // view: [quarter tiles of the shard] the logs' cursors
    int32_t* ord_ctr = nullptr;          // view: [8] the ordering kernel's per-XCD quarter counters (arena only)
    unsigned long long* d_dstat = nullptr;   // view: [512] 256 x {drains that ran the box walk, boxes they walked} sharded counters (arena only)
    int64_t pairs_tested = 0;
    int64_t drains = 0, drain_boxes = 0; // of the last count whose drain held the broad phase (stats "drains", "drain_boxes"); 0 otherwise

    // ---- k-nearest graph (kernels_knn.hip): installed in colptr / rowval / nzval like an r-disc graph, graph_r = its longest entry ----
    int64_t knn_k = 0;                   // > 0 with graph_filled: the resident graph is the k-nearest one of this k (never "a filled graph of radius graph_r")
    mpfmt_dbuf<uint64_t> knn_mutual;      // [ceil(nnz/64)] mutual bit per entry (row y in column x: x in knn(y))
    mpfmt_dbuf<double> knn_st;            // [2][supertiles][d] boxes of 64 consecutive tiles
    mpfmt_dbuf<void> knn_bitmap;          // [workgroups][ceil(N/64)] selection bitmaps
    mpfmt_dbuf<void> knn_lists;           // the rounds' short-column lists and counters
    int64_t knn_pairs = 0, knn_rounds = 0, knn_short = 0, knn_scan = 0;      // stats of the last build

    // ---- steering graphs (double integrator, Dubins, Reeds-Shepp): share colptr / rowval / nzval / graph_free ---------------
    mpfmt_steer steer_kind = MPFMT_STEER_DI;     // which steering graph the steer_* state describes
    double steer_r = 0.0;                // cost radius of the built graph
    bool steer_counted = false, steer_filled = false, steer_swept = false;
    mpfmt_dbuf<uint8_t> steer_nseg;       // [nnz] workspace segment tests the reference would have made per edge
    int32_t di_S = 1;
    double di_rho = 1.0;
    mpfmt_dbuf<int32_t> di_pool_i; mpfmt_dbuf<double> di_pool_c, di_pool_t;                   // DI single-pass slot lists
    int64_t di_pool_cap = 0; bool di_pool_valid = false;
    mpfmt_dbuf<void> di_ops;              // matrix-core prefilter of the double-integrator build (kernels_di_mfma.hip): target- and source-role operands
    bool di_mf = false; float di_negT = 0.f;     // the counted DI graph went through it; its threshold
    int32_t steer_shapes_delta = 0;      // option: 1 = shape edits under a swept steering graph update mask and counts in place
    int32_t di_path = 0;                 // option: 0 auto, 1 vector-ALU candidate test, 2 matrix-core prefilter
    double car_rt = 1.0, car_sp = 1.0;   // Dubins turning radius / speed of the built graph
    mpfmt_dbuf<uint64_t> car_keep;        // keep bits over the candidate (positions) graph
    mpfmt_ctx* aux = nullptr;            // helper ctx: Euclidean r-disc graph of the positions (Dubins build)
    mpfmt_dbuf<double> tvaltmp;           // [nnz] optimal times, unsorted staging
    mpfmt_dbuf<double> tval;              // [nnz] optimal times t* per entry

    // ---- obstacles -----------------------------------------------------------------------------
    mpfmt_dbuf<double> boxes;             // [M][2][dw]
    std::vector<double> boxes_host;      // the same on the host
    int32_t M = 0, dw = 0;
    bool have_boxes = false;
    int32_t cc_kind = 0;                 // collision checker: 0 = PointRobotNDBoxes, 1 = PointRobot2D (SAT)
    mpfmt_dbuf<mpfmt_shape2d> shapes2d;   // [M] when cc_kind == 1
    std::vector<mpfmt_shape2d> shapes_host;      // the same on the host
    mpfmt_aabb2d aabb2d;                 // Compound2D bounding box
    mpfmt_ss ss;
    // in-place edits of the box list (mpfmt_boxes_add / _remove, kernels_boxdelta.hip) and of the 2-D shape list (mpfmt_shapes2d_add /
    // _remove, kernels_shapedelta.hip): the flagged columns, their count and the
    // entries tested (device), and the stats of the last call
    mpfmt_dbuf<int32_t> bd_cols;          // [N]
    mpfmt_dbuf<unsigned long long> bd_ctr; // [2] flagged columns, entries that reached an exact test
    int32_t bd_path = 0;                 // 1: the resident mask was updated in place, 0: invalidated
    int64_t bd_columns = 0, bd_entries = 0;

    // ---- growth of the sample set (mpfmt_samples_add, kernels_grow.hip): the grown graph is built in these spare buffers, which change
    // places with colptr / rowval / nzval / graph_free once everything has succeeded (the ctx holds the graph twice at the peak)
    mpfmt_dbuf<int64_t> colptr_next;
    mpfmt_dbuf<int32_t> rowval_next;
    mpfmt_dbuf<double> nzval_next;
    mpfmt_dbuf<uint64_t> free_next;
    mpfmt_dbuf<void> grow_counts, grow_lists, grow_bytes;      // the call's temporaries (grow-only): counters and offsets | the new samples' lists | one byte per grown entry
    int32_t grow_path = 0;               // 1: the resident graph was grown in place, 0: invalidated
    int64_t grow_candidates = 0, grow_entries = 0, grow_dropped = 0;      // stats of the last call
    int64_t grow_flagged = 0;            // stat: the changed columns of the last in-place call (new | lost an entry | gained a row)
    int32_t grow_keeps_fields = 0;       // option "samples_add_keeps_fields": 1 = an in-place growth carries the tracked fields
    int32_t grow_carried = 0;            // stat: bit 0 the cost-to-come field, bit 1 the cost-to-go field was carried by the last call

    // ---- scratch -------------------------------------------------------------------------------
    mpfmt_dbuf<void> scratch;
    std::map<std::string, mpfmt_timer> timers;
    mpfmt_timer_state* timer_state = nullptr;      // HIP-event timing records of this ctx (mpfmt_capi.hip)
    bool timing_enabled = true;
    bool rebuild_index = false;          // option "rebuild_index": graph_build_device rebuilds the cell grid every call

    // ---- multi-GPU exchange (mpfmt_comm.hip) and the device-resident wavefront FMT* driver (kernels_wavefront.hip) ----
    mpfmt_comm* comm = nullptr;          // RCCL communicator + communication stream of this ctx
    int32_t step_state = 0; double step_r = 0.0;   // graph_step_launch / _finish: 0 none, 1 speculative kernels in flight, 2 complete
    int32_t wf_graphs = 0;               // option (off: measured, no gain -- the solve is bound by k_wf_connect, 3.2 of 5.4 ms, not by launches): replay a captured
                                         // hipGraph of a group of 8 steps instead of launching its ~48 kernels
    int32_t wf_pos_space = 1;            // option: the device solve gathers its sets by cell-sorted position from the second solve on a graph
                                         // on (0: always by caller index, 2: from the first solve -- measurements, tests)
    int64_t wf_seen_epoch = -1; double wf_seen_r = -1.0; int64_t wf_seen_nnz = -1;      // the graph the last device solve ran on
    int32_t wf_pos_used = 0;             // stat: the last device solve gathered by position
    int32_t wf_force_sharded = 0;        // option: run the sharded form of the wavefront step (own-column marking, triples, exchange) at world = 1
    mpfmt_wf* wf = nullptr;              // W / H / C / A and the batch lists of a running wavefront solve

    // ---- PRM* shortest-path field (kernels_sssp.hip): labels, parents, the three changed-sample bitmaps, round state, point bitmap ----
    mpfmt_dbuf<double> sssp_C;            // [N]
    mpfmt_dbuf<int64_t> sssp_A;           // [N] 1-based parents
    mpfmt_dbuf<uint64_t> sssp_bm;         // [3][ceil(N/64)]
    mpfmt_dbuf<void> sssp_state;          // sssp_state (device) and its pinned host mirror
    mpfmt_hbuf<void> sssp_state_host;
    mpfmt_dbuf<uint64_t> sssp_F;          // [ceil(N/64)] checkpts bitmap of the call
    hipEvent_t sssp_ev[2] = {nullptr, nullptr};
    int64_t sssp_rounds = 0, sssp_relax = 0, sssp_reached = 0;      // stats of the last source
    // cost-to-go (kernels_sssp_to.hip): G and S live in sssp_C / sssp_A, the ring in sssp_bm (+ a fourth bitmap: the targets)
    mpfmt_dbuf<unsigned long long> sssp_to_best;      // [N] successor pass 1: lowest bits(G[x]) among the exact achievers of y
    mpfmt_dbuf<int64_t> sssp_to_tgt;      // [ntgt] 1-based targets of the call
    mpfmt_dbuf<void> sssp_to_state;       // sssp_to_state (device) and its pinned host mirror
    mpfmt_hbuf<void> sssp_to_state_host;
    int64_t sssp_to_atomics = 0, sssp_to_entries = 0, sssp_to_columns = 0;      // stats of the last cost-to-go field

    // ---- adaptive shortcutting (kernels_shortcut.hip): stats of the last batch ----
    int64_t shortcut_tests = 0, shortcut_checks = 0;
    int64_t ssc_tests = 0, ssc_checks = 0;       // the same for the steering shortcut (kernels_steershortcut.hip)
    // ---- time discretisation (kernels_discretize.hip): stats of the last batch ----
    int64_t disc_steps = 0, disc_samples = 0;

    // ---- roadmap queries for external states (kernels_roadmap.hip, the seeded field of kernels_sssp.hip) ----
    mpfmt_dbuf<double> sssp_seed;         // [N] seed labels of the running pair query (+Inf: no usable edge from the start)
    int64_t roadmap_candidates = 0, roadmap_near_total = 0;      // stats of the last call
    int64_t steer_roadmap_steered = 0;    // exact steers run by the last call on a steering graph (steer_roadmap.h)

    // ---- many-source fields and cost matrices (kernels_sssp_multi.hip): buffers of their own, grow-only ----
    mpfmt_dbuf<double> ms_L;              // [N][64] labels, lane = source
    mpfmt_dbuf<int64_t> ms_A;             // [N][64] 1-based parents (only once parents were asked for)
    mpfmt_dbuf<uint64_t> ms_bm;           // [3][ceil(N/64)] changed-sample bitmaps
    mpfmt_dbuf<void> ms_state;            // ms_state (device) and its pinned host mirror
    mpfmt_hbuf<void> ms_state_host;
    mpfmt_dbuf<void> ms_stage;            // [64][min(N, 65536)] transposed chunk of the copy-out
    mpfmt_dbuf<int64_t> ms_src;           // [64] 0-based sources of the running group
    hipEvent_t ms_ev[2] = {nullptr, nullptr};
    int64_t ms_groups = 0, ms_rounds = 0, ms_rows = 0, ms_bytes = 0;      // stats of the last call

    // ---- tracked cost-to-come field (kernels_field.hip): buffers of its own that no other call writes ----
    // graph_epoch counts the graph builds (bumped wherever a graph becomes filled), sweep_epoch the whole sweeps of the mask (bumped wherever
    // graph_swept becomes true).  A tracked field belongs to one sample set and one graph identity (radius or k; an import drops it); it
    // keeps its delta history -- Ab and the dirty bitmap mean something -- only while neither a build nor a whole sweep intervened
    int64_t graph_epoch = 0, sweep_epoch = 0;
    bool graph_imported = false;         // the resident r-disc graph came through mpfmt_graph_import: its symmetry is the caller's word only
    mpfmt_dbuf<double> fld_C;             // [N] labels
    mpfmt_dbuf<int64_t> fld_A;            // [N] 1-based parents
    mpfmt_dbuf<int64_t> fld_Ab;           // [N] entry index of the parent edge (undefined where A == 0)
    mpfmt_dbuf<uint64_t> fld_bm;          // [4][ceil(N/64)]: dirty columns (the repair's "seen" set while it runs) | the ring of three
    mpfmt_dbuf<void> fld_state;           // field_state (device) and its pinned host mirror
    mpfmt_hbuf<void> fld_state_host;
    bool fld_tracked = false;
    int64_t fld_source0 = -1; int32_t fld_checkpts = 0;
    int64_t fld_samples_epoch = -1, fld_graph_epoch = -1, fld_sweep_epoch = -1, fld_N = 0, fld_knn_k = 0;
    double fld_graph_r = -1.0;
    bool fld_dirty_any = false;          // a delta call has flagged columns since the field was last valid
    bool fld_grown = false;              // the sample set grew under the field: nothing of the ctx's N to read before the next update
    mpfmt_dbuf<double> fld_C_next;        // the spare buffers of the carry (mpfmt_field_carry): they change places with the four above
    mpfmt_dbuf<int64_t> fld_A_next, fld_Ab_next;
    mpfmt_dbuf<uint64_t> fld_bm_next;
    // stats of the last mpfmt_field_begin / _update
    int32_t fld_path = 0;
    int64_t fld_invalidated = 0, fld_dirty_columns = 0, fld_columns_read = 0, fld_column_visits = 0, fld_entries_read = 0, fld_rounds = 0,
            fld_relax = 0, fld_reached = 0;

    // ---- tracked cost-to-go field (kernels_togo.hip): buffers of its own that no other call writes, on any resident swept graph ----
    // steer_epoch counts the builds of a steering graph (bumped wherever steer_filled becomes true), steer_sweep_epoch its whole sweeps
    // (wherever steer_swept becomes true): what graph_epoch / sweep_epoch are to the Euclidean graph state
    int64_t steer_epoch = 0, steer_sweep_epoch = 0;
    mpfmt_dbuf<double> tg_G;              // [N] labels
    mpfmt_dbuf<unsigned long long> tg_S;  // [N] 1-based successors (0: targets, unreached samples)
    mpfmt_dbuf<unsigned long long> tg_best;      // [N] successor pass 1
    mpfmt_dbuf<uint64_t> tg_bm;           // [7][ceil(N/64)]: the ring of three | targets | dirty columns | invalidated | columns read
    mpfmt_dbuf<int64_t> tg_tgt;           // [ntgt] 1-based targets
    mpfmt_dbuf<void> tg_state;            // togo_state (device) and its pinned host mirror
    mpfmt_hbuf<void> tg_state_host;
    std::vector<int64_t> tg_targets;     // the targets on the host (a recomputation starts from them)
    bool tg_tracked = false, tg_steer = false;
    int32_t tg_checkpts = 0;
    int64_t tg_samples_epoch = -1, tg_build_epoch = -1, tg_sweep_epoch = -1, tg_N = 0, tg_knn_k = 0;
    double tg_graph_r = -1.0, tg_steer_a = 0.0, tg_steer_b = 0.0;      // the graph's identity: radius (or k), steering parameters
    mpfmt_steer tg_steer_kind = MPFMT_STEER_DI;
    bool tg_dirty_any = false;           // a delta call has flagged columns since the field was last valid
    bool tg_grown = false;               // the sample set grew under the field: nothing of the ctx's N to read before the next update
    mpfmt_dbuf<double> tg_G_next;         // the spare buffers of the carry (mpfmt_togo_carry)
    mpfmt_dbuf<unsigned long long> tg_S_next;
    mpfmt_dbuf<uint64_t> tg_bm_next;
    // stats of the last mpfmt_togo_begin / _update
    int32_t tg_path = 0, tg_seed_form = 0;
    int64_t tg_invalidated = 0, tg_dirty_columns = 0, tg_columns_read = 0, tg_column_visits = 0, tg_entries_read = 0, tg_rounds = 0,
            tg_relax = 0, tg_atomics = 0, tg_reached = 0;
};

// error helpers ---------------------------------------------------------------------------------
#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return mpfmt_fail((ctx), MPFMT_ERR_HIP, "%s failed: %s (%s:%d)", #call,                \
                              hipGetErrorString(e_), __FILE__, __LINE__);                          \
    } while (0)

int32_t mpfmt_scratch(mpfmt_ctx* ctx, size_t bytes, void** out);
// the filled r-disc graph of radius r is resident (the k-nearest graph shares its slots and is never "a graph of radius graph_r")
inline bool euclid_resident(const mpfmt_ctx* ctx, double r) { return ctx->graph_filled && ctx->graph_r == r && !ctx->knn_k; }
// a ctx without the counter arena: the pair counters / the logs' overflow flag as allocations of their own, made once
inline int32_t mpfmt_own_pairs(mpfmt_ctx* ctx)
{
    if (ctx->d_pairs) return MPFMT_OK;
    const int32_t rc = ctx->d_pairs_own.ensure(ctx, 514 * sizeof(unsigned long long));      // (512 pair counters + the Euclidean build's longest-column word + the fullest quarter: one size everywhere)
    ctx->d_pairs = ctx->d_pairs_own;
    return rc;
}
inline int32_t mpfmt_own_pool_flag(mpfmt_ctx* ctx)
{
    if (ctx->pool_flag) return MPFMT_OK;
    const int32_t rc = ctx->pool_flag_own.ensure(ctx, sizeof(int32_t));
    ctx->pool_flag = ctx->pool_flag_own;
    return rc;
}
// the samples on the host (X: [N][d]) and their first k coordinates (P: [N][k], the workspace points of steering-space states)
int32_t mpfmt_states_host(mpfmt_ctx* ctx, int k, std::vector<double>& X, std::vector<double>& P);
void mpfmt_time_begin(mpfmt_ctx* ctx);
void mpfmt_time_end(mpfmt_ctx* ctx, const char* name);
void mpfmt_time_abandon(mpfmt_ctx* ctx);
// one timed interval; an error return between begin and end abandons it (the stack depth and the opening event are given
// back), so failed calls cannot wedge the timers of the ctx
struct mpfmt_timed {
    mpfmt_ctx* ctx; bool open;
    explicit mpfmt_timed(mpfmt_ctx* c) : ctx(c), open(true) { mpfmt_time_begin(c); }
    void end(const char* name) { if (open) { mpfmt_time_end(ctx, name); open = false; } }
    ~mpfmt_timed() { if (open) mpfmt_time_abandon(ctx); }
    mpfmt_timed(const mpfmt_timed&) = delete;
    mpfmt_timed& operator=(const mpfmt_timed&) = delete;
};

// mpfmt_capi.hip: the side stream (see mpfmt_ctx::side_stream)
int32_t mpfmt_side_fork(mpfmt_ctx* ctx, hipStream_t* main_out);      // ctx->stream := the side stream, ordered after everything issued so far
int32_t mpfmt_side_back(mpfmt_ctx* ctx, hipStream_t main);           // ctx->stream := main again; the side work is pending
int32_t mpfmt_side_join(mpfmt_ctx* ctx);                             // ctx->stream waits for the pending side work (no-op without)

// kernels_rdisc.hip -----------------------------------------------------------------------------
int32_t mpfmt_build_grid(mpfmt_ctx* ctx, double r, bool whole = false);      // whole: every tile is built even on a sharded ctx
int32_t mpfmt_launch_rdisc_count(mpfmt_ctx* ctx, double r);
int32_t mpfmt_rdisc_count_launch(mpfmt_ctx* ctx, double r, bool spec);
int32_t mpfmt_rdisc_count_finish(mpfmt_ctx* ctx, double r, bool* spec_failed);
int32_t mpfmt_graph_step(mpfmt_ctx* ctx, double r);
int32_t mpfmt_graph_step_launch_impl(mpfmt_ctx* ctx, double r);
int32_t mpfmt_graph_step_finish_impl(mpfmt_ctx* ctx);
int32_t mpfmt_launch_rdisc_fill(mpfmt_ctx* ctx, double r);
int32_t mpfmt_mfma_prepare(mpfmt_ctx* ctx, double r, float* negT_out, bool* usable);
int32_t mpfmt_mfma_build_operands(mpfmt_ctx* ctx);
template <int MODE> int32_t mpfmt_launch_rdisc_mfma(mpfmt_ctx* ctx, double r, float negT);
int32_t mpfmt_order_logs(mpfmt_ctx* ctx, const int32_t* spec_fail = nullptr, int64_t mask_entries = -1);      // kernels_order.hip
int32_t mpfmt_mask_preset(mpfmt_ctx* ctx, int64_t entries);
int32_t mpfmt_sweep_prepare_ss(mpfmt_ctx* ctx);          // kernels_sweep.hip: device copy of the state-space bounds + the all-samples-inside flag
#define MPFMT_ORD_MAXDEG 2048        // longest column the log-ordering kernel stages in LDS (ORD_STG in kernels_order.hip)
int32_t mpfmt_mfma_build_lists(mpfmt_ctx* ctx, double r, bool* usable, bool spec = false, bool half = false);
int mpfmt_slices_for(const mpfmt_ctx* ctx, int64_t units, bool mfma);      // slices per tile of the pair kernels (odd: kernels_rdisc_mfma.hip)
int32_t mpfmt_launch_log_degrees(mpfmt_ctx* ctx);
int32_t mpfmt_launch_sample_masks(mpfmt_ctx* ctx, double r, void* zero = nullptr, size_t zero_bytes = 0, bool* zeroed = nullptr);      // (zero: a buffer the kernel clears on the side)
int32_t mpfmt_rdisc_stream_impl(mpfmt_ctx* ctx, double r, const double* C_host, const uint64_t* H_host, int32_t want_free,
                                int64_t* deg, int64_t* nfree, int64_t* parent, double* cost, int64_t* nnz_out);
int32_t mpfmt_launch_exact_pairs(mpfmt_ctx* ctx, const int32_t* spec_fail);
// the library's own exclusive scan of int64 items on ctx->stream (k_scan_block / _single / _add, kernels_rdisc.hip); in == out allowed
size_t mpfmt_scan_tmp_bytes(size_t n);
int32_t mpfmt_scan_i64_tmp(mpfmt_ctx* ctx, const int64_t* in, int64_t* out, size_t n, void* tmp);      // tmp: mpfmt_scan_tmp_bytes(n) bytes of device memory
int32_t mpfmt_scan_i64(mpfmt_ctx* ctx, const int64_t* in, int64_t* out, size_t n);                     // tmp from the ctx's scratch buffer
int32_t mpfmt_launch_rdisc_query(mpfmt_ctx* ctx, int64_t v0, double r, int64_t* k_out,
                                 int64_t* inds_host, double* ds_host, int64_t cap);

// kernels_knn.hip -------------------------------------------------------------------------------
int32_t mpfmt_knn_build(mpfmt_ctx* ctx, int64_t k);      // exact k-nearest graph + mutual bits, installed as the resident graph

// kernels_sweep.hip -----------------------------------------------------------------------------
int32_t mpfmt_launch_points_free(mpfmt_ctx* ctx, const int64_t* d_idx1, int64_t n, uint64_t* d_mask);
int32_t mpfmt_2d_launch_points(mpfmt_ctx* ctx, const double* X, const int64_t* idx1, int64_t n, uint64_t* d_mask);
int32_t mpfmt_2d_launch_edges(mpfmt_ctx* ctx, const int64_t* s1, const int64_t* t1, const double* P, const double* Q, int64_t E, uint64_t* d_mask);
int32_t mpfmt_2d_launch_graph(mpfmt_ctx* ctx);
// the reference's shape constructors (kernels_sat2d.hip): Circle / convex Polygon from the ABI's encoding, refused as SAT2D.jl refuses
int32_t mpfmt_build_shape2d(mpfmt_ctx* ctx, int idx, int32_t kind, int32_t n, const double* data, mpfmt_shape2d* S);
int32_t mpfmt_launch_states_free(mpfmt_ctx* ctx, const double* d_P, int64_t n, uint64_t* d_mask);
int32_t mpfmt_launch_edges_free(mpfmt_ctx* ctx, const int64_t* d_src1, const int64_t* d_dst1, int64_t E, uint64_t* d_mask);
int32_t mpfmt_launch_motions_free(mpfmt_ctx* ctx, const double* d_P, const double* d_Q, int64_t n, uint64_t* d_mask);
int32_t mpfmt_launch_mc_edges(mpfmt_ctx* ctx, const int64_t* d_src1, const int64_t* d_dst1, int64_t E, double sigma, int64_t rollouts,
                              uint64_t seed, unsigned long long* d_hits);
int32_t mpfmt_launch_mc_is_edges(mpfmt_ctx* ctx, const int64_t* d_src1, const int64_t* d_dst1, int64_t E, double sigma, int64_t rollouts,
                                 uint64_t seed, unsigned long long* d_wsum);
int32_t mpfmt_launch_mc_ais_edges(mpfmt_ctx* ctx, const int64_t* d_src1, const int64_t* d_dst1, int64_t E, double sigma, int64_t rollouts,
                                  uint64_t seed, unsigned long long* d_wsum, double* d_mu);
int32_t mpfmt_launch_graph_sweep(mpfmt_ctx* ctx, const int32_t* spec_fail = nullptr, int64_t mask_entries = -1);

// kernels_boxdelta.hip --------------------------------------------------------------------------
int32_t mpfmt_boxdelta_apply(mpfmt_ctx* ctx, const double* d_delta, int32_t nd, bool remove);
// the same for a resident, swept steering graph (steer_delta.h): mask AND segment counts; flag + update launched on ctx->stream
int32_t mpfmt_di_delta_launch(mpfmt_ctx* ctx, const double* d_delta, int32_t nd, bool remove);      // kernels_di.hip
int32_t mpfmt_car_delta_launch(mpfmt_ctx* ctx, const double* d_delta, int32_t nd, bool remove);     // kernels_car.hip
int32_t mpfmt_steer_delta_run(mpfmt_ctx* ctx, const std::function<int32_t()>& launch);             // kernels_boxdelta.hip: set-up, launch, counters
// the same for an edit of the shape list of the 2-D SAT world (option "steer_shapes_delta"): Bold / M_before describe the list before it
int32_t mpfmt_di_sdelta_launch(mpfmt_ctx* ctx, const mpfmt_shape2d* d_delta, int32_t nd, bool remove, const mpfmt_aabb2d& Bold, int32_t M_before);
int32_t mpfmt_car_sdelta_launch(mpfmt_ctx* ctx, const mpfmt_shape2d* d_delta, int32_t nd, bool remove, const mpfmt_aabb2d& Bold, int32_t M_before);
bool mpfmt_di_sweep_fits(int64_t M, int m);              // M boxes of an m-dimensional workspace are within the whole sweep's LDS limit

// kernels_di.hip ----------------------------------------------------------------------------------
#include <functional>
#include <vector>
int32_t mpfmt_csc_transpose_device(mpfmt_ctx* ctx, mpfmt_csr_host* out);      // kernels_di.hip; needs nnz < 2^32
int32_t mpfmt_csc_transpose_resident(mpfmt_ctx* ctx, int64_t* d_rowptr, int32_t* d_colidx);   // the same, result left on the device
int32_t mpfmt_car_build(mpfmt_ctx* ctx, mpfmt_steer kind, double rt, double sp, double r);      // kind Dubins or Reeds-Shepp
int32_t mpfmt_car_sweep(mpfmt_ctx* ctx);
int32_t mpfmt_car_steer_batch(mpfmt_ctx* ctx, mpfmt_steer kind, const double* d_X0, const double* d_X1, int64_t n, double rt, double sp, double* d_cost,
                              double* d_ctrl, int32_t* d_nseg);
struct di_args;
int32_t mpfmt_di_mf_prepare(mpfmt_ctx* ctx, double rho, double r, float* negT, bool* usable, double* sp_out, double* sv_out, double* pc);      // kernels_di_mfma.hip
int32_t mpfmt_di_mf_build_operands(mpfmt_ctx* ctx, double sp, double sv, const double* pc_host);
int32_t mpfmt_di_mf_launch(mpfmt_ctx* ctx, const di_args& a, int mode, float negT, unsigned nblk);
int32_t mpfmt_di_count(mpfmt_ctx* ctx, double rho, double r);
int32_t mpfmt_di_fill(mpfmt_ctx* ctx);
int32_t mpfmt_di_sweep(mpfmt_ctx* ctx);
int32_t mpfmt_di_steer_launch(mpfmt_ctx* ctx, int m, const double* dX0, const double* dX1, int64_t n, double rho, double r,
                              double* dcost, double* dt);

// mpfmt_comm.hip -----------------------------------------------------------------------------------
int32_t mpfmt_comm_allgather_inplace(mpfmt_ctx* ctx, void* buf, size_t bytes_per_rank, hipStream_t stream);
int32_t mpfmt_comm_world(const mpfmt_ctx* ctx, int* rank, int* world);      // 1 when a communicator exists

// kernels_steer.hip ---------------------------------------------------------------------------------
int32_t mpfmt_launch_euclid_steer(mpfmt_ctx* ctx, const int64_t* d_src1, const int64_t* d_dst1, int64_t E, double* d_t, double* d_u);
int32_t mpfmt_launch_euclid_propagate(mpfmt_ctx* ctx, const int64_t* d_src1, int64_t E, const double* d_t, const double* d_u,
                                      const double* d_s, double* d_out);

// kernels_wavefront.hip -----------------------------------------------------------------------------
void mpfmt_wf_free(mpfmt_ctx* ctx);
int32_t mpfmt_wf_run(mpfmt_ctx* ctx);
int32_t mpfmt_wf_begin_directed(mpfmt_ctx* ctx, int64_t init_idx, int32_t checkpts, const uint64_t* F_host, int32_t goal_kind,
                                const double* goal_params, int32_t gd, double band, int32_t flags);
void mpfmt_wf_info_now(mpfmt_ctx* ctx, mpfmt_wf_info* info);

// kernels_sssp.hip ---------------------------------------------------------------------------------
// one source (0-based) over the resident graph and mask; d_F = point bitmap on the device or nullptr; C_host [N] / A_host [N] (may be
// nullptr) receive the field; the labels and parents also stay in ctx->sssp_C / sssp_A
int32_t mpfmt_sssp_device(mpfmt_ctx* ctx, int64_t source0, const uint64_t* d_F, double* C_host, int64_t* A_host, mpfmt_sssp_info* info);
void mpfmt_sssp_free(mpfmt_ctx* ctx);
// kernels_sssp_to.hip: the cost-to-go field of a target set (1-based, on the host, validated) over the resident graph and mask; G_host [N],
// S_host [N] or nullptr (no successor passes); labels and successors also stay in ctx->sssp_C / sssp_A
void mpfmt_sssp_to_launch_successors(mpfmt_ctx* ctx, const uint64_t* d_F, const double* G, const uint64_t* bm, unsigned long long* best,
                                     unsigned long long* S);      // the successor passes of the cost-to-go, on ctx->stream
int32_t mpfmt_sssp_to_device(mpfmt_ctx* ctx, const int64_t* targets1, int64_t ntgt, const uint64_t* d_F, double* G_host, int64_t* S_host,
                             mpfmt_sssp_info* info);
// kernels_field.hip: the tracked field.  d_F: the point bitmap of the current obstacle set or nullptr (checkpts = false)
int32_t mpfmt_field_compute(mpfmt_ctx* ctx, int64_t source0, int32_t checkpts, const uint64_t* d_F, mpfmt_field_info* info);   // whole field into the tracked buffers
int32_t mpfmt_field_repair(mpfmt_ctx* ctx, const uint64_t* d_F, mpfmt_field_info* info);                                       // steps 2-4 on the tracked buffers
int32_t mpfmt_dirty_columns_into(mpfmt_ctx* ctx, unsigned long long* D);      // k_field_dirty: bd_cols[0 .. bd_columns) ORed into D, on ctx->stream
int32_t mpfmt_field_mark_dirty(mpfmt_ctx* ctx);          // ORs ctx->bd_cols[0 .. bd_columns) into the dirty bitmap, on ctx->stream
void mpfmt_field_drop_internal(mpfmt_ctx* ctx);
bool mpfmt_field_live(mpfmt_ctx* ctx);                   // a tracked field of the resident samples and graph (drops one of another graph)
bool mpfmt_field_history(const mpfmt_ctx* ctx);          // no graph build and no whole sweep since the field was last valid
// the field follows a growth of the sample set (ctx->N is the grown size, the field is that of the first n_old samples): C / A extended,
// Ab found again in the grown columns, the dirty bitmap re-laid and ORed with `changed` -- all into the spare buffers, on ctx->stream.
// mpfmt_field_carry_commit changes them for the tracked ones and moves the field's identity to the ctx's (after the call has succeeded)
int32_t mpfmt_field_carry(mpfmt_ctx* ctx, int64_t n_old, const int64_t* colptr_new, const int32_t* rowval_new, const uint64_t* changed);
void mpfmt_field_carry_commit(mpfmt_ctx* ctx);
// the tracked cost-to-go field (kernels_togo.hip)
int32_t mpfmt_togo_compute(mpfmt_ctx* ctx, const int64_t* targets1, int64_t ntgt, int32_t checkpts, const uint64_t* d_F, mpfmt_togo_info* info);
int32_t mpfmt_togo_repair(mpfmt_ctx* ctx, const uint64_t* d_F, mpfmt_togo_info* info);      // steps 2-5 on the tracked buffers
int32_t mpfmt_togo_mark_dirty(mpfmt_ctx* ctx);           // ORs ctx->bd_cols[0 .. bd_columns) into its own dirty bitmap, on ctx->stream
void mpfmt_togo_drop_internal(mpfmt_ctx* ctx);
bool mpfmt_togo_live(mpfmt_ctx* ctx);                    // a tracked field of the resident samples and graph (drops one of another graph)
bool mpfmt_togo_history(const mpfmt_ctx* ctx);           // no graph build and no whole sweep since the field was last valid
int32_t mpfmt_togo_carry(mpfmt_ctx* ctx, int64_t n_old, const uint64_t* changed);      // as mpfmt_field_carry: G / S / targets / dirty
void mpfmt_togo_carry_commit(mpfmt_ctx* ctx);
int32_t mpfmt_togo_add_targets(mpfmt_ctx* ctx, const int64_t* targets1, int64_t ntgt);      // validated 1-based targets join the tracked set (label decreases)
// the field of the usable seeds of one external start: entries [n] of a near list (1-based samples, distances, bits: 2 = usable) become
// C[y] = seed[y] = fl(0 + dist); labels stay in ctx->sssp_C, parents in ctx->sssp_A (1-based, -1 = the start, 0 = none)
int32_t mpfmt_sssp_seeded_device(mpfmt_ctx* ctx, const int64_t* d_idx1, const double* d_dist, const uint8_t* d_bits, int64_t n, const uint64_t* d_F,
                                 mpfmt_sssp_info* info);

// kernels_roadmap.hip --------------------------------------------------------------------------------
struct mpfmt_rm_list {                   // near lists of a batch of external states, CSR, on the device (owned by the call's mpfmt_tmp)
    int64_t* ptr = nullptr; int64_t* idx1 = nullptr; double* dist = nullptr; uint8_t* bits = nullptr;      // bits: 1 free, 2 usable
    std::vector<int64_t> ptr_host, usable_host;
    int64_t total = 0;
};
int32_t mpfmt_roadmap_grid(mpfmt_ctx* ctx);
// count_only: ptr_host / total alone (no list is filled)
int32_t mpfmt_roadmap_lists(mpfmt_ctx* ctx, mpfmt_tmp& tmp, const double* d_Q, int64_t nq, int dir, const uint64_t* d_F, mpfmt_rm_list* out,
                            bool count_only = false);
int32_t mpfmt_roadmap_reduce(mpfmt_ctx* ctx, mpfmt_tmp& tmp, const double* d_Q, int64_t nq, const double* d_C, double* d_cost, int64_t* d_parent);
int32_t mpfmt_roadmap_goal(mpfmt_ctx* ctx, const mpfmt_rm_list& L, int64_t q, const double* d_C, const int64_t* d_A, int64_t* d_res);
// the same lists and reduction for a resident steering graph (steer_roadmap.h).  d_X / nx: the samples the queries meet (ctx->Xo / N);
// pair: query i meets d_X[i] alone (the direct edge of pair i, d_X = the goals)
int32_t mpfmt_steer_roadmap_lists(mpfmt_ctx* ctx, mpfmt_tmp& tmp, const double* d_Q, int64_t nq, int dir, const uint64_t* d_F, mpfmt_rm_list* out,
                                  bool count_only, const double* d_X, int64_t nx, bool pair);
int32_t mpfmt_steer_roadmap_reduce(mpfmt_ctx* ctx, mpfmt_tmp& tmp, const double* d_Q, int64_t nq, const double* d_C, double* d_cost, int64_t* d_parent);

// kernels_grow.hip -----------------------------------------------------------------------------------
// The ctx holds the grown sample set (N, Xo, bounding box) and, untouched, the swept graph of its first n_old samples: the graph and
// mask of radius r_new over all N are built in the spare buffers and change places with the ctx's own.  An error return has changed
// neither the graph's arrays nor its flags (the cell grid may be that of the grown set: the caller marks it stale).
// carry (option "samples_add_keeps_fields"): bit 0 = the tracked cost-to-come field, bit 1 = the tracked cost-to-go field follow the
// growth into their spare buffers (mpfmt_field_carry / mpfmt_togo_carry); the caller commits them once the whole call has succeeded.
int32_t mpfmt_grow_apply(mpfmt_ctx* ctx, int64_t n_old, double r_new, int32_t carry);

// kernels_sssp_multi.hip ----------------------------------------------------------------------------
// nsrc fields (sources 1-based, on the host) in groups of 64 over the resident graph and mask; C_host [nsrc][N], A_host [nsrc][N] or nullptr
int32_t mpfmt_sssp_multi_device(mpfmt_ctx* ctx, const int64_t* sources1, int64_t nsrc, const uint64_t* d_F, double* C_host, int64_t* A_host,
                                mpfmt_sssp_info* info);
// the cost matrix of ns external starts and ng external goals from their near lists (tail lists Ls, head lists Lg) and the three bit arrays
// (start free, goal free, motion bit of pair i * ng + j); d_cost / d_status [ns][ng] on the device; info: groups, rounds, ms_device
int32_t mpfmt_roadmap_matrix_device(mpfmt_ctx* ctx, const double* d_S, int64_t ns, const double* d_G, int64_t ng, const uint64_t* d_F,
                                    const uint64_t* d_sfree, const uint64_t* d_gfree, const uint64_t* d_direct, const mpfmt_rm_list& Ls,
                                    const mpfmt_rm_list& Lg, double* d_cost, int32_t* d_status, mpfmt_roadmap_matrix_info* info);
int32_t mpfmt_roadmap_pairs(mpfmt_ctx* ctx, const double* d_S, int64_t ns, const double* d_G, int64_t ng, double* d_P, double* d_Q);      // P / Q [ns * ng][d]
void mpfmt_sssp_multi_free(mpfmt_ctx* ctx);

// kernels_shortcut.hip -----------------------------------------------------------------------------
// the batch on the device; arguments already validated (mpfmt_adaptive_shortcut_batch, mpfmt_capi.hip)
int32_t mpfmt_shortcut_batch_device(mpfmt_ctx* ctx, const double* P, const int64_t* offsets, int64_t B, int32_t iterations, int64_t max_states,
                                    double* out_P, int64_t* out_offsets, int64_t out_cap, double* cumcost, mpfmt_shortcut_info* info);

// kernels_discretize.hip ---------------------------------------------------------------------------
// the batch on the device; arguments already validated (mpfmt_discretize_batch, mpfmt_capi.hip)
int32_t mpfmt_discretize_batch_device(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const int64_t* offsets,
                                      int64_t B, int32_t mode, double dt, int64_t n_samples, int32_t append_end, double* out_X, double* out_T,
                                      int32_t* out_seg, int64_t* out_offsets, int64_t out_cap, mpfmt_disc_info* info);

// kernels_steershortcut.hip ------------------------------------------------------------------------
// the pair primitive and the batch on the device; arguments already validated (mpfmt_steer_motions_free, mpfmt_steer_shortcut_batch)
int32_t mpfmt_steer_pairs_device(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const double* Q, int64_t n,
                                 uint64_t* mask, double* cost, double* dur, int32_t* nseg);
int32_t mpfmt_steer_shortcut_batch_device(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const int64_t* offsets,
                                          int64_t B, int32_t iterations, int64_t max_states, double* out_P, int64_t* out_offsets, int64_t out_cap,
                                          double* cumcost, int32_t* out_origin, mpfmt_steer_shortcut_info* info);

// kernels_expand.hip ----------------------------------------------------------------------------
int32_t mpfmt_launch_expand(mpfmt_ctx* ctx, const uint64_t* d_W, const uint64_t* d_H, const uint64_t* d_F,
                            const double* d_C, const int64_t* d_zs1, int64_t nz,
                            int64_t* d_xs, int64_t* d_ymin, double* d_cmin, uint8_t* d_free, int64_t cap,
                            int64_t* nx_host);
