// C ABI of libmpfmt.so (see include/mpfmt.h).  Host-side plumbing only: argument checks, device
// buffers for caller-owned host arrays, 1-based <-> 0-based conversion, and the sequential FMT*
// recursion of the reference (src/planners/fmt.jl:68-90) run over GPU-built arrays.
// There is NO CPU fallback for any compute entry point: without a gfx950 device ctx_create fails.
#include "mpfmt_internal.h"
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <chrono>
#include <functional>
#include <algorithm>
#include <vector>

static thread_local std::string g_create_err;

int32_t mpfmt_fail(mpfmt_ctx* ctx, int32_t code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_err = buf;
    return code;
}

int32_t mpfmt_scratch(mpfmt_ctx* ctx, size_t bytes, void** out)
{
    int32_t rc;
    if (bytes > ctx->scratch.bytes() && (rc = ctx->scratch.ensure(ctx, bytes + bytes / 4 + 4096))) return rc;
    *out = ctx->scratch;
    return MPFMT_OK;
}

// ---- timing: HIP events on the launch stream.  Begin/end only RECORD events (no host sync in the hot path);
//      pending intervals are resolved when a timing is queried.  A small stack lets groups nest.
#define TIMER_DEPTH 4
struct timer_rec { std::string name; hipEvent_t a, b; };
struct mpfmt_timer_state {
    std::vector<hipEvent_t> free_events;
    std::vector<timer_rec> pending;
    hipEvent_t open_a[TIMER_DEPTH];
    int depth = 0;
};
static mpfmt_timer_state& timers_of(mpfmt_ctx* ctx)
{
    if (!ctx->timer_state) ctx->timer_state = new mpfmt_timer_state();
    return *ctx->timer_state;
}

static hipEvent_t timer_event(mpfmt_timer_state& t)
{
    if (!t.free_events.empty()) { hipEvent_t e = t.free_events.back(); t.free_events.pop_back(); return e; }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}

static void timer_resolve(mpfmt_ctx* ctx)
{
    if (!ctx->timer_state) return;
    mpfmt_timer_state& t = timers_of(ctx);
    for (timer_rec& r : t.pending) {
        hipEventSynchronize(r.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            mpfmt_timer& tm = ctx->timers[r.name];
            tm.total_ms += ms;
            tm.launches += 1;
        }
        t.free_events.push_back(r.a);
        t.free_events.push_back(r.b);
    }
    t.pending.clear();
}

int32_t mpfmt_side_fork(mpfmt_ctx* ctx, hipStream_t* main_out)
{
    if (!ctx->side_stream) {
        // (lowest priority: what runs there is never the longer of the two sides)
        int prio_lo = 0, prio_hi = 0;
        HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->side_stream, hipStreamNonBlocking, prio_lo));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    }
    int32_t rc;
    if ((rc = mpfmt_side_join(ctx))) return rc;               // (one fork at a time)
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
    *main_out = ctx->stream;
    ctx->stream = ctx->side_stream;
    return MPFMT_OK;
}

int32_t mpfmt_side_back(mpfmt_ctx* ctx, hipStream_t main)
{
    const hipError_t e = hipEventRecord(ctx->ev_join, ctx->side_stream);
    ctx->stream = main;
    ctx->side_pending = true;
    HIPCHK(ctx, e);
    return MPFMT_OK;
}

int32_t mpfmt_side_join(mpfmt_ctx* ctx)
{
    if (!ctx->side_pending) return MPFMT_OK;
    ctx->side_pending = false;
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    return MPFMT_OK;
}

void mpfmt_time_begin(mpfmt_ctx* ctx)
{
    if (!ctx->timing_enabled) return;
    mpfmt_timer_state& t = timers_of(ctx);
    if (t.depth < TIMER_DEPTH) {
        t.open_a[t.depth] = timer_event(t);
        hipEventRecord(t.open_a[t.depth], ctx->stream);
    }
    ++t.depth;
}

void mpfmt_time_end(mpfmt_ctx* ctx, const char* name)
{
    if (!ctx->timing_enabled) return;
    mpfmt_timer_state& t = timers_of(ctx);
    if (t.depth <= 0) return;
    --t.depth;
    if (t.depth >= TIMER_DEPTH) return;
    timer_rec r;
    r.name = name; r.a = t.open_a[t.depth]; r.b = timer_event(t);
    hipEventRecord(r.b, ctx->stream);
    t.pending.push_back(r);
    if (t.pending.size() > 4096) timer_resolve(ctx);
}

void mpfmt_time_abandon(mpfmt_ctx* ctx)
{
    if (!ctx->timing_enabled) return;
    mpfmt_timer_state& t = timers_of(ctx);
    if (t.depth <= 0) return;
    --t.depth;
    if (t.depth < TIMER_DEPTH) t.free_events.push_back(t.open_a[t.depth]);
}

// ---- small conversion kernels --------------------------------------------------------------------------
__global__ void k_add1_i64(const int64_t* __restrict__ in, int64_t n, int64_t* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] + 1;
}
__global__ void k_i32_to_i64_add1(const int32_t* __restrict__ in, int64_t n, int64_t* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int64_t)in[i] + 1;
}

extern "C" {

const char* mpfmt_version(void) { return "mpfmt 0.2.0 gfx950"; }

const char* mpfmt_last_error(const mpfmt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int32_t mpfmt_ctx_create(int32_t device, mpfmt_ctx** out)
{
    if (!out) return mpfmt_fail(nullptr, MPFMT_ERR_ARG, "ctx_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return mpfmt_fail(nullptr, MPFMT_ERR_NODEVICE, "no HIP device visible (%s); libmpfmt has no CPU fallback",
                          e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return mpfmt_fail(nullptr, MPFMT_ERR_ARG, "device %d out of range [0,%d)", device, ndev);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return mpfmt_fail(nullptr, MPFMT_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return mpfmt_fail(nullptr, MPFMT_ERR_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    if ((e = hipSetDevice(device)) != hipSuccess)
        return mpfmt_fail(nullptr, MPFMT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    mpfmt_ctx* ctx = new mpfmt_ctx();
    ctx->device = device;
    ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ctx->ss.has = 0; ctx->ss.d = 0;
    if ((e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        delete ctx;
        return mpfmt_fail(nullptr, MPFMT_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return MPFMT_OK;
}

int32_t mpfmt_ctx_destroy(mpfmt_ctx* ctx)
{
    if (!ctx) return MPFMT_OK;
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    // (refused while another thread's open group still has to post this ctx's gather: the ctx stays whole and usable)
    { const int32_t rc = mpfmt_comm_destroy(ctx); if (rc) return rc; }
    if (ctx->side_stream) { hipStreamSynchronize(ctx->side_stream); hipStreamDestroy(ctx->side_stream); hipEventDestroy(ctx->ev_fork); hipEventDestroy(ctx->ev_join); }
    for (int k = 0; k < 2; ++k) { if (ctx->copy_stream[k]) hipStreamDestroy(ctx->copy_stream[k]); if (ctx->ev_conv[k]) hipEventDestroy(ctx->ev_conv[k]); if (ctx->ev_copy[k]) hipEventDestroy(ctx->ev_copy[k]); }
    mpfmt_wf_free(ctx);
    mpfmt_sssp_free(ctx);
    mpfmt_sssp_multi_free(ctx);
    if (ctx->aux) { mpfmt_ctx_destroy(ctx->aux); ctx->aux = nullptr; }
    timer_resolve(ctx);
    if (ctx->timer_state) {
        for (hipEvent_t e : ctx->timer_state->free_events) hipEventDestroy(e);
        delete ctx->timer_state;
    }
    // the ctx's buffers release themselves: on ctx->device (the aux ctx lives there too), and before the stream they were used on goes
    const hipStream_t own = ctx->own_stream;
    delete ctx;
    if (own) hipStreamDestroy(own);
    return MPFMT_OK;
}

int32_t mpfmt_set_stream(mpfmt_ctx* ctx, void* hip_stream)
{
    if (!ctx) return MPFMT_ERR_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return MPFMT_OK;
}

int32_t mpfmt_set_shard(mpfmt_ctx* ctx, int32_t rank, int32_t world)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (world < 1 || rank < 0 || rank >= world) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "bad shard %d of %d", rank, world);
    ctx->rank = rank; ctx->world = world;
    mpfmt_field_drop_internal(ctx);
    mpfmt_togo_drop_internal(ctx);
    ctx->deg_zero_valid = false;
    ctx->grid_r = -1.0; ctx->ops_r = -1.0; ctx->lists_r = -1.0;      // (the cell order and the built part of the index belong to the shard)
    ctx->graph_r = -1.0; ctx->graph_counted = ctx->graph_filled = ctx->graph_swept = false; ctx->knn_k = 0;
    return MPFMT_OK;
}

// per-block partial bounding boxes of a device-resident sample set + a count of non-finite coordinates; with dst the same pass is the
// copy into the ctx's sample buffer (thread = one coordinate: coalesced whatever d is; the box per axis needs d | the stride, so a
// thread's coordinates are those of ONE axis when the block's stride is a multiple of d -- the launch rounds it)
#define BBOX_THREADS 1024
__global__ __launch_bounds__(BBOX_THREADS) void k_bbox_partials(const double* __restrict__ X, double* __restrict__ dst, int64_t N, int d, int64_t stride,
                                                                double* __restrict__ part, int32_t* __restrict__ bad)
{
    __shared__ double s_lo[MPFMT_MAX_DIM], s_hi[MPFMT_MAX_DIM];
    __shared__ unsigned long long s_lob[MPFMT_MAX_DIM], s_hib[MPFMT_MAX_DIM];
    (void)s_lo; (void)s_hi;
    // total order of doubles as unsigned integers (sign flip), so that the per-axis minimum / maximum are LDS atomics
    auto enc = [](double a) -> unsigned long long { const unsigned long long u = (unsigned long long)__double_as_longlong(a); return (u >> 63) ? ~u : (u | 0x8000000000000000ull); };
    auto dec = [](unsigned long long e) -> double { const unsigned long long u = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e; return __longlong_as_double((long long)u); };
    if (threadIdx.x < MPFMT_MAX_DIM) { s_lob[threadIdx.x] = ~0ull; s_hib[threadIdx.x] = 0ull; }
    __syncthreads();
    const int64_t total = N * d;
    // stride (a multiple of d) coordinates apart: this thread's coordinates all belong to axis (first index) mod d
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int axis = (int)(first % d);
    double lo = INFINITY, hi = -INFINITY;
    int nbad = 0;
    for (int64_t t = (first < stride) ? first : total; t < total; t += stride) {
        const double a = X[t];
        if (dst) dst[t] = a;
        if (!(fabs(a) <= 1.7976931348623157e308)) ++nbad;
        lo = fmin(lo, a); hi = fmax(hi, a);
    }
    if (lo <= hi) { atomicMin(&s_lob[axis], enc(lo)); atomicMax(&s_hib[axis], enc(hi)); }
    if (__ballot(nbad != 0) && (threadIdx.x & 63) == 0) atomicAdd(bad, 1);
    __syncthreads();
    if (threadIdx.x < d) {
        const int i = threadIdx.x;
        part[((int64_t)blockIdx.x * 2 + 0) * MPFMT_MAX_DIM + i] = (s_lob[i] == ~0ull) ? INFINITY : dec(s_lob[i]);
        part[((int64_t)blockIdx.x * 2 + 1) * MPFMT_MAX_DIM + i] = (s_hib[i] == 0ull) ? -INFINITY : dec(s_hib[i]);
    }
}

// Both uploads: the copy into the ctx's sample buffer (host-to-device or device-to-device) and, beside it on the same stream, the
// finiteness check and the bounding box as ONE reduction on the device (a host loop over 6e6 coordinates costs 3 ms -- more than the
// PCIe copy of them), one small read-back, one synchronisation.  The copy goes to a SECOND buffer that changes places with the ctx's
// sample buffer only when the check has passed: a refused set (non-finite coordinate) leaves the ctx exactly as it was -- previous
// samples, index, graph and hints included (round 5 overwrote first and left the ctx empty: ADVICE r5).
static int32_t adopt_samples(mpfmt_ctx* ctx, const double* src, bool src_on_host, int64_t N, int32_t d)
{
    if (N < 0 || N >= ((int64_t)1 << 31) - 64) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "N = %lld out of range", (long long)N);
    if (d < 1 || d > MPFMT_MAX_DIM) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "d = %d out of range [1,%d]", d, MPFMT_MAX_DIM);
    if (N > 0 && !src) return mpfmt_fail(ctx, MPFMT_ERR_ARG, src_on_host ? "X is NULL" : "dX is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    constexpr int NB = 256;
    struct bb_block { double part[NB][2][MPFMT_MAX_DIM]; int32_t bad; int32_t pad_; };
    if ((rc = ctx->bb_dev.ensure(ctx, sizeof(bb_block)))) return rc;
    if ((rc = ctx->bb_host.ensure(ctx, sizeof(bb_block)))) return rc;
    bb_block* dev = (bb_block*)ctx->bb_dev.get();
    // blocks x threads rounded up to a multiple of d: a thread then stays on one axis (k_bbox_partials)
    const int nb = (int)std::min<int64_t>(NB, (N * d + BBOX_THREADS - 1) / BBOX_THREADS);
    const int64_t stride = std::max<int64_t>(((int64_t)std::max(nb, 1) * BBOX_THREADS / d) * d, d);      // (rounded DOWN: every residue below it has a thread)
    double lo[MPFMT_MAX_DIM], hi[MPFMT_MAX_DIM];
    for (int i = 0; i < d; ++i) { lo[i] = 0.0; hi[i] = 0.0; }
    if ((rc = ctx->Xo_next.ensure(ctx, sizeof(double) * (size_t)N * d))) return rc;
    if (N > 0) {
        HIPCHK(ctx, hipMemsetAsync(&dev->bad, 0, sizeof(int32_t), ctx->stream));
        // host samples: the PCIe copy, then the reduction over the copy; device samples: the reduction IS the copy
        if (src_on_host) HIPCHK(ctx, hipMemcpyAsync(ctx->Xo_next, src, sizeof(double) * (size_t)N * d, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_bbox_partials, dim3(nb), dim3(BBOX_THREADS), 0, ctx->stream, src_on_host ? (const double*)ctx->Xo_next : src, src_on_host ? (double*)nullptr : ctx->Xo_next,
                           N, d, stride, &dev->part[0][0][0], &dev->bad);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(ctx->bb_host, dev, sizeof(bb_block), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (N > 0) {
        const bb_block* h = (const bb_block*)ctx->bb_host.get();
        if (h->bad) {
            if (src_on_host)                                         // (name the sample, as the host check used to)
                for (int64_t p = 0; p < N; ++p)
                    for (int i = 0; i < d; ++i)
                        if (!std::isfinite(src[p * d + i]))
                            return mpfmt_fail(ctx, MPFMT_ERR_ARG, "sample %lld has a non-finite coordinate (the ctx keeps the sample set it had)", (long long)(p + 1));
            return mpfmt_fail(ctx, MPFMT_ERR_ARG, "the sample set has a non-finite coordinate (the ctx keeps the sample set it had)");
        }
    }
    // accepted: the new buffer becomes the ctx's sample set (the two members change places, capacities with them)
    ctx->Xo.swap(ctx->Xo_next);
    ctx->samples_epoch += 1;
    mpfmt_field_drop_internal(ctx);
    mpfmt_togo_drop_internal(ctx);
    ctx->grid_r = -1.0; ctx->graph_r = -1.0; ctx->ops_r = -1.0; ctx->lists_r = -1.0;
    ctx->graph_counted = ctx->graph_filled = ctx->graph_swept = false; ctx->knn_k = 0;
    ctx->steer_counted = ctx->steer_filled = ctx->steer_swept = false;
    ctx->nnz = 0;
    if (N > 0) {
        const bb_block* h = (const bb_block*)ctx->bb_host.get();
        for (int i = 0; i < d; ++i) { lo[i] = INFINITY; hi[i] = -INFINITY; }
        for (int b = 0; b < nb; ++b)
            for (int i = 0; i < d; ++i) { lo[i] = std::min(lo[i], h->part[b][0][i]); hi[i] = std::max(hi[i], h->part[b][1][i]); }
    }
    for (int i = 0; i < d; ++i) { ctx->bb_lo[i] = lo[i]; ctx->bb_hi[i] = hi[i]; }
    ctx->N = N; ctx->d = d;
    return MPFMT_OK;
}

int32_t mpfmt_upload_samples(mpfmt_ctx* ctx, const double* X, int64_t N, int32_t d)
{
    if (!ctx) return MPFMT_ERR_ARG;
    return adopt_samples(ctx, X, true, N, d);
}

// The same for a sample set that already lives in HBM (a batch made on the device: the library's own sampler, a ROCArray, a torch
// tensor): one device-to-device copy instead of the PCIe one.
int32_t mpfmt_upload_samples_device(mpfmt_ctx* ctx, const double* dX, int64_t N, int32_t d)
{
    if (!ctx) return MPFMT_ERR_ARG;
    return adopt_samples(ctx, dX, false, N, d);
}

// ---- growing the sample set (kernels_grow.hip) ---------------------------------------------------------------------------------------
// the resident graph and mask can follow the new samples instead of being thrown away
static bool samples_add_in_place(const mpfmt_ctx* ctx, double r_new)
{
    return ctx->world == 1 && ctx->cc_kind == 0 && ctx->have_boxes && ctx->dw == ctx->d && ctx->graph_filled && !ctx->knn_k && ctx->graph_swept &&
           !ctx->steer_counted && !ctx->steer_filled && (ctx->nnz == 0 || ctx->graph_free) && ctx->step_state != 1 && r_new <= ctx->graph_r;
}

// Both forms: the grown set is assembled in the spare sample buffer -- the old samples device to device, no host round trip; the new ones
// beside the finiteness check and their bounding box, as adopt_samples does -- and changes places with the ctx's own once it is accepted.
static int32_t samples_add(mpfmt_ctx* ctx, const double* src, bool src_on_host, int64_t n_add, double r_new)
{
    if (n_add < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "n_add = %lld < 0", (long long)n_add);
    if (n_add > 0 && !src) return mpfmt_fail(ctx, MPFMT_ERR_ARG, src_on_host ? "X_add is NULL" : "dX_add is NULL");
    if (!(r_new > 0.0) || !std::isfinite(r_new)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "r_new must be finite and > 0");
    if (!ctx->Xo || ctx->d < 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded (samples are added to a set: mpfmt_upload_samples fixes d)");
    const int64_t n_old = ctx->N, N = n_old + n_add;
    const int32_t d = ctx->d;
    if (N >= ((int64_t)1 << 31) - 64) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "N + n_add = %lld out of range", (long long)N);
    if (n_add == 0) return MPFMT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = mpfmt_side_join(ctx))) return rc;
    constexpr int NB = 256;
    struct bb_block { double part[NB][2][MPFMT_MAX_DIM]; int32_t bad; int32_t pad_; };
    if ((rc = ctx->bb_dev.ensure(ctx, sizeof(bb_block)))) return rc;
    if ((rc = ctx->bb_host.ensure(ctx, sizeof(bb_block)))) return rc;
    bb_block* dev = (bb_block*)ctx->bb_dev.get();
    const int nb = (int)std::min<int64_t>(NB, (n_add * d + BBOX_THREADS - 1) / BBOX_THREADS);
    const int64_t stride = std::max<int64_t>(((int64_t)std::max(nb, 1) * BBOX_THREADS / d) * d, d);
    if ((rc = ctx->Xo_next.ensure(ctx, sizeof(double) * (size_t)N * d))) return rc;
    double* dst = ctx->Xo_next.get() + (size_t)n_old * d;
    mpfmt_timed tm(ctx);
    if (n_old > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->Xo_next, ctx->Xo, sizeof(double) * (size_t)n_old * d, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(&dev->bad, 0, sizeof(int32_t), ctx->stream));
    if (src_on_host) HIPCHK(ctx, hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n_add * d, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_bbox_partials, dim3(nb), dim3(BBOX_THREADS), 0, ctx->stream, src_on_host ? (const double*)dst : src, src_on_host ? (double*)nullptr : dst,
                       n_add, d, stride, &dev->part[0][0][0], &dev->bad);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->bb_host, dev, sizeof(bb_block), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const bb_block* h = (const bb_block*)ctx->bb_host.get();
    if (h->bad) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "an added sample has a non-finite coordinate (the ctx keeps the sample set and graph it had)");
    double lo[MPFMT_MAX_DIM], hi[MPFMT_MAX_DIM], lo_was[MPFMT_MAX_DIM], hi_was[MPFMT_MAX_DIM];
    for (int i = 0; i < d; ++i) {
        lo_was[i] = ctx->bb_lo[i]; hi_was[i] = ctx->bb_hi[i];
        lo[i] = n_old > 0 ? lo_was[i] : INFINITY; hi[i] = n_old > 0 ? hi_was[i] : -INFINITY;
        for (int b = 0; b < nb; ++b) { lo[i] = std::min(lo[i], h->part[b][0][i]); hi[i] = std::max(hi[i], h->part[b][1][i]); }
    }
    const bool in_place = samples_add_in_place(ctx, r_new);
    // the tracked fields that follow the growth (option "samples_add_keeps_fields"): live fields of the old set whose delta history stands,
    // asked BEFORE the ctx takes the grown set (a field of another N is not live).  One that needs a recomputation anyway is dropped
    int32_t carry = 0;
    if (in_place && ctx->grow_keeps_fields) {
        if (mpfmt_field_live(ctx) && mpfmt_field_history(ctx)) carry |= 1;
        if (mpfmt_togo_live(ctx) && !ctx->tg_steer && mpfmt_togo_history(ctx)) carry |= 2;
    }
    ctx->Xo.swap(ctx->Xo_next);
    ctx->N = N;
    for (int i = 0; i < d; ++i) { ctx->bb_lo[i] = lo[i]; ctx->bb_hi[i] = hi[i]; }
    if (in_place) {
        if ((rc = mpfmt_grow_apply(ctx, n_old, r_new, carry))) {     // the ctx is again what it was; the cell order is rebuilt by whoever needs it next
            ctx->Xo.swap(ctx->Xo_next);
            ctx->N = n_old;
            for (int i = 0; i < d; ++i) { ctx->bb_lo[i] = lo_was[i]; ctx->bb_hi[i] = hi_was[i]; }
            ctx->grid_r = -1.0; ctx->ops_r = -1.0; ctx->lists_r = -1.0;
            return rc;
        }
    }
    ctx->samples_epoch += 1;
    if (carry & 1) mpfmt_field_carry_commit(ctx); else mpfmt_field_drop_internal(ctx);
    if (carry & 2) mpfmt_togo_carry_commit(ctx); else mpfmt_togo_drop_internal(ctx);
    ctx->grow_carried = carry;
    ctx->steer_counted = ctx->steer_filled = ctx->steer_swept = false;
    ctx->grow_path = in_place ? 1 : 0;
    if (!in_place) {                                         // what mpfmt_upload_samples of the concatenated set leaves
        ctx->grid_r = -1.0; ctx->graph_r = -1.0; ctx->ops_r = -1.0; ctx->lists_r = -1.0;
        ctx->graph_counted = ctx->graph_filled = ctx->graph_swept = false; ctx->knn_k = 0;
        ctx->nnz = 0;
        ctx->grow_candidates = ctx->grow_entries = ctx->grow_dropped = ctx->grow_flagged = 0;
    }
    tm.end("samples_add");
    return MPFMT_OK;
}

int32_t mpfmt_graph_radius(mpfmt_ctx* ctx, double* r)
{
    if (!ctx || !r) return MPFMT_ERR_ARG;
    if (!ctx->graph_filled || ctx->knn_k || ctx->steer_filled) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no resident r-disc graph");
    *r = ctx->graph_r;
    return MPFMT_OK;
}

int32_t mpfmt_samples_add(mpfmt_ctx* ctx, const double* X_add, int64_t n_add, double r_new)
{
    if (!ctx) return MPFMT_ERR_ARG;
    return samples_add(ctx, X_add, true, n_add, r_new);
}

int32_t mpfmt_samples_add_device(mpfmt_ctx* ctx, const double* dX_add, int64_t n_add, double r_new)
{
    if (!ctx) return MPFMT_ERR_ARG;
    return samples_add(ctx, dX_add, false, n_add, r_new);
}

// state-space bounds on their own: the BoundedStateSpace lo / hi for any state dimension (src/statespaces.jl:29-34).  The 2-D SAT
// world's upload takes the two workspace bounds only; a steering space over it (double integrator R^4, SE2 cars) sets its own.
int32_t mpfmt_set_state_bounds(mpfmt_ctx* ctx, const double* ss_lo, const double* ss_hi, int32_t d_state)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if ((ss_lo == nullptr) != (ss_hi == nullptr)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "ss_lo / ss_hi must both be given or both NULL");
    if (ss_lo && (d_state < 1 || d_state > MPFMT_MAX_DIM)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "d_state out of range");
    ctx->ss.has = ss_lo ? 1 : 0;
    ctx->ss.d = ss_lo ? d_state : 0;
    for (int i = 0; i < MPFMT_MAX_DIM; ++i) { ctx->ss.lo[i] = -INFINITY; ctx->ss.hi[i] = INFINITY; }
    if (ss_lo) for (int i = 0; i < d_state; ++i) { ctx->ss.lo[i] = ss_lo[i]; ctx->ss.hi[i] = ss_hi[i]; }
    ctx->graph_swept = false; ctx->steer_swept = false; ctx->pend_valid = false;     // (a pending list belongs to the obstacle set it was made against)
    mpfmt_field_drop_internal(ctx);
    mpfmt_togo_drop_internal(ctx);
    return MPFMT_OK;
}

int32_t mpfmt_upload_boxes(mpfmt_ctx* ctx, const double* lohi, int32_t M, int32_t dw,
                           const double* ss_lo, const double* ss_hi, int32_t d_state)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (M < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "M = %d < 0", M);
    if (dw < 1 || dw > MPFMT_MAX_DIM) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "dw = %d out of range", dw);
    if (M > 0 && !lohi) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "lohi is NULL");
    if ((ss_lo == nullptr) != (ss_hi == nullptr)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "ss_lo / ss_hi must both be given or both NULL");
    if (ss_lo && (d_state < 1 || d_state > MPFMT_MAX_DIM)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "d_state = %d out of range", d_state);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = ctx->boxes.ensure(ctx, sizeof(double) * (size_t)M * 2 * dw))) return rc;
    if (M > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->boxes, lohi, sizeof(double) * (size_t)M * 2 * dw, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->M = M; ctx->dw = dw; ctx->have_boxes = true; ctx->cc_kind = 0;
    ctx->boxes_host.assign(lohi, lohi + (size_t)M * 2 * dw);      // (a host copy: sizes the pending-pair list from the obstacles' extents)
    ctx->ss.has = ss_lo ? 1 : 0;
    ctx->ss.d = ss_lo ? d_state : 0;
    for (int i = 0; i < MPFMT_MAX_DIM; ++i) { ctx->ss.lo[i] = -INFINITY; ctx->ss.hi[i] = INFINITY; }
    if (ss_lo) for (int i = 0; i < d_state; ++i) { ctx->ss.lo[i] = ss_lo[i]; ctx->ss.hi[i] = ss_hi[i]; }
    ctx->graph_swept = false; ctx->pend_valid = false;
    ctx->steer_swept = false;
    mpfmt_field_drop_internal(ctx);
    return MPFMT_OK;
}

// ---- in-place edits of the box list (kernels_boxdelta.hip) ----------------------------------------------------------------------
// the resident mask can be brought up to date instead of being thrown away
static bool boxes_delta_in_place(const mpfmt_ctx* ctx)
{
    return ctx->world == 1 && ctx->cc_kind == 0 && ctx->dw == ctx->d && ctx->graph_filled && ctx->graph_swept && ctx->nnz > 0 &&
           ctx->graph_free && ctx->step_state != 1;
}

// the same for a resident, swept steering graph (double integrator, cars): mask and segment counts follow (steer_delta.h).  The
// conditions are those under which the space's whole sweep would accept the resulting list.
static bool steer_delta_in_place(const mpfmt_ctx* ctx)
{
    if (!(ctx->world == 1 && ctx->cc_kind == 0 && ctx->steer_filled && ctx->steer_swept && ctx->nnz > 0 && ctx->graph_free && ctx->steer_nseg))
        return false;
    if (ctx->steer_kind == MPFMT_STEER_DI) {
        const int m = ctx->d / 2;
        return ctx->d % 2 == 0 && m >= 1 && m <= 6 && ctx->dw == m && (!ctx->ss.has || ctx->ss.d == ctx->d) && mpfmt_di_sweep_fits(ctx->M, m);
    }
    return ctx->d == 3 && ctx->dw == 2 && (!ctx->ss.has || ctx->ss.d == 3);
}

static int32_t steer_delta_apply(mpfmt_ctx* ctx, const double* d_delta, int32_t nd, bool remove)
{
    return mpfmt_steer_delta_run(ctx, [&]() {
        return ctx->steer_kind == MPFMT_STEER_DI ? mpfmt_di_delta_launch(ctx, d_delta, nd, remove) : mpfmt_car_delta_launch(ctx, d_delta, nd, remove);
    });
}

// the list has been edited: the mask follows in place (delta = the boxes added or a copy of those removed) or goes stale
static int32_t boxes_delta_finish(mpfmt_ctx* ctx, const double* d_delta, int32_t nd, bool remove)
{
    ctx->bd_columns = ctx->bd_entries = 0;
    ctx->pend_valid = false;                                 // (a pending list belongs to the obstacle set it was made against)
    if (steer_delta_in_place(ctx)) {                         // (a steering graph is resident: the Euclidean graph state is not)
        ctx->bd_path = 1;
        ctx->graph_swept = false;
        const int32_t rc = steer_delta_apply(ctx, d_delta, nd, remove);
        if (rc) { ctx->steer_swept = false; ctx->bd_path = 0; return rc; }   // (the list stands, the mask is swept again)
        return mpfmt_togo_mark_dirty(ctx);                   // (a tracked cost-to-go field learns which columns the edit read)
    }
    ctx->steer_swept = false;
    ctx->bd_path = boxes_delta_in_place(ctx) ? 1 : 0;
    if (!ctx->bd_path) { ctx->graph_swept = false; return MPFMT_OK; }
    const int32_t rc = mpfmt_boxdelta_apply(ctx, d_delta, nd, remove);
    if (rc) { ctx->graph_swept = false; ctx->bd_path = 0; return rc; }   // (the list stands, the mask is swept again)
    const int32_t rf = mpfmt_field_mark_dirty(ctx);          // (a tracked field learns which columns the edit read:
    if (rf) return rf;                                       //  each of the two has a dirty bitmap of its own)
    return mpfmt_togo_mark_dirty(ctx);
}

int32_t mpfmt_boxes_add(mpfmt_ctx* ctx, const double* lohi, int32_t M_add)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (M_add < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "M_add = %d < 0", M_add);
    if (M_add > 0 && !lohi) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "lohi is NULL");
    if (!ctx->have_boxes || ctx->cc_kind != 0)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "boxes are added to a PointRobotNDBoxes set (mpfmt_upload_boxes), not to the 2-D SAT world");
    if (M_add == 0) return MPFMT_OK;
    if ((int64_t)ctx->M + M_add > INT32_MAX) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "more than 2^31 - 1 boxes");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t per = (size_t)2 * ctx->dw, old_n = (size_t)ctx->M * per, add_n = (size_t)M_add * per;
    int32_t rc;
    mpfmt_dbuf<double> nb;                                   // the new list beside the old one: a failure leaves the ctx as it was
    if ((rc = nb.ensure(ctx, sizeof(double) * (old_n + add_n)))) return rc;
    if (old_n) HIPCHK(ctx, hipMemcpyAsync(nb, ctx->boxes, sizeof(double) * old_n, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(nb.get() + old_n, lohi, sizeof(double) * add_n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->boxes_host.reserve(old_n + add_n);
    ctx->boxes_host.insert(ctx->boxes_host.end(), lohi, lohi + add_n);
    ctx->boxes.swap(nb);
    ctx->M += M_add;
    return boxes_delta_finish(ctx, ctx->boxes.get() + old_n, M_add, false);
}

int32_t mpfmt_boxes_remove(mpfmt_ctx* ctx, const int64_t* ids, int32_t n_ids)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n_ids < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "n_ids = %d < 0", n_ids);
    if (n_ids > 0 && !ids) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "ids is NULL");
    if (!ctx->have_boxes || ctx->cc_kind != 0)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "boxes are removed from a PointRobotNDBoxes set (mpfmt_upload_boxes), not from the 2-D SAT world");
    const int32_t M = ctx->M;
    std::vector<char> out((size_t)std::max(M, 1), 0);
    for (int32_t j = 0; j < n_ids; ++j) {
        if (ids[j] < 1 || ids[j] > M) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "box id %lld out of range 1..%d", (long long)ids[j], M);
        if (out[(size_t)(ids[j] - 1)]) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "box id %lld given twice", (long long)ids[j]);
        out[(size_t)(ids[j] - 1)] = 1;
    }
    if (n_ids == 0) return MPFMT_OK;
    if ((int64_t)ctx->boxes_host.size() != (int64_t)M * 2 * ctx->dw) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the host copy of the box list is not whole");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t per = (size_t)2 * ctx->dw;
    std::vector<double> keep, gone;
    keep.reserve((size_t)(M - n_ids) * per); gone.reserve((size_t)n_ids * per);
    for (int32_t k = 0; k < M; ++k) {
        std::vector<double>& to = out[(size_t)k] ? gone : keep;
        to.insert(to.end(), ctx->boxes_host.begin() + (size_t)k * per, ctx->boxes_host.begin() + (size_t)(k + 1) * per);
    }
    int32_t rc;
    mpfmt_dbuf<double> nb, removed;                          // the remaining list beside the old one; a copy of what leaves, for the kernel
    if ((rc = nb.ensure(ctx, sizeof(double) * keep.size()))) return rc;
    if ((rc = removed.ensure(ctx, sizeof(double) * gone.size()))) return rc;
    if (!keep.empty()) HIPCHK(ctx, hipMemcpyAsync(nb, keep.data(), sizeof(double) * keep.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(removed, gone.data(), sizeof(double) * gone.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->boxes_host.swap(keep);
    ctx->boxes.swap(nb);
    ctx->M = M - n_ids;
    return boxes_delta_finish(ctx, removed, n_ids, true);    // (synchronises before `removed` goes)
}

// ---- r-disc graph ------------------------------------------------------------------------------------

int32_t mpfmt_graph_build_device(mpfmt_ctx* ctx, double r, int64_t* nnz)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!(r >= 0.0) || !std::isfinite(r)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "radius must be finite and >= 0");
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    ctx->steer_counted = ctx->steer_filled = ctx->steer_swept = false;
    if (ctx->rebuild_index) { ctx->grid_r = -1.0; ctx->ops_r = -1.0; ctx->lists_r = -1.0; }    // index build (cell grid + operands) is part of the build
    if ((rc = mpfmt_launch_rdisc_count(ctx, r))) return rc;
    if ((rc = mpfmt_launch_rdisc_fill(ctx, r))) return rc;
    if (nnz) *nnz = ctx->nnz;
    return MPFMT_OK;
}

int32_t mpfmt_graph_step_device(mpfmt_ctx* ctx, double r, int64_t* nnz)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!(r >= 0.0) || !std::isfinite(r)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "radius must be finite and >= 0");
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    ctx->steer_counted = ctx->steer_filled = ctx->steer_swept = false;
    if (ctx->rebuild_index) { ctx->grid_r = -1.0; ctx->ops_r = -1.0; ctx->lists_r = -1.0; }
    if ((rc = mpfmt_graph_step(ctx, r))) return rc;
    // results are complete on return (the speculative path has synchronised after its last launch already; the careful
    // path launched the sweep after its last read-back)
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (nnz) *nnz = ctx->nnz;
    return MPFMT_OK;
}

int32_t mpfmt_graph_step_launch(mpfmt_ctx* ctx, double r)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!(r >= 0.0) || !std::isfinite(r)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "radius must be finite and >= 0");
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->steer_counted = ctx->steer_filled = ctx->steer_swept = false;
    if (ctx->rebuild_index) { ctx->grid_r = -1.0; ctx->ops_r = -1.0; ctx->lists_r = -1.0; }
    return mpfmt_graph_step_launch_impl(ctx, r);
}

int32_t mpfmt_graph_step_finish(mpfmt_ctx* ctx, int64_t* nnz)
{
    if (!ctx) return MPFMT_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = mpfmt_graph_step_finish_impl(ctx))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (nnz) *nnz = ctx->nnz;
    return MPFMT_OK;
}

// the resident colptr handed to the caller, 1-based: converted in scratch, copied, and there when this returns
static int32_t colptr_to_host(mpfmt_ctx* ctx, int64_t* colptr)
{
    const int64_t n1 = ctx->N + 1;
    void* scr;
    int32_t rc;
    if ((rc = mpfmt_scratch(ctx, sizeof(int64_t) * n1, &scr))) return rc;
    hipLaunchKernelGGL(k_add1_i64, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, ctx->stream, ctx->colptr, n1, (int64_t*)scr);
    HIPCHK(ctx, hipMemcpyAsync(colptr, scr, sizeof(int64_t) * n1, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

int32_t mpfmt_rdisc_count(mpfmt_ctx* ctx, double r, int64_t* colptr, int64_t* nnz)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!colptr || !nnz) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "colptr / nnz is NULL");
    if (!(r >= 0.0) || !std::isfinite(r)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "radius must be finite and >= 0");
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    ctx->steer_counted = ctx->steer_filled = ctx->steer_swept = false;
    if ((rc = mpfmt_launch_rdisc_count(ctx, r))) return rc;
    if ((rc = colptr_to_host(ctx, colptr))) return rc;
    *nnz = ctx->nnz;
    return MPFMT_OK;
}

int32_t mpfmt_rdisc_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->graph_counted) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "rdisc_fill before rdisc_count");
    if (ctx->nnz > 0 && (!rowval || !nzval)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rowval / nzval is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if (!ctx->graph_filled && (rc = mpfmt_launch_rdisc_fill(ctx, ctx->graph_r))) return rc;
    const int64_t nnz = ctx->nnz;
    if (nnz > 0) {
        // convert in slabs so the staging buffer stays small
        const int64_t slab = std::min<int64_t>(nnz, (int64_t)1 << 26);
        void* scr;
        if ((rc = mpfmt_scratch(ctx, sizeof(int64_t) * slab, &scr))) return rc;
        for (int64_t o = 0; o < nnz; o += slab) {
            const int64_t n = std::min(slab, nnz - o);
            hipLaunchKernelGGL(k_i32_to_i64_add1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                               ctx->rowval + o, n, (int64_t*)scr);
            HIPCHK(ctx, hipMemcpyAsync(rowval + o, scr, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        HIPCHK(ctx, hipMemcpyAsync(nzval, ctx->nzval, sizeof(double) * nnz, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MPFMT_OK;
}

// Install a previously exported r-disc graph (the reference's ImmutableNNC(D, r), nearneighbors.jl:23-28,
// whose saveNN / loadNN! were left commented out, :114-116) so that re-plans on the same samples -- new obstacles, new
// goals, another process -- skip the pair phase.  Same format mpfmt_rdisc_count / _fill hand out.
int32_t mpfmt_graph_import(mpfmt_ctx* ctx, double r, const int64_t* colptr, const int64_t* rowval, const double* nzval)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "graph_import needs an unsharded ctx");
    if (!(r >= 0.0) || !std::isfinite(r)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "radius must be finite and >= 0");
    if (!colptr) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "colptr is NULL");
    const int64_t N = ctx->N;
    if (colptr[0] != 1) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "colptr[1] must be 1 (1-based CSC)");
    for (int64_t j = 0; j < N; ++j)
        if (colptr[j + 1] < colptr[j]) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "colptr decreases at column %lld", (long long)(j + 1));
    const int64_t nnz = colptr[N] - 1;
    if (nnz > 0 && (!rowval || !nzval)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rowval / nzval is NULL");
    char verr[160];
    if (mpfmt_validate_csc(N, colptr, rowval, verr, sizeof verr) != 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%s", verr);
    std::vector<int64_t> cp0((size_t)N + 1);
    std::vector<int32_t> rv0((size_t)std::max<int64_t>(nnz, 1));
    for (int64_t j = 0; j <= N; ++j) cp0[j] = colptr[j] - 1;
    for (int64_t e = 0; e < nnz; ++e) rv0[e] = (int32_t)(rowval[e] - 1);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = ctx->colptr.ensure(ctx, sizeof(int64_t) * (size_t)(N + 1)))) return rc;
    if ((rc = ctx->rowval.ensure(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(nnz, 1)))) return rc;
    if ((rc = ctx->nzval.ensure(ctx, sizeof(double) * (size_t)std::max<int64_t>(nnz, 1)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->colptr, cp0.data(), sizeof(int64_t) * (size_t)(N + 1), hipMemcpyHostToDevice, ctx->stream));
    if (nnz > 0) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->rowval, rv0.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->nzval, nzval, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->nnz = nnz;
    ctx->graph_r = r;
    ctx->graph_counted = ctx->graph_filled = true; ctx->knn_k = 0;
    ctx->graph_epoch += 1; ctx->graph_imported = true;
    mpfmt_field_drop_internal(ctx);
    mpfmt_togo_drop_internal(ctx);
    ctx->graph_swept = false; ctx->pend_valid = false;
    ctx->pool_valid = false;
    ctx->rowpos_valid = false;
    ctx->steer_counted = ctx->steer_filled = ctx->steer_swept = false;
    return MPFMT_OK;
}

int32_t mpfmt_rdisc_query(mpfmt_ctx* ctx, int64_t v, double r, int64_t* inds, double* ds, int64_t cap, int64_t* k)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!k) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "k is NULL");
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (v < 1 || v > ctx->N) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "query index %lld out of range [1,%lld]", (long long)v, (long long)ctx->N);
    if (!(r >= 0.0) || !std::isfinite(r)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "radius must be finite and >= 0");
    if (cap < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "cap < 0");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc = mpfmt_launch_rdisc_query(ctx, v - 1, r, k, inds, ds, cap);
    if (rc == MPFMT_ERR_CAPACITY) return mpfmt_fail(ctx, rc, "rdisc_query: %lld neighbours exceed capacity %lld", (long long)*k, (long long)cap);
    return rc;
}

// ---- validity sweeps ---------------------------------------------------------------------------------

static int32_t up_i64(mpfmt_ctx* ctx, mpfmt_tmp& tmp, const int64_t* h, int64_t n, int64_t** d)
{
    *d = nullptr;
    HIPCHK(ctx, tmp.get(d, sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1)));
    if (n > 0) HIPCHK(ctx, hipMemcpyAsync(*d, h, sizeof(int64_t) * n, hipMemcpyHostToDevice, ctx->stream));
    return MPFMT_OK;
}

static int32_t check_idx(mpfmt_ctx* ctx, const int64_t* idx, int64_t n, const char* what)
{
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 1 || idx[i] > ctx->N)
            return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%s[%lld] = %lld out of range [1,%lld]", what, (long long)i, (long long)idx[i], (long long)ctx->N);
    return MPFMT_OK;
}

int32_t mpfmt_points_free(mpfmt_ctx* ctx, const int64_t* idx, int64_t n, uint64_t* mask)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (!idx) n = ctx->N;
    if (n < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "n < 0");
    if (n > 0 && !mask) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "mask is NULL");
    if (n == 0) return MPFMT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if (idx && (rc = check_idx(ctx, idx, n, "idx"))) return rc;
    const int64_t words = (n + 63) / 64;
    mpfmt_tmp tmp;
    int64_t* d_idx = nullptr; uint64_t* d_mask = nullptr;
    if (idx && (rc = up_i64(ctx, tmp, idx, n, &d_idx))) return rc;
    HIPCHK(ctx, tmp.get(&d_mask, sizeof(uint64_t) * words));
    rc = mpfmt_launch_points_free(ctx, d_idx, n, d_mask);
    if (rc == MPFMT_OK) {
        hipError_t e = hipMemcpyAsync(mask, d_mask, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = mpfmt_fail(ctx, MPFMT_ERR_HIP, "points_free copy back: %s", hipGetErrorString(e));
    }
    return rc;
}

int32_t mpfmt_edges_free(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, uint64_t* mask)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (E < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "E < 0");
    if (E == 0) return MPFMT_OK;
    if (!src || !dst || !mask) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "src / dst / mask is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = check_idx(ctx, src, E, "src")) || (rc = check_idx(ctx, dst, E, "dst"))) return rc;
    const int64_t words = (E + 63) / 64;
    mpfmt_tmp tmp;
    int64_t *d_s = nullptr, *d_t = nullptr; uint64_t* d_mask = nullptr;
    if ((rc = up_i64(ctx, tmp, src, E, &d_s))) return rc;
    if ((rc = up_i64(ctx, tmp, dst, E, &d_t))) return rc;
    HIPCHK(ctx, tmp.get(&d_mask, sizeof(uint64_t) * words));
    rc = mpfmt_launch_edges_free(ctx, d_s, d_t, E, d_mask);
    if (rc == MPFMT_OK) {
        hipError_t e = hipMemcpyAsync(mask, d_mask, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = mpfmt_fail(ctx, MPFMT_ERR_HIP, "edges_free copy back: %s", hipGetErrorString(e));
    }
    return rc;
}

int32_t mpfmt_mc_edges_collision(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, double sigma, int64_t rollouts,
                                 uint64_t seed, int64_t* hits)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (E < 0 || E >= ((int64_t)1 << 32)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "E out of range");
    if (rollouts < 0 || rollouts >= ((int64_t)1 << 32)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rollouts out of range [0, 2^32)");
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "sigma must be finite and >= 0");
    if (E == 0) return MPFMT_OK;
    if (!src || !dst || !hits) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "src / dst / hits is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = check_idx(ctx, src, E, "src")) || (rc = check_idx(ctx, dst, E, "dst"))) return rc;
    mpfmt_tmp tmp;
    int64_t *d_s = nullptr, *d_t = nullptr; unsigned long long* d_h = nullptr;
    if ((rc = up_i64(ctx, tmp, src, E, &d_s))) return rc;
    if ((rc = up_i64(ctx, tmp, dst, E, &d_t))) return rc;
    HIPCHK(ctx, tmp.get(&d_h, sizeof(unsigned long long) * E));
    HIPCHK(ctx, hipMemsetAsync(d_h, 0, sizeof(unsigned long long) * E, ctx->stream));
    if ((rc = mpfmt_launch_mc_edges(ctx, d_s, d_t, E, sigma, rollouts, seed, d_h))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(hits, d_h, sizeof(int64_t) * E, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

int32_t mpfmt_mc_edges_collision_is(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, double sigma, int64_t rollouts,
                                    uint64_t seed, uint64_t* wsum)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (E < 0 || E >= ((int64_t)1 << 32)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "E out of range");
    if (rollouts < 0 || rollouts >= ((int64_t)1 << 22)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rollouts out of range [0, 2^22): the weights are summed in 64 bits at 2^-40");
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "sigma must be finite and >= 0");
    if (E == 0) return MPFMT_OK;
    if (!src || !dst || !wsum) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "src / dst / wsum is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = check_idx(ctx, src, E, "src")) || (rc = check_idx(ctx, dst, E, "dst"))) return rc;
    mpfmt_tmp tmp;
    int64_t *d_s = nullptr, *d_t = nullptr; unsigned long long* d_h = nullptr;
    if ((rc = up_i64(ctx, tmp, src, E, &d_s))) return rc;
    if ((rc = up_i64(ctx, tmp, dst, E, &d_t))) return rc;
    HIPCHK(ctx, tmp.get(&d_h, sizeof(unsigned long long) * E));
    HIPCHK(ctx, hipMemsetAsync(d_h, 0, sizeof(unsigned long long) * E, ctx->stream));
    if ((rc = mpfmt_launch_mc_is_edges(ctx, d_s, d_t, E, sigma, rollouts, seed, d_h))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(wsum, d_h, sizeof(uint64_t) * E, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

// the ADAPTIVE estimator: pilot (4096 rollouts per edge, inflated noise) -> cross-entropy mean shift per edge -> mixture run
int32_t mpfmt_mc_edges_collision_ais(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, double sigma, int64_t rollouts,
                                     uint64_t seed, uint64_t* wsum, double* shifts)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (E < 0 || E >= ((int64_t)1 << 32)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "E out of range");
    if (rollouts < 0 || rollouts >= ((int64_t)1 << 22)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rollouts out of range [0, 2^22): the weights are summed in 64 bits at 2^-40");
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "sigma must be finite and >= 0");
    if (E == 0) return MPFMT_OK;
    if (!src || !dst || !wsum) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "src / dst / wsum is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = check_idx(ctx, src, E, "src")) || (rc = check_idx(ctx, dst, E, "dst"))) return rc;
    mpfmt_tmp tmp;
    int64_t *d_s = nullptr, *d_t = nullptr; unsigned long long* d_h = nullptr; double* d_mu = nullptr;
    if ((rc = up_i64(ctx, tmp, src, E, &d_s))) return rc;
    if ((rc = up_i64(ctx, tmp, dst, E, &d_t))) return rc;
    HIPCHK(ctx, tmp.get(&d_h, sizeof(unsigned long long) * E));
    HIPCHK(ctx, tmp.get(&d_mu, sizeof(double) * (size_t)E * 2 * MPFMT_MAX_DIM));
    HIPCHK(ctx, hipMemsetAsync(d_h, 0, sizeof(unsigned long long) * E, ctx->stream));
    if ((rc = mpfmt_launch_mc_ais_edges(ctx, d_s, d_t, E, sigma, rollouts, seed, d_h, d_mu))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(wsum, d_h, sizeof(uint64_t) * E, hipMemcpyDeviceToHost, ctx->stream));
    if (shifts)       // [E][2 d] out of the [E][2 MPFMT_MAX_DIM] device rows
        HIPCHK(ctx, hipMemcpy2DAsync(shifts, sizeof(double) * 2 * ctx->d, d_mu, sizeof(double) * 2 * MPFMT_MAX_DIM, sizeof(double) * 2 * ctx->d, (size_t)E,
                                     hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

static int32_t explicit_sweep(mpfmt_ctx* ctx, const double* P, const double* Q, int64_t n, uint64_t* mask)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "n < 0");
    if (n == 0) return MPFMT_OK;
    if (!P || !mask) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "P / mask is NULL");
    if (!ctx->have_boxes) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no obstacle set uploaded (mpfmt_upload_boxes)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int d = ctx->dw;
    const int64_t words = (n + 63) / 64;
    const size_t pb = sizeof(double) * (size_t)n * d;
    mpfmt_tmp tmp;
    double *dP = nullptr, *dQ = nullptr; uint64_t* d_mask = nullptr;
    HIPCHK(ctx, tmp.get(&dP, pb));
    HIPCHK(ctx, hipMemcpyAsync(dP, P, pb, hipMemcpyHostToDevice, ctx->stream));
    if (Q) {
        HIPCHK(ctx, tmp.get(&dQ, pb));
        HIPCHK(ctx, hipMemcpyAsync(dQ, Q, pb, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, tmp.get(&d_mask, sizeof(uint64_t) * words));
    int32_t rc = Q ? mpfmt_launch_motions_free(ctx, dP, dQ, n, d_mask) : mpfmt_launch_states_free(ctx, dP, n, d_mask);
    if (rc == MPFMT_OK) {
        hipError_t e = hipMemcpyAsync(mask, d_mask, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = mpfmt_fail(ctx, MPFMT_ERR_HIP, "sweep copy back: %s", hipGetErrorString(e));
    }
    return rc;
}

int32_t mpfmt_states_free(mpfmt_ctx* ctx, const double* P, int64_t n, uint64_t* mask) { return explicit_sweep(ctx, P, nullptr, n, mask); }

extern "C++" int32_t mpfmt_states_host(mpfmt_ctx* ctx, int k, std::vector<double>& X, std::vector<double>& P)
{
    const int64_t N = ctx->N;
    const int d = ctx->d;
    X.resize((size_t)N * d);
    HIPCHK(ctx, hipMemcpy(X.data(), ctx->Xo, sizeof(double) * (size_t)N * d, hipMemcpyDeviceToHost));
    P.resize((size_t)N * k);
    for (int64_t i = 0; i < N; ++i) for (int q = 0; q < k; ++q) P[(size_t)i * k + q] = X[(size_t)i * d + q];
    return MPFMT_OK;
}

int32_t mpfmt_motions_free(mpfmt_ctx* ctx, const double* P, const double* Q, int64_t n, uint64_t* mask)
{
    if (ctx && n > 0 && !Q) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "Q is NULL");
    return explicit_sweep(ctx, P, Q, n, mask);
}

int32_t mpfmt_path_free(mpfmt_ctx* ctx, const double* P, int64_t n, int32_t* free_out, uint64_t* seg_mask)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!free_out) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "free_out is NULL");
    if (n < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "n < 0");
    *free_out = 1;
    if (n < 2) return MPFMT_OK;
    if (!P) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "P is NULL");
    if (!ctx->have_boxes) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no obstacle set uploaded (mpfmt_upload_boxes)");
    const int d = ctx->dw;
    const int64_t ns = n - 1, words = (ns + 63) / 64;
    std::vector<uint64_t> m((size_t)words, 0);
    int32_t rc;
    if ((rc = explicit_sweep(ctx, P, P + d, ns, m.data()))) return rc;       // segment i = (p[i], p[i+1]): the same array, one state on
    for (int64_t i = 0; i < ns; ++i) if (!((m[i >> 6] >> (i & 63)) & 1ull)) { *free_out = 0; break; }
    if (seg_mask) memcpy(seg_mask, m.data(), sizeof(uint64_t) * (size_t)words);
    return MPFMT_OK;
}

int32_t mpfmt_graph_sweep_device(mpfmt_ctx* ctx)
{
    if (!ctx) return MPFMT_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->pend_valid = false;                                 // (outside a step: the whole sweep -- nobody checks a pending list's overflow flag here)
    return mpfmt_launch_graph_sweep(ctx);
}

int32_t mpfmt_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask)
{
    if (!ctx) return MPFMT_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if (!ctx->graph_counted) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "graph_edges_free before rdisc_count");
    if (!ctx->graph_filled && (rc = mpfmt_launch_rdisc_fill(ctx, ctx->graph_r))) return rc;
    ctx->pend_valid = false;
    if ((rc = mpfmt_launch_graph_sweep(ctx))) return rc;
    const int64_t words = (ctx->nnz + 63) / 64;
    if (words > 0) {
        if (!mask) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "mask is NULL");
        HIPCHK(ctx, hipMemcpyAsync(mask, ctx->graph_free, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MPFMT_OK;
}

// per-column reductions of the r-disc graph without storing it (kernels_rdisc_mfma.hip, MODE 3)
int32_t mpfmt_rdisc_stream(mpfmt_ctx* ctx, double r, const double* C, const uint64_t* H, int32_t want_free,
                           int64_t* deg, int64_t* free_deg, int64_t* parent, double* cost, int64_t* nnz)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->Xo && ctx->N > 0) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (!(r >= 0.0) || !std::isfinite(r)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "radius must be finite and >= 0");
    if (H && !C) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "an open set without costs");
    if (C && (!parent || !cost)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "parent / cost is NULL");
    if (want_free && !free_deg) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "free_deg is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return mpfmt_rdisc_stream_impl(ctx, r, C, H, want_free, deg, free_deg, parent, cost, nnz);
}

// ---- the resident graph + mask to the host in the ABI's format, at link speed ----------------------------------------------------------
// mpfmt_rdisc_count / _fill / mpfmt_graph_edges_free rebuild or re-sweep what a step has already left in HBM, and copy slab by slab with
// a synchronisation each.  This call hands out what mpfmt_graph_step_device left resident -- colptr and rowval as 1-based Int64, nzval,
// the free mask (BitVector chunks) -- with the index conversion on the compute stream two slabs ahead of two copy streams, so the link
// is the only thing waited for when the destinations are page-locked (mpfmt_pinned_alloc).
int32_t mpfmt_pinned_alloc(int64_t bytes, void** out)
{
    if (!out || bytes < 0) return MPFMT_ERR_ARG;
    *out = nullptr;
    if (bytes == 0) return MPFMT_OK;
    return hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault) == hipSuccess ? MPFMT_OK : MPFMT_ERR_HIP;
}

int32_t mpfmt_pinned_free(void* p)
{
    if (!p) return MPFMT_OK;
    return hipHostFree(p) == hipSuccess ? MPFMT_OK : MPFMT_ERR_HIP;
}

int32_t mpfmt_graph_export(mpfmt_ctx* ctx, int64_t* colptr, int64_t* rowval, double* nzval, uint64_t* mask, double* gb_per_s)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->graph_filled) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no resident graph (mpfmt_graph_step_device / mpfmt_graph_build_device)");
    if (mask && !ctx->graph_swept) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the resident graph has not been swept");
    const int64_t N = ctx->N, nnz = ctx->nnz;
    if (!colptr || (nnz > 0 && (!rowval || !nzval))) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "colptr / rowval / nzval is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->copy_stream[0]) {
        for (int k = 0; k < 2; ++k) {
            HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream[k], hipStreamNonBlocking));
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_conv[k], hipEventDisableTiming));
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_copy[k], hipEventDisableTiming));
        }
    }
    int32_t rc;
    const int64_t slab = (int64_t)1 << 24;                    // entries per conversion slab: 128 MB of Int64, two in flight
    void* scr;
    if ((rc = mpfmt_scratch(ctx, sizeof(int64_t) * (size_t)(2 * slab + N + 1), &scr))) return rc;
    int64_t* stg[2] = {(int64_t*)scr, (int64_t*)scr + slab};
    int64_t* cp1 = (int64_t*)scr + 2 * slab;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // the step's kernels are done: the clock below sees the export alone
    const auto t0 = std::chrono::steady_clock::now();
    // stream B: nzval, mask; stream A: colptr, rowval slabs as they are converted
    hipLaunchKernelGGL(k_add1_i64, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, ctx->stream, ctx->colptr, N + 1, cp1);
    HIPCHK(ctx, hipEventRecord(ctx->ev_conv[0], ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream[0], ctx->ev_conv[0], 0));
    HIPCHK(ctx, hipMemcpyAsync(colptr, cp1, sizeof(int64_t) * (size_t)(N + 1), hipMemcpyDeviceToHost, ctx->copy_stream[0]));
    if (nnz > 0) {
        const int64_t half = nnz / 2;
        // (the distances in two pieces, one per copy stream, so both engines stay busy while the row indices are converted)
        HIPCHK(ctx, hipMemcpyAsync(nzval, ctx->nzval, sizeof(double) * (size_t)half, hipMemcpyDeviceToHost, ctx->copy_stream[1]));
        int k = 0;
        for (int64_t o = 0; o < nnz; o += slab, ++k) {
            const int64_t n = std::min(slab, nnz - o);
            const int b = k & 1;
            if (k >= 2) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_copy[b], 0));      // the slab's staging buffer has been copied out
            hipLaunchKernelGGL(k_i32_to_i64_add1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rowval + o, n, stg[b]);
            HIPCHK(ctx, hipEventRecord(ctx->ev_conv[b], ctx->stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream[0], ctx->ev_conv[b], 0));
            HIPCHK(ctx, hipMemcpyAsync(rowval + o, stg[b], sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->copy_stream[0]));
            HIPCHK(ctx, hipEventRecord(ctx->ev_copy[b], ctx->copy_stream[0]));
        }
        HIPCHK(ctx, hipMemcpyAsync(nzval + half, ctx->nzval + half, sizeof(double) * (size_t)(nnz - half), hipMemcpyDeviceToHost, ctx->copy_stream[1]));
        if (mask) HIPCHK(ctx, hipMemcpyAsync(mask, ctx->graph_free, sizeof(uint64_t) * (size_t)((nnz + 63) / 64), hipMemcpyDeviceToHost, ctx->copy_stream[1]));
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream[0]));
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream[1]));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const double bytes = 8.0 * (double)(N + 1) + 16.0 * (double)nnz + (mask ? (double)((nnz + 63) / 64) * 8.0 : 0.0);
    if (gb_per_s) *gb_per_s = sec > 0.0 ? bytes / sec / 1e9 : 0.0;
    return MPFMT_OK;
}

// Page-locked export arena that lives as long as the ctx (grow-only, freed by mpfmt_ctx_destroy): page-locking gigabytes costs
// ~0.2 s per GB (hipHostMalloc), far more than the copy it speeds up -- paid once per ctx here, not once per graph.
int32_t mpfmt_export_arena(mpfmt_ctx* ctx, int64_t bytes, void** out)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!out || bytes < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "mpfmt_export_arena: bad arguments");
    *out = nullptr;
    if ((size_t)bytes > ctx->export_arena.bytes()) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        // (an eighth of slack: the next graph of the same problem -- new samples, new obstacles -- finds its room in place)
        int32_t rc;
        if ((rc = ctx->export_arena.ensure(ctx, (size_t)bytes + (size_t)bytes / 8 + 4096))) return rc;
    }
    *out = ctx->export_arena;
    return MPFMT_OK;
}

// mpfmt_graph_export into the ctx's own arena: the four arrays are carved out of it (64-byte aligned) and stay valid until the next
// export of this ctx or its destruction -- the drop-in precompute! of julia/MPFmtHIP.jl wraps them without a copy.
int32_t mpfmt_graph_export_pinned(mpfmt_ctx* ctx, int64_t** colptr, int64_t** rowval, double** nzval, uint64_t** mask, int64_t* nnz_out, double* gb_per_s)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!colptr || !rowval || !nzval) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "colptr / rowval / nzval is NULL");
    if (!ctx->graph_filled) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no resident graph (mpfmt_graph_step_device / mpfmt_graph_build_device)");
    // (every state error of mpfmt_graph_export is raised BEFORE the arena is touched: growing it frees the block the previous export's
    // pointers -- still held by the caller on a failed call -- point into)
    if (mask && !ctx->graph_swept) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the resident graph has not been swept");
    const int64_t N = ctx->N, nnz = ctx->nnz, words = (nnz + 63) / 64;
    auto al = [](size_t b) { return (b + 63) & ~(size_t)63; };
    const size_t o_cp = 0, o_rv = al(8 * (size_t)(N + 1)), o_nz = o_rv + al(8 * (size_t)std::max<int64_t>(nnz, 1));
    const size_t o_mk = o_nz + al(8 * (size_t)std::max<int64_t>(nnz, 1)), total = o_mk + al(8 * (size_t)std::max<int64_t>(words, 1));
    void* base = nullptr;
    int32_t rc;
    if ((rc = mpfmt_export_arena(ctx, (int64_t)total, &base))) return rc;
    char* b = (char*)base;
    *colptr = (int64_t*)(b + o_cp); *rowval = (int64_t*)(b + o_rv); *nzval = (double*)(b + o_nz);
    if (mask) *mask = (uint64_t*)(b + o_mk);
    if (nnz_out) *nnz_out = nnz;
    return mpfmt_graph_export(ctx, *colptr, *rowval, *nzval, mask ? *mask : nullptr, gb_per_s);
}

int32_t mpfmt_graph_device_ptrs(mpfmt_ctx* ctx, void** colptr, void** rowval, void** nzval, void** free_mask)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->graph_filled) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no resident graph");
    if (colptr) *colptr = ctx->colptr;
    if (rowval) *rowval = ctx->rowval;
    if (nzval) *nzval = ctx->nzval;
    if (free_mask) *free_mask = ctx->graph_swept ? ctx->graph_free : nullptr;
    return MPFMT_OK;
}

int32_t mpfmt_shard_info(mpfmt_ctx* ctx, int64_t* col_begin, int64_t* col_end, int64_t* shard_nnz)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->graph_counted) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no graph counted");
    if (col_begin) *col_begin = std::min<int64_t>(ctx->tile_begin * 64, ctx->N);
    if (col_end) *col_end = std::min<int64_t>(ctx->tile_end * 64, ctx->N);
    if (shard_nnz) *shard_nnz = ctx->nnz;
    return MPFMT_OK;
}

// ---- Euclidean per-edge steer (geometric.jl:18-19) ---------------------------------------------------------------------

int32_t mpfmt_euclid_steer(mpfmt_ctx* ctx, const int64_t* src, const int64_t* dst, int64_t E, double* t, double* u)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (E < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "E < 0");
    if (E == 0) return MPFMT_OK;
    if (!src || !dst || !t || !u) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "src / dst / t / u is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = check_idx(ctx, src, E, "src")) || (rc = check_idx(ctx, dst, E, "dst"))) return rc;
    const int d = ctx->d;
    mpfmt_tmp tmp;
    int64_t *d_s = nullptr, *d_t = nullptr; double *dt = nullptr, *du = nullptr;
    if ((rc = up_i64(ctx, tmp, src, E, &d_s))) return rc;
    if ((rc = up_i64(ctx, tmp, dst, E, &d_t))) return rc;
    HIPCHK(ctx, tmp.get(&dt, sizeof(double) * (size_t)E));
    HIPCHK(ctx, tmp.get(&du, sizeof(double) * (size_t)E * d));
    if ((rc = mpfmt_launch_euclid_steer(ctx, d_s, d_t, E, dt, du))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(t, dt, sizeof(double) * (size_t)E, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(u, du, sizeof(double) * (size_t)E * d, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

int32_t mpfmt_euclid_propagate(mpfmt_ctx* ctx, const int64_t* src, int64_t E, const double* t, const double* u, const double* s, double* out)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (E < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "E < 0");
    if (E == 0) return MPFMT_OK;
    if (!src || !t || !u || !out) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "src / t / u / out is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = check_idx(ctx, src, E, "src"))) return rc;
    const int d = ctx->d;
    mpfmt_tmp tmp;
    int64_t* d_s = nullptr; double *dt = nullptr, *du = nullptr, *ds = nullptr, *dout = nullptr;
    if ((rc = up_i64(ctx, tmp, src, E, &d_s))) return rc;
    HIPCHK(ctx, tmp.get(&dt, sizeof(double) * (size_t)E));
    HIPCHK(ctx, tmp.get(&du, sizeof(double) * (size_t)E * d));
    HIPCHK(ctx, tmp.get(&dout, sizeof(double) * (size_t)E * d));
    HIPCHK(ctx, hipMemcpyAsync(dt, t, sizeof(double) * (size_t)E, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(du, u, sizeof(double) * (size_t)E * d, hipMemcpyHostToDevice, ctx->stream));
    if (s) {
        HIPCHK(ctx, tmp.get(&ds, sizeof(double) * (size_t)E));
        HIPCHK(ctx, hipMemcpyAsync(ds, s, sizeof(double) * (size_t)E, hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = mpfmt_launch_euclid_propagate(ctx, d_s, E, dt, du, ds, dout))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out, dout, sizeof(double) * (size_t)E * d, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

// ---- expand --------------------------------------------------------------------------------------------

int32_t mpfmt_expand(mpfmt_ctx* ctx, const uint64_t* W, const uint64_t* H, const uint64_t* F, const double* C,
                     const int64_t* zs, int64_t nz,
                     int64_t* xs, int64_t* ymin, double* cmin, uint8_t* free_out, int64_t cap, int64_t* nx)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!W || !H || !C || !nx) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "W / H / C / nx is NULL");
    if (nz < 0 || cap < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "nz / cap < 0");
    if (!ctx->graph_filled) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "expand needs a built r-disc graph (mpfmt_rdisc_count + fill)");
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "expand runs on an unsharded ctx (a shard holds only its own columns: the frontier would be partial); the sharded batch step is mpfmt_wf_step");
    if (!ctx->have_boxes) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no obstacle set uploaded (mpfmt_upload_boxes)");
    *nx = 0;
    if (nz == 0) return MPFMT_OK;
    if (!zs) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "zs is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = check_idx(ctx, zs, nz, "zs"))) return rc;
    const int64_t N = ctx->N, words = (N + 63) / 64;
    mpfmt_tmp tmp;
    uint64_t *dW = nullptr, *dH = nullptr, *dF = nullptr; double* dC = nullptr; int64_t* dz = nullptr;
    int64_t *dxs = nullptr, *dym = nullptr; double* dcm = nullptr; uint8_t* dfr = nullptr;
    const int64_t capd = std::max<int64_t>(cap, 1);
    HIPCHK(ctx, tmp.get(&dW, 8 * words)); HIPCHK(ctx, tmp.get(&dH, 8 * words));
    HIPCHK(ctx, tmp.get(&dC, 8 * N));
    HIPCHK(ctx, hipMemcpyAsync(dW, W, 8 * words, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dH, H, 8 * words, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dC, C, 8 * N, hipMemcpyHostToDevice, ctx->stream));
    if (F) { HIPCHK(ctx, tmp.get(&dF, 8 * words)); HIPCHK(ctx, hipMemcpyAsync(dF, F, 8 * words, hipMemcpyHostToDevice, ctx->stream)); }
    if ((rc = up_i64(ctx, tmp, zs, nz, &dz))) return rc;
    HIPCHK(ctx, tmp.get(&dxs, 8 * capd)); HIPCHK(ctx, tmp.get(&dym, 8 * capd));
    HIPCHK(ctx, tmp.get(&dcm, 8 * capd)); HIPCHK(ctx, tmp.get(&dfr, capd));
    rc = mpfmt_launch_expand(ctx, dW, dH, dF, dC, dz, nz, dxs, dym, dcm, dfr, cap, nx);
    if (rc == MPFMT_OK && *nx > 0) {
        const int64_t n = *nx;
        if (!xs || !ymin || !cmin || !free_out) rc = mpfmt_fail(ctx, MPFMT_ERR_ARG, "output array is NULL");
        else {
            hipMemcpyAsync(xs, dxs, 8 * n, hipMemcpyDeviceToHost, ctx->stream);
            hipMemcpyAsync(ymin, dym, 8 * n, hipMemcpyDeviceToHost, ctx->stream);
            hipMemcpyAsync(cmin, dcm, 8 * n, hipMemcpyDeviceToHost, ctx->stream);
            hipMemcpyAsync(free_out, dfr, n, hipMemcpyDeviceToHost, ctx->stream);
            hipError_t e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) rc = mpfmt_fail(ctx, MPFMT_ERR_HIP, "expand copy back: %s", hipGetErrorString(e));
        }
    }
    return rc;
}

// ---- what the single-shot planners share with the calls around them (the planners themselves: "one driver", below) ------------

// The sequential recursion itself (fmt.jl:43-101 over finished arrays), the binary heap, the goal predicates and the goal pick live in
// mpfmt_host.cpp: plain C++ without HIP, so the same translation unit is also built with -fsanitize=address,undefined for the
// CPU test suite (tests/asan/).
static inline bool bit(const std::vector<uint64_t>& m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1ull; }

using stamp = std::chrono::steady_clock::time_point;
static stamp now() { return std::chrono::steady_clock::now(); }

// the timing fields of a plan from its stamps: start, checkpts bitmap, graph built, graph swept, recursion begun, recursion done
static void fmt_times(const mpfmt_ctx* ctx, mpfmt_fmt_result* res, const stamp (&t)[6])
{
    auto ms = [](stamp a, stamp b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    res->nnz = ctx->nnz;
    res->ms_graph = ms(t[1], t[2]);
    res->ms_sweep = ms(t[0], t[1]) + ms(t[2], t[3]);
    res->ms_host_loop = ms(t[4], t[5]);
}

// the resident graph on the host for a recursion there: CSC (0-based rows), per-edge free bits and, for a steering graph, the
// per-edge segment counts of its sweep
struct host_graph {
    std::vector<int64_t> colptr; std::vector<int32_t> rowval; std::vector<double> nzval; std::vector<uint64_t> efree; std::vector<uint8_t> nseg;
};

static int32_t graph_to_host(mpfmt_ctx* ctx, bool want_nseg, host_graph& g)
{
    const int64_t N = ctx->N, nnz = ctx->nnz;
    const size_t n1 = (size_t)std::max<int64_t>(nnz, 1), words = (size_t)(nnz + 63) / 64;
    g.colptr.resize(N + 1);
    g.rowval.resize(n1);
    g.nzval.resize(n1);
    g.efree.resize(std::max<size_t>(words, 1));
    if (want_nseg) g.nseg.resize(n1);
    HIPCHK(ctx, hipMemcpy(g.colptr.data(), ctx->colptr, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost));
    if (nnz > 0) {
        HIPCHK(ctx, hipMemcpy(g.rowval.data(), ctx->rowval, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(g.nzval.data(), ctx->nzval, sizeof(double) * nnz, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(g.efree.data(), ctx->graph_free, sizeof(uint64_t) * words, hipMemcpyDeviceToHost));
        if (want_nseg) HIPCHK(ctx, hipMemcpy(g.nseg.data(), ctx->steer_nseg, (size_t)nnz, hipMemcpyDeviceToHost));
    }
    return MPFMT_OK;
}

// ---- k-nearest connections (connections = :K, fmt.jl:6,17-19; mutualknnF! / knnB!, nearneighbors.jl:9-11; kernels_knn.hip) ----------

static bool knn_resident(const mpfmt_ctx* ctx) { return ctx->knn_k > 0 && ctx->graph_filled; }
// ... and it is the graph a call with this k would build: a column holds min(k, N - 1) entries
static bool knn_resident_k(const mpfmt_ctx* ctx, int64_t k) { return knn_resident(ctx) && std::min(ctx->knn_k, ctx->N - 1) == std::min(k, ctx->N - 1); }

int32_t mpfmt_knn_count(mpfmt_ctx* ctx, int64_t k, int64_t* colptr, int64_t* nnz)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!colptr || !nnz) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "colptr / nnz is NULL");
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the k-nearest graph needs an unsharded ctx");
    if (k < 1) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "k must be >= 1");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = mpfmt_knn_build(ctx, k))) return rc;
    if ((rc = colptr_to_host(ctx, colptr))) return rc;
    *nnz = ctx->nnz;
    return MPFMT_OK;
}

int32_t mpfmt_knn_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval, uint64_t* mutual)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!knn_resident(ctx)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "knn_fill before knn_count");
    if (ctx->nnz > 0 && (!rowval || !nzval)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rowval / nzval is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    const int64_t nnz = ctx->nnz;
    if (nnz > 0) {
        const int64_t slab = std::min<int64_t>(nnz, (int64_t)1 << 26);
        void* scr;
        if ((rc = mpfmt_scratch(ctx, sizeof(int64_t) * slab, &scr))) return rc;
        for (int64_t o = 0; o < nnz; o += slab) {
            const int64_t n = std::min(slab, nnz - o);
            hipLaunchKernelGGL(k_i32_to_i64_add1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rowval + o, n, (int64_t*)scr);
            HIPCHK(ctx, hipMemcpyAsync(rowval + o, scr, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        HIPCHK(ctx, hipMemcpyAsync(nzval, ctx->nzval, sizeof(double) * nnz, hipMemcpyDeviceToHost, ctx->stream));
        if (mutual) HIPCHK(ctx, hipMemcpyAsync(mutual, ctx->knn_mutual, sizeof(uint64_t) * (size_t)((nnz + 63) / 64), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MPFMT_OK;
}

int32_t mpfmt_knn_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!knn_resident(ctx)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "knn_graph_edges_free before knn_count");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    ctx->pend_valid = false;
    if ((rc = mpfmt_launch_graph_sweep(ctx))) return rc;
    const int64_t words = (ctx->nnz + 63) / 64;
    if (words > 0) {
        if (!mask) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "mask is NULL");
        HIPCHK(ctx, hipMemcpyAsync(mask, ctx->graph_free, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MPFMT_OK;
}

// ---- PRM* roadmap queries: shortest paths over the resident free-edge graph (kernels_sssp.hip) -------------------------------------------

// the checks every field over the resident graph starts with -- r-disc, k-nearest or a filled and swept steering graph (the same device
// slots and the same direction convention); nothing in the ctx has been touched when one of them refuses
static int32_t sssp_ready(mpfmt_ctx* ctx)
{
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "roadmap queries run on an unsharded ctx");
    if (ctx->Xo && ctx->steer_filled) {
        if (!ctx->steer_swept || !ctx->graph_free)                  // (as for the Euclidean mask; only checkpts asks for an obstacle set)
            return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no free-edge mask for the resident steering graph and the current obstacle set (sweep it: "
                                                    "mpfmt_di_graph_edges_free, mpfmt_dubins_graph_edges_free, mpfmt_reedsshepp_graph_edges_free)");
        return MPFMT_OK;
    }
    if (!ctx->Xo || !ctx->graph_filled) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no resident r-disc or k-nearest graph (mpfmt_graph_step_device, mpfmt_knn_count)");
    if (!ctx->graph_swept || !ctx->graph_free)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no free-edge mask for the resident graph and the current obstacle set (sweep it: mpfmt_graph_step_device, "
                                                "mpfmt_graph_edges_free, mpfmt_knn_graph_edges_free)");
    return MPFMT_OK;
}

// what the tracked cost-to-come field and the Euclidean external-state queries ask: a Euclidean graph (the repair of kernels_field.hip
// rests on the Euclidean graph state, and mpfmt_roadmap_* attach by the Euclidean distance and segment test -- a steering graph has
// mpfmt_steer_roadmap_*, below; the tracked cost-to-go field of kernels_togo.hip asks sssp_ready alone)
static int32_t sssp_ready_euclid(mpfmt_ctx* ctx)
{
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "roadmap queries run on an unsharded ctx");
    if (ctx->Xo && ctx->steer_filled)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "tracked fields and external states: Euclidean graphs only (the resident graph is a steering graph)");
    return sssp_ready(ctx);
}

static int32_t steer_point_bitmap(mpfmt_ctx* ctx);      // (with the steering planners' prelude, below)

// the Euclidean checkpts bitmap of the current samples and obstacle set into ctx->sssp_F
static int32_t sssp_point_bitmap(mpfmt_ctx* ctx)
{
    int32_t rc;
    if ((rc = ctx->sssp_F.ensure(ctx, sizeof(uint64_t) * (size_t)((ctx->N + 63) / 64)))) return rc;
    return mpfmt_launch_points_free(ctx, nullptr, ctx->N, ctx->sssp_F);
}

// the checkpts bitmap of a field over the RESIDENT graph, for the entry points that sssp_ready has just admitted: what is resident is a
// steering graph (the bitmap of the steering planners) or a Euclidean one.  Planners that build a graph of their own do not come here: a
// steering graph left in the ctx says nothing about the graph they are about to build.
static int32_t sssp_resident_bitmap(mpfmt_ctx* ctx)
{
    if (!ctx->steer_filled) return sssp_point_bitmap(ctx);
    int32_t rc;
    if ((rc = ctx->sssp_F.ensure(ctx, sizeof(uint64_t) * (size_t)((ctx->N + 63) / 64)))) return rc;
    return steer_point_bitmap(ctx);
}

// The prelude of a field call over the resident graph: the ready check (euclid: the Euclidean graph the tracked field asks for), the
// checkpts refusal, the 1-based index list idx[0 .. n) (`what` names it in the error), hipSetDevice, and with checkpts the point bitmap:
// *d_F = ctx->sssp_F, or nullptr without checkpts.  A caller that will run nothing (no source) passes d_F = nullptr and gets the checks
// alone.  Nothing in the ctx has been touched when a check refuses.
static int32_t field_prelude(mpfmt_ctx* ctx, const int64_t* idx, int64_t n, const char* what, bool euclid, int32_t checkpts, const uint64_t** d_F)
{
    int32_t rc;
    if (d_F) *d_F = nullptr;
    if ((rc = euclid ? sssp_ready_euclid(ctx) : sssp_ready(ctx))) return rc;
    if (checkpts && !ctx->have_boxes && ctx->cc_kind == 0) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "checkpts needs an obstacle set");
    if ((rc = check_idx(ctx, idx, n, what))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!checkpts || !d_F) return MPFMT_OK;
    if ((rc = sssp_resident_bitmap(ctx))) return rc;                     // (the Euclidean bitmap whenever euclid: no steering graph got past)
    *d_F = ctx->sssp_F.get();
    return MPFMT_OK;
}

int32_t mpfmt_graph_sssp(mpfmt_ctx* ctx, const int64_t* sources, int64_t nsrc, int32_t checkpts, double* C, int64_t* A, mpfmt_sssp_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (nsrc < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "nsrc < 0");
    if (nsrc > 0 && (!sources || !C)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "sources / C is NULL");
    int32_t rc;
    const uint64_t* d_F = nullptr;
    if ((rc = field_prelude(ctx, sources, nsrc, "sources", false, checkpts, nsrc > 0 ? &d_F : nullptr))) return rc;
    const int64_t N = ctx->N;
    for (int64_t q = 0; q < nsrc; ++q)
        if ((rc = mpfmt_sssp_device(ctx, sources[q] - 1, d_F, C + q * N, A ? A + q * N : nullptr, info ? info + q : nullptr))) return rc;
    return MPFMT_OK;
}

// the same fields, up to 64 sources per pass over the graph (kernels_sssp_multi.hip)
int32_t mpfmt_graph_sssp_multi(mpfmt_ctx* ctx, const int64_t* sources, int64_t nsrc, int32_t checkpts, double* C, int64_t* A, mpfmt_sssp_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (nsrc < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "nsrc < 0");
    if (nsrc > 0 && (!sources || !C)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "sources / C is NULL");
    int32_t rc;
    const uint64_t* d_F = nullptr;
    if ((rc = field_prelude(ctx, sources, nsrc, "sources", false, checkpts, nsrc > 0 ? &d_F : nullptr))) return rc;
    if (nsrc == 0) return MPFMT_OK;
    return mpfmt_sssp_multi_device(ctx, sources, nsrc, d_F, C, A, info);
}

// the cost-to-go field of a target set over whatever swept graph is resident (kernels_sssp_to.hip)
int32_t mpfmt_graph_sssp_to(mpfmt_ctx* ctx, const int64_t* targets, int64_t ntgt, int32_t checkpts, double* G, int64_t* S, mpfmt_sssp_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (ntgt < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "ntgt < 0");
    if (!G || (ntgt > 0 && !targets)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "targets / G is NULL");
    int32_t rc;
    const uint64_t* d_F;
    if ((rc = field_prelude(ctx, targets, ntgt, "targets", false, checkpts, &d_F))) return rc;
    return mpfmt_sssp_to_device(ctx, targets, ntgt, d_F, G, S, info);
}

// ---- a tracked field: kept valid across in-place box edits (kernels_field.hip) -----------------------------------------------------------

int32_t mpfmt_field_begin(mpfmt_ctx* ctx, int64_t source, int32_t checkpts, mpfmt_field_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    int32_t rc;
    const uint64_t* d_F;
    if ((rc = field_prelude(ctx, &source, 1, "source", true, checkpts, &d_F))) return rc;
    return mpfmt_field_compute(ctx, source - 1, checkpts ? 1 : 0, d_F, info);
}

int32_t mpfmt_field_update(mpfmt_ctx* ctx, mpfmt_field_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!mpfmt_field_live(ctx)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no tracked field (mpfmt_field_begin)");
    int32_t rc;
    const bool history = mpfmt_field_history(ctx);                       // no build and no whole sweep since the field was last valid
    const bool stands = history && !ctx->fld_dirty_any;                   // nothing was flagged: the field stands, and no bitmap is needed
    const int32_t checkpts = ctx->fld_checkpts;                           // (begun over an obstacle set, and a ctx never loses its set)
    const uint64_t* d_F = nullptr;
    if ((rc = field_prelude(ctx, nullptr, 0, nullptr, true, checkpts, stands ? nullptr : &d_F))) return rc;
    if (stands) {
        ctx->fld_path = 1;
        ctx->fld_invalidated = ctx->fld_dirty_columns = ctx->fld_columns_read = ctx->fld_column_visits = ctx->fld_entries_read = 0;
        ctx->fld_rounds = ctx->fld_relax = 0;
        if (info) {
            memset(info, 0, sizeof *info);
            info->reached = ctx->fld_reached; info->path = 1;
        }
        return MPFMT_OK;
    }
    if (!history) return mpfmt_field_compute(ctx, ctx->fld_source0, checkpts, d_F, info);
    if ((rc = mpfmt_field_repair(ctx, d_F, info))) { mpfmt_field_drop_internal(ctx); return rc; }      // (a repair cut short leaves no field)
    return MPFMT_OK;
}

int32_t mpfmt_field_read(mpfmt_ctx* ctx, double* C, int64_t* A)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!mpfmt_field_live(ctx)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no tracked field (mpfmt_field_begin)");
    if (ctx->fld_grown) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the sample set grew since the tracked field was last valid (mpfmt_field_update)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)ctx->N;
    if (C) HIPCHK(ctx, hipMemcpyAsync(C, ctx->fld_C, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream));
    if (A) HIPCHK(ctx, hipMemcpyAsync(A, ctx->fld_A, sizeof(int64_t) * N, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

int32_t mpfmt_field_goal(mpfmt_ctx* ctx, int32_t goal_kind, const double* goal_params, int64_t* path, mpfmt_fmt_result* res)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!path || !res || !goal_params) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "NULL output / goal pointer");
    if (goal_kind < 0 || goal_kind > 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "unknown goal kind %d", goal_kind);
    if (ctx->Xo && ctx->steer_filled)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "tracked fields and external states: Euclidean graphs only (the resident graph is a steering graph)");
    if (!mpfmt_field_live(ctx)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no tracked field (mpfmt_field_begin)");
    if (ctx->fld_grown) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the sample set grew since the tracked field was last valid (mpfmt_field_update)");
    if (ctx->fld_dirty_any || !mpfmt_field_history(ctx) || !ctx->graph_swept)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the box set was edited since the tracked field was last valid (mpfmt_field_update)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t N = ctx->N, init_idx = ctx->fld_source0 + 1;
    const int d = ctx->d;
    memset(res, 0, sizeof *res);
    const stamp t0 = now();
    std::vector<double> X((size_t)N * d), C((size_t)N);
    std::vector<int64_t> A((size_t)N);
    HIPCHK(ctx, hipMemcpyAsync(X.data(), ctx->Xo, sizeof(double) * (size_t)N * d, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(C.data(), ctx->fld_C, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(A.data(), ctx->fld_A, sizeof(int64_t) * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    mpfmt_walk_back(N, C.data(), A.data(), init_idx, mpfmt_goal_pick(N, d, d, X.data(), C.data(), goal_kind, goal_params), path, res);
    res->nnz = ctx->nnz;
    res->ms_host_loop = std::chrono::duration<double, std::milli>(now() - t0).count();
    return MPFMT_OK;
}

int32_t mpfmt_field_drop(mpfmt_ctx* ctx)
{
    if (!ctx) return MPFMT_ERR_ARG;
    mpfmt_field_drop_internal(ctx);
    return MPFMT_OK;
}

// ---- a tracked cost-to-go field: kept valid across in-place box edits on any resident swept graph (kernels_togo.hip) -----------------------

int32_t mpfmt_togo_begin(mpfmt_ctx* ctx, const int64_t* targets, int64_t ntgt, int32_t checkpts, mpfmt_togo_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (ntgt < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "ntgt < 0");
    if (ntgt > 0 && !targets) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "targets is NULL");
    int32_t rc;
    const uint64_t* d_F;
    if ((rc = field_prelude(ctx, targets, ntgt, "targets", false, checkpts, &d_F))) return rc;
    return mpfmt_togo_compute(ctx, targets, ntgt, checkpts ? 1 : 0, d_F, info);
}

int32_t mpfmt_togo_update(mpfmt_ctx* ctx, mpfmt_togo_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!mpfmt_togo_live(ctx)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no tracked cost-to-go field (mpfmt_togo_begin)");
    int32_t rc;
    const bool history = mpfmt_togo_history(ctx);                        // no build and no whole sweep since the field was last valid
    const bool stands = history && !ctx->tg_dirty_any;                    // nothing was flagged: the field stands, and no bitmap is needed
    const int32_t checkpts = ctx->tg_checkpts;                            // (begun over an obstacle set, and a ctx never loses its set)
    const uint64_t* d_F = nullptr;
    if ((rc = field_prelude(ctx, nullptr, 0, nullptr, false, checkpts, stands ? nullptr : &d_F))) return rc;
    if (stands) {
        ctx->tg_path = 1;
        ctx->tg_invalidated = ctx->tg_dirty_columns = ctx->tg_columns_read = ctx->tg_column_visits = ctx->tg_entries_read = 0;
        ctx->tg_rounds = ctx->tg_relax = ctx->tg_atomics = 0;
        if (info) {
            memset(info, 0, sizeof *info);
            info->reached = ctx->tg_reached; info->path = 1;
        }
        return MPFMT_OK;
    }
    if (!history) return mpfmt_togo_compute(ctx, ctx->tg_targets.data(), (int64_t)ctx->tg_targets.size(), checkpts, d_F, info);
    if ((rc = mpfmt_togo_repair(ctx, d_F, info))) { mpfmt_togo_drop_internal(ctx); return rc; }      // (a repair cut short leaves no field)
    return MPFMT_OK;
}

int32_t mpfmt_togo_read(mpfmt_ctx* ctx, double* G, int64_t* S)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!mpfmt_togo_live(ctx)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no tracked cost-to-go field (mpfmt_togo_begin)");
    if (ctx->tg_grown) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "the sample set grew since the tracked cost-to-go field was last valid (mpfmt_togo_update)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)ctx->N;
    if (G) HIPCHK(ctx, hipMemcpyAsync(G, ctx->tg_G, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream));
    if (S) HIPCHK(ctx, hipMemcpyAsync(S, ctx->tg_S, sizeof(int64_t) * N, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

// targets that join the tracked set: label decreases, pending until the next mpfmt_togo_update.  A refusal has touched nothing
int32_t mpfmt_togo_targets_add(mpfmt_ctx* ctx, const int64_t* targets, int64_t ntgt)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (ntgt < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "ntgt < 0");
    if (ntgt > 0 && !targets) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "targets is NULL");
    if (!mpfmt_togo_live(ctx)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no tracked cost-to-go field (mpfmt_togo_begin)");
    int32_t rc;
    if ((rc = check_idx(ctx, targets, ntgt, "targets"))) return rc;
    if (ntgt == 0) return MPFMT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return mpfmt_togo_add_targets(ctx, targets, ntgt);
}

int32_t mpfmt_togo_drop(mpfmt_ctx* ctx)
{
    if (!ctx) return MPFMT_ERR_ARG;
    mpfmt_togo_drop_internal(ctx);
    return MPFMT_OK;
}

// ---- roadmap queries for external states (kernels_roadmap.hip, the seeded field of kernels_sssp.hip) ---------------------------------------

// what every call on external states asks of the ctx; nothing has been touched when it refuses
static int32_t roadmap_ready(mpfmt_ctx* ctx)
{
    // (what the ctx IS comes before what it has ready: a wrong checker or workspace is named as such, not as the stale mask its upload left)
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "roadmap queries run on an unsharded ctx");
    if (ctx->Xo && ctx->steer_filled)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "tracked fields and external states: Euclidean graphs only (the resident graph is a steering graph)");
    if (ctx->knn_k > 0 && ctx->graph_filled) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "external states attach to an r-disc graph: the resident graph is a k-nearest one");
    if (ctx->cc_kind != 0) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "external states need the N-D box checker (the 2-D SAT world is resident)");
    if (ctx->have_boxes && ctx->Xo && ctx->dw != ctx->d)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "external states need an identity workspace (dw = %d, d = %d)", ctx->dw, ctx->d);
    int32_t rc;
    if ((rc = sssp_ready_euclid(ctx))) return rc;
    if (!(ctx->graph_r >= 0.0)) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no resident r-disc graph");
    if (!ctx->have_boxes) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no obstacle set uploaded (mpfmt_upload_boxes)");
    return MPFMT_OK;
}

// ---- adaptive shortcutting of solution paths (kernels_shortcut.hip; host reference: mpfmt_host_adaptive_shortcut) ------------------------

int32_t mpfmt_adaptive_shortcut_batch(mpfmt_ctx* ctx, const double* P, const int64_t* offsets, int64_t B, int32_t iterations, int64_t max_states,
                                      double* out_P, int64_t* out_offsets, int64_t out_cap, double* cumcost, mpfmt_shortcut_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (B < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: B < 0");
    if (!offsets || !out_offsets) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: offsets / out_offsets is NULL");
    if (B > 0 && (!P || !out_P || !cumcost || !info)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: P / out_P / cumcost / info is NULL");
    if (iterations < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: iterations < 0");
    if (max_states < 2 || max_states > (1 << 20)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: max_states must lie in [2, 2^20]");
    if (out_cap < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: out_cap < 0");
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "adaptive_shortcut runs on an unsharded ctx");
    if (!ctx->have_boxes) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no obstacle set uploaded (mpfmt_upload_boxes / mpfmt_upload_shapes2d)");
    const int d = ctx->dw;
    if (offsets[0] != 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: offsets[0] must be 0");
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        if (n < 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: path %lld has %lld states (a path has at least 2)", (long long)(b + 1), (long long)n);
        if (n > max_states) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: path %lld has %lld states > max_states = %lld", (long long)(b + 1), (long long)n, (long long)max_states);
    }
    const int64_t total = offsets[B];
    for (int64_t i = 0; i < total * d; ++i)
        if (!std::isfinite(P[i])) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: non-finite coordinate in state %lld", (long long)(i / d + 1));
    out_offsets[0] = 0;
    if (B == 0) return MPFMT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return mpfmt_shortcut_batch_device(ctx, P, offsets, B, iterations, max_states, out_P, out_offsets, out_cap, cumcost, info);
}

int32_t mpfmt_adaptive_shortcut(mpfmt_ctx* ctx, const double* P, int64_t n, int32_t iterations, int64_t max_states, double* out_P, int64_t out_cap,
                                double* cumcost, mpfmt_shortcut_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n < 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "adaptive_shortcut: a path has at least 2 states");
    const int64_t offsets[2] = {0, n};
    int64_t out_offsets[2] = {0, 0};
    return mpfmt_adaptive_shortcut_batch(ctx, P, offsets, 1, iterations, max_states, out_P, out_offsets, out_cap, cumcost, info);
}

// ---- time discretisation of solution paths (kernels_discretize.hip; host reference: mpfmt_host_discretize) --------------------------------
int32_t mpfmt_discretize_batch(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const int64_t* offsets,
                               int64_t B, int32_t mode, double dt, int64_t n_samples, int32_t append_end, double* out_X, double* out_T,
                               int32_t* out_seg, int64_t* out_offsets, int64_t out_cap, mpfmt_disc_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (B < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: B < 0");
    if (!offsets || !out_offsets) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: offsets / out_offsets is NULL");
    if (B > 0 && (!P || !info)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: P / info is NULL");
    if (out_cap < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: out_cap < 0");
    if (out_cap > 0 && (!out_X || !out_T)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: out_X / out_T is NULL");
    if (const char* why = mpfmt_disc_check(space, d, params, mode, dt, n_samples)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: %s", why);
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "discretize runs on an unsharded ctx");
    if (offsets[0] != 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: offsets[0] must be 0");
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        if (n < 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: path %lld has %lld states (a path has at least 2)", (long long)(b + 1), (long long)n);
    }
    const int64_t total = offsets[B];
    if (total > (int64_t)1 << 40) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: the batch holds more than 2^40 states");
    for (int64_t i = 0; i < total * d; ++i)
        if (!std::isfinite(P[i])) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: non-finite coordinate in state %lld", (long long)(i / d + 1));
    out_offsets[0] = 0;
    ctx->disc_steps = 0; ctx->disc_samples = 0;
    if (B == 0) return MPFMT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return mpfmt_discretize_batch_device(ctx, space, d, params, P, offsets, B, mode, dt, n_samples, append_end, out_X, out_T, out_seg, out_offsets,
                                         out_cap, info);
}

int32_t mpfmt_discretize(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, int64_t n, int32_t mode, double dt,
                         int64_t n_samples, int32_t append_end, double* out_X, double* out_T, int32_t* out_seg, int64_t out_cap,
                         mpfmt_disc_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n < 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: a path has at least 2 states");
    const int64_t offsets[2] = {0, n};
    int64_t out_offsets[2];
    return mpfmt_discretize_batch(ctx, space, d, params, P, offsets, 1, mode, dt, n_samples, append_end, out_X, out_T, out_seg, out_offsets, out_cap,
                                  info);
}

// ---- steering shortcut (kernels_steershortcut.hip): the pair primitive and the batch --------------------------------------------------------
// space / d / params and the resident checker, bound as the space's graph sweep expects it
static int32_t steer_space_check(mpfmt_ctx* ctx, const char* who, int32_t space, int32_t d, const double* params)
{
    if (space == MPFMT_SPACE_EUCLID) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%s: a steering space is needed (the Euclidean calls are mpfmt_motions_free / mpfmt_adaptive_shortcut)", who);
    if (const char* why = mpfmt_disc_check(space, d, params, MPFMT_DISC_N, 0.0, 2)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%s: %s", who, why);
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "%s runs on an unsharded ctx", who);
    if (!ctx->have_boxes) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "%s: no obstacle set uploaded (mpfmt_upload_boxes / mpfmt_upload_shapes2d)", who);
    const int dw = space == MPFMT_SPACE_DI ? d / 2 : 2;
    if (ctx->dw != dw) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "%s: the checker's workspace has %d dims, the space needs %d", who, ctx->dw, dw);
    if (ctx->ss.has && ctx->ss.d != d) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "%s: state-space bounds have %d dims, states %d", who, ctx->ss.d, d);
    return MPFMT_OK;
}

int32_t mpfmt_steer_motions_free(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const double* Q, int64_t n,
                                 uint64_t* mask, double* cost, double* dur, int32_t* nseg)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_motions_free: n < 0");
    if (n > 0 && (!P || !Q || !mask)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_motions_free: P / Q / mask is NULL");
    int32_t rc;
    if ((rc = steer_space_check(ctx, "steer_motions_free", space, d, params))) return rc;
    if (n > (int64_t)1 << 40) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_motions_free: more than 2^40 pairs");
    for (int64_t i = 0; i < n * d; ++i)
        if (!std::isfinite(P[i]) || !std::isfinite(Q[i])) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_motions_free: non-finite coordinate in pair %lld", (long long)(i / d + 1));
    if (n == 0) return MPFMT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return mpfmt_steer_pairs_device(ctx, space, d, params, P, Q, n, mask, cost, dur, nseg);
}

int32_t mpfmt_steer_shortcut_batch(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const int64_t* offsets,
                                   int64_t B, int32_t iterations, int64_t max_states, double* out_P, int64_t* out_offsets, int64_t out_cap,
                                   double* cumcost, int32_t* out_origin, mpfmt_steer_shortcut_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (B < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: B < 0");
    if (!offsets || !out_offsets) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: offsets / out_offsets is NULL");
    if (B > 0 && (!P || !info)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: P / info is NULL");
    if (out_cap < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: out_cap < 0");
    if (B > 0 && out_cap > 0 && (!out_P || !cumcost)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: out_P / cumcost is NULL");
    if (iterations < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: iterations < 0");
    if (max_states < 2 || max_states > (1 << 16)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: max_states must lie in [2, 2^16]");
    int32_t rc;
    if ((rc = steer_space_check(ctx, "steer_shortcut", space, d, params))) return rc;
    if (offsets[0] != 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: offsets[0] must be 0");
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        if (n < 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: path %lld has %lld states (a path has at least 2)", (long long)(b + 1), (long long)n);
        if (n > max_states) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: path %lld has %lld states > max_states = %lld", (long long)(b + 1), (long long)n, (long long)max_states);
    }
    const int64_t total = offsets[B];
    for (int64_t i = 0; i < total * d; ++i)
        if (!std::isfinite(P[i])) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: non-finite coordinate in state %lld", (long long)(i / d + 1));
    out_offsets[0] = 0;
    if (B == 0) return MPFMT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return mpfmt_steer_shortcut_batch_device(ctx, space, d, params, P, offsets, B, iterations, max_states, out_P, out_offsets, out_cap, cumcost,
                                             out_origin, info);
}

int32_t mpfmt_steer_shortcut(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, int64_t n, int32_t iterations,
                             int64_t max_states, double* out_P, int64_t out_cap, double* cumcost, int32_t* out_origin,
                             mpfmt_steer_shortcut_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n < 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "steer_shortcut: a path has at least 2 states");
    const int64_t offsets[2] = {0, n};
    int64_t out_offsets[2] = {0, 0};
    return mpfmt_steer_shortcut_batch(ctx, space, d, params, P, offsets, 1, iterations, max_states, out_P, out_offsets, out_cap, cumcost, out_origin,
                                      info);
}

// ---- steering spaces: double integrator (LinearQuadratic quasi-metric), Dubins and Reeds-Shepp cars (kernels_di.hip, kernels_car.hip)

static int32_t di_check(mpfmt_ctx* ctx, double rho, double r)
{
    if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
    if (ctx->d % 2 != 0 || ctx->d / 2 < 1 || ctx->d / 2 > 6)
        return mpfmt_fail(ctx, MPFMT_ERR_ARG, "double-integrator states need an even dimension 2..12 (got %d)", ctx->d);
    if (!(rho > 0.0) || !std::isfinite(rho)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rho must be finite and > 0");
    if (!(r > 0.0) || !std::isfinite(r)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "cost radius must be finite and > 0");
    return MPFMT_OK;
}

// What the shared drivers need to know of a space: the state and workspace dimensions (the obstacles and the workspace goals act
// on the first dw coordinates of a state) and whether its graph is symmetric (Reeds-Shepp: forward and backward sets coincide,
// nearneighbors.jl:200-203) or directed (double integrator, Dubins).
struct steer_space { mpfmt_steer kind; int d, dw; bool symmetric; };

static bool steer_symmetric(mpfmt_steer kind) { return kind == MPFMT_STEER_REEDSSHEPP; }

static steer_space steer_space_of(const mpfmt_ctx* ctx, mpfmt_steer kind)
{
    if (kind == MPFMT_STEER_DI) return {kind, ctx->d, ctx->d / 2, false};
    return {kind, 3, 2, steer_symmetric(kind)};
}

// is_free_state(v, CC, SS) = in_state_space(v) && point-vs-obstacles on the workspace coordinates, of n states V [n][d] on the host
// into the bitmap F.  The point test runs on the workspace points with the state-space bounds (which have the states' dimension)
// switched off; they are applied here.  Shared by the samples' bitmap (steer_state_bitmap) and the external states of a pair query.
static int32_t steer_states_free(mpfmt_ctx* ctx, const steer_space& s, const double* V, int64_t n, std::vector<uint64_t>& F)
{
    std::vector<double> P((size_t)n * s.dw);
    for (int64_t i = 0; i < n; ++i)
        for (int q = 0; q < s.dw; ++q) P[(size_t)i * s.dw + q] = V[(size_t)i * s.d + q];
    F.assign((size_t)(n + 63) / 64, 0);
    const mpfmt_ss keep = ctx->ss;
    ctx->ss.has = 0;
    const int32_t rc = mpfmt_states_free(ctx, P.data(), n, F.data());
    ctx->ss = keep;
    if (rc) return rc;
    if (keep.has)
        for (int64_t i = 0; i < n; ++i) {
            const double* v = V + (size_t)i * s.d;
            bool ok = true;
            for (int q = 0; q < s.d; ++q) ok = ok && (keep.lo[q] <= v[q]) && (v[q] <= keep.hi[q]);
            if (!ok) F[(size_t)(i >> 6)] &= ~(1ull << (i & 63));
        }
    return MPFMT_OK;
}

// that predicate over every sample: the states on the host (X) and the bitmap F.  Shared by the planners' prelude and by the checkpts
// bitmap of the fields over a resident steering graph (steer_point_bitmap).
static int32_t steer_state_bitmap(mpfmt_ctx* ctx, const steer_space& s, std::vector<double>& X, std::vector<uint64_t>& F)
{
    X.resize((size_t)ctx->N * ctx->d);
    HIPCHK(ctx, hipMemcpy(X.data(), ctx->Xo, sizeof(double) * X.size(), hipMemcpyDeviceToHost));
    return steer_states_free(ctx, s, X.data(), ctx->N, F);
}

// that bitmap for the resident steering graph, left on the device in ctx->sssp_F (allocated by the caller)
static int32_t steer_upload_bitmap(mpfmt_ctx* ctx, const std::vector<uint64_t>& F)
{
    HIPCHK(ctx, hipMemcpyAsync(ctx->sssp_F, F.data(), sizeof(uint64_t) * F.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

static int32_t steer_point_bitmap(mpfmt_ctx* ctx)
{
    const steer_space s = steer_space_of(ctx, ctx->steer_kind);
    if (ctx->dw != s.dw) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "workspace dim %d does not fit the resident steering graph (%d)", ctx->dw, s.dw);
    std::vector<double> X;
    std::vector<uint64_t> F;
    int32_t rc;
    if ((rc = steer_state_bitmap(ctx, s, X, F))) return rc;
    return steer_upload_bitmap(ctx, F);
}

// ---- roadmap queries for external states on a resident steering graph (steer_roadmap.h) -------------------------------------

// what every such call asks of the ctx; nothing has been touched when it refuses
static int32_t steer_roadmap_ready(mpfmt_ctx* ctx)
{
    if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "roadmap queries run on an unsharded ctx");
    if (!(ctx->Xo && ctx->steer_filled)) {
        if (ctx->Xo && ctx->graph_filled)
            return mpfmt_fail(ctx, MPFMT_ERR_STATE, "steering graphs only: the resident graph is a Euclidean %s graph (mpfmt_roadmap_near / _attach / _query)",
                              ctx->knn_k > 0 ? "k-nearest" : "r-disc");
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no resident steering graph (mpfmt_di_graph, mpfmt_dubins_graph, mpfmt_reedsshepp_graph, or a steering PRM* planner)");
    }
    if (ctx->cc_kind != 0) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "external states need the N-D box checker (the 2-D SAT world is resident)");
    int32_t rc;
    if ((rc = sssp_ready(ctx))) return rc;                                  // (swept, and a mask)
    if (!ctx->have_boxes) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no obstacle set uploaded (mpfmt_upload_boxes)");
    const steer_space s = steer_space_of(ctx, ctx->steer_kind);
    if (ctx->dw != s.dw || ctx->d != s.d)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, "workspace dim %d / state dim %d do not fit the resident steering graph (%d / %d)", ctx->dw, ctx->d, s.dw, s.d);
    if (ctx->ss.has && ctx->ss.d != ctx->d) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "state-space bounds have %d dims, states %d", ctx->ss.d, ctx->d);
    return MPFMT_OK;
}

// ---- the calls on external states, Euclidean and steering: one body per call --------------------------------------------
// A public call names its space.  The spaces differ in the ready check, the prefix of the call's name in messages, how the free bits of the
// external states are obtained, the checkpts bitmap, the list / reduce launchers and the direct edge of a pair: each is a switch on `steer`
// in one of the helpers below, and the bodies have none.

struct ext_call {                        // one public call: its space, its temporaries, its stats (a running sum over its list calls)
    mpfmt_ctx* ctx; bool steer;
    mpfmt_tmp tmp;
    int64_t cand = 0, near = 0, steered = 0;
    const char* pre() const { return steer ? "steer_" : ""; }
};

static int32_t ext_ready(ext_call& c) { return c.steer ? steer_roadmap_ready(c.ctx) : roadmap_ready(c.ctx); }

static int32_t ext_finite(ext_call& c, const double* Q, int64_t nq, const char* call)
{
    for (int64_t i = 0; i < nq * c.ctx->d; ++i)
        if (!std::isfinite(Q[i]))
            return mpfmt_fail(c.ctx, MPFMT_ERR_ARG, "%sroadmap_%s: non-finite coordinate in state %lld", c.pre(), call, (long long)(i / c.ctx->d + 1));
    return MPFMT_OK;
}

static int32_t up_d(ext_call& c, const double* h, size_t n, double** d)
{
    HIPCHK(c.ctx, c.tmp.get(d, sizeof(double) * n));
    HIPCHK(c.ctx, hipMemcpyAsync(*d, h, sizeof(double) * n, hipMemcpyHostToDevice, c.ctx->stream));
    return MPFMT_OK;
}

// One list call of the public call; its stats join the call's sums, which the ctx holds from then on.  d_pair (steering): query i meets
// d_pair[i] alone -- the direct edges, which count as candidates and steers and are no near-set entries.
static int32_t ext_lists(ext_call& c, const double* dQ, int64_t nq, int dir, const uint64_t* d_F, mpfmt_rm_list* L, bool count_only = false,
                         const double* d_pair = nullptr)
{
    mpfmt_ctx* ctx = c.ctx;
    const int32_t rc = !c.steer ? mpfmt_roadmap_lists(ctx, c.tmp, dQ, nq, dir, d_F, L, count_only)
                     : d_pair   ? mpfmt_steer_roadmap_lists(ctx, c.tmp, dQ, nq, dir, d_F, L, count_only, d_pair, nq, true)
                                : mpfmt_steer_roadmap_lists(ctx, c.tmp, dQ, nq, dir, d_F, L, count_only, ctx->Xo, ctx->N, false);
    if (rc) return rc;
    ctx->roadmap_candidates = c.cand += ctx->roadmap_candidates;
    ctx->roadmap_near_total = c.near += d_pair ? 0 : ctx->roadmap_near_total;
    if (c.steer) ctx->steer_roadmap_steered = c.steered += ctx->steer_roadmap_steered;
    return MPFMT_OK;
}

static int32_t ext_near(mpfmt_ctx* ctx, bool steer, const double* Q, int64_t nq, int32_t direction, int64_t* ptr, int64_t cap, int64_t* idx, double* dist,
                        uint64_t* free_mask, int64_t* total)
{
    if (!ctx) return MPFMT_ERR_ARG;
    ext_call c{ctx, steer};
    const char* p = c.pre();
    if (nq < 0 || cap < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%sroadmap_near: nq / cap < 0", p);
    if (direction != 0 && direction != 1) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%sroadmap_near: direction must be 0 (tail) or 1 (head)", p);
    if (nq > 0 && (!Q || !ptr || !total)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%sroadmap_near: Q / ptr / total is NULL", p);
    if (nq > 0 && cap > 0 && (!idx || !dist || !free_mask)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%sroadmap_near: idx / dist / free_mask is NULL", p);
    int32_t rc;
    if ((rc = ext_ready(c))) return rc;
    if (nq == 0) return MPFMT_OK;
    if ((rc = ext_finite(c, Q, nq, "near"))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double* dQ = nullptr;
    if ((rc = up_d(c, Q, (size_t)nq * ctx->d, &dQ))) return rc;
    mpfmt_rm_list L;
    if ((rc = ext_lists(c, dQ, nq, direction, nullptr, &L, cap == 0))) return rc;      // (cap == 0 asks for the sizes: the count pass alone)
    memcpy(ptr, L.ptr_host.data(), sizeof(int64_t) * (size_t)(nq + 1));
    *total = L.total;
    if (L.total > cap) return mpfmt_fail(ctx, MPFMT_ERR_CAPACITY, "%sroadmap_near: %lld entries exceed capacity %lld", p, (long long)L.total, (long long)cap);
    if (L.total == 0) return MPFMT_OK;
    std::vector<uint8_t> bits((size_t)L.total);
    HIPCHK(ctx, hipMemcpyAsync(idx, L.idx1, sizeof(int64_t) * (size_t)L.total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dist, L.dist, sizeof(double) * (size_t)L.total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(bits.data(), L.bits, (size_t)L.total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t w = 0; w < (L.total + 63) / 64; ++w) free_mask[w] = 0;
    for (int64_t e = 0; e < L.total; ++e) if (bits[(size_t)e] & 1) free_mask[e >> 6] |= 1ull << (e & 63);
    return MPFMT_OK;
}

static int32_t ext_attach(mpfmt_ctx* ctx, bool steer, const double* Q, int64_t nq, const double* C, int64_t* parent, double* cost)
{
    if (!ctx) return MPFMT_ERR_ARG;
    ext_call c{ctx, steer};
    if (nq < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%sroadmap_attach: nq < 0", c.pre());
    if (nq > 0 && (!Q || !C || !parent || !cost)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%sroadmap_attach: Q / C / parent / cost is NULL", c.pre());
    int32_t rc;
    if ((rc = ext_ready(c))) return rc;
    if (nq == 0) return MPFMT_OK;
    if ((rc = ext_finite(c, Q, nq, "attach"))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *dQ = nullptr, *dC = nullptr, *d_cost = nullptr; int64_t* d_par = nullptr;
    if ((rc = up_d(c, Q, (size_t)nq * ctx->d, &dQ))) return rc;
    if ((rc = up_d(c, C, (size_t)ctx->N, &dC))) return rc;
    HIPCHK(ctx, c.tmp.get(&d_cost, sizeof(double) * (size_t)nq));
    HIPCHK(ctx, c.tmp.get(&d_par, sizeof(int64_t) * (size_t)nq));
    if ((rc = (steer ? mpfmt_steer_roadmap_reduce : mpfmt_roadmap_reduce)(ctx, c.tmp, dQ, nq, dC, d_cost, d_par))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(cost, d_cost, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(parent, d_par, sizeof(int64_t) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

// The external states of the two sides of a pair query or a cost matrix: uploaded, with their free bits.
//   Euclidean: mpfmt_launch_states_free on the device; the bits stay there, d_m = [S: ws words | G: wg words | extra words for the caller's
//              motion bits].  pairs: S[i] -> G[i] are the pairs of a query -- their motion bits (mpfmt_launch_motions_free) fill the extra
//              words and all of d_m is on its way to m (it has arrived once a list call has synchronised the stream).
//   steering:  the host predicate ahead of the upload, the bits in fs / fg.
struct ext_sides { double *dS = nullptr, *dG = nullptr; uint64_t* d_m = nullptr; std::vector<uint64_t> m, fs, fg; };

static int32_t ext_sides_free(ext_call& c, const double* S, int64_t ns, const double* G, int64_t ng, int64_t extra, bool pairs, ext_sides* o)
{
    mpfmt_ctx* ctx = c.ctx;
    const int d = ctx->d;
    const int64_t ws = (ns + 63) / 64, wg = (ng + 63) / 64;
    int32_t rc;
    if (c.steer) {
        const steer_space s = steer_space_of(ctx, ctx->steer_kind);
        if ((rc = steer_states_free(ctx, s, S, ns, o->fs))) return rc;
        if ((rc = steer_states_free(ctx, s, G, ng, o->fg))) return rc;
    }
    if ((rc = up_d(c, S, (size_t)ns * d, &o->dS))) return rc;
    if ((rc = up_d(c, G, (size_t)ng * d, &o->dG))) return rc;
    if (c.steer) return MPFMT_OK;
    HIPCHK(ctx, c.tmp.get(&o->d_m, sizeof(uint64_t) * (size_t)(ws + wg + extra)));
    if ((rc = mpfmt_launch_states_free(ctx, o->dS, ns, o->d_m))) return rc;
    if ((rc = mpfmt_launch_states_free(ctx, o->dG, ng, o->d_m + ws))) return rc;
    if (!pairs) return MPFMT_OK;
    if ((rc = mpfmt_launch_motions_free(ctx, o->dS, o->dG, ns, o->d_m + ws + wg))) return rc;
    o->m.resize((size_t)(ws + wg + extra));
    HIPCHK(ctx, hipMemcpyAsync(o->m.data(), o->d_m, sizeof(uint64_t) * o->m.size(), hipMemcpyDeviceToHost, ctx->stream));
    return MPFMT_OK;
}

// the checkpts bitmap of the resident graph's samples: ctx->sssp_F, or nullptr without checkpts
static int32_t ext_bitmap(ext_call& c, int32_t checkpts, const uint64_t** d_F)
{
    int32_t rc;
    if (checkpts && (rc = c.steer ? sssp_resident_bitmap(c.ctx) : sssp_point_bitmap(c.ctx))) return rc;
    *d_F = checkpts ? c.ctx->sssp_F.get() : nullptr;
    return MPFMT_OK;
}

// The list calls of a pair query in their order, and the direct edge of every pair as (direct[q], dsg[q]: its weight, +Inf without).
//   steering:  a 1 x 1 tail-list evaluation ahead of the attachments (query s_i against the single "sample" g_i), weight and free bit read back.
//   Euclidean: the squared distance folded on the host against r * r, and the motion bit of ext_sides_free, which has arrived with the
//              lists; the free bits of the two sides move to fs / fg, where the steering space has them.
static int32_t ext_query_lists(ext_call& c, ext_sides& e, const double* S, const double* G, int64_t nq, const uint64_t* d_F, mpfmt_rm_list* Ls,
                               mpfmt_rm_list* Lg, std::vector<uint8_t>& direct, std::vector<double>& dsg)
{
    mpfmt_ctx* ctx = c.ctx;
    int32_t rc;
    direct.assign((size_t)nq, 0);
    dsg.assign((size_t)nq, INFINITY);
    if (c.steer) {
        mpfmt_rm_list Ld;
        if ((rc = ext_lists(c, e.dS, nq, 0, nullptr, &Ld, false, e.dG))) return rc;
        std::vector<double> w((size_t)Ld.total);
        std::vector<uint8_t> b((size_t)Ld.total);
        if (Ld.total > 0) {
            HIPCHK(ctx, hipMemcpyAsync(w.data(), Ld.dist, sizeof(double) * (size_t)Ld.total, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(b.data(), Ld.bits, (size_t)Ld.total, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        for (int64_t q = 0; q < nq; ++q) {
            const int64_t at = Ld.ptr_host[(size_t)q];
            if (Ld.ptr_host[(size_t)q + 1] > at && (b[(size_t)at] & 1)) { direct[(size_t)q] = 1; dsg[(size_t)q] = w[(size_t)at]; }
        }
    }
    if ((rc = ext_lists(c, e.dS, nq, 0, d_F, Ls))) return rc;
    if ((rc = ext_lists(c, e.dG, nq, 1, nullptr, Lg))) return rc;
    if (c.steer) return MPFMT_OK;
    const int d = ctx->d;
    const int64_t words = (nq + 63) / 64;
    const double r2 = ctx->graph_r * ctx->graph_r;
    e.fs.assign(e.m.begin(), e.m.begin() + words);
    e.fg.assign(e.m.begin() + words, e.m.begin() + 2 * words);
    for (int64_t q = 0; q < nq; ++q) {
        double dsg2 = 0.0;
        for (int i = 0; i < d; ++i) { const double t = S[q * d + i] - G[q * d + i]; const double tt = t * t; dsg2 = (i == 0) ? tt : dsg2 + tt; }
        if (dsg2 <= r2 && ((e.m[(size_t)(2 * words + (q >> 6))] >> (q & 63)) & 1ull)) { direct[(size_t)q] = 1; dsg[(size_t)q] = std::sqrt(dsg2); }
    }
    return MPFMT_OK;
}

static int32_t ext_query(mpfmt_ctx* ctx, bool steer, const double* S, const double* G, int64_t nq, int32_t checkpts, double* cost, int64_t* path_ptr,
                         int64_t* path, int64_t path_cap, mpfmt_roadmap_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    ext_call c{ctx, steer};
    if (nq < 0 || path_cap < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%sroadmap_query: nq / path_cap < 0", c.pre());
    if (nq > 0 && (!S || !G || !cost || !path_ptr || (path_cap > 0 && !path)))
        return mpfmt_fail(ctx, MPFMT_ERR_ARG, "%sroadmap_query: S / G / cost / path_ptr / path is NULL", c.pre());
    int32_t rc;
    if ((rc = ext_ready(c))) return rc;
    if (nq == 0) return MPFMT_OK;
    if ((rc = ext_finite(c, S, nq, "query (S)"))) return rc;
    if ((rc = ext_finite(c, G, nq, "query (G)"))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t N = ctx->N;
    // the two states of every pair, the direct edge, and all attachments: one count and one fill launch each way
    ext_sides e;
    const uint64_t* d_F;
    mpfmt_rm_list Ls, Lg;
    std::vector<uint8_t> direct;
    std::vector<double> dsg;
    if ((rc = ext_sides_free(c, S, nq, G, nq, (nq + 63) / 64, true, &e))) return rc;
    if ((rc = ext_bitmap(c, checkpts, &d_F))) return rc;
    if ((rc = ext_query_lists(c, e, S, G, nq, d_F, &Ls, &Lg, direct, dsg))) return rc;
    int64_t* d_res = nullptr;
    HIPCHK(ctx, c.tmp.get(&d_res, sizeof(int64_t) * (size_t)(N + 8)));
    int64_t res[3];
    std::vector<int64_t> hops;
    int64_t used = 0;
    bool over = false;
    path_ptr[0] = 0;
    for (int64_t q = 0; q < nq; ++q) {
        mpfmt_roadmap_info inf;
        memset(&inf, 0, sizeof inf);
        inf.near_s = Ls.ptr_host[(size_t)q + 1] - Ls.ptr_host[(size_t)q]; inf.usable_s = Ls.usable_host[(size_t)q];
        inf.near_g = Lg.ptr_host[(size_t)q + 1] - Lg.ptr_host[(size_t)q]; inf.usable_g = Lg.usable_host[(size_t)q];
        cost[q] = INFINITY;
        int64_t len = 0;
        if (!bit(e.fs, q)) inf.status = 2;
        else if (!bit(e.fg, q)) inf.status = 3;
        else {
            const int64_t s0 = Ls.ptr_host[(size_t)q];
            mpfmt_sssp_info fi;
            if ((rc = mpfmt_sssp_seeded_device(ctx, Ls.idx1 + s0, Ls.dist + s0, Ls.bits + s0, inf.near_s, d_F, &fi))) return rc;
            inf.rounds = fi.rounds; inf.ms_device = fi.ms_device;
            if ((rc = mpfmt_roadmap_goal(ctx, Lg, q, ctx->sssp_C, ctx->sssp_A, d_res))) return rc;
            HIPCHK(ctx, hipMemcpyAsync(res, d_res, sizeof(int64_t) * 3, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            double best; memcpy(&best, &res[0], sizeof best);
            const int64_t last = res[1];
            if (direct[(size_t)q] && (last == 0 || dsg[(size_t)q] <= best)) { cost[q] = dsg[(size_t)q]; inf.status = 0; }
            else if (last == 0) inf.status = 1;
            else {
                cost[q] = best; inf.status = 0; len = res[2];
                if (used + len <= path_cap) {
                    hops.resize((size_t)len);
                    HIPCHK(ctx, hipMemcpyAsync(hops.data(), d_res + 3, sizeof(int64_t) * (size_t)len, hipMemcpyDeviceToHost, ctx->stream));
                    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
                    for (int64_t i = 0; i < len; ++i) path[used + i] = hops[(size_t)(len - 1 - i)];
                } else over = true;
            }
        }
        inf.path_len = len;
        used += len;
        path_ptr[q + 1] = used;
        if (info) info[q] = inf;
    }
    if (over) return mpfmt_fail(ctx, MPFMT_ERR_CAPACITY, "%sroadmap_query: %lld path samples exceed capacity %lld", c.pre(), (long long)used, (long long)path_cap);
    return MPFMT_OK;
}

int32_t mpfmt_roadmap_near(mpfmt_ctx* ctx, const double* Q, int64_t nq, int32_t direction, int64_t* ptr, int64_t cap, int64_t* idx, double* dist,
                           uint64_t* free_mask, int64_t* total)
{ return ext_near(ctx, false, Q, nq, direction, ptr, cap, idx, dist, free_mask, total); }

int32_t mpfmt_steer_roadmap_near(mpfmt_ctx* ctx, const double* Q, int64_t nq, int32_t direction, int64_t* ptr, int64_t cap, int64_t* idx, double* dist,
                                 uint64_t* free_mask, int64_t* total)
{ return ext_near(ctx, true, Q, nq, direction, ptr, cap, idx, dist, free_mask, total); }

int32_t mpfmt_roadmap_attach(mpfmt_ctx* ctx, const double* Q, int64_t nq, const double* C, int64_t* parent, double* cost)
{ return ext_attach(ctx, false, Q, nq, C, parent, cost); }

int32_t mpfmt_steer_roadmap_attach(mpfmt_ctx* ctx, const double* Q, int64_t nq, const double* C, int64_t* parent, double* cost)
{ return ext_attach(ctx, true, Q, nq, C, parent, cost); }

int32_t mpfmt_roadmap_query(mpfmt_ctx* ctx, const double* S, const double* G, int64_t nq, int32_t checkpts, double* cost, int64_t* path_ptr,
                            int64_t* path, int64_t path_cap, mpfmt_roadmap_info* info)
{ return ext_query(ctx, false, S, G, nq, checkpts, cost, path_ptr, path, path_cap, info); }

int32_t mpfmt_steer_roadmap_query(mpfmt_ctx* ctx, const double* S, const double* G, int64_t nq, int32_t checkpts, double* cost, int64_t* path_ptr,
                                  int64_t* path, int64_t path_cap, mpfmt_roadmap_info* info)
{ return ext_query(ctx, true, S, G, nq, checkpts, cost, path_ptr, path, path_cap, info); }

// the ns x ng cost matrix between external starts and goals at the price of ns fields (kernels_sssp_multi.hip); Euclidean graphs
int32_t mpfmt_roadmap_matrix(mpfmt_ctx* ctx, const double* S, int64_t ns, const double* G, int64_t ng, int32_t checkpts, double* cost, int32_t* status,
                             mpfmt_roadmap_matrix_info* info)
{
    if (!ctx) return MPFMT_ERR_ARG;
    ext_call c{ctx, false};
    if (ns < 0 || ng < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "roadmap_matrix: ns / ng < 0");
    if (ns > 0 && ng > 0 && (!S || !G || !cost)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "roadmap_matrix: S / G / cost is NULL");
    int32_t rc;
    if ((rc = ext_ready(c))) return rc;
    if (info) memset(info, 0, sizeof *info);
    if (ns == 0 || ng == 0) return MPFMT_OK;
    if ((rc = ext_finite(c, S, ns, "matrix (S)"))) return rc;
    if ((rc = ext_finite(c, G, ng, "matrix (G)"))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int d = ctx->d;
    const int64_t np = ns * ng, ws = (ns + 63) / 64, wg = (ng + 63) / 64, wp = (np + 63) / 64;
    double *dP = nullptr, *dQ = nullptr, *d_cost = nullptr;
    int32_t* d_status = nullptr;
    HIPCHK(ctx, c.tmp.get(&dP, sizeof(double) * (size_t)np * d));
    HIPCHK(ctx, c.tmp.get(&dQ, sizeof(double) * (size_t)np * d));
    HIPCHK(ctx, c.tmp.get(&d_cost, sizeof(double) * (size_t)np));
    HIPCHK(ctx, c.tmp.get(&d_status, sizeof(int32_t) * (size_t)np));
    // the states of both sides and the direct edge of every pair: the tests of the pair query, through the same kernels
    ext_sides e;
    if ((rc = ext_sides_free(c, S, ns, G, ng, wp, false, &e))) return rc;
    uint64_t* d_direct = e.d_m + ws + wg;
    if ((rc = mpfmt_roadmap_pairs(ctx, e.dS, ns, e.dG, ng, dP, dQ))) return rc;
    if ((rc = mpfmt_launch_motions_free(ctx, dP, dQ, np, d_direct))) return rc;
    // all attachments, one launch each way
    const uint64_t* d_F;
    mpfmt_rm_list Ls, Lg;
    if ((rc = ext_bitmap(c, checkpts, &d_F))) return rc;
    if ((rc = ext_lists(c, e.dS, ns, 0, d_F, &Ls))) return rc;
    if ((rc = ext_lists(c, e.dG, ng, 1, nullptr, &Lg))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // (the lists' usable counts have arrived)
    mpfmt_roadmap_matrix_info inf;
    memset(&inf, 0, sizeof inf);
    if ((rc = mpfmt_roadmap_matrix_device(ctx, e.dS, ns, e.dG, ng, d_F, e.d_m, e.d_m + ws, d_direct, Ls, Lg, d_cost, d_status, &inf))) return rc;
    inf.near_s = Ls.total; inf.near_g = Lg.total;
    for (int64_t v : Ls.usable_host) inf.usable_s += v;
    for (int64_t v : Lg.usable_host) inf.usable_g += v;
    HIPCHK(ctx, hipMemcpyAsync(cost, d_cost, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(ctx, hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (info) *info = inf;
    return MPFMT_OK;
}

// The planners' common prelude: the checks of the ctx against the space, then the states on the host (X) and the checkpts bitmap F,
// is_free_state(v, CC, SS) = in_state_space(v) && point-vs-obstacles on the workspace coordinates.  The point test runs on the
// workspace points with the state-space bounds (which have the states' dimension) switched off; they are applied here.
// rho / r: the double integrator's build parameters, checked with the samples.
static int32_t steer_prelude(mpfmt_ctx* ctx, const steer_space& s, double rho, double r, int64_t init_idx, int32_t goal_kind,
                             std::vector<double>& X, std::vector<uint64_t>& F)
{
    int32_t rc;
    if (s.kind == MPFMT_STEER_DI) {
        if ((rc = di_check(ctx, rho, r))) return rc;
        if (!ctx->have_boxes) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no obstacle set uploaded (mpfmt_upload_boxes)");
    } else {
        if (!ctx->Xo || ctx->d != s.d) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "car planning needs SE2 samples (d = 3)");
        if (!ctx->have_boxes || ctx->dw != s.dw)
            return mpfmt_fail(ctx, MPFMT_ERR_STATE, "car planning needs a 2-D workspace checker (mpfmt_upload_boxes with dw = 2, or mpfmt_upload_shapes2d)");
    }
    const int64_t N = ctx->N;
    if (init_idx < 1 || init_idx > N) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "init_idx out of range");
    if (goal_kind < 0 || goal_kind > 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "unknown goal kind %d", goal_kind);
    if (ctx->dw != s.dw) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "workspace dim %d != state dim / 2 = %d", ctx->dw, s.dw);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = steer_state_bitmap(ctx, s, X, F))) return rc;
    if (!bit(F, init_idx - 1)) return mpfmt_fail(ctx, MPFMT_ERR_INFEASIBLE, "initial state is infeasible");
    return MPFMT_OK;
}

// the graph of a space: (a, b) = (rho, -) for the double integrator, (turning radius, speed) for the cars
static int32_t steer_build(mpfmt_ctx* ctx, mpfmt_steer kind, double a, double b, double r)
{
    if (kind != MPFMT_STEER_DI) return mpfmt_car_build(ctx, kind, a, b, r);
    int32_t rc;
    if ((rc = mpfmt_di_count(ctx, a, r))) return rc;
    return mpfmt_di_fill(ctx);
}

static int32_t steer_sweep(mpfmt_ctx* ctx, mpfmt_steer kind) { return kind == MPFMT_STEER_DI ? mpfmt_di_sweep(ctx) : mpfmt_car_sweep(ctx); }

static bool steer_resident(const mpfmt_ctx* ctx, mpfmt_steer kind, double a, double b, double r)
{
    return ctx->steer_filled && ctx->steer_kind == kind && ctx->steer_r == r &&
           (kind == MPFMT_STEER_DI ? ctx->di_rho == a : (ctx->car_rt == a && ctx->car_sp == b));
}

// ---- the single-shot planners, every space and solver: one driver ----------------------------------------------------------
// A plan is five stages -- plan_check, plan_points, plan_graph, a solver, plan_finish -- and an exported planner is a plan_call, a reuse
// policy and a solver.  What differs between the planners is data of the call: the space, the policy, where the point bitmap lives and a
// few flags for the checks.

enum plan_space { PLAN_R, PLAN_K, PLAN_STEER };          // Euclidean r-disc graph | Euclidean k-nearest graph | a steering space (kind, a, b, r)
// what a plan takes from the ctx: nothing (graph and mask anew) | a resident graph of its space and parameters, swept again | that graph
// and its mask while it is valid (it stays valid across mpfmt_boxes_add / mpfmt_boxes_remove, which bring it up to date in place)
enum plan_policy { PLAN_REBUILD, PLAN_RESWEEP, PLAN_RESIDENT };
enum {
    PLAN_PRM = 1,            // a roadmap planner: "prmstar" in its messages, the Euclidean point bitmap on the device (ctx->sssp_F)
    PLAN_WAVEFRONT = 2,      // the recursion on the device: A / C / path may be NULL, and res is filled by the solve alone
    PLAN_K_FIRST = 4,        // mpfmt_knn_prmstar looks at k before anything else
};

struct plan_call {
    mpfmt_ctx* ctx; plan_space space; int flags;
    double r; int64_t k; mpfmt_steer kind; double a, b;                  // the space: r | k | (kind, a, b, r), (a, b) as for steer_build
    int64_t init_idx; int32_t checkpts, goal_kind; const double* goal_params;
    int64_t* A; double* C; int64_t* path; mpfmt_fmt_result* res;          // the caller's
    double band = 0.0; int32_t wf_flags = 0; mpfmt_wf_info* info = nullptr;      // (the wavefront form's)
    steer_space s{};                                                      // (of `kind`, once the ctx is known to be there)
    stamp t[6];                                                           // as for fmt_times
    std::vector<double> X; std::vector<uint64_t> F;                       // the states and the point bitmap, where they are on the host
    bool steer() const { return space == PLAN_STEER; }
    // coordinates the goal reads: the state in a Euclidean space; in a steering space the workspace ones, and the whole state for POINT
    // (StateGoal is exact state equality, goals.jl:128-131)
    int gd() const { return !steer() ? ctx->d : goal_kind == MPFMT_GOAL_POINT ? s.d : s.dw; }
};

// The refusals.  Every exported planner keeps its own order of checks and its own words: the Euclidean ones check ctx, pointers, samples,
// obstacle set, world, init_idx, goal kind and r or k here; a steering one leaves what concerns its space to steer_prelude (plan_points).
static int32_t plan_check(plan_call& c)
{
    mpfmt_ctx* ctx = c.ctx;
    const bool prm = c.flags & PLAN_PRM, tree = !(c.flags & PLAN_WAVEFRONT);
    if (ctx && (c.flags & PLAN_K_FIRST) && c.k < 1) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "k must be >= 1");
    if (!ctx) return MPFMT_ERR_ARG;
    if (!c.res || !c.goal_params || (tree && (!c.A || !c.C || !c.path))) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "NULL output / goal pointer");
    if (c.steer()) {                                                     // (only the roadmap planners ask for an unsharded ctx here)
        if (prm && ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "prmstar runs on an unsharded ctx");
        c.s = steer_space_of(ctx, c.kind);
    } else {
        if (!ctx->Xo) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no samples uploaded");
        if (!ctx->have_boxes) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no obstacle set uploaded (mpfmt_upload_boxes)");
        if (ctx->world != 1) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "%s runs on an unsharded ctx", prm ? "prmstar" : "fmtstar");
        if (c.init_idx < 1 || c.init_idx > ctx->N) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "init_idx out of range");
        if (c.goal_kind < 0 || c.goal_kind > 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "unknown goal kind %d", c.goal_kind);
        if (c.space == PLAN_R && (!(c.r > 0.0) || !std::isfinite(c.r))) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "radius must be finite and > 0");
        if (c.space == PLAN_K && c.k < 1) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "k must be >= 1");
        HIPCHK(ctx, hipSetDevice(ctx->device));
    }
    if (tree) {
        memset(c.res, 0, sizeof *c.res);
        c.res->cost = INFINITY;
    }
    return MPFMT_OK;
}

// The checkpts bitmap (fmt.jl:31-36), which also answers is_free_state(init) (fmt.jl:24-29).  Three forms, each where its solver reads it:
// Euclidean FMT* on the host (c.F), Euclidean PRM* on the device (ctx->sssp_F, one word read back), a steering space on the host with the
// states (c.X, c.F) behind the space's own checks.
static int32_t plan_points(plan_call& c)
{
    mpfmt_ctx* ctx = c.ctx;
    int32_t rc;
    if (c.steer()) {
        c.t[0] = now();
        if ((rc = steer_prelude(ctx, c.s, c.a, c.r, c.init_idx, c.goal_kind, c.X, c.F))) return rc;
        c.t[1] = now();
        return MPFMT_OK;
    }
    const int64_t N = ctx->N, i0 = c.init_idx - 1;
    bool init_free;
    if (c.flags & PLAN_PRM) {
        c.t[0] = now();
        if ((rc = sssp_point_bitmap(ctx))) return rc;
        uint64_t init_word = 0;
        HIPCHK(ctx, hipMemcpyAsync(&init_word, ctx->sssp_F + (i0 >> 6), sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        init_free = (init_word >> (i0 & 63)) & 1ull;
    } else {
        c.F.assign((size_t)(N + 63) / 64, 0);
        c.t[0] = now();
        if ((rc = mpfmt_points_free(ctx, nullptr, N, c.F.data()))) return rc;
        init_free = bit(c.F, i0);
    }
    if (!init_free) return mpfmt_fail(ctx, MPFMT_ERR_INFEASIBLE, "initial state is infeasible");
    c.t[1] = now();
    return MPFMT_OK;
}

// Reuse or build the graph, then reuse or sweep its mask, as the policy says; t[2] = the graph stands, t[3] = its mask does.
//   steering:  steer_build / steer_sweep; a graph just built is not swept yet.
//   Euclidean: PLAN_RESWEEP builds the graph alone (mpfmt_graph_build_device, mpfmt_knn_build) and sweeps; PLAN_RESIDENT builds graph and
//              mask in one (mpfmt_graph_step_device), or the k-nearest graph and then its sweep, and charges a reused r-disc graph nothing
//              (t[2] = t[1]).
static int32_t plan_graph(plan_call& c, plan_policy policy)
{
    mpfmt_ctx* ctx = c.ctx;
    int32_t rc;
    if (c.steer()) {
        if (!(policy != PLAN_REBUILD && steer_resident(ctx, c.kind, c.a, c.b, c.r)) && (rc = steer_build(ctx, c.kind, c.a, c.b, c.r))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        c.t[2] = now();
        if (!(policy == PLAN_RESIDENT && ctx->steer_swept) && (rc = steer_sweep(ctx, c.kind))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        c.t[3] = now();
        return MPFMT_OK;
    }
    const bool keep_mask = policy == PLAN_RESIDENT;
    if (c.space == PLAN_K) {
        if (!knn_resident_k(ctx, c.k)) {
            if ((rc = mpfmt_knn_build(ctx, c.k))) return rc;
            if (keep_mask) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        c.t[2] = now();
    } else if (!euclid_resident(ctx, c.r)) {
        if ((rc = keep_mask ? mpfmt_graph_step_device(ctx, c.r, nullptr) : mpfmt_graph_build_device(ctx, c.r, nullptr))) return rc;
        c.t[2] = now();
    } else c.t[2] = keep_mask ? c.t[1] : now();
    if (!(keep_mask && ctx->graph_swept)) {
        ctx->pend_valid = false;
        if ((rc = mpfmt_launch_graph_sweep(ctx))) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    c.t[3] = now();
    return MPFMT_OK;
}

// the states on the host, for the Euclidean planners (a steering one has had them since its prelude)
static int32_t plan_states(plan_call& c)
{
    c.X.resize((size_t)c.ctx->N * c.ctx->d);
    HIPCHK(c.ctx, hipMemcpy(c.X.data(), c.ctx->Xo, sizeof(double) * c.X.size(), hipMemcpyDeviceToHost));
    return MPFMT_OK;
}

// The solvers; t[4] = the solve begins, t[5] = it is done.

// the symmetric recursion on the host, column = inball: the r-disc graph (every edge check one test, behind the state-space bounds), and
// the Reeds-Shepp graph, whose forward and backward sets coincide (the segment counts of its sweep)
static int32_t plan_solve_symmetric(plan_call& c)
{
    mpfmt_ctx* ctx = c.ctx;
    int32_t rc;
    host_graph g;
    if ((rc = graph_to_host(ctx, c.steer(), g))) return rc;
    if (!c.steer() && (rc = plan_states(c))) return rc;
    c.t[4] = now();
    const bool ss = !c.steer() && ctx->ss.has;
    if ((rc = mpfmt_host_fmt_recursion_impl(ctx->N, ctx->d, c.X.data(), g.colptr.data(), g.rowval.data(), g.nzval.data(), g.efree.data(),
                                            c.checkpts ? c.F.data() : nullptr, ss ? ctx->ss.lo : nullptr, ss ? ctx->ss.hi : nullptr, c.init_idx,
                                            c.goal_kind, c.goal_params, c.gd(), c.steer() ? g.nseg.data() : nullptr, c.A, c.C, c.path, c.res)))
        return mpfmt_fail(ctx, rc, "host recursion rejected its arguments");
    c.t[5] = now();
    return MPFMT_OK;
}

// the forward sets of the resident directed graph for the recursion on the host (without them it builds its own)
struct csr_forward { mpfmt_csr_host host; mpfmt_csr_view view; const mpfmt_csr_view* ptr = nullptr; };

static void csr_forward_view(mpfmt_ctx* ctx, csr_forward& f)
{
    if (mpfmt_csc_transpose_device(ctx, &f.host) != MPFMT_OK) return;
    f.view = {f.host.rowptr.data(), f.host.colidx.data(), f.host.centry.data()};
    f.ptr = &f.view;
}

// the directed recursion on the host over the column graph and its transposed view: the k-nearest graph (fmt.jl:43-101 with
// nearF = mutualknnF, nearB = knnB: the mutual bits restrict the forward sets), the double integrator and the Dubins car (the segment
// counts of the sweep).  A steering plan counts the transposition into ms_host_loop, the k-nearest one does not.
static int32_t plan_solve_directed(plan_call& c)
{
    mpfmt_ctx* ctx = c.ctx;
    const int d = ctx->d;
    int32_t rc;
    host_graph g;
    if ((rc = graph_to_host(ctx, c.steer(), g))) return rc;
    std::vector<uint64_t> mutual;
    csr_forward fwd;
    if (c.steer()) c.t[4] = now();
    else {
        const size_t words = (size_t)(ctx->nnz + 63) / 64;
        mutual.assign(std::max<size_t>(words, 1), 0);
        if (words > 0) HIPCHK(ctx, hipMemcpy(mutual.data(), ctx->knn_mutual, sizeof(uint64_t) * words, hipMemcpyDeviceToHost));
        if ((rc = plan_states(c))) return rc;
    }
    csr_forward_view(ctx, fwd);
    if (!c.steer()) c.t[4] = now();
    auto goal_hit = [&](int64_t z) { return mpfmt_is_goal_pt(&c.X[(size_t)z * d], c.gd(), c.goal_kind, c.goal_params); };
    mpfmt_directed_fmt_recursion(ctx->N, g.colptr.data(), g.rowval.data(), g.nzval.data(), g.efree.data(), c.steer() ? g.nseg.data() : nullptr,
                                 c.checkpts ? c.F.data() : nullptr, c.init_idx, goal_hit, c.A, c.C, c.path, c.res, fwd.ptr,
                                 c.steer() ? nullptr : mutual.data());
    c.t[5] = now();
    return MPFMT_OK;
}

// the recursion on the device over the resident steering graph (kernels_wavefront.hip, directed form; the Reeds-Shepp graph is
// structurally symmetric, so its rows are its columns and the same form applies): the transpose (forward sets) on the device, then
// cost-band batches; MPFMT_WF_SINGLE reproduces the host recursion's pop order exactly
static int32_t plan_solve_wavefront(plan_call& c)
{
    mpfmt_ctx* ctx = c.ctx;
    int32_t rc;
    c.t[4] = c.t[3];
    if ((rc = mpfmt_wf_begin_directed(ctx, c.init_idx, c.checkpts, c.F.data(), c.goal_kind, c.goal_params, c.s.dw, c.band, c.wf_flags))) return rc;
    if ((rc = mpfmt_wf_run(ctx))) return rc;
    if ((rc = mpfmt_wf_finish(ctx, c.A, c.C, c.path, c.res))) return rc;
    c.t[5] = now();
    return MPFMT_OK;
}

// PRM*: the cost-to-come field from init_idx over the resident graph and mask (kernels_sssp.hip), the goal pick and the walk back
static int32_t plan_solve_field(plan_call& c)
{
    mpfmt_ctx* ctx = c.ctx;
    int32_t rc;
    if ((rc = c.steer() ? sssp_ready(ctx) : sssp_ready_euclid(ctx))) return rc;
    if (c.steer() && c.checkpts) {                                       // (the Euclidean bitmap is on the device already)
        if ((rc = ctx->sssp_F.ensure(ctx, sizeof(uint64_t) * c.F.size()))) return rc;
        if ((rc = steer_upload_bitmap(ctx, c.F))) return rc;
    }
    c.t[4] = now();
    mpfmt_sssp_info inf;
    if ((rc = mpfmt_sssp_device(ctx, c.init_idx - 1, c.checkpts ? ctx->sssp_F.get() : nullptr, c.C, c.A, &inf))) return rc;
    if (!c.steer() && (rc = plan_states(c))) return rc;
    const int64_t z = mpfmt_goal_pick(ctx->N, ctx->d, c.gd(), c.X.data(), c.C, c.goal_kind, c.goal_params);
    mpfmt_walk_back(ctx->N, c.C, c.A, c.init_idx, z, c.path, c.res);
    c.t[5] = now();
    return MPFMT_OK;
}

// the timing fields and, for the wavefront form, its counters
static void plan_finish(plan_call& c)
{
    fmt_times(c.ctx, c.res, c.t);
    if (c.flags & PLAN_WAVEFRONT) mpfmt_wf_info_now(c.ctx, c.info);
}

static int32_t plan_run(plan_call& c, plan_policy policy, int32_t (*solve)(plan_call&))
{
    int32_t rc;
    if ((rc = plan_check(c)) || (rc = plan_points(c)) || (rc = plan_graph(c, policy)) || (rc = solve(c))) return rc;
    plan_finish(c);
    return MPFMT_OK;
}

// fmtstar! over the r-disc graph, the recursion on the host.  A filled graph of the same samples and radius (a previous plan, or
// mpfmt_graph_import) is reused: only the obstacle-dependent sweep is redone.
int32_t mpfmt_fmtstar(mpfmt_ctx* ctx, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                      int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{
    plan_call c{ctx, PLAN_R, 0, r, 0, MPFMT_STEER_DI, 0.0, 0.0, init_idx, checkpts, goal_kind, goal_params, A, C, path, res};
    return plan_run(c, PLAN_RESWEEP, plan_solve_symmetric);
}

// ... with connections = :K (a resident k-nearest graph of the same samples and the same effective k is reused)
int32_t mpfmt_knn_fmtstar(mpfmt_ctx* ctx, int64_t k, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                          int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{
    plan_call c{ctx, PLAN_K, 0, 0.0, k, MPFMT_STEER_DI, 0.0, 0.0, init_idx, checkpts, goal_kind, goal_params, A, C, path, res};
    return plan_run(c, PLAN_RESWEEP, plan_solve_directed);
}

// PRM*: graph and mask (both reused while resident and valid), the field from init_idx, the best goal sample
int32_t mpfmt_prmstar(mpfmt_ctx* ctx, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                      int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{
    plan_call c{ctx, PLAN_R, PLAN_PRM, r, 0, MPFMT_STEER_DI, 0.0, 0.0, init_idx, checkpts, goal_kind, goal_params, A, C, path, res};
    return plan_run(c, PLAN_RESIDENT, plan_solve_field);
}

int32_t mpfmt_knn_prmstar(mpfmt_ctx* ctx, int64_t k, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                          int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{
    plan_call c{ctx, PLAN_K, PLAN_PRM | PLAN_K_FIRST, 0.0, k, MPFMT_STEER_DI, 0.0, 0.0, init_idx, checkpts, goal_kind, goal_params, A, C, path, res};
    return plan_run(c, PLAN_RESIDENT, plan_solve_field);
}

// fmtstar! in a steering space with the recursion on the host; the graph and its edge bits are built anew for every plan
static int32_t steer_fmtstar(mpfmt_ctx* ctx, mpfmt_steer kind, double a, double b, double r, int64_t init_idx, int32_t checkpts,
                             int32_t goal_kind, const double* goal_params, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{
    plan_call c{ctx, PLAN_STEER, 0, r, 0, kind, a, b, init_idx, checkpts, goal_kind, goal_params, A, C, path, res};
    return plan_run(c, PLAN_REBUILD, steer_symmetric(kind) ? plan_solve_symmetric : plan_solve_directed);
}

// ... with the recursion on the device.  A resident graph of the same space and parameters -- (rho, r) for the double integrator; kind,
// turning radius, speed and r for the cars -- is reused, and its sweep too while it is valid: it stays valid across mpfmt_boxes_add /
// mpfmt_boxes_remove, which bring the mask and the segment counts up to date in place (steer_delta.h), and goes with mpfmt_upload_boxes,
// new bounds or new samples.
static int32_t steer_fmtstar_wavefront(mpfmt_ctx* ctx, mpfmt_steer kind, double a, double b, double r, int64_t init_idx, int32_t checkpts,
                                       int32_t goal_kind, const double* goal_params, double band, int32_t flags, int64_t* A, double* C,
                                       int64_t* path, mpfmt_fmt_result* res, mpfmt_wf_info* info)
{
    plan_call c{ctx, PLAN_STEER, PLAN_WAVEFRONT, r, 0, kind, a, b, init_idx, checkpts, goal_kind, goal_params, A, C, path, res, band, flags, info};
    return plan_run(c, PLAN_RESIDENT, plan_solve_wavefront);
}

// PRM* in a steering space: graph and sweep as steer_fmtstar_wavefront takes them, then the field over the resident graph
static int32_t steer_prmstar(mpfmt_ctx* ctx, mpfmt_steer kind, double a, double b, double r, int64_t init_idx, int32_t checkpts,
                             int32_t goal_kind, const double* goal_params, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{
    plan_call c{ctx, PLAN_STEER, PLAN_PRM, r, 0, kind, a, b, init_idx, checkpts, goal_kind, goal_params, A, C, path, res};
    return plan_run(c, PLAN_RESIDENT, plan_solve_field);
}

int32_t mpfmt_di_prmstar(mpfmt_ctx* ctx, double rho, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind, const double* goal_params,
                         int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{ return steer_prmstar(ctx, MPFMT_STEER_DI, rho, 0.0, r, init_idx, checkpts, goal_kind, goal_params, A, C, path, res); }
int32_t mpfmt_dubins_prmstar(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind,
                             const double* goal_params, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{ return steer_prmstar(ctx, MPFMT_STEER_DUBINS, turn_radius, speed, r, init_idx, checkpts, goal_kind, goal_params, A, C, path, res); }
int32_t mpfmt_reedsshepp_prmstar(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind,
                                 const double* goal_params, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{ return steer_prmstar(ctx, MPFMT_STEER_REEDSSHEPP, turn_radius, speed, r, init_idx, checkpts, goal_kind, goal_params, A, C, path, res); }

// the graph accessors: (a, b) as for steer_build; tval (the double integrator's optimal times) may be NULL
static int32_t steer_graph_count(mpfmt_ctx* ctx, mpfmt_steer kind, double a, double b, double r, int64_t* colptr, int64_t* nnz)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!colptr || !nnz) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "colptr / nnz is NULL");
    int32_t rc;
    if (kind == MPFMT_STEER_DI) {
        if ((rc = di_check(ctx, a, r))) return rc;
        HIPCHK(ctx, hipSetDevice(ctx->device));
        if ((rc = mpfmt_di_count(ctx, a, r))) return rc;
    } else if ((rc = mpfmt_car_build(ctx, kind, a, b, r))) return rc;
    if ((rc = colptr_to_host(ctx, colptr))) return rc;
    *nnz = ctx->nnz;
    return MPFMT_OK;
}

// (a car graph is filled when it is counted; a double-integrator one on the first call that needs its entries)
static int32_t steer_graph_fill(mpfmt_ctx* ctx, mpfmt_steer kind, int64_t* rowval, double* nzval, double* tval)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->steer_counted || ctx->steer_kind != kind)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, kind == MPFMT_STEER_DI ? "di_graph_fill before di_graph_count" : "car graph_fill before graph_count");
    if (ctx->nnz > 0 && (!rowval || !nzval)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rowval / nzval is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if (!ctx->steer_filled && (rc = mpfmt_di_fill(ctx))) return rc;
    const int64_t nnz = ctx->nnz;
    if (nnz > 0) {
        void* scr;
        if ((rc = mpfmt_scratch(ctx, sizeof(int64_t) * nnz, &scr))) return rc;
        hipLaunchKernelGGL(k_i32_to_i64_add1, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rowval, nnz, (int64_t*)scr);
        HIPCHK(ctx, hipMemcpyAsync(rowval, scr, sizeof(int64_t) * nnz, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(nzval, ctx->nzval, sizeof(double) * nnz, hipMemcpyDeviceToHost, ctx->stream));
        if (tval) HIPCHK(ctx, hipMemcpyAsync(tval, ctx->tval, sizeof(double) * nnz, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MPFMT_OK;
}

static int32_t steer_graph_edges_free(mpfmt_ctx* ctx, mpfmt_steer kind, uint64_t* mask, uint8_t* nseg)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->steer_counted || ctx->steer_kind != kind)
        return mpfmt_fail(ctx, MPFMT_ERR_STATE, kind == MPFMT_STEER_DI ? "di_graph_edges_free before di_graph_count" : "car graph_edges_free before graph_count");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if (!ctx->steer_filled && (rc = mpfmt_di_fill(ctx))) return rc;
    if ((rc = steer_sweep(ctx, kind))) return rc;
    const int64_t nnz = ctx->nnz, words = (nnz + 63) / 64;
    if (nnz > 0) {
        if (!mask) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "mask is NULL");
        HIPCHK(ctx, hipMemcpyAsync(mask, ctx->graph_free, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, ctx->stream));
        if (nseg) HIPCHK(ctx, hipMemcpyAsync(nseg, ctx->steer_nseg, (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MPFMT_OK;
}

// the resident, swept mask and counts as they are (after in-place box edits: what a whole sweep of the list would write); no sweep
int32_t mpfmt_steer_mask_read(mpfmt_ctx* ctx, uint64_t* mask, uint8_t* nseg)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->steer_filled || !ctx->steer_swept) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no swept steering graph resident");
    const int64_t nnz = ctx->nnz, words = (nnz + 63) / 64;
    if (nnz == 0) return MPFMT_OK;
    if (!mask) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "mask is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(mask, ctx->graph_free, sizeof(uint64_t) * (size_t)words, hipMemcpyDeviceToHost, ctx->stream));
    if (nseg) HIPCHK(ctx, hipMemcpyAsync(nseg, ctx->steer_nseg, (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

// ---- double integrator ----------------------------------------------------------------------------------------------

int32_t mpfmt_di_graph_count(mpfmt_ctx* ctx, double rho, double r, int64_t* colptr, int64_t* nnz)
{ return steer_graph_count(ctx, MPFMT_STEER_DI, rho, 0.0, r, colptr, nnz); }
int32_t mpfmt_di_graph_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval, double* tval)
{ return steer_graph_fill(ctx, MPFMT_STEER_DI, rowval, nzval, tval); }
int32_t mpfmt_di_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask, uint8_t* nseg) { return steer_graph_edges_free(ctx, MPFMT_STEER_DI, mask, nseg); }

// the double-integrator graph and its edge bits with every output left in HBM (bench.py --workload cfg4: no PCIe in the timed region)
int32_t mpfmt_di_graph_step_device(mpfmt_ctx* ctx, double rho, double r, int64_t* nnz)
{
    if (!ctx) return MPFMT_ERR_ARG;
    int32_t rc;
    if ((rc = di_check(ctx, rho, r))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = mpfmt_di_count(ctx, rho, r))) return rc;
    if ((rc = mpfmt_di_fill(ctx))) return rc;
    if (ctx->have_boxes && (rc = mpfmt_di_sweep(ctx))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (nnz) *nnz = ctx->nnz;
    return MPFMT_OK;
}

int32_t mpfmt_di_graph_device_ptrs(mpfmt_ctx* ctx, void** colptr, void** rowval, void** nzval, void** tval, void** free_mask, void** nseg)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->steer_filled || ctx->steer_kind != MPFMT_STEER_DI) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no double-integrator graph resident");
    if (colptr) *colptr = ctx->colptr;
    if (rowval) *rowval = ctx->rowval;
    if (nzval) *nzval = ctx->nzval;
    if (tval) *tval = ctx->tval;
    if (free_mask) *free_mask = ctx->steer_swept ? (void*)ctx->graph_free.get() : nullptr;
    if (nseg) *nseg = ctx->steer_swept ? (void*)ctx->steer_nseg.get() : nullptr;
    return MPFMT_OK;
}

int32_t mpfmt_di_steer(mpfmt_ctx* ctx, const double* X0, const double* X1, int64_t n, int32_t m, double rho, double r,
                       double* cost, double* topt)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "n < 0");
    if (n == 0) return MPFMT_OK;
    if (!X0 || !X1 || !cost || !topt) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "NULL array");
    if (m < 1 || m > 6) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "workspace dim m must be 1..6");
    if (!(rho > 0.0) || !(r > 0.0)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rho and r must be > 0");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t pb = sizeof(double) * (size_t)n * 2 * m;
    mpfmt_tmp tmp;
    double *d0 = nullptr, *d1 = nullptr, *dc = nullptr, *dt = nullptr;
    HIPCHK(ctx, tmp.get(&d0, pb)); HIPCHK(ctx, tmp.get(&d1, pb));
    HIPCHK(ctx, tmp.get(&dc, 8 * n)); HIPCHK(ctx, tmp.get(&dt, 8 * n));
    HIPCHK(ctx, hipMemcpyAsync(d0, X0, pb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d1, X1, pb, hipMemcpyHostToDevice, ctx->stream));
    int32_t rc = mpfmt_di_steer_launch(ctx, m, d0, d1, n, rho, r, dc, dt);
    if (rc == MPFMT_OK) {
        hipMemcpyAsync(cost, dc, 8 * n, hipMemcpyDeviceToHost, ctx->stream);
        hipMemcpyAsync(topt, dt, 8 * n, hipMemcpyDeviceToHost, ctx->stream);
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = mpfmt_fail(ctx, MPFMT_ERR_HIP, "di_steer copy back: %s", hipGetErrorString(e));
    }
    return rc;
}

int32_t mpfmt_di_fmtstar(mpfmt_ctx* ctx, double rho, double r, int64_t init_idx, int32_t checkpts,
                         int32_t goal_kind, const double* goal_params,
                         int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{ return steer_fmtstar(ctx, MPFMT_STEER_DI, rho, 0.0, r, init_idx, checkpts, goal_kind, goal_params, A, C, path, res); }

// `single` reproduces mpfmt_di_fmtstar / the reference's pop order exactly
int32_t mpfmt_di_fmtstar_wavefront(mpfmt_ctx* ctx, double rho, double r, int64_t init_idx, int32_t checkpts, int32_t goal_kind,
                                   const double* goal_params, double band, int32_t flags, int64_t* A, double* C, int64_t* path,
                                   mpfmt_fmt_result* res, mpfmt_wf_info* info)
{ return steer_fmtstar_wavefront(ctx, MPFMT_STEER_DI, rho, 0.0, r, init_idx, checkpts, goal_kind, goal_params, band, flags, A, C, path, res, info); }

// ---- Dubins and Reeds-Shepp cars ------------------------------------------------------------------------------------

// controls out: [n][nctl][3]; nctl = 3 (Dubins) or 5 (Reeds-Shepp); nsegs (may be NULL) = segments used per pair
static int32_t car_steer_pairs(mpfmt_ctx* ctx, mpfmt_steer kind, const double* X0, const double* X1, int64_t n, double turn_radius, double speed,
                               double* cost, double* controls, int32_t* nsegs)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (n < 0) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "n < 0");
    if (n == 0) return MPFMT_OK;
    if (!X0 || !X1 || !cost) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "NULL array");
    if (!(turn_radius > 0.0) || !(speed > 0.0)) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "turning radius and speed must be > 0");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    mpfmt_tmp tmp;
    double *d0, *d1, *dc, *du; int32_t* dn;
    int32_t rc;
    HIPCHK(ctx, tmp.get(&d0, sizeof(double) * 3 * n));
    HIPCHK(ctx, tmp.get(&d1, sizeof(double) * 3 * n));
    HIPCHK(ctx, tmp.get(&dc, sizeof(double) * n));
    HIPCHK(ctx, tmp.get(&du, sizeof(double) * 15 * n));
    HIPCHK(ctx, tmp.get(&dn, sizeof(int32_t) * n));
    HIPCHK(ctx, hipMemcpyAsync(d0, X0, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d1, X1, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = mpfmt_car_steer_batch(ctx, kind, d0, d1, n, turn_radius, speed, dc, du, dn))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(cost, dc, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> u5;
    if (controls) { u5.resize((size_t)15 * n); HIPCHK(ctx, hipMemcpyAsync(u5.data(), du, sizeof(double) * 15 * n, hipMemcpyDeviceToHost, ctx->stream)); }
    if (nsegs) HIPCHK(ctx, hipMemcpyAsync(nsegs, dn, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (controls) {
        const int nctl = kind == MPFMT_STEER_REEDSSHEPP ? 5 : 3;
        for (int64_t i = 0; i < n; ++i) memcpy(controls + (size_t)i * nctl * 3, u5.data() + (size_t)i * 15, sizeof(double) * nctl * 3);
    }
    return MPFMT_OK;
}

int32_t mpfmt_dubins_fmtstar_wavefront(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                                       int32_t goal_kind, const double* goal_params, double band, int32_t flags, int64_t* A, double* C,
                                       int64_t* path, mpfmt_fmt_result* res, mpfmt_wf_info* info)
{ return steer_fmtstar_wavefront(ctx, MPFMT_STEER_DUBINS, turn_radius, speed, r, init_idx, checkpts, goal_kind, goal_params, band, flags, A, C, path, res, info); }
int32_t mpfmt_reedsshepp_fmtstar_wavefront(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                                           int32_t goal_kind, const double* goal_params, double band, int32_t flags, int64_t* A, double* C,
                                           int64_t* path, mpfmt_fmt_result* res, mpfmt_wf_info* info)
{ return steer_fmtstar_wavefront(ctx, MPFMT_STEER_REEDSSHEPP, turn_radius, speed, r, init_idx, checkpts, goal_kind, goal_params, band, flags, A, C, path, res, info); }

int32_t mpfmt_dubins_graph_count(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t* colptr, int64_t* nnz)
{ return steer_graph_count(ctx, MPFMT_STEER_DUBINS, turn_radius, speed, r, colptr, nnz); }
int32_t mpfmt_dubins_graph_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval) { return steer_graph_fill(ctx, MPFMT_STEER_DUBINS, rowval, nzval, nullptr); }
int32_t mpfmt_dubins_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask, uint8_t* nseg) { return steer_graph_edges_free(ctx, MPFMT_STEER_DUBINS, mask, nseg); }
int32_t mpfmt_dubins_steer(mpfmt_ctx* ctx, const double* X0, const double* X1, int64_t n, double turn_radius, double speed,
                           double* cost, double* controls)
{ return car_steer_pairs(ctx, MPFMT_STEER_DUBINS, X0, X1, n, turn_radius, speed, cost, controls, nullptr); }
int32_t mpfmt_dubins_fmtstar(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                             int32_t goal_kind, const double* goal_params, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{ return steer_fmtstar(ctx, MPFMT_STEER_DUBINS, turn_radius, speed, r, init_idx, checkpts, goal_kind, goal_params, A, C, path, res); }

int32_t mpfmt_reedsshepp_graph_count(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t* colptr, int64_t* nnz)
{ return steer_graph_count(ctx, MPFMT_STEER_REEDSSHEPP, turn_radius, speed, r, colptr, nnz); }
int32_t mpfmt_reedsshepp_graph_fill(mpfmt_ctx* ctx, int64_t* rowval, double* nzval) { return steer_graph_fill(ctx, MPFMT_STEER_REEDSSHEPP, rowval, nzval, nullptr); }
int32_t mpfmt_reedsshepp_graph_edges_free(mpfmt_ctx* ctx, uint64_t* mask, uint8_t* nseg) { return steer_graph_edges_free(ctx, MPFMT_STEER_REEDSSHEPP, mask, nseg); }
int32_t mpfmt_reedsshepp_steer(mpfmt_ctx* ctx, const double* X0, const double* X1, int64_t n, double turn_radius, double speed,
                               double* cost, double* controls, int32_t* nsegs)
{ return car_steer_pairs(ctx, MPFMT_STEER_REEDSSHEPP, X0, X1, n, turn_radius, speed, cost, controls, nsegs); }
int32_t mpfmt_reedsshepp_fmtstar(mpfmt_ctx* ctx, double turn_radius, double speed, double r, int64_t init_idx, int32_t checkpts,
                                 int32_t goal_kind, const double* goal_params, int64_t* A, double* C, int64_t* path, mpfmt_fmt_result* res)
{ return steer_fmtstar(ctx, MPFMT_STEER_REEDSSHEPP, turn_radius, speed, r, init_idx, checkpts, goal_kind, goal_params, A, C, path, res); }

// ---- measurement ---------------------------------------------------------------------------------------

int32_t mpfmt_timing_reset(mpfmt_ctx* ctx)
{
    if (!ctx) return MPFMT_ERR_ARG;
    timer_resolve(ctx);
    ctx->timers.clear();
    return MPFMT_OK;
}

int32_t mpfmt_timing_get(mpfmt_ctx* ctx, const char* name, double* avg_ms, int64_t* launches)
{
    if (!ctx || !name) return MPFMT_ERR_ARG;
    timer_resolve(ctx);
    auto it = ctx->timers.find(name);
    double a = 0.0; int64_t n = 0;
    if (it != ctx->timers.end() && it->second.launches > 0) { n = it->second.launches; a = it->second.total_ms / (double)n; }
    if (avg_ms) *avg_ms = a;
    if (launches) *launches = n;
    return MPFMT_OK;
}

int32_t mpfmt_set_option(mpfmt_ctx* ctx, const char* name, int64_t value)
{
    if (!ctx || !name) return MPFMT_ERR_ARG;
    if (strcmp(name, "rdisc_path") == 0) {
        if (value < 0 || value > 2) return mpfmt_fail(ctx, MPFMT_ERR_ARG, "rdisc_path must be 0 (auto), 1 (fp64 VALU) or 2 (MFMA filter)");
        ctx->rdisc_path = (int32_t)value;
        ctx->graph_r = -1.0; ctx->graph_counted = ctx->graph_filled = ctx->graph_swept = false;
        return MPFMT_OK;
    }
    if (strcmp(name, "rebuild_index") == 0) { ctx->rebuild_index = value != 0; return MPFMT_OK; }
    if (strcmp(name, "rdisc_pool") == 0) { ctx->use_pool = value != 0; return MPFMT_OK; }
    if (strcmp(name, "wf_graphs") == 0) { ctx->wf_graphs = value != 0; return MPFMT_OK; }
    if (strcmp(name, "debug_small_lists") == 0) { ctx->debug_small_lists = value != 0; return MPFMT_OK; }
    if (strcmp(name, "fuse_broad") == 0) {
        ctx->fuse_broad = (int)value;                           // 0 off, 1 flagged entries listed by the ordering pass (k_sweep_pending), 2 flagged pairs tested before it (k_exact_pairs)
        ctx->graph_r = -1.0; ctx->graph_counted = ctx->graph_filled = ctx->graph_swept = false; ctx->spec_ready = false;
        return MPFMT_OK;
    }
    if (strcmp(name, "rdisc_half") == 0) {
        ctx->use_half = value != 0;
        ctx->graph_r = -1.0; ctx->graph_counted = ctx->graph_filled = ctx->graph_swept = false; ctx->spec_ready = false; ctx->lists_r = -1.0;
        return MPFMT_OK;
    }
    if (strcmp(name, "mf_tail_permille") == 0) { ctx->mf_tail_permille = (int32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 1000); return MPFMT_OK; }
    if (strcmp(name, "ord_draw") == 0) { ctx->ord_draw = (int32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 2); return MPFMT_OK; }
    if (strcmp(name, "mf_tail_min_items") == 0) { ctx->mf_tail_min_items = std::max<int64_t>(value, 0); return MPFMT_OK; }
    if (strcmp(name, "mf_tail_slices") == 0) { ctx->mf_tail_slices = (int32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 63); return MPFMT_OK; }
    if (strcmp(name, "mf_xcd_mode") == 0) { ctx->mf_xcd_mode = (int32_t)value; return MPFMT_OK; }
    if (strcmp(name, "overlap") == 0) { ctx->overlap = (int32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 2); return MPFMT_OK; }
    if (strcmp(name, "wf_pos_space") == 0) { ctx->wf_pos_space = value < 0 ? 0 : (value > 2 ? 2 : (int32_t)value); return MPFMT_OK; }
    if (strcmp(name, "shard_blocks") == 0) { ctx->shard_blocks = value != 0; ctx->grid_r = -1.0; ctx->ops_r = -1.0; ctx->lists_r = -1.0; ctx->cut_key.clear(); return MPFMT_OK; }
    if (strcmp(name, "index_halo") == 0) { ctx->index_halo = value != 0; ctx->grid_r = -1.0; ctx->ops_r = -1.0; ctx->lists_r = -1.0; return MPFMT_OK; }
    if (strcmp(name, "cell_fb_max") == 0) { ctx->cell_fb_max = (int32_t)std::min<int64_t>(8, std::max<int64_t>(0, value)); ctx->grid_r = -1.0; return MPFMT_OK; }
    if (strcmp(name, "mf_target_items") == 0) { ctx->mf_target_items = value; return MPFMT_OK; }
    if (strcmp(name, "timing") == 0) { ctx->timing_enabled = value != 0; return MPFMT_OK; }
    if (strcmp(name, "sweep_rounds") == 0) {
        ctx->sweep_rounds = value != 0;
        return MPFMT_OK;
    }
    if (strcmp(name, "di_path") == 0) { ctx->di_path = (int32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 2); ctx->steer_counted = ctx->steer_filled = ctx->steer_swept = false; return MPFMT_OK; }
    if (strcmp(name, "wf_force_sharded") == 0) { ctx->wf_force_sharded = value != 0; return MPFMT_OK; }
    if (strcmp(name, "steer_shapes_delta") == 0) { ctx->steer_shapes_delta = value != 0; return MPFMT_OK; }
    if (strcmp(name, "samples_add_keeps_fields") == 0) { ctx->grow_keeps_fields = value != 0; return MPFMT_OK; }
    return mpfmt_fail(ctx, MPFMT_ERR_ARG, "unknown option %s", name);
}

int32_t mpfmt_get_stat(mpfmt_ctx* ctx, const char* name, int64_t* value)
{
    if (!ctx || !name || !value) return MPFMT_ERR_ARG;
    if (strcmp(name, "rdisc_path_used") == 0) { *value = ctx->rdisc_path_used; return MPFMT_OK; }
    if (strcmp(name, "rdisc_half_used") == 0) { *value = ctx->half_used ? 1 : 0; return MPFMT_OK; }
    if (strcmp(name, "sweep_form") == 0) {                   // how the resident mask was made: 0 whole sweep, 1 pending entries, 2 pairs before the ordering
        *value = ctx->sweep_in_order ? 2 : (ctx->sweep_pending_used && ctx->pend_valid) ? 1 : 0; return MPFMT_OK;
    }
    if (strcmp(name, "pair_items") == 0) {                   // (a synchronising read) pending pairs the last half build listed for k_exact_pairs
        *value = 0;
        const int64_t items = 1024;
        if (ctx->bits_in_records && ctx->pair_cnt && items > 0) {
            std::vector<int32_t> h((size_t)items);
            HIPCHK(ctx, hipMemcpyAsync(h.data(), ctx->pair_cnt, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            for (int32_t v : h) *value += v;
        }
        return MPFMT_OK;
    }
    if (strcmp(name, "samples_add_path") == 0) { *value = ctx->grow_path; return MPFMT_OK; }
    if (strcmp(name, "samples_add_candidates") == 0) { *value = ctx->grow_candidates; return MPFMT_OK; }
    if (strcmp(name, "samples_add_entries") == 0) { *value = ctx->grow_entries; return MPFMT_OK; }
    if (strcmp(name, "samples_add_dropped") == 0) { *value = ctx->grow_dropped; return MPFMT_OK; }
    if (strcmp(name, "samples_add_flagged_columns") == 0) { *value = ctx->grow_flagged; return MPFMT_OK; }
    if (strcmp(name, "samples_add_fields_carried") == 0) { *value = ctx->grow_carried; return MPFMT_OK; }
    if (strcmp(name, "samples_add_keeps_fields") == 0) { *value = ctx->grow_keeps_fields; return MPFMT_OK; }
    if (strcmp(name, "pend_overflowed") == 0) { *value = ctx->pend_overflowed ? 1 : 0; return MPFMT_OK; }
    if (strcmp(name, "redo_count") == 0) { *value = ctx->redo_count; return MPFMT_OK; }
    if (strcmp(name, "redo_reason") == 0) { *value = ctx->redo_reason; ctx->redo_reason = 0; return MPFMT_OK; }      // (bits since the last read)
    if (strcmp(name, "ord_per_cu") == 0) { *value = ctx->ord_per_cu; return MPFMT_OK; }
    if (strcmp(name, "qcap") == 0) { *value = ctx->qcap; return MPFMT_OK; }
    if (strcmp(name, "pool_used") == 0) { *value = ctx->pool_valid ? 1 : 0; return MPFMT_OK; }
    if (strcmp(name, "list_cap") == 0) { *value = ctx->list_cap; return MPFMT_OK; }
    if (strcmp(name, "list_max") == 0) {                     // (a synchronising read) longest chunk list of the last list build
        *value = 0;
        const int64_t nt = ctx->tile_end - ctx->tile_begin;
        if (ctx->list_len && nt > 0) {
            int32_t v = 0;
            HIPCHK(ctx, hipMemcpyAsync(&v, ctx->list_max, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            *value = v;
        }
        return MPFMT_OK;
    }
    if (strncmp(name, "list_q", 6) == 0 || strcmp(name, "list_argmax") == 0 || strcmp(name, "list_sum") == 0) {
        // (synchronising reads, diagnostics) list_q<permille>: that quantile of the tiles' chunk-list lengths; list_argmax: the tile (counted
        // from the shard's first) with the longest list; list_sum: all entries
        *value = 0;
        const int64_t nt = ctx->tile_end - ctx->tile_begin;
        if (ctx->list_len && nt > 0) {
            std::vector<int32_t> h((size_t)nt);
            HIPCHK(ctx, hipMemcpyAsync(h.data(), ctx->list_len, sizeof(int32_t) * (size_t)nt, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            if (strcmp(name, "list_argmax") == 0) *value = (int64_t)(std::max_element(h.begin(), h.end()) - h.begin());
            else if (strcmp(name, "list_sum") == 0) { int64_t t = 0; for (int32_t v : h) t += v; *value = t; }
            else {
                const int64_t q = std::min<int64_t>(1000, std::max<int64_t>(0, atoll(name + 6)));
                std::sort(h.begin(), h.end());
                *value = h[(size_t)std::min<int64_t>(nt - 1, nt * q / 1000)];
            }
        }
        return MPFMT_OK;
    }
    if (strcmp(name, "knn_pairs_tested") == 0) { *value = ctx->knn_pairs; return MPFMT_OK; }
    if (strcmp(name, "knn_rounds") == 0) { *value = ctx->knn_rounds; return MPFMT_OK; }
    if (strcmp(name, "knn_short_columns") == 0) { *value = ctx->knn_short; return MPFMT_OK; }
    if (strcmp(name, "knn_scan_columns") == 0) { *value = ctx->knn_scan; return MPFMT_OK; }
    if (strcmp(name, "sssp_rounds") == 0) { *value = ctx->sssp_rounds; return MPFMT_OK; }
    if (strcmp(name, "sssp_relaxations") == 0) { *value = ctx->sssp_relax; return MPFMT_OK; }
    if (strcmp(name, "sssp_reached") == 0) { *value = ctx->sssp_reached; return MPFMT_OK; }
    if (strcmp(name, "sssp_to_columns") == 0) { *value = ctx->sssp_to_columns; return MPFMT_OK; }
    if (strcmp(name, "sssp_to_entries_read") == 0) { *value = ctx->sssp_to_entries; return MPFMT_OK; }
    if (strcmp(name, "sssp_to_atomics") == 0) { *value = ctx->sssp_to_atomics; return MPFMT_OK; }
    if (strcmp(name, "sssp_multi_groups") == 0) { *value = ctx->ms_groups; return MPFMT_OK; }
    if (strcmp(name, "sssp_multi_rounds") == 0) { *value = ctx->ms_rounds; return MPFMT_OK; }
    if (strcmp(name, "sssp_multi_rows_read") == 0) { *value = ctx->ms_rows; return MPFMT_OK; }
    if (strcmp(name, "sssp_multi_bytes") == 0) { *value = ctx->ms_bytes; return MPFMT_OK; }
    if (strcmp(name, "roadmap_candidates") == 0) { *value = ctx->roadmap_candidates; return MPFMT_OK; }
    if (strcmp(name, "roadmap_near_total") == 0) { *value = ctx->roadmap_near_total; return MPFMT_OK; }
    if (strcmp(name, "steer_roadmap_steered") == 0) { *value = ctx->steer_roadmap_steered; return MPFMT_OK; }
    if (strcmp(name, "shortcut_tests_evaluated") == 0) { *value = ctx->shortcut_tests; return MPFMT_OK; }
    if (strcmp(name, "shortcut_checks") == 0) { *value = ctx->shortcut_checks; return MPFMT_OK; }
    if (strcmp(name, "steer_shortcut_tests_evaluated") == 0) { *value = ctx->ssc_tests; return MPFMT_OK; }
    if (strcmp(name, "steer_shortcut_checks") == 0) { *value = ctx->ssc_checks; return MPFMT_OK; }
    if (strcmp(name, "discretize_steps") == 0) { *value = ctx->disc_steps; return MPFMT_OK; }
    if (strcmp(name, "discretize_samples") == 0) { *value = ctx->disc_samples; return MPFMT_OK; }
    if (strcmp(name, "steer_swept") == 0) { *value = (ctx->steer_filled && ctx->steer_swept) ? 1 : 0; return MPFMT_OK; }
    if (strcmp(name, "steer_shapes_delta") == 0) { *value = ctx->steer_shapes_delta; return MPFMT_OK; }
    if (strcmp(name, "boxes_delta_path") == 0) { *value = ctx->bd_path; return MPFMT_OK; }
    if (strcmp(name, "boxes_delta_columns") == 0) { *value = ctx->bd_columns; return MPFMT_OK; }
    if (strcmp(name, "boxes_delta_entries") == 0) { *value = ctx->bd_entries; return MPFMT_OK; }
    if (strcmp(name, "togo_tracked") == 0) { *value = mpfmt_togo_live(ctx) ? 1 : 0; return MPFMT_OK; }
    if (strcmp(name, "togo_path") == 0) { *value = ctx->tg_path; return MPFMT_OK; }
    if (strcmp(name, "togo_seed_form") == 0) { *value = ctx->tg_seed_form; return MPFMT_OK; }
    if (strcmp(name, "togo_reached") == 0) { *value = ctx->tg_reached; return MPFMT_OK; }
    if (strcmp(name, "togo_invalidated") == 0) { *value = ctx->tg_invalidated; return MPFMT_OK; }
    if (strcmp(name, "togo_dirty_columns") == 0) { *value = ctx->tg_dirty_columns; return MPFMT_OK; }
    if (strcmp(name, "togo_columns_read") == 0) { *value = ctx->tg_columns_read; return MPFMT_OK; }
    if (strcmp(name, "togo_column_visits") == 0) { *value = ctx->tg_column_visits; return MPFMT_OK; }
    if (strcmp(name, "togo_entries_read") == 0) { *value = ctx->tg_entries_read; return MPFMT_OK; }
    if (strcmp(name, "togo_rounds") == 0) { *value = ctx->tg_rounds; return MPFMT_OK; }
    if (strcmp(name, "togo_relaxations") == 0) { *value = ctx->tg_relax; return MPFMT_OK; }
    if (strcmp(name, "togo_atomics") == 0) { *value = ctx->tg_atomics; return MPFMT_OK; }
    if (strcmp(name, "field_tracked") == 0) { *value = mpfmt_field_live(ctx) ? 1 : 0; return MPFMT_OK; }
    if (strcmp(name, "field_update_path") == 0) { *value = ctx->fld_path; return MPFMT_OK; }
    if (strcmp(name, "field_invalidated") == 0) { *value = ctx->fld_invalidated; return MPFMT_OK; }
    if (strcmp(name, "field_dirty_columns") == 0) { *value = ctx->fld_dirty_columns; return MPFMT_OK; }
    if (strcmp(name, "field_columns_read") == 0) { *value = ctx->fld_columns_read; return MPFMT_OK; }
    if (strcmp(name, "field_column_visits") == 0) { *value = ctx->fld_column_visits; return MPFMT_OK; }
    if (strcmp(name, "field_entries_read") == 0) { *value = ctx->fld_entries_read; return MPFMT_OK; }
    if (strcmp(name, "field_rounds") == 0) { *value = ctx->fld_rounds; return MPFMT_OK; }
    if (strcmp(name, "field_relaxations") == 0) { *value = ctx->fld_relax; return MPFMT_OK; }
    if (strcmp(name, "field_reached") == 0) { *value = ctx->fld_reached; return MPFMT_OK; }
    if (strcmp(name, "boxes") == 0) { *value = ctx->have_boxes ? ctx->M : 0; return MPFMT_OK; }
    if (strcmp(name, "graph_swept") == 0) { *value = ctx->graph_swept ? 1 : 0; return MPFMT_OK; }
    if (strcmp(name, "survivors") == 0) { *value = ctx->survivors; return MPFMT_OK; }
    if (strcmp(name, "drains") == 0) { *value = ctx->drains; return MPFMT_OK; }
    if (strcmp(name, "drain_boxes") == 0) { *value = ctx->drain_boxes; return MPFMT_OK; }
    if (strcmp(name, "pairs_tested") == 0) { *value = ctx->pairs_tested; return MPFMT_OK; }
    if (strcmp(name, "nnz") == 0) { *value = ctx->nnz; return MPFMT_OK; }
    if (strcmp(name, "slices") == 0) { *value = ctx->S; return MPFMT_OK; }
    if (strcmp(name, "cells") == 0) { *value = ctx->grid.ncells; return MPFMT_OK; }
    if (strcmp(name, "filter_valu") == 0) { *value = ctx->filter_valu ? 1 : 0; return MPFMT_OK; }
    if (strcmp(name, "wf_pos_space_used") == 0) { *value = ctx->wf_pos_used; return MPFMT_OK; }
    if (strcmp(name, "di_path_used") == 0) { *value = ctx->di_mf ? 2 : 1; return MPFMT_OK; }
    return mpfmt_fail(ctx, MPFMT_ERR_ARG, "unknown stat %s", name);
}

int32_t mpfmt_graph_stats(mpfmt_ctx* ctx, int64_t* pairs_tested, int64_t* tiles, int64_t* slices, int64_t* cells)
{
    if (!ctx) return MPFMT_ERR_ARG;
    if (!ctx->graph_counted) return mpfmt_fail(ctx, MPFMT_ERR_STATE, "no graph counted");
    if (pairs_tested) *pairs_tested = ctx->pairs_tested;
    if (tiles) *tiles = ctx->tile_end - ctx->tile_begin;
    if (slices) *slices = ctx->S;
    if (cells) *cells = ctx->grid.ncells;
    return MPFMT_OK;
}

}  // extern "C"
