// views.hip -- sfm_extract_views / sfm_extract_views_u8: ExtractSift for a rank's share of the images (BASELINE configs[4]),
// host threads around the per-view launchers of sift.hip.
#include "common.hpp"
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

extern "C" {
// 8-bit grey values -> float (exact), four pixels per thread; count is a multiple of four (the pitch is a multiple of 128)
__global__ __launch_bounds__(256)
void views_u8_to_float_kernel(const uchar4 *__restrict__ src, float4 *__restrict__ dst, size_t count4)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count4) return;
    const uchar4 v = src[i];
    dst[i] = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
}
}

namespace sfm {

static int views_buffers(sfm_ctx *c, size_t floats)
{
    if (!c->views_ev) SFM_HIP_TRY(hipEventCreateWithFlags(&c->views_ev, hipEventDisableTiming));
    if (c->views_floats >= floats) return SFM_OK;
    SFM_HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->views_pinned) (void)hipHostFree(c->views_pinned);
    c->views_pinned = nullptr; c->views_floats = 0;     // (the size counts for both: the device image grows last)
    SFM_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&c->views_pinned), floats * sizeof(float), hipHostMallocDefault));
    return grow(&c->views_image, &c->views_floats, floats, c->stream);
}

// EIGHT contexts (the caller's + the auxiliary lanes): one image's per-level kernels leave most CUs idle, and every view
// ends with a host synchronisation (its feature count), so eight views are in flight on eight streams.
constexpr int NC = sfm_ctx::kViewLanes;           // contexts
constexpr int NR = 2 * NC;                        // pinned staging buffers (two per context)
constexpr int NT = 3;                             // helper threads that fill them

// device image per context; pinned staging buffers filled by helper threads that run ahead of the enqueueing threads:
// the row-by-row copy into pinned memory is the host-side cost of a view (~0.1 ms for 720 x 576, about what its
// extraction takes and more than its upload), so it must neither sit between two enqueues nor be done by ONE thread
struct ViewRing {
    sfm_ctx *cs[NC];
    float *ring[NR], *image[NC];
    // view i: staged once its pixels are in ring[i % NR], finished once its count is back (ring[i % NR] may be refilled)
    std::vector<std::atomic<int>> staged, finished;
    explicit ViewRing(int nown) : staged((size_t)nown), finished((size_t)nown)
    {
        for (auto &f : staged) f.store(0, std::memory_order_relaxed);
        for (auto &f : finished) f.store(0, std::memory_order_relaxed);
    }
};

// one sfm_extract_views call: what its threads share
struct ViewsCall {
    sfm_ctx *ctx;
    const void *const *h_images;      // float images (bytes_per_pixel 4) or 8-bit grey images (bytes_per_pixel 1: a quarter of the PCIe
    int bytes_per_pixel;              // traffic, the conversion -- exact -- runs on the device in front of the extraction)
    int width, height, first, stride;
    char *block;
    size_t slot_bytes;
    int max_pts, num_octaves;
    double init_blur;
    float thresh, lowest_scale;
    int scale_up;
    int nown, pitch;
    size_t floats;
    ViewRing ring;
    std::vector<int> counts;
    std::atomic<int> stop{0}, first_rc{SFM_OK};
    std::mutex err_mutex;
    char err_text[512] = "";

    // the first error of any thread is the call's; everybody stops
    void fail(int rc)
    {
        int expected = SFM_OK;
        if (first_rc.compare_exchange_strong(expected, rc)) {
            std::lock_guard<std::mutex> g(err_mutex);
            snprintf(err_text, sizeof(err_text), "%s", sfm_last_error());      // (the message lives in this thread's buffer)
        }
        stop.store(1, std::memory_order_relaxed);
    }
    bool stopped() const { return stop.load(std::memory_order_relaxed) != 0; }
};

// stager t: views t, t + NT, ... -> buffer i % NR, once view i - NR is through
static void stage_views(ViewsCall &c, int t)
{
    ViewRing &r = c.ring;
    for (int i = t; i < c.nown && !c.stopped(); i += NT) {
        while (i >= NR && r.finished[(size_t)(i - NR)].load(std::memory_order_acquire) == 0 && !c.stopped()) std::this_thread::yield();
        char *pin = reinterpret_cast<char *>(r.ring[i % NR]);
        const char *src = static_cast<const char *>(c.h_images[c.first + i * c.stride]);
        const size_t px = (size_t)c.bytes_per_pixel;
        for (int y = 0; y < c.height; ++y) {
            memcpy(pin + (size_t)y * c.pitch * px, src + (size_t)y * c.width * px, (size_t)c.width * px);
            if (c.pitch > c.width) memset(pin + ((size_t)y * c.pitch + c.width) * px, 0, (size_t)(c.pitch - c.width) * px);
        }
        r.staged[(size_t)i].store(1, std::memory_order_release);
    }
}

// view i from its staging buffer into context k's device image (8-bit images: widened there)
static hipError_t upload_view(ViewsCall &c, int k, int i)
{
    ViewRing &r = c.ring;
    if (c.bytes_per_pixel != 1) return hipMemcpyAsync(r.image[k], r.ring[i % NR], c.floats * sizeof(float), hipMemcpyHostToDevice, r.cs[k]->stream);
    // (the second half of the context's device image buffer holds the bytes until the kernel has widened them)
    unsigned char *d_bytes = reinterpret_cast<unsigned char *>(r.image[k] + c.floats);
    const hipError_t e = hipMemcpyAsync(d_bytes, r.ring[i % NR], c.floats, hipMemcpyHostToDevice, r.cs[k]->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(views_u8_to_float_kernel, dim3((unsigned)((c.floats / 4 + 255) / 256)), dim3(256), 0, r.cs[k]->stream,
                       reinterpret_cast<const uchar4 *>(d_bytes), reinterpret_cast<float4 *>(r.image[k]), c.floats / 4);
    return hipGetLastError();
}

// the worker of context k uploads, enqueues and reads back the count of the views i = k, k + NC, ... -- about fifteen runtime
// calls per view, 60-100 us of host time
static void extract_views(ViewsCall &c, int k)
{
    ViewRing &r = c.ring;
    if (hipSetDevice(c.ctx->device) != hipSuccess) { set_error("hipSetDevice failed in a view worker"); c.fail(SFM_E_HIP); return; }
    for (int i = k; i < c.nown && !c.stopped(); i += NC) {
        while (r.staged[(size_t)i].load(std::memory_order_acquire) == 0 && !c.stopped()) std::this_thread::yield();
        if (c.stopped()) break;
        const hipError_t e = upload_view(c, k, i);
        if (e != hipSuccess) { set_error("view upload failed: %s", hipGetErrorString(e)); c.fail(SFM_E_HIP); break; }
        int rc = launch_extract_sift_begin(r.cs[k], reinterpret_cast<sfm_sift_point *>(c.block + (size_t)i * c.slot_bytes), c.max_pts, r.image[k],
                                           c.width, c.height, c.pitch, c.num_octaves, c.init_blur, c.thresh, c.lowest_scale, c.scale_up ? 1 : 0, nullptr);
        int n = 0, stored = 0;
        if (rc == SFM_OK) rc = launch_extract_sift_end(r.cs[k], &n, &stored);    // waits for this context's stream: its upload is done too
        if (rc != SFM_OK) { c.fail(rc); break; }
        c.counts[(size_t)i] = n;
        r.finished[(size_t)i].store(1, std::memory_order_release);           // staging buffer i % NR may be refilled
    }
}

// Threads: NT stagers fill the pinned buffers; one worker per context.  With float images the uploads (1.66 MB per 720 x 576
// view, one copy engine) bound the front end and a single enqueueing thread is enough; with 8-bit images (a quarter of the
// bytes) the enqueueing thread did.  Returns after every thread has ended and, on failure, every stream has drained.
static int run_threads(ViewsCall &c)
{
    std::vector<std::thread> threads;
    // the caller's thread takes the LAST context: it starts after the others have been spawned, and the last contexts get one
    // view fewer when the views do not divide evenly (36 views on eight contexts: 5 5 5 5 4 4 4 4)
    const int lanes_used = c.nown < NC ? c.nown : NC;
    bool spawned = true;
    try {
        for (int t = 0; t < NT && t < c.nown; ++t) threads.emplace_back(stage_views, std::ref(c), t);
        for (int k = 0; k + 1 < lanes_used; ++k) threads.emplace_back(extract_views, std::ref(c), k);
    } catch (...) {                                       // (std::system_error: the process is out of threads)
        spawned = false;
        c.stop.store(1, std::memory_order_relaxed);
    }
    if (spawned) extract_views(c, lanes_used - 1);
    for (std::thread &t : threads) t.join();
    if (spawned && c.first_rc.load() == SFM_OK) return SFM_OK;
    for (sfm_ctx *lc : c.ring.cs) (void)hipStreamSynchronize(lc->stream);
    if (!spawned) { set_error("sfm_extract_views could not start its worker threads"); return SFM_E_NOMEM; }
    set_error("%s", c.err_text);
    return c.first_rc.load();
}

// the arguments of the call; *nown: how many of the views are this caller's
static int check_views(sfm_ctx *ctx, const void *const *h_images, int num_views, int width, int height, int first, int stride, void *d_block,
                       size_t slot_bytes, int max_pts, int num_octaves, int *nown)
{
    SFM_REQUIRE(ctx && h_images && d_block, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(num_views >= 0 && first >= 0 && stride >= 1, SFM_E_INVALID, "bad view range");
    SFM_REQUIRE(width > 0 && height > 0 && width <= 16384 && height <= 16384, SFM_E_INVALID, "image size %d x %d", width, height);
    SFM_REQUIRE(num_octaves >= 1 && num_octaves <= 7 && max_pts > 0, SFM_E_INVALID, "bad extraction parameters");
    SFM_REQUIRE(slot_bytes >= (size_t)max_pts * sizeof(sfm_sift_point) + 4 && slot_bytes % 16 == 0, SFM_E_INVALID,
                "slot_bytes %zu: need max_pts records + the count, a multiple of 16", slot_bytes);
    *nown = 0;
    for (int v = first; v < num_views; v += stride) { SFM_REQUIRE(h_images[v], SFM_E_INVALID, "view %d: null image", v); ++*nown; }
    return SFM_OK;
}

// the contexts, their device images and staging buffers; the lanes start after what the caller enqueued
static int open_ring(ViewsCall &c)
{
    ViewRing &r = c.ring;
    int rc = lane_contexts(c.ctx, NC, r.cs);
    for (int k = 0; k < NC && rc == SFM_OK; ++k) rc = views_buffers(r.cs[k], 2 * c.floats);
    if (rc != SFM_OK) return rc;
    for (int k = 0; k < NC; ++k) { r.ring[k] = r.cs[k]->views_pinned; r.ring[NC + k] = r.cs[k]->views_pinned + c.floats; r.image[k] = r.cs[k]->views_image; }
    return start_lanes_after(c.ctx, r.cs, NC, c.ctx->views_ev);
}

static int extract_views_impl(sfm_ctx *ctx, const void *const *h_images, int bytes_per_pixel, int num_views, int width, int height, int first, int stride,
                              void *d_block, size_t slot_bytes, int max_pts, int num_octaves, double init_blur, float thresh,
                              float lowest_scale, int scale_up, int *h_counts)
{
    int nown = 0;
    int rc = check_views(ctx, h_images, num_views, width, height, first, stride, d_block, slot_bytes, max_pts, num_octaves, &nown);
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    const int pitch = round_up(width, 128);
    ViewsCall c{ ctx, h_images, bytes_per_pixel, width, height, first, stride, static_cast<char *>(d_block), slot_bytes, max_pts, num_octaves,
                 init_blur, thresh, lowest_scale, scale_up, nown, pitch, (size_t)pitch * height, ViewRing(nown), std::vector<int>((size_t)nown, 0) };
    rc = open_ring(c);
    if (rc != SFM_OK || nown == 0) return rc;
    rc = run_threads(c);
    if (rc != SFM_OK) return rc;
    // the feature counts of all slots with ONE strided copy
    SFM_HIP_TRY(hipMemcpy2DAsync(c.block + (size_t)max_pts * sizeof(sfm_sift_point), slot_bytes, c.counts.data(), sizeof(int), sizeof(int), (size_t)nown,
                                 hipMemcpyHostToDevice, ctx->stream));
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (h_counts) memcpy(h_counts, c.counts.data(), (size_t)nown * sizeof(int));
    return SFM_OK;
}

} // namespace sfm

using namespace sfm;

extern "C" {

int sfm_extract_views(sfm_ctx *ctx, const float *const *h_images, int num_views, int width, int height, int first, int stride,
                      void *d_block, size_t slot_bytes, int max_pts, int num_octaves, double init_blur, float thresh,
                      float lowest_scale, int scale_up, int *h_counts)
{
    return extract_views_impl(ctx, reinterpret_cast<const void *const *>(h_images), 4, num_views, width, height, first, stride, d_block, slot_bytes,
                              max_pts, num_octaves, init_blur, thresh, lowest_scale, scale_up, h_counts);
}

int sfm_extract_views_u8(sfm_ctx *ctx, const unsigned char *const *h_images, int num_views, int width, int height, int first, int stride,
                         void *d_block, size_t slot_bytes, int max_pts, int num_octaves, double init_blur, float thresh,
                         float lowest_scale, int scale_up, int *h_counts)
{
    return extract_views_impl(ctx, reinterpret_cast<const void *const *>(h_images), 1, num_views, width, height, first, stride, d_block, slot_bytes,
                              max_pts, num_octaves, init_blur, thresh, lowest_scale, scale_up, h_counts);
}

} // extern "C"
