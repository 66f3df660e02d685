// grt_backward.hip — the backward pass of Gaussian-only frames (include/grt.h: grt_backward / grt_backward_rays):
// gradients of a loss on (rgbf, alpha) with respect to the activated attributes of the Gaussians, discrete decisions held fixed.
//
// The device text is grt_bwd.h; this unit instantiates k_backward<MERGE> from it and holds what exists once for the three backward
// units: the flush kernels, the context's gradient buffers, and the host path every entry point takes (grt_internal.h: bwd_fill_args,
// bwd_launch; the work mappings set_window and set_rays are grt_frame.hip's) — and, for grt_stats.hip and grt_features.hip as well,
// the launch of a one-ray-per-lane kernel (lane_launch, lane_launch_done), and the mesh units' step-range refusal (check_step_range).
#include <algorithm>
#include <cstring>
#include <string>

#include "grt_bwd.h"

namespace grt {
namespace {

template <bool MERGE>
__global__ __launch_bounds__(kBlock) void k_backward(const RenderArgs a, const BwdArgs b)
{
    backward_body<MERGE, true, false>(a, b, RayOut{});
}

// the context's gradient buffer -> the caller's arrays (added), and zeroed for the next call; one thread per float of a row
__global__ __launch_bounds__(256) void k_bwd_flush(float* __restrict__ acc, uint64_t n_floats, float* __restrict__ g_pos, float* __restrict__ g_scale,
                                                   float* __restrict__ g_quat, float* __restrict__ g_opacity, float* __restrict__ g_sh)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= n_floats) return;
    const float v = acc[t];
    if (v == 0.0f) return;
    acc[t] = 0.0f;
    const uint64_t i = t / kRow;
    const uint32_t k = (uint32_t)(t % kRow);
    if (k < 3u) { if (g_pos) g_pos[i * 3 + k] += v; }
    else if (k < 6u) { if (g_scale) g_scale[i * 3 + (k - 3u)] += v; }
    else if (k < 10u) { if (g_quat) g_quat[i * 4 + (k - 6u)] += v; }
    else if (k == 10u) { if (g_opacity) g_opacity[i] += v; }
    else if (k < 14u) { if (g_sh) g_sh[i * 48 + (k - 11u)] += v; }
}
__global__ __launch_bounds__(256) void k_bwd_flush_sh(float* __restrict__ acc_sh, uint64_t n_floats, float* __restrict__ g_sh)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= n_floats) return;
    const float v = acc_sh[t];
    if (v == 0.0f) return;
    acc_sh[t] = 0.0f;
    g_sh[(t / kShHi) * 48 + 3 + (t % kShHi)] += v;
}

} // namespace
} // namespace grt

using namespace grt;

// The context's gradient buffers for n particles (hi: the higher-SH buffer as well), zeroed when new; a backward on another stream
// than the last one's waits for that one's flush (the buffers belong to the context).
static int bwd_buffers(grt_ctx* c, uint64_t n, bool hi, hipStream_t s)
{
    if (c->gacc_cap < n) {
        (void)hipFree(c->d_gacc); (void)hipFree(c->d_gacc_sh);
        c->d_gacc = c->d_gacc_sh = nullptr;
        c->gacc_cap = 0; c->gacc_sh_cap = 0;
        CHK(c, hipMalloc(&c->d_gacc, n * kRow * sizeof(float)));
        CHK(c, hipMemsetAsync(c->d_gacc, 0, n * kRow * sizeof(float), s));
        c->gacc_cap = n;
    }
    if (hi && c->gacc_sh_cap < n) {
        (void)hipFree(c->d_gacc_sh);
        c->d_gacc_sh = nullptr;
        c->gacc_sh_cap = 0;
        CHK(c, hipMalloc(&c->d_gacc_sh, n * kShHi * sizeof(float)));
        CHK(c, hipMemsetAsync(c->d_gacc_sh, 0, n * kShHi * sizeof(float), s));
        c->gacc_sh_cap = n;
    }
    if (c->bwd_pending && c->bwd_stream != s) CHK(c, hipStreamWaitEvent(s, c->ev_bwd, 0));
    return GRT_OK;
}

// The flush behind a backward kernel on s: the buffers added into the caller's arrays and zeroed; ev1 and the context's
// "last backward" event recorded behind it.
static int bwd_flush(grt_ctx* c, uint64_t n, bool hi, const grt_gaussian_grads* g, hipStream_t s)
{
    const uint64_t nf = n * kRow;
    hipLaunchKernelGGL(k_bwd_flush, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, c->d_gacc, nf, g->pos, g->scale, g->quat, g->opacity, g->sh);
    if (hi) {
        const uint64_t nh = n * kShHi;
        hipLaunchKernelGGL(k_bwd_flush_sh, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, c->d_gacc_sh, nh, g->sh);
    }
    int rc = lane_launch_done(c, s);
    if (rc != GRT_OK) return rc;
    if (!c->ev_bwd) CHK(c, hipEventCreateWithFlags(&c->ev_bwd, hipEventDisableTiming));
    CHK(c, hipEventRecord(c->ev_bwd, s));
    c->bwd_pending = true; c->bwd_stream = s;
    return GRT_OK;
}

namespace grt {

int bwd_fill_args(grt_ctx* c, const grt_params* p, bool mesh, RenderArgs* a, const char* fn, const char* gauss_only)
{
    if (!c) return GRT_ERR_INVALID;
    if (!p) { c->err = std::string(fn) + ": null parameters"; return GRT_ERR_INVALID; }
    const grt_ctx* sc = scene_of(c);
    if (!sc->built) { c->err = std::string(fn) + ": grt_build_bvh has not been called after the last upload"; return GRT_ERR_INVALID; }
    if (!mesh && sc->n_faces) { c->err = std::string(fn) + ": meshes are set (" + gauss_only + ")"; return GRT_ERR_INVALID; }
    if (c->opt_counters) { c->err = std::string(fn) + ": GRT_OPT_COUNTERS = 1 (the backward kernel is not instrumented)"; return GRT_ERR_INVALID; }
    if (p->sh_degree_max > 3) { c->err = std::string(fn) + ": sh_degree_max must be 0..3"; return GRT_ERR_INVALID; }
    if (mesh && (p->type < 0 || p->type > 2)) { c->err = std::string(fn) + ": type must be MIRROR/NORMAL/GLASS"; return GRT_ERR_INVALID; }
    if (!(p->t_min > 0.0f)) { c->err = std::string(fn) + ": t_min must be > 0"; return GRT_ERR_INVALID; }
    memset(a, 0, sizeof(*a));
    a->p = *p;
    a->rec = sc->d_rec;
    a->nodes = sc->gbvh.nodes;
    a->root_ref = sc->gbvh.root_ref;
    a->n_prox = sc->gbvh.n_prims;
    a->has_pieces = sc->has_pieces ? 1u : 0u;
    a->color0 = sc->d_color0;
    a->sh = sc->d_sh;
    a->mroot = kNoRoot;
    if (mesh) { // the mesh side, as the per-lane aux launch has it (grt_frame.hip: fill_common)
        a->mnodes = sc->mbvh.nodes;
        a->tri = sc->d_tri;
        a->mroot = sc->n_faces ? sc->mbvh.root_ref : kNoRoot;
        a->n_faces = sc->n_faces;
        a->faces = sc->d_faces;
        a->vnormals = sc->d_vnormals;
    }
    a->swizzle_chunk = (uint32_t)c->opt_swizzle;
    a->err_word = c->d_err;
    return GRT_OK;
}

int check_step_range(grt_ctx* c, uint32_t step_first, uint32_t step_last, const char* fn)
{
    if (step_last == 0u || step_first <= step_last) return GRT_OK;
    c->err = std::string(fn) + ": step_first > step_last (iterations are counted from 1; step_last = 0 leaves the range open)";
    return GRT_ERR_INVALID;
}

int lane_launch(grt_ctx* c, const RenderArgs& a, const void* kernel, void** args, hipStream_t s, const char* fn)
{
    const grt_ctx* sc = scene_of(c);
    // one LDS stack per lane, for the Gaussian tree and, in a frame with meshes, for the mesh tree in turn
    // (no particle or an empty tree: depth 1; the kernels' guard makes every ray untraced and the stack is not touched)
    const uint32_t depth = std::max(std::max(sc->gbvh.height, a.n_faces ? sc->mbvh.height : 0u), 1u);
    const size_t lds = (size_t)kBlock * sizeof(uint32_t) * depth;
    if (lds > 160 * 1024) { c->err = std::string(fn) + ": BVH height " + std::to_string(depth) + " needs more than 160 KiB of LDS stack"; return GRT_ERR_LIMIT; }
    CHK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CHK(c, hipEventRecord(c->ev0, s));
    (void)hipLaunchKernel(kernel, dim3(a.n_blocks), dim3(kBlock), args, lds, s); // (a failed launch: hipGetLastError in lane_launch_done)
    return GRT_OK;
}

int lane_launch_done(grt_ctx* c, hipStream_t s)
{
    CHK(c, hipGetLastError());
    CHK(c, hipEventRecord(c->ev1, s));
    c->have_timing = true;
    return GRT_OK;
}

int bwd_launch(grt_ctx* c, const grt_params* p, const RenderArgs& a, const float* d_grad_rgbf, const float* d_grad_alpha,
               const grt_gaussian_grads* g, const BwdUnit& u, void* stream, const char* fn)
{
    const grt_ctx* sc = scene_of(c);
    const uint64_t n = sc->n;
    const bool want_geom = g && (g->pos || g->scale || g->quat || g->opacity);
    const bool want_sh = g && g->sh;
    const bool gauss = (want_geom || want_sh) && n != 0 && sc->gbvh.root_ref != kNoRoot;
    // no ray, or nothing to differentiate (a unit with work of its own still runs on an empty scene or an empty tree: the rays-only kernel writes the zeros)
    if (a.n_blocks == 0 || (!gauss && !u.own_work)) { c->have_timing = false; return GRT_OK; }
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const bool hi = gauss && p->sh_degree_max > 0 && want_sh;
    if (gauss) {
        int rc = bwd_buffers(c, n, hi, s);
        if (rc != GRT_OK) return rc;
    }
    BwdArgs b;
    b.pos = sc->d_pos; b.scale = sc->d_scale; b.quat = sc->d_quat; b.opacity = sc->d_opacity;
    b.g_rgb = d_grad_rgbf; b.g_alpha = d_grad_alpha;
    b.acc = gauss ? c->d_gacc : nullptr; b.acc_sh = hi ? c->d_gacc_sh : nullptr;
    b.want_geom = (want_geom || u.own_work) ? 1u : 0u; // (own work: the rays need m = A^T g_p of every event)
    b.want_sh = (gauss && want_sh) ? 1u : 0u;
    void* args[3] = {const_cast<RenderArgs*>(&a), &b, u.arg}; // (a kernel without an argument of its unit's takes the first two)
    int rc = lane_launch(c, a, u.kernels[!gauss ? 0 : (c->opt_bwd_plain ? 1 : 2)], args, s, fn);
    if (rc != GRT_OK) return rc;
    return gauss ? bwd_flush(c, n, hi, g, s) : lane_launch_done(c, s);
}

} // namespace grt

static int launch(grt_ctx* c, const grt_params* p, const RenderArgs& a, const float* d_rgbf, const float* d_alpha, const float* d_grad_rgbf,
                  const float* d_grad_alpha, const grt_gaussian_grads* g, void* stream, const char* fn)
{
    if (!d_rgbf || !d_alpha || !d_grad_rgbf || !g) { c->err = std::string(fn) + ": null pointer (d_rgbf, d_alpha, d_grad_rgbf and the grads structure are required)"; return GRT_ERR_INVALID; }
    static const void* const kernels[3] = {nullptr, reinterpret_cast<const void*>(k_backward<false>), reinterpret_cast<const void*>(k_backward<true>)};
    return bwd_launch(c, p, a, d_grad_rgbf, d_grad_alpha, g, BwdUnit{kernels, nullptr, false}, stream, fn);
}

extern "C" {

int grt_backward(grt_ctx* c, const grt_params* p, const float* d_rgbf, const float* d_alpha, const float* d_grad_rgbf, const float* d_grad_alpha,
                 const grt_gaussian_grads* g, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_backward";
    RenderArgs a;
    int rc = bwd_fill_args(c, p, false, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, p, a, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, g, stream, fn);
}

int grt_backward_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_rgbf, const float* d_alpha,
                      const float* d_grad_rgbf, const float* d_grad_alpha, const grt_gaussian_grads* g, void* stream)
{
    const char* fn = "grt_backward_rays";
    RenderArgs a;
    int rc = bwd_fill_args(c, p, false, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    if (n == 0) { // (no ray: nothing to read either)
        if (!g) { c->err = "grt_backward_rays: null grads structure"; return GRT_ERR_INVALID; }
        c->have_timing = false;
        return GRT_OK;
    }
    return launch(c, p, a, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, g, stream, fn);
}

} // extern "C"
