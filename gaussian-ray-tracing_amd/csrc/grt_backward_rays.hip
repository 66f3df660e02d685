// grt_backward_rays.hip — the backward pass with gradients with respect to the rays (include/grt.h: grt_backward_ex /
// grt_backward_rays_ex) as a translation unit of its own: the same source as grt_backward.hip — its two sweeps,
// event_terms and scatter — with the kernel named k_backward_rays<MERGE, GAUSS> and a third argument for the per-ray output.
//   GAUSS = true   the Gaussians' gradients as grt_backward scatters them, plus six accumulators per lane;
//   GAUSS = false  the rays' gradients alone: no scatter, no atomic, no gradient buffer, no flush.
// A ray's gradient belongs to one lane, is summed in the ray's own event order and written once with plain stores: the same bits
// from call to call and from either instantiation.
#define GRT_BWD_RAYS_TU 1
#include "grt_backward.hip"

// a: mode, window / rays and n_blocks set by the caller
static int backward_ex_launch(grt_ctx* c, const grt_params* p, RenderArgs& a, const float* d_rgbf, const float* d_alpha, const float* d_grad_rgbf,
                              const float* d_grad_alpha, const grt_gaussian_grads* g, float* d_ray_grads, void* stream, const char* fn)
{
    const grt_ctx* sc = c->parent ? c->parent : c;
    if (!d_rgbf || !d_alpha || !d_grad_rgbf) { c->err = std::string(fn) + ": null pointer (d_rgbf, d_alpha and d_grad_rgbf are required)"; return GRT_ERR_INVALID; }
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    const uint64_t n = sc->n;
    const bool want_geom = g && (g->pos || g->scale || g->quat || g->opacity);
    const bool want_sh = g && g->sh;
    // (an empty scene or an empty tree: the rays-only kernel writes the zeros)
    const bool gauss = (want_geom || want_sh) && n != 0 && sc->gbvh.root_ref != kNoRoot;
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const bool hi = gauss && p->sh_degree_max > 0 && want_sh;
    if (gauss) {
        int rc = bwd_buffers(c, n, hi, s);
        if (rc != GRT_OK) return rc;
    }
    const uint32_t depth = std::max(sc->gbvh.height, 1u);
    const size_t lds = (size_t)kBlock * sizeof(uint32_t) * depth;
    if (lds > 160 * 1024) { c->err = std::string(fn) + ": BVH height " + std::to_string(depth) + " needs more than 160 KiB of LDS stack"; return GRT_ERR_LIMIT; }
    BwdArgs b;
    b.pos = sc->d_pos; b.scale = sc->d_scale; b.quat = sc->d_quat; b.opacity = sc->d_opacity;
    b.g_rgb = d_grad_rgbf; b.g_alpha = d_grad_alpha;
    b.acc = gauss ? c->d_gacc : nullptr; b.acc_sh = hi ? c->d_gacc_sh : nullptr;
    b.want_geom = 1u; // the rays need m = A^T g_p of every event
    b.want_sh = (gauss && want_sh) ? 1u : 0u;
    RayOut ro;
    ro.rays = d_ray_grads;
    ro.scatter_geom = (gauss && want_geom) ? 1u : 0u;
    auto fnk = !gauss ? k_backward_rays<false, false> : (c->opt_bwd_plain ? k_backward_rays<false, true> : k_backward_rays<true, true>);
    CHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(fnk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CHK(c, hipEventRecord(c->ev0, s));
    hipLaunchKernelGGL(fnk, dim3(a.n_blocks), dim3(kBlock), lds, s, a, b, ro);
    if (gauss) return bwd_flush(c, n, hi, g, s);
    CHK(c, hipGetLastError());
    CHK(c, hipEventRecord(c->ev1, s));
    c->have_timing = true;
    return GRT_OK;
}

extern "C" {

int grt_backward_ex(grt_ctx* c, const grt_params* p, const float* d_rgbf, const float* d_alpha, const float* d_grad_rgbf, const float* d_grad_alpha,
                    const grt_backward_out* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    if (!c) return GRT_ERR_INVALID;
    if (!out || (!out->gaussians && !out->rays)) { c->err = "grt_backward_ex: no output (gaussians and rays are both NULL)"; return GRT_ERR_INVALID; }
    if (!out->rays) return grt_backward(c, p, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, out->gaussians, x0, y0, x1, y1, stream);
    RenderArgs a;
    int rc = backward_common(c, p, &a, "grt_backward_ex");
    if (rc != GRT_OK) return rc;
    if (x1 > p->width || y1 > p->height || x0 > x1 || y0 > y1) { c->err = "grt_backward_ex: window outside the frame"; return GRT_ERR_INVALID; }
    a.mode = 0;
    a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1;
    a.nbx = (x1 - x0 + 15) / 16;
    a.nby = (y1 - y0 + 15) / 16;
    a.n_blocks = a.nbx * a.nby;
    return backward_ex_launch(c, p, a, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, out->gaussians, out->rays, stream, "grt_backward_ex");
}

int grt_backward_rays_ex(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_rgbf, const float* d_alpha,
                         const float* d_grad_rgbf, const float* d_grad_alpha, const grt_backward_out* out, void* stream)
{
    if (!c) return GRT_ERR_INVALID;
    if (!out || (!out->gaussians && !out->rays)) { c->err = "grt_backward_rays_ex: no output (gaussians and rays are both NULL)"; return GRT_ERR_INVALID; }
    if (!out->rays) return grt_backward_rays(c, p, d_rays, n, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, out->gaussians, stream);
    RenderArgs a;
    int rc = backward_common(c, p, &a, "grt_backward_rays_ex");
    if (rc != GRT_OK) return rc;
    if (n && !d_rays) { c->err = "grt_backward_rays_ex: null ray buffer"; return GRT_ERR_INVALID; }
    if (n > 0xFFFFFFFFull * 64) { c->err = "grt_backward_rays_ex: too many rays"; return GRT_ERR_LIMIT; }
    a.mode = 2;
    a.rays = d_rays; a.n_rays = n;
    a.n_blocks = (uint32_t)((n + 255) / 256);
    return backward_ex_launch(c, p, a, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, out->gaussians, out->rays, stream, "grt_backward_rays_ex");
}

} // extern "C"
