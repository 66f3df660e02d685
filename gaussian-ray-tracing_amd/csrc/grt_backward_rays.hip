// grt_backward_rays.hip — the backward pass with gradients with respect to the rays (include/grt.h: grt_backward_ex /
// grt_backward_rays_ex): k_backward_rays<MERGE, GAUSS>, the body of k_backward (grt_bwd.h) with the per-ray output.
//   GAUSS = true   the Gaussians' gradients as grt_backward scatters them, plus six accumulators per lane;
//   GAUSS = false  the rays' gradients alone: no scatter, no atomic, no gradient buffer, no flush.
// A ray's gradient belongs to one lane, is summed in the ray's own event order and written once with plain stores: the same bits
// from call to call and from either instantiation.
#include <string>

#include "grt_bwd.h"

namespace grt {
namespace {

template <bool MERGE, bool GAUSS>
__global__ __launch_bounds__(kBlock) void k_backward_rays(const RenderArgs a, const BwdArgs b, const RayOut ro)
{
    backward_body<MERGE, GAUSS, true>(a, b, ro);
}

} // namespace
} // namespace grt

using namespace grt;

static int launch(grt_ctx* c, const grt_params* p, const RenderArgs& a, const float* d_rgbf, const float* d_alpha, const float* d_grad_rgbf,
                  const float* d_grad_alpha, const grt_backward_out* out, void* stream, const char* fn)
{
    if (!d_rgbf || !d_alpha || !d_grad_rgbf) { c->err = std::string(fn) + ": null pointer (d_rgbf, d_alpha and d_grad_rgbf are required)"; return GRT_ERR_INVALID; }
    static const void* const kernels[3] = {reinterpret_cast<const void*>(k_backward_rays<false, false>), reinterpret_cast<const void*>(k_backward_rays<false, true>),
                                           reinterpret_cast<const void*>(k_backward_rays<true, true>)};
    const grt_gaussian_grads* g = out->gaussians;
    RayOut ro;
    ro.rays = out->rays;
    ro.scatter_geom = (g && (g->pos || g->scale || g->quat || g->opacity)) ? 1u : 0u; // (read by the GAUSS = true kernels alone)
    return bwd_launch(c, p, a, d_grad_rgbf, d_grad_alpha, g, BwdUnit{kernels, &ro, true}, stream, fn);
}

extern "C" {

int grt_backward_ex(grt_ctx* c, const grt_params* p, const float* d_rgbf, const float* d_alpha, const float* d_grad_rgbf, const float* d_grad_alpha,
                    const grt_backward_out* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_backward_ex";
    if (!c) return GRT_ERR_INVALID;
    if (!out || (!out->gaussians && !out->rays)) { c->err = std::string(fn) + ": no output (gaussians and rays are both NULL)"; return GRT_ERR_INVALID; }
    if (!out->rays) return grt_backward(c, p, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, out->gaussians, x0, y0, x1, y1, stream);
    RenderArgs a;
    int rc = bwd_fill_args(c, p, false, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, p, a, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, out, stream, fn);
}

int grt_backward_rays_ex(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_rgbf, const float* d_alpha,
                         const float* d_grad_rgbf, const float* d_grad_alpha, const grt_backward_out* out, void* stream)
{
    const char* fn = "grt_backward_rays_ex";
    if (!c) return GRT_ERR_INVALID;
    if (!out || (!out->gaussians && !out->rays)) { c->err = std::string(fn) + ": no output (gaussians and rays are both NULL)"; return GRT_ERR_INVALID; }
    if (!out->rays) return grt_backward_rays(c, p, d_rays, n, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, out->gaussians, stream);
    RenderArgs a;
    int rc = bwd_fill_args(c, p, false, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, p, a, d_rgbf, d_alpha, d_grad_rgbf, d_grad_alpha, out, stream, fn);
}

} // extern "C"
