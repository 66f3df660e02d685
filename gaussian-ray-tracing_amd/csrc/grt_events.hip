// grt_events.hip — per-ray event lists of a Gaussian-only frame, with gradients (include/grt.h: grt_ray_events_frame / _rays,
// grt_backward_events_frame / _rays): for every ray of a window or of a ray buffer the composited events first ..
// first + K - 1 as (original id, key distance, alpha) in slot-major arrays [K][N], the count of ALL its events and the transmittance
// in front of event `first`; and, given dloss/dalpha per listed event, the gradients with respect to pos, scale, quat and opacity.
//
// Both kernels are ONE sweep_events call (grt_bwd.h) as k_ray_picks is: lane_ray gives the ray, one ray per lane, an 8x8 tile per
// wave, and a per-lane counter n numbers the lane's events.
//   k_ray_events            the event n with first <= n < first + K goes to slot n - first by up to three plain vector stores; after
//                           the sweep the lane fills its slots behind the last listed event with none, 0, 0 and stores count and
//                           T_in.  No atomic, no wave operation, no buffer of the context.  A NULL output is a wave-uniform branch on
//                           a kernel argument.
//   k_backward_events<MERGE> a pre-scan of the lane's column of the upstream (K loads, coalesced across the lanes of a ray buffer)
//                           leaves a ray whose values are all 0 untraced; a listed event with g != 0 below the 0.99 clamp forms its
//                           11 geometry / opacity values with dLda = g (alpha_terms) and the whole wave calls scatter<MERGE> for every
//                           slot.  It launches through bwd_launch with EvUp behind (RenderArgs, BwdArgs): gradient buffer and flush.
// The sweep runs on behind the last listed slot: count needs it in the forward; in the backward it is cost.
#include <string>

#include "grt_bwd.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "the event kernels run gps_round (grt_kround.h): its per-lane stack stride is the launch block size");

struct EvOut {
    grt_ray_events e;
    uint64_t n; // N: elements of a slot plane (width * height, or the rays of the buffer)
};
struct EvUp {
    const float* g; // upstream [K][N]
    uint64_t n;     // N
    uint32_t first, max_events;
};

__global__ __launch_bounds__(kBlock) void k_ray_events(const RenderArgs a, const EvOut k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out);
    // the raygen loop's guard, as the backward has it (shaders/tracer.cu:59)
    live = live && (length3(d) > 0.1f) && (a.p.max_bounces > 0u) && (a.root_ref != kNoRoot);
    const uint32_t first = k.e.first, Kn = k.e.max_events;
    const size_t N = (size_t)k.n;
    uint32_t n = 0;    // this lane's composited events so far
    float T = 1.0f, T_in = 1.0f;

    if (__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        sweep_events(a, stk, o, d, mk_rayinv(o, d), a.p.t_max, live, T, [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t key) {
            if (ev) { // (a lane with an event is live, and a live lane owns element idx)
                if (n == first) T_in = Tb; // Tb: the transmittance before the event
                const uint32_t s = n - first; // (n < first wraps past K)
                if (s < Kn) {
                    const size_t at = (size_t)s * N + idx;
                    if (k.e.id) k.e.id[at] = id;
                    if (k.e.t) k.e.t[at] = key_t(key);
                    if (k.e.alpha) k.e.alpha[at] = hitAlpha;
                }
                n++;
            }
        });
    }
    if (has_out) { // every element of the window or of the buffer once per requested array
        if (n <= first) T_in = T; // no event `first`: the ray's final transmittance (1 for a ray that was not traced)
        for (uint32_t s = (n > first) ? ((n - first < Kn) ? n - first : Kn) : 0u; s < Kn; s++) { // behind the last listed event
            const size_t at = (size_t)s * N + idx;
            if (k.e.id) k.e.id[at] = GRT_PICK_NONE;
            if (k.e.t) k.e.t[at] = 0.0f;
            if (k.e.alpha) k.e.alpha[at] = 0.0f;
        }
        if (k.e.count) k.e.count[idx] = n;
        if (k.e.T_in) k.e.T_in[idx] = T_in;
    }
}

template <bool MERGE>
__global__ __launch_bounds__(kBlock) void k_backward_events(const RenderArgs a, const BwdArgs b, const EvUp u)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    const float* __restrict__ g = u.g;
    const uint32_t first = u.first, Kn = u.max_events;
    const size_t N = (size_t)u.n;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out);
    // the raygen loop's guard (shaders/tracer.cu:59): such a ray renders, and differentiates, to nothing
    live = live && (length3(d) > 0.1f) && (a.p.max_bounces > 0u) && (a.root_ref != kNoRoot);
    bool any = false;
    if (live) { // the lane's column of the upstream
        for (uint32_t s = 0; s < Kn; s++) any = any || (g[(size_t)s * N + idx] != 0.0f);
    }
    live = live && any; // a ray whose K upstream values are all exactly 0 is not traced
    if (!__builtin_amdgcn_ballot_w64(live)) return; // wave-uniform

    RayAcc ra;    // (dead: alpha_terms<false> does not touch it)
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);
    uint32_t n = 0; // this lane's composited events so far
    float T = 1.0f;
    // every lane of the wave in step: the scatter is wave-cooperative
    sweep_events(a, stk, o, d, mk_rayinv(o, d), a.p.t_max, live, T, [&](bool ev, uint32_t id, float, float hitAlpha, uint64_t) {
        bool geom = false;
        float v[kVals];
#pragma unroll
        for (int i = 0; i < kVals; i++) v[i] = 0.0f;
        if (ev) {
            const uint32_t s = n - first; // (n < first wraps past K)
            if (s < Kn && hitAlpha < 0.99f) { // (where the 0.99 clamp binds nothing goes into opacity or geometry)
                const float dLda = g[(size_t)s * N + idx];
                if (dLda != 0.0f) {
                    geom = true;
                    alpha_terms<false>(b, id, o, d, dLda, v, ra);
                }
            }
            n++;
        }
        scatter<MERGE>(b.acc, geom, id, v, geom, false, lane);
    });
}

} // namespace
} // namespace grt

using namespace grt;

// what the four entry points refuse before they look at their rays: the backward's refusals in the entry point's name, a scene with
// meshes, and a slot range that is empty or overflows
static int fill(grt_ctx* c, const grt_params* p, bool have_range, uint32_t first, uint32_t max_events, RenderArgs* a, const char* fn)
{
    int rc = bwd_fill_args(c, p, false, a, fn, "ray events are listed for Gaussian-only frames");
    if (rc != GRT_OK || !have_range) return rc;
    if (max_events == 0) { c->err = std::string(fn) + ": max_events must be >= 1"; return GRT_ERR_INVALID; }
    if (first > 0xFFFFFFFFu - max_events) {
        c->err = std::string(fn) + ": first + max_events overflows (" + std::to_string(first) + " + " + std::to_string(max_events) + ")";
        return GRT_ERR_INVALID;
    }
    return GRT_OK;
}

static bool wanted(const grt_ray_events* o) { return o && (o->id || o->t || o->alpha || o->count || o->T_in); }

// N: the elements of a slot plane
static uint64_t plane(const RenderArgs& a) { return a.mode == 2 ? a.n_rays : (uint64_t)a.p.width * a.p.height; }

static int launch_forward(grt_ctx* c, const RenderArgs& a, const grt_ray_events* out, void* stream, const char* fn)
{
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced and its elements "none")
    EvOut k;
    k.e = *out; k.n = plane(a);
    void* args[2] = {const_cast<RenderArgs*>(&a), &k};
    int rc = lane_launch(c, a, reinterpret_cast<const void*>(k_ray_events), args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

static int no_output(grt_ctx* c, const char* fn)
{
    c->err = std::string(fn) + ": no output (id, t, alpha, count and T_in are all NULL)";
    return GRT_ERR_INVALID;
}

// the backward's arguments, checked in the header's order
static int check_backward(grt_ctx* c, const float* d_grad_alpha, const grt_gaussian_grads* g, const char* fn)
{
    if (g && g->sh) { c->err = std::string(fn) + ": sh must be NULL (colour does not depend on the listed events' alpha)"; return GRT_ERR_INVALID; }
    if (!g || (!g->pos && !g->scale && !g->quat && !g->opacity)) {
        c->err = std::string(fn) + ": no output (pos, scale, quat and opacity are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (!d_grad_alpha) { c->err = std::string(fn) + ": null pointer (the upstream gradient is required)"; return GRT_ERR_INVALID; }
    return GRT_OK;
}

static int launch_backward(grt_ctx* c, const grt_params* p, const RenderArgs& a, const float* d_grad_alpha, uint32_t first, uint32_t max_events,
                           const grt_gaussian_grads* g, void* stream, const char* fn)
{
    EvUp u;
    u.g = d_grad_alpha; u.n = plane(a); u.first = first; u.max_events = max_events;
    // ([0]: a call without a geometry group is refused; no ray, no particle or an empty tree: bwd_launch writes nothing)
    static const void* const kernels[3] = {nullptr, reinterpret_cast<const void*>(k_backward_events<false>),
                                           reinterpret_cast<const void*>(k_backward_events<true>)};
    return bwd_launch(c, p, a, nullptr, nullptr, g, BwdUnit{kernels, &u, false}, stream, fn); // (no upstream on (rgbf, alpha): BwdArgs' stay null)
}

extern "C" {

int grt_ray_events_frame(grt_ctx* c, const grt_params* p, const grt_ray_events* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_ray_events_frame";
    RenderArgs a;
    int rc = fill(c, p, wanted(out), out ? out->first : 0u, out ? out->max_events : 0u, &a, fn);
    if (rc == GRT_OK && !wanted(out)) rc = no_output(c, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, out, stream, fn);
}

int grt_ray_events_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const grt_ray_events* out, void* stream)
{
    const char* fn = "grt_ray_events_rays";
    RenderArgs a;
    int rc = fill(c, p, wanted(out), out ? out->first : 0u, out ? out->max_events : 0u, &a, fn);
    if (rc == GRT_OK && !wanted(out)) rc = no_output(c, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, out, stream, fn);
}

int grt_backward_events_frame(grt_ctx* c, const grt_params* p, const float* d_grad_alpha, uint32_t first, uint32_t max_events,
                              const grt_gaussian_grads* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_backward_events_frame";
    RenderArgs a;
    int rc = fill(c, p, true, first, max_events, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, d_grad_alpha, out, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, d_grad_alpha, first, max_events, out, stream, fn);
}

int grt_backward_events_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_grad_alpha, uint32_t first,
                             uint32_t max_events, const grt_gaussian_grads* out, void* stream)
{
    const char* fn = "grt_backward_events_rays";
    RenderArgs a;
    int rc = fill(c, p, true, first, max_events, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, d_grad_alpha, out, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, d_grad_alpha, first, max_events, out, stream, fn);
}

} // extern "C"
