// grt_depth.hip — differentiable ray depth of a Gaussian-only scene (include/grt.h: grt_ray_depth_frame / _rays,
// grt_backward_depth_frame / _rays): over the events i that trace() composites on a whole ray (t_min, t_max, T = 1)
//     dist = sum_i w_i tau_i,   dist2 = sum_i w_i tau_i^2,   T_out = prod_i (1 - alpha_i),   count        w_i = T_i alpha_i
// with tau_i the event's key distance (GRT_DEPTH_KEY: grt_aux_out::depth) or the distance of the particle's maximum response
// d_val,i = -(o_g.d_g) / max(1e-6, d_g.d_g) (GRT_DEPTH_PEAK: computeResponse's own d_val, smooth in the ray and in the particle); and,
// given dloss/ddist, dloss/ddist2 and dloss/dT_out, the gradients with respect to pos, scale, quat, opacity and to the rays.
//
// One ray per lane, an 8x8 tile per wave (lane_ray).
//   k_ray_depth<PEAK>          ONE sweep_events call (grt_bwd.h); dist and dist2 are accumulated in on_slot as the aux depth is
//                              ((T alpha) tau, and ((T alpha) tau) tau, before T is updated), plain vector stores behind the sweep.  No
//                              atomic, no wave operation, no buffer of the context.  PEAK re-derives d_val per event from the library's
//                              attribute copies, with A formed as alpha_terms forms it.
//   k_backward_depth<MERGE, GAUSS, RAYS, PEAK>
//                              the two sweeps of k_backward_segments — sweep 0: F = sum_i w_i f_i (f_i = g_D tau_i + g_D2 tau_i^2) and
//                              T_out; sweep 1: every composited event's terms,
//                                  dloss/dalpha_i = T_i f_i - (S_i + g_T T_out) / (1 - alpha_i),  S_i = F - sum_{j<=i} w_j f_j
//                              through alpha_terms (zero where the 0.99 clamp binds), and under PEAK dloss/dtau_i = w_i (g_D + 2 g_D2
//                              tau_i) down to pos, scale, quat and the ray (tau_terms, grt_depth.h; NOT gated by the clamp).  Both fill the 11
//                              geometry slots of v[kVals]: scatter<MERGE> as it is.  RAYS: the ray's six floats are summed in its own
//                              event order and stored once.  It launches through bwd_launch with DepthBwd behind (RenderArgs, BwdArgs).
// grt_bwd.h is untouched, so no other unit's code moves.
#include <string>

#include "grt_bwd.h"
#include "grt_depth.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "the depth kernels run gps_round (grt_kround.h): its per-lane stack stride is the launch block size");

struct DepthFwd {
    const float* pos;   // [n][3] by original id (the uploaded attributes; read under PEAK alone)
    const float* scale; // [n][3]
    const float* quat;  // [n][4]
    grt_depth_out o;
};
struct DepthBwd {
    const float* g_dist;  // [N] or null: 0
    const float* g_dist2; // [N] or null: 0
    const float* g_T;     // [N] or null: 0
    float* rays;          // [N][6], written (RAYS)
};

template <bool PEAK>
__global__ __launch_bounds__(kBlock) void k_ray_depth(const RenderArgs a, const DepthFwd k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out);
    // the events are trace()'s on the whole ray: max_bounces is not looked at
    live = live && (length3(d) > 0.1f) && (a.root_ref != kNoRoot);
    float dist = 0.0f, dist2 = 0.0f, T = 1.0f;
    uint32_t n = 0;

    if (__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        sweep_events(a, stk, o, d, mk_rayinv(o, d), a.p.t_max, live, T, [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t key) {
            if (ev) { // Tb: the transmittance before the event
                float tau = key_t(key);
                if (PEAK) {
                    PeakFrame f;
                    tau = peak_tau(k.pos, k.scale, k.quat, id, o, d, f);
                }
                const float wt = (Tb * hitAlpha) * tau;
                dist += wt;
                dist2 += wt * tau;
                n++;
            }
        });
    }
    if (has_out) { // every element of the window or of the buffer once per requested array
        if (k.o.dist) k.o.dist[idx] = dist;
        if (k.o.dist2) k.o.dist2[idx] = dist2;
        if (k.o.T_out) k.o.T_out[idx] = T;
        if (k.o.count) k.o.count[idx] = n;
    }
}

template <bool MERGE, bool GAUSS, bool RAYS, bool PEAK>
__global__ __launch_bounds__(kBlock) void k_backward_depth(const RenderArgs a, const BwdArgs b, const DepthBwd k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out; // RAYS: this lane's six floats are written whatever becomes of the wave
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out);
    live = live && (length3(d) > 0.1f) && (a.root_ref != kNoRoot);
    float gD = 0.0f, gD2 = 0.0f, gT = 0.0f;
    if (live) { // a ray whose three upstream values are exactly 0 is not traced
        if (k.g_dist) gD = k.g_dist[idx];
        if (k.g_dist2) gD2 = k.g_dist2[idx];
        if (k.g_T) gT = k.g_T[idx];
        live = (gD != 0.0f) || (gD2 != 0.0f) || (gT != 0.0f);
    }
    RayAcc ra;
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);
    if (!__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        if constexpr (RAYS) {
            if (has_out) {
#pragma unroll
                for (int i = 0; i < 6; i++) k.rays[idx * 6 + i] = 0.0f;
            }
        }
        return;
    }

    const rayinv ri = mk_rayinv(o, d);
    // two sweeps over the same events — sweep 0: F = sum w f and T_out (the forward's events in the forward's order); sweep 1: every
    // composited event's terms with S_i = F - C_<=i.  Every lane of the wave in step: the scatter of sweep 1 is wave-cooperative.
    float F = 0.0f, Tend = 1.0f;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        float T = 1.0f, C = 0.0f;
        sweep_events(a, stk, o, d, ri, a.p.t_max, live, T, [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t key) {
            bool geom = false;
            float v[kVals];
#pragma unroll
            for (int i = 0; i < kVals; i++) v[i] = 0.0f;
            if (ev) {
                PeakFrame f;
                float tau = key_t(key);
                if (PEAK) tau = peak_tau(b.pos, b.scale, b.quat, id, o, d, f);
                const float w = Tb * hitAlpha;
                const float fi = gD * tau + (gD2 * tau) * tau;
                C += w * fi;
                if (pass == 0) {
                    F = C;
                } else if (b.want_geom) {
                    if (hitAlpha < 0.99f) { // (where the 0.99 clamp binds nothing goes into opacity or geometry THROUGH ALPHA)
                        const float dLda = Tb * fi - ((F - C) + gT * Tend) * (1.0f / (1.0f - hitAlpha));
                        alpha_terms<RAYS>(b, id, o, d, dLda, v, ra);
                        geom = true;
                    }
                    if (PEAK) { // tau does not pass through the clamp
                        tau_terms<RAYS>(b, id, d, f, tau, w * (gD + (2.0f * gD2) * tau), v, ra);
                        geom = true;
                    }
                }
            }
            if (GAUSS && pass) scatter<MERGE>(b.acc, ev, id, v, geom, false, lane);
        });
        if (pass == 0) Tend = T;
    }
    if constexpr (RAYS) {
        if (has_out) { // dloss/do = -sum m + sum gtau dtau/do; dloss/dd = -sum d_val m + sum gtau dtau/dd   (a lane that was not live holds zeros)
            float* r = k.rays + idx * 6;
            r[0] = 0.0f - ra.go.x; r[1] = 0.0f - ra.go.y; r[2] = 0.0f - ra.go.z;
            r[3] = 0.0f - ra.gd.x; r[4] = 0.0f - ra.gd.y; r[5] = 0.0f - ra.gd.z;
        }
    }
}

} // namespace
} // namespace grt

using namespace grt;

// what the four entry points refuse before they look at their rays: the backward's refusals in the entry point's name, a scene with meshes
// and an unknown kind
static int fill(grt_ctx* c, const grt_params* p, int kind, RenderArgs* a, const char* fn)
{
    int rc = bwd_fill_args(c, p, false, a, fn, "the ray depth is the Gaussian-only call: compose mesh paths from grt_trace_segments");
    if (rc == GRT_OK && kind != GRT_DEPTH_KEY && kind != GRT_DEPTH_PEAK) {
        c->err = std::string(fn) + ": unknown kind " + std::to_string(kind) + " (GRT_DEPTH_KEY = 0, GRT_DEPTH_PEAK = 1)";
        return GRT_ERR_INVALID;
    }
    return rc;
}

static int check_forward(grt_ctx* c, const grt_depth_out* o, const char* fn)
{
    if (o && (o->dist || o->dist2 || o->T_out || o->count)) return GRT_OK;
    c->err = std::string(fn) + ": no output (dist, dist2, T_out and count are all NULL)";
    return GRT_ERR_INVALID;
}

static bool geom_wanted(const grt_gaussian_grads* g) { return g && (g->pos || g->scale || g->quat || g->opacity); }

// the backward's arguments, checked in the header's order
static int check_backward(grt_ctx* c, const grt_depth_upstream* up, const grt_backward_out* out, const char* fn)
{
    if (!up || (!up->dist && !up->dist2 && !up->T_out)) {
        c->err = std::string(fn) + ": no upstream (dist, dist2 and T_out are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (!out || (!geom_wanted(out->gaussians) && !out->rays)) {
        c->err = std::string(fn) + ": no output (pos, scale, quat and opacity of gaussians and rays are all NULL; sh is not a depth gradient)";
        return GRT_ERR_INVALID;
    }
    return GRT_OK;
}

static int launch_forward(grt_ctx* c, const RenderArgs& a, int kind, const grt_depth_out* out, void* stream, const char* fn)
{
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced)
    const grt_ctx* sc = scene_of(c);
    DepthFwd k;
    k.pos = sc->d_pos; k.scale = sc->d_scale; k.quat = sc->d_quat;
    k.o = *out;
    void* args[2] = {const_cast<RenderArgs*>(&a), &k};
    const void* kernel = kind == GRT_DEPTH_PEAK ? reinterpret_cast<const void*>(k_ray_depth<true>) : reinterpret_cast<const void*>(k_ray_depth<false>);
    int rc = lane_launch(c, a, kernel, args, st, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, st);
}

template <bool PEAK>
static const void* const* backward_kernels(bool rays)
{
    // ([0]: the rays alone — no scatter, no atomic, no gradient buffer; without a rays output a call has a gradient group, or was refused)
    static const void* const with_rays[3] = {reinterpret_cast<const void*>(k_backward_depth<false, false, true, PEAK>),
                                             reinterpret_cast<const void*>(k_backward_depth<false, true, true, PEAK>),
                                             reinterpret_cast<const void*>(k_backward_depth<true, true, true, PEAK>)};
    // ([0] null: a call that launches from this table must hand bwd_launch own_work = false, or an empty scene launches a null kernel)
    static const void* const gauss_only[3] = {nullptr, reinterpret_cast<const void*>(k_backward_depth<false, true, false, PEAK>),
                                              reinterpret_cast<const void*>(k_backward_depth<true, true, false, PEAK>)};
    return rays ? with_rays : gauss_only;
}

static int launch_backward(grt_ctx* c, const grt_params* p, const RenderArgs& a, int kind, const grt_depth_upstream* up,
                           const grt_backward_out* out, void* stream, const char* fn)
{
    DepthBwd k;
    k.g_dist = up->dist; k.g_dist2 = up->dist2; k.g_T = up->T_out;
    k.rays = out->rays;
    grt_gaussian_grads g; // (sh is left untouched and is no request: bwd_launch sees it NULL)
    const bool gauss = geom_wanted(out->gaussians);
    if (gauss) { g = *out->gaussians; g.sh = nullptr; }
    const bool rays = out->rays != nullptr;
    const void* const* kernels = kind == GRT_DEPTH_PEAK ? backward_kernels<true>(rays) : backward_kernels<false>(rays);
    // (BwdArgs::g_rgb / g_alpha stay NULL: the upstreams are DepthBwd's.  own_work: the rays' gradients, written on an empty scene too)
    return bwd_launch(c, p, a, nullptr, nullptr, gauss ? &g : nullptr, BwdUnit{kernels, &k, rays}, stream, fn);
}

extern "C" {

int grt_ray_depth_frame(grt_ctx* c, const grt_params* p, int kind, const grt_depth_out* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                        void* stream)
{
    const char* fn = "grt_ray_depth_frame";
    RenderArgs a;
    int rc = fill(c, p, kind, &a, fn);
    if (rc == GRT_OK) rc = check_forward(c, out, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, kind, out, stream, fn);
}

int grt_ray_depth_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, int kind, const grt_depth_out* out, void* stream)
{
    const char* fn = "grt_ray_depth_rays";
    RenderArgs a;
    int rc = fill(c, p, kind, &a, fn);
    if (rc == GRT_OK) rc = check_forward(c, out, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, kind, out, stream, fn);
}

int grt_backward_depth_frame(grt_ctx* c, const grt_params* p, int kind, const grt_depth_upstream* up, const grt_backward_out* out, uint32_t x0,
                             uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_backward_depth_frame";
    RenderArgs a;
    int rc = fill(c, p, kind, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, up, out, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, kind, up, out, stream, fn);
}

int grt_backward_depth_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, int kind, const grt_depth_upstream* up,
                            const grt_backward_out* out, void* stream)
{
    const char* fn = "grt_backward_depth_rays";
    RenderArgs a;
    int rc = fill(c, p, kind, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, up, out, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, kind, up, out, stream, fn);
}

} // extern "C"
