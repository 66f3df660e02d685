// grt_features.hip — per-particle feature channels composited through the Gaussians, with gradients (include/grt.h:
// grt_render_features_frame / _rays, grt_backward_features_frame / _rays): F[ray][c] = sum_i T_i alpha_i feat[id_i][c]
// over the composited events of a Gaussian-only frame, and the gradients of sum g.F with respect to feat and to the Gaussians.
//
// Both kernels stand on grt_bwd.h as grt_stats.hip does: lane_ray gives the ray, one ray per lane, an 8x8 tile per wave, the events
// from sweep_events, every lane of the wave in step.  The channel count C is a runtime argument; the channel loops run to the
// compile-time CP in {4, 8, 16} under the guard c < C, so that a lane's C accumulators (forward) or C upstream values (backward)
// are registers.
//   k_render_features<CP>            ONE sweep: F_c = F_c + w f_c per event, plain stores at the end, no atomic.
//   k_backward_features<MERGE, CP, GEOM>
//     GEOM = true   two sweeps as backward_body: sweep 0 forms Phi = sum_i w_i phi_i with phi_i = sum_c g_c feat[id_i][c]; sweep 1
//                   walks the same events, forms P_i and hands event_terms<true, false> the one-channel radiance L = (phi_i, 0, 0),
//                   S = (Phi - P_i, 0, 0), g_rad = (1, 0, 0), gAp = 0: its dLda is T_i phi_i - (Phi - P_i) / (1 - alpha_i), its 11
//                   geometry / opacity values go through scatter<MERGE> into the slot's gradient buffer, and grt_backward.hip's
//                   flush adds them into the caller's arrays.
//     GEOM = false  pos, scale, quat and opacity are all NULL: sweep 1 alone, no phi, no event_terms, no gradient buffer, no flush.
//     The C feature gradients w_i g_c go straight into the caller's [n][C] array by float atomics, merged per group of lanes that hold
//     the same particle (wave_groups, as scatter: wave_sum per channel, lane c adds channel c); a lane alone with its particle adds its own.
// The backward launches through bwd_launch (grt_internal.h) with its own FeatArgs behind (RenderArgs, BwdArgs); of BwdArgs the kernel
// reads what event_terms and scatter read.  A feature gradient with no geometry group is the unit's own work: kernels[0], GEOM = false.
#include <string>

#include "grt_bwd.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "the feature kernels run gps_round (grt_kround.h): its per-lane stack stride is the launch block size");
static_assert(GRT_MAX_FEATURE_CHANNELS == 16, "the instantiations below are CP = 4, 8, 16");

struct FeatOut {
    const float* feat; // [n][C] by original id
    float* out;        // [pixels or rays][C], written
    uint32_t channels;
};
struct FeatArgs {
    const float* up;   // upstream [pixels or rays][C]
    const float* feat; // [n][C] by original id
    float* gfeat;      // the feature gradient [n][C], added to, or null
    uint32_t channels;
};

template <int CP>
__global__ __launch_bounds__(kBlock) void k_render_features(const RenderArgs a, const FeatOut f)
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
    const uint32_t C = f.channels;
    float F[CP];
#pragma unroll
    for (int c = 0; c < CP; c++) F[c] = 0.0f;

    if (__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        float T = 1.0f;
        sweep_events(a, stk, o, d, mk_rayinv(o, d), a.p.t_max, live, T, [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t) {
            if (ev) {
                const float* fr = f.feat + (size_t)id * C;
                const float w = Tb * hitAlpha; // Tb: the transmittance before the event
#pragma unroll
                for (int c = 0; c < CP; c++) {
                    if ((uint32_t)c < C) F[c] = F[c] + w * fr[c];
                }
            }
        });
    }
    if (has_out) { // every element of the window or of the buffer once: zeros for a ray that was not traced
        float* r = f.out + idx * C;
#pragma unroll
        for (int c = 0; c < CP; c++) {
            if ((uint32_t)c < C) r[c] = F[c];
        }
    }
}

// one lane's C values w g_c to its particle's row of the feature gradient
template <int CP>
__device__ __forceinline__ void feat_add_own(float* __restrict__ gfeat, uint32_t C, uint32_t id, float w, const float g[CP])
{
    float* row = gfeat + (size_t)id * C;
#pragma unroll
    for (int c = 0; c < CP; c++) {
        if ((uint32_t)c < C) atomicAdd(row + c, w * g[c]);
    }
}

// Called by the WHOLE wave (ev: this lane has an event of particle id with weight w).  MERGE: lanes with the same particle add once.
template <bool MERGE, int CP>
__device__ __forceinline__ void feat_scatter(float* __restrict__ gfeat, uint32_t C, bool ev, uint32_t id, float w, const float g[CP], uint32_t lane)
{
    if (!MERGE) {
        if (ev) feat_add_own<CP>(gfeat, C, id, w, g);
        return;
    }
    const bool solo = wave_groups(ev, id, [&](uint32_t lid, bool mine, uint32_t, uint32_t) {
        float out = 0.0f;
#pragma unroll
        for (int c = 0; c < CP; c++) {
            if ((uint32_t)c < C) { // (wave-uniform: a kernel argument)
                const float s = wave_sum(mine ? w * g[c] : 0.0f);
                out = (lane == (uint32_t)c) ? s : out;
            }
        }
        if (lane < C && out != 0.0f) atomicAdd(gfeat + (size_t)lid * C + lane, out);
    });
    if (solo) feat_add_own<CP>(gfeat, C, id, w, g);
}

template <bool MERGE, int CP, bool GEOM>
__global__ __launch_bounds__(kBlock) void k_backward_features(const RenderArgs a, const BwdArgs b, const FeatArgs f)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    const float* __restrict__ up = f.up;
    const float* __restrict__ feat = f.feat;
    float* __restrict__ gfeat = f.gfeat;
    const uint32_t C = f.channels;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out);
    // the raygen loop's guard (shaders/tracer.cu:59): such a ray renders, and differentiates, to nothing
    live = live && (length3(d) > 0.1f) && (a.p.max_bounces > 0u) && (a.root_ref != kNoRoot);
    float g[CP];
    bool any = false;
#pragma unroll
    for (int c = 0; c < CP; c++) {
        g[c] = 0.0f;
        if (live && (uint32_t)c < C) {
            g[c] = up[idx * C + c];
            any = any || (g[c] != 0.0f);
        }
    }
    live = live && any; // a ray whose C upstream values are all exactly 0 is not traced
    if (!__builtin_amdgcn_ballot_w64(live)) return; // wave-uniform

    const rayinv ri = mk_rayinv(o, d);
    RayAcc ra;    // (dead: event_terms<., false> does not touch it)
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);

    // GEOM: two sweeps over the same events (sweep_events), as backward_body has them — sweep 0: Phi; sweep 1: every composited
    // event's terms.  Without GEOM sweep 1 alone.  Every lane of the wave in step: the scatters are wave-cooperative.
    float Phi = 0.0f;
#pragma unroll 1
    for (int pass = GEOM ? 0 : 1; pass < 2; pass++) {
        float T = 1.0f, P = 0.0f;
        sweep_events(a, stk, o, d, ri, a.p.t_max, live, T, [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t) {
            bool geom = false;
            float w = 0.0f;
            float v[kVals];
#pragma unroll
            for (int k = 0; k < kVals; k++) v[k] = 0.0f;
            if (ev) {
                w = Tb * hitAlpha; // Tb: the transmittance before the event
                if constexpr (GEOM) {
                    const float* fr = feat + (size_t)id * C;
                    float phi = 0.0f;
#pragma unroll
                    for (int c = 0; c < CP; c++) {
                        if ((uint32_t)c < C) phi = phi + g[c] * fr[c];
                    }
                    P = P + w * phi; // (sweep 0: this is Phi, term by term)
                    if (pass == 0) {
                        Phi = P;
                    } else {
                        geom = event_terms<true, false>(a, b, id, o, d, d, mk3(phi, 0, 0), Tb, hitAlpha, mk3(Phi - P, 0, 0), mk3(1, 0, 0), 0.0f,
                                                        0.0f, v, ra);
                    }
                }
            }
            if (pass) {
                if constexpr (GEOM) scatter<MERGE>(b.acc, ev, id, v, geom, false, lane);
                if (gfeat) feat_scatter<MERGE, CP>(gfeat, C, ev, id, w, g, lane); // (wave-uniform: a kernel argument)
            }
        });
    }
}

} // namespace
} // namespace grt

using namespace grt;

// what the four entry points refuse before they look at their rays: the backward's refusals in the entry point's name, a scene with
// meshes, and a channel count outside 1 .. GRT_MAX_FEATURE_CHANNELS
static int fill(grt_ctx* c, const grt_params* p, uint32_t channels, RenderArgs* a, const char* fn)
{
    int rc = bwd_fill_args(c, p, false, a, fn, "feature channels are rendered for Gaussian-only frames");
    if (rc != GRT_OK) return rc;
    if (channels == 0 || channels > GRT_MAX_FEATURE_CHANNELS) {
        c->err = std::string(fn) + ": channels must be 1.." + std::to_string(GRT_MAX_FEATURE_CHANNELS) + ", not " + std::to_string(channels);
        return GRT_ERR_INVALID;
    }
    return GRT_OK;
}

static int launch_forward(grt_ctx* c, const RenderArgs& a, const float* d_feat, uint32_t channels, float* d_out, void* stream, const char* fn)
{
    if (!d_feat || !d_out) { c->err = std::string(fn) + ": null pointer (the features and the output are required)"; return GRT_ERR_INVALID; }
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced and its element zero)
    FeatOut f;
    f.feat = d_feat; f.out = d_out; f.channels = channels;
    static const void* const kernels[3] = {reinterpret_cast<const void*>(k_render_features<4>), reinterpret_cast<const void*>(k_render_features<8>),
                                           reinterpret_cast<const void*>(k_render_features<16>)};
    const void* fnk = kernels[channels <= 4u ? 0 : (channels <= 8u ? 1 : 2)];
    void* args[2] = {const_cast<RenderArgs*>(&a), &f};
    int rc = lane_launch(c, a, fnk, args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

// bwd_launch's kernel table of one CP: [0] no geometry group (nothing goes through the gradient buffer), [1] plain atomics, [2] merged
template <int CP>
static void backward_kernels(bool plain, const void* k[3])
{
    k[0] = plain ? reinterpret_cast<const void*>(k_backward_features<false, CP, false>) : reinterpret_cast<const void*>(k_backward_features<true, CP, false>);
    k[1] = reinterpret_cast<const void*>(k_backward_features<false, CP, true>);
    k[2] = reinterpret_cast<const void*>(k_backward_features<true, CP, true>);
}

static int launch_backward(grt_ctx* c, const grt_params* p, const RenderArgs& a, const float* d_feat, uint32_t channels, const float* d_grad_out,
                           const grt_feature_grads* g, void* stream, const char* fn)
{
    if (!d_feat || !d_grad_out) { c->err = std::string(fn) + ": null pointer (the features and the upstream gradient are required)"; return GRT_ERR_INVALID; }
    if (!g || (!g->pos && !g->scale && !g->quat && !g->opacity && !g->feat)) {
        c->err = std::string(fn) + ": no output (pos, scale, quat, opacity and feat are all NULL)";
        return GRT_ERR_INVALID;
    }
    const grt_ctx* sc = scene_of(c);
    // no ray, no particle or an empty tree: nothing is composited, nothing is written
    if (a.n_blocks == 0 || sc->n == 0 || sc->gbvh.root_ref == kNoRoot) { c->have_timing = false; return GRT_OK; }
    FeatArgs f;
    f.up = d_grad_out; f.feat = d_feat; f.gfeat = g->feat; f.channels = channels;
    const grt_gaussian_grads gg = {g->pos, g->scale, g->quat, g->opacity, nullptr}; // (no SH group: the higher-SH buffer is never made)
    const bool plain = c->opt_bwd_plain != 0;
    const void* kernels[3];
    if (channels <= 4u) backward_kernels<4>(plain, kernels);
    else if (channels <= 8u) backward_kernels<8>(plain, kernels);
    else backward_kernels<16>(plain, kernels);
    return bwd_launch(c, p, a, nullptr, nullptr, &gg, BwdUnit{kernels, &f, g->feat != nullptr}, stream, fn); // (no upstream on (rgbf, alpha): BwdArgs' stay null)
}

extern "C" {

int grt_render_features_frame(grt_ctx* c, const grt_params* p, const float* d_feat, uint32_t channels, float* d_out, uint32_t x0, uint32_t y0,
                              uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_render_features_frame";
    RenderArgs a;
    int rc = fill(c, p, channels, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, d_feat, channels, d_out, stream, fn);
}

int grt_render_features_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_feat, uint32_t channels, float* d_out,
                             void* stream)
{
    const char* fn = "grt_render_features_rays";
    RenderArgs a;
    int rc = fill(c, p, channels, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, d_feat, channels, d_out, stream, fn);
}

int grt_backward_features_frame(grt_ctx* c, const grt_params* p, const float* d_feat, uint32_t channels, const float* d_grad_out,
                                const grt_feature_grads* grads, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_backward_features_frame";
    RenderArgs a;
    int rc = fill(c, p, channels, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, d_feat, channels, d_grad_out, grads, stream, fn);
}

int grt_backward_features_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_feat, uint32_t channels,
                               const float* d_grad_out, const grt_feature_grads* grads, void* stream)
{
    const char* fn = "grt_backward_features_rays";
    RenderArgs a;
    int rc = fill(c, p, channels, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, d_feat, channels, d_grad_out, grads, stream, fn);
}

} // extern "C"
