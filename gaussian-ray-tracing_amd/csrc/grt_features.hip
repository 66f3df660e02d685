// grt_features.hip — per-particle feature channels composited through the Gaussians, with gradients (include/grt.h:
// grt_render_features_frame / _rays, grt_backward_features_frame / _rays): F[ray][c] = sum_i T_i alpha_i feat[id_i][c]
// over the composited events of a Gaussian-only frame, and the gradients of sum g.F with respect to feat and to the Gaussians.
//
// Both kernels stand on grt_bwd.h as grt_stats.hip does: lane_ray gives the ray, one ray per lane, an 8x8 tile per wave, k = 7 rounds
// of gps_round (grt_kround.h) through a single call site, every lane of the wave in step.  The channel count C is a runtime argument;
// the channel loops run to the compile-time CP in {4, 8, 16} under the guard c < C, so that a lane's C accumulators (forward) or C
// upstream values (backward) are registers.
//   k_render_features<CP>            ONE sweep, k_particle_stats' loop: F_c = F_c + w f_c per event, plain stores at the end, no atomic.
//   k_backward_features<MERGE, CP, GEOM>
//     GEOM = true   two sweeps as backward_body: sweep 0 forms Phi = sum_i w_i phi_i with phi_i = sum_c g_c feat[id_i][c]; sweep 1
//                   walks the same events, forms P_i and hands event_terms<true, false> the one-channel radiance L = (phi_i, 0, 0),
//                   S = (Phi - P_i, 0, 0), g_rad = (1, 0, 0), gAp = 0: its dLda is T_i phi_i - (Phi - P_i) / (1 - alpha_i), its 11
//                   geometry / opacity values go through scatter<MERGE> into the slot's gradient buffer, and grt_backward.hip's
//                   flush adds them into the caller's arrays.
//     GEOM = false  pos, scale, quat and opacity are all NULL: sweep 1 alone, no phi, no event_terms, no gradient buffer, no flush.
//     The C feature gradients w_i g_c go straight into the caller's [n][C] array by float atomics, merged per group of lanes that hold
//     the same particle as scatter does (wave_sum per channel, lane c adds channel c); a lane alone with its particle adds its own.
// The backward launches through bwd_launch (grt_internal.h), whose kernels take (RenderArgs, BwdArgs, RayOut): the three pointers it
// fills carry this unit's arrays — BwdArgs::g_rgb the upstream [rays][C], BwdArgs::g_alpha the features [n][C], RayOut::rays the
// feature gradient [n][C] (or null) — and the channel count rides in RenderArgs::tile_w, a field of the tile mapping that a window
// or a ray buffer leaves unused.  A non-null RayOut::rays with no geometry group is bwd_launch's "nothing to scatter into the buffer"
// case: it runs kernels[0], the GEOM = false instantiation, and neither makes the buffer nor flushes.
#include <algorithm>
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
        const rayinv ri = mk_rayinv(o, d);
        const float epsT = 1e-9f;
        const float t_max = a.p.t_max;
        const float t_hi = t_max + epsT;
        const float minT = a.p.minTransmittance;
        KBuf<K> kb;
        grt::Cnt cnt; // (dead: no counters, no watchdog)

        // one sweep over the events trace() composites (shaders/tracer.cuh:328-373), k_particle_stats' loop
        float T = 1.0f, lastT = a.p.t_min;
        uint64_t last_key = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
        bool act = live && (lastT <= t_max) && (T > minT);
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                gps_round<false, false, K>(a, stk, o, d, ri, last_key, t_hi, kb, cnt, 0xFFFFFFFFu);
                if (kb.key[0] == kKeyInvalid) act = false;
            }
#pragma unroll 1
            for (int i = 0; i < K; i++) {
                uint64_t key = kKeyInvalid;
                float hitAlpha = 0.0f;
#pragma unroll
                for (int j = 0; j < K; j++) {
                    if (j == i) { key = kb.key[j]; hitAlpha = kb.alpha[j]; }
                }
                if (act && key != kKeyInvalid && T > minT) {
                    lastT = fmaxf(key_t(key), lastT);
                    if (a.p.alpha_min < hitAlpha) {
                        const float* fr = f.feat + (size_t)key_id(key) * C;
                        const float w = T * hitAlpha; // T: the transmittance before the event
#pragma unroll
                        for (int c = 0; c < CP; c++) {
                            if ((uint32_t)c < C) F[c] = F[c] + w * fr[c];
                        }
                        T *= (1.0f - hitAlpha);
                    }
                }
            }
            if (act) {
                if (kb.key[K - 1] == kKeyInvalid) act = false;
                else last_key = kb.key[K - 1];
                act = act && (lastT <= t_max) && (T > minT);
            }
        }
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
    uint64_t todo = __builtin_amdgcn_ballot_w64(ev);
    bool solo = false;
    while (todo) { // wave-uniform
        const int leader = __builtin_ctzll(todo);
        const uint32_t lid = (uint32_t)__builtin_amdgcn_readlane((int)id, leader);
        const bool mine = ev && id == lid;
        const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
        todo &= ~m;
        if (__builtin_popcountll(m) == 1) { // alone with its particle: its own adds, once the groups are done
            solo = solo || mine;
            continue;
        }
        float out = 0.0f;
#pragma unroll
        for (int c = 0; c < CP; c++) {
            if ((uint32_t)c < C) { // (wave-uniform: a kernel argument)
                const float s = wave_sum(mine ? w * g[c] : 0.0f);
                out = (lane == (uint32_t)c) ? s : out;
            }
        }
        if (lane < C && out != 0.0f) atomicAdd(gfeat + (size_t)lid * C + lane, out);
    }
    if (solo) feat_add_own<CP>(gfeat, C, id, w, g);
}

template <bool MERGE, int CP, bool GEOM>
__global__ __launch_bounds__(kBlock) void k_backward_features(const RenderArgs a, const BwdArgs b, const RayOut ro)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    const float* __restrict__ up = b.g_rgb;     // upstream [pixels or rays][C]
    const float* __restrict__ feat = b.g_alpha; // features [n][C]
    float* __restrict__ gfeat = ro.rays;        // feature gradient [n][C] or null
    const uint32_t C = a.tile_w;                // (see the head of this file)
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
    const float epsT = 1e-9f;
    const float t_max = a.p.t_max;
    const float t_hi = t_max + epsT;
    const float minT = a.p.minTransmittance;
    const uint64_t key0 = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
    KBuf<K> kb;
    grt::Cnt cnt; // (dead: no counters, no watchdog)
    RayAcc ra;    // (dead: event_terms<., false> does not touch it)
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);

    // GEOM: two sweeps over the same events through ONE call site of the traversal, as backward_body has them — sweep 0: Phi; sweep 1:
    // every composited event's terms.  Without GEOM sweep 1 alone.  Every lane of the wave in step: the scatters are wave-cooperative.
    float Phi = 0.0f;
#pragma unroll 1
    for (int pass = GEOM ? 0 : 1; pass < 2; pass++) {
        float T = 1.0f, lastT = a.p.t_min, P = 0.0f;
        uint64_t last_key = key0;
        bool act = live && (lastT <= t_max) && (T > minT);
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                gps_round<false, false, K>(a, stk, o, d, ri, last_key, t_hi, kb, cnt, 0xFFFFFFFFu);
                if (kb.key[0] == kKeyInvalid) act = false;
            }
#pragma unroll 1
            for (int i = 0; i < K; i++) {
                bool ev = false, geom = false;
                uint32_t id = 0;
                float w = 0.0f;
                float v[kVals];
#pragma unroll
                for (int k = 0; k < kVals; k++) v[k] = 0.0f;
                uint64_t key = kKeyInvalid;
                float hitAlpha = 0.0f;
#pragma unroll
                for (int j = 0; j < K; j++) {
                    if (j == i) { key = kb.key[j]; hitAlpha = kb.alpha[j]; }
                }
                if (act && key != kKeyInvalid && T > minT) {
                    lastT = fmaxf(key_t(key), lastT);
                    if (a.p.alpha_min < hitAlpha) {
                        id = key_id(key);
                        w = T * hitAlpha; // T: the transmittance before the event
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
                                ev = true;
                                geom = event_terms<true, false>(a, b, id, o, d, d, mk3(phi, 0, 0), T, hitAlpha, mk3(Phi - P, 0, 0), mk3(1, 0, 0), 0.0f,
                                                                0.0f, v, ra);
                            }
                        } else {
                            ev = true;
                        }
                        T *= (1.0f - hitAlpha);
                    }
                }
                if (pass) {
                    if constexpr (GEOM) scatter<MERGE>(b.acc, ev, id, v, geom, false, lane);
                    if (gfeat) feat_scatter<MERGE, CP>(gfeat, C, ev, id, w, g, lane); // (wave-uniform: a kernel argument)
                }
            }
            if (act) {
                if (kb.key[K - 1] == kKeyInvalid) act = false;
                else last_key = kb.key[K - 1];
                act = act && (lastT <= t_max) && (T > minT);
            }
        }
    }
}

} // namespace
} // namespace grt

using namespace grt;

// what the four entry points refuse before they look at their rays: the backward's refusals in the entry point's name, a scene with
// meshes, and a channel count outside 1 .. GRT_MAX_FEATURE_CHANNELS
static int fill(grt_ctx* c, const grt_params* p, uint32_t channels, RenderArgs* a, const char* fn)
{
    if (!c) return GRT_ERR_INVALID;
    const grt_ctx* sc = scene_of(c);
    if (p && sc->built && sc->n_faces) {
        c->err = std::string(fn) + ": meshes are set (feature channels are rendered for Gaussian-only frames)";
        return GRT_ERR_INVALID;
    }
    int rc = bwd_fill_args(c, p, false, a, fn);
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
    const grt_ctx* sc = scene_of(c);
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced and its element zero; the stack is not touched)
    const uint32_t depth = std::max(sc->gbvh.height, 1u);
    const size_t lds = (size_t)kBlock * sizeof(uint32_t) * depth; // one LDS stack per lane
    if (lds > 160 * 1024) { c->err = std::string(fn) + ": BVH height " + std::to_string(depth) + " needs more than 160 KiB of LDS stack"; return GRT_ERR_LIMIT; }
    FeatOut f;
    f.feat = d_feat; f.out = d_out; f.channels = channels;
    static const void* const kernels[3] = {reinterpret_cast<const void*>(k_render_features<4>), reinterpret_cast<const void*>(k_render_features<8>),
                                           reinterpret_cast<const void*>(k_render_features<16>)};
    const void* fnk = kernels[channels <= 4u ? 0 : (channels <= 8u ? 1 : 2)];
    CHK(c, hipFuncSetAttribute(fnk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CHK(c, hipEventRecord(c->ev0, s));
    void* args[2] = {const_cast<RenderArgs*>(&a), &f};
    (void)hipLaunchKernel(fnk, dim3(a.n_blocks), dim3(kBlock), args, lds, s);
    CHK(c, hipGetLastError());
    CHK(c, hipEventRecord(c->ev1, s));
    c->have_timing = true;
    return GRT_OK;
}

// bwd_launch's kernel table of one CP: [0] no geometry group (nothing goes through the gradient buffer), [1] plain atomics, [2] merged
template <int CP>
static void backward_kernels(bool plain, const void* k[3])
{
    k[0] = plain ? reinterpret_cast<const void*>(k_backward_features<false, CP, false>) : reinterpret_cast<const void*>(k_backward_features<true, CP, false>);
    k[1] = reinterpret_cast<const void*>(k_backward_features<false, CP, true>);
    k[2] = reinterpret_cast<const void*>(k_backward_features<true, CP, true>);
}

static int launch_backward(grt_ctx* c, const grt_params* p, RenderArgs& a, const float* d_feat, uint32_t channels, const float* d_grad_out,
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
    a.tile_w = channels; // (see the head of this file)
    const grt_gaussian_grads gg = {g->pos, g->scale, g->quat, g->opacity, nullptr}; // (no SH group: the higher-SH buffer is never made)
    const bool plain = c->opt_bwd_plain != 0;
    const void* kernels[3];
    if (channels <= 4u) backward_kernels<4>(plain, kernels);
    else if (channels <= 8u) backward_kernels<8>(plain, kernels);
    else backward_kernels<16>(plain, kernels);
    return bwd_launch(c, p, a, d_grad_out, d_feat, &gg, g->feat, kernels, stream, fn);
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
