// grt_features_mesh.hip — per-particle feature channels composited through mirror, glass and normal-shaded meshes, with gradients
// (include/grt.h: grt_render_features_mesh_frame / _rays, grt_backward_features_mesh_frame / _rays): what
// grt_features.hip computes for a Gaussian-only frame, for rays that bounce.  A ray has ONE event list with ONE running
// transmittance, cut into the segments of its iterations (grt_backward_mesh.hip); every composited event i of segment s has the weight
// w_i = T_i alpha_i, and its feature row enters the pixel with the colour weight c_s w_i (grt_stats_mesh.hip: c_s is 1 - A_{s-1} of a
// Gaussian pass, D_S (1 - B_{S-1}) of the last pass, 1 of a terminating hit):
//     Phi_s[c] = sum_{i in s} w_i feat[id_i][c],     F[c] = sum_s c_s Phi_s[c].
// A mesh surface itself contributes no feature, and nothing is clamped.  The step filter (step_first, step_last) is a per-lane
// predicate on the iteration's number: an event outside the range is composited — T, A and B run through it — with a feature row of
// zero; it changes no control flow.
//
// Both kernels: one ray per lane, an 8x8 tile or 64 buffer rays per wave.  Both keep the raygen loop WRITTEN OUT as they had it before
// grt_mesh_walk.h, statement for statement mesh_walk's and sweep_events' (that header: the loop, its convergence contract and why it
// cannot hang; a change there is a change here), their own step filter included: on mesh_walk the 16-channel instantiations ran 0.9 to
// 1.4 % behind.  The channel count C is a runtime argument; the channel loops run to the compile-time CP in
// {4, 8, 16} under the guard c < C, as in grt_features.hip.
//   k_render_features_mesh<CP>   ONE sweep: the last pass's c_S = D_S (1 - B_{S-1}) is needed only when that segment ends, where D_S
//                                is known.  Two sets of CP accumulators, Phi_s and F; plain stores at the end, no atomic.
//   k_backward_features_mesh<MERGE, CP, GEOM>   two sweeps as k_backward_mesh: sweep 0 collects its seven per-lane totals and D_fin
//                                with the one-channel radiance phi_i = sum_c g_c feat[id_i][c] (0 outside the step range), g_C =
//                                (1, 0, 0), g_A = 0 and no ncol term; sweep 1 hands event_terms that radiance, scatter<MERGE> writes the
//                                11 geometry / opacity values into the slot's gradient buffer, and the feature gradient c_s w_i g_c of
//                                a counted event goes into the caller's [n][C] array by float atomics, merged through wave_groups
//                                as in k_backward_features.
//     GEOM = false  pos, scale, quat and opacity are all NULL: still two sweeps (D_fin), but no phi, no totals, no event_terms, no
//                   gradient buffer and no flush are in its text.
//
// Wave convergence: scatter<MERGE> and feat_scatter<MERGE, CP> (DPP, v_readlane) are reached by every lane of the wave for every slot
// of every round of every iteration; the loops are entered and left as grt_mesh_walk.h's head states.
#include <string>

#include "grt_mesh_walk.h"

namespace grt {
namespace {

static_assert(GRT_MAX_FEATURE_CHANNELS == 16, "the instantiations below are CP = 4, 8, 16");

// the iterations whose events carry their feature row: first..last, 1-based, inclusive; last = 0: open
struct FeatMeshOut {
    const float* feat; // [n][C] by original id
    float* out;        // [pixels or rays][C], written
    uint32_t channels;
    uint32_t first, last;
};
struct FeatMeshArgs {
    const float* up;   // upstream [pixels or rays][C]
    const float* feat; // [n][C] by original id
    float* gfeat;      // the feature gradient [n][C], added to, or null
    uint32_t channels;
    uint32_t first, last;
};

template <int CP>
__global__ __launch_bounds__(kBlock) void k_render_features_mesh(const RenderArgs a, const FeatMeshOut f)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    const bool live = lane_ray(a, lane, o, d, idx, has_out) && (a.root_ref != kNoRoot);
    const uint32_t C = f.channels;
    float F[CP], Phi[CP];
#pragma unroll
    for (int c = 0; c < CP; c++) F[c] = 0.0f;

    if (__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        const float epsT = 1e-9f;
        const float minT = a.p.minTransmittance;
        const uint64_t key0 = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
        KBuf<K> kb;
        grt::Cnt cnt; // (dead: no counters, no watchdog)

        f3 curO = o, curD = d;
        float A = 0.0f, B = 0.0f, density = 0.0f;
        uint32_t numBounces = 0u, timeout = 0u, step = 0u;
        bool going = live;
        // ---- the raygen loop (shaders/tracer.cu:58-106), the whole wave in step ----
        while (true) {
            const bool it = going && (length3(curD) > 0.1f) && (numBounces < a.p.max_bounces);
            going = it;
            if (!__builtin_amdgcn_ballot_w64(it)) break; // wave-uniform
            const f3 ray_o = curO, ray_d = curD;
            int state = LastGaussianPass;
            float seg_tmax = a.p.t_max;
            f3 normal = mk3(0, 0, 0);
            if (it) { // per lane: no wave operation inside
                uint32_t n0 = 0, n1 = 0;
                const MeshHit mh = mesh_closest_t<false, kBlock>(a, stk, ray_o, ray_d, kTraceMeshTmin, kTraceMeshTmax, n0, n1);
                mesh_shade(a, mh, ray_o, ray_d, state, seg_tmax, normal, curO, curD, numBounces);
                step++;
            }
            // ---- this iteration's Gaussian segment [t_min, seg_tmax] on (ray_o, ray_d), T carried on (trace(), tracer.cuh:328-373) ----
            const rayinv ri = mk_rayinv(ray_o, ray_d);
            const float t_hi = seg_tmax + epsT;
            float T = 1.0f - density, lastT = a.p.t_min;
            uint64_t last_key = key0;
            const bool counted = (step >= f.first) && (f.last == 0u || step <= f.last);
#pragma unroll
            for (int c = 0; c < CP; c++) Phi[c] = 0.0f;
            bool act = it && (lastT <= seg_tmax) && (T > minT);
            while (__builtin_amdgcn_ballot_w64(act)) {
                if (act) {
                    gps_round<false, false, K>(a, stk, ray_o, ray_d, ri, last_key, t_hi, kb, cnt, 0xFFFFFFFFu);
                    if (kb.key[0] == kKeyInvalid) act = false;
                }
#pragma unroll 1
                for (int i = 0; i < K; i++) {
                    bool hit = false;
                    uint32_t id = 0;
                    uint64_t key = kKeyInvalid;
                    float hitAlpha = 0.0f;
#pragma unroll
                    for (int j = 0; j < K; j++) {
                        if (j == i) { key = kb.key[j]; hitAlpha = kb.alpha[j]; }
                    }
                    if (act && key != kKeyInvalid && T > minT) {
                        lastT = fmaxf(key_t(key), lastT);
                        if (a.p.alpha_min < hitAlpha) {
                            hit = true;
                            id = key_id(key);
                        }
                    }
                    if (hit && counted) {
                        const float* fr = f.feat + (size_t)id * C;
                        const float w = T * hitAlpha; // T: the transmittance before the event
#pragma unroll
                        for (int c = 0; c < CP; c++) {
                            if ((uint32_t)c < C) Phi[c] = Phi[c] + w * fr[c];
                        }
                    }
                    if (hit) T *= (1.0f - hitAlpha);
                }
                if (act) {
                    if (kb.key[K - 1] == kKeyInvalid) act = false;
                    else last_key = kb.key[K - 1];
                    act = act && (lastT <= seg_tmax) && (T > minT);
                }
            }
            // ---- the iteration's step of the loop (shade_ray, grt_render.hip): the segment's features enter with c_s ----
            if (it) {
                density = 1.0f - T;
                const float D = density;
                float c_s;
                if (state == Terminate) {
                    c_s = 1.0f;
                    going = false;
                } else if (state == LastGaussianPass) { // A = clamp(A + D)
                    c_s = D * (1.0f - B);
                    A = clampf(A + D, 0.0f, 1.0f);
                } else { // A = clamp(A + D); B = clamp(B + D)
                    c_s = 1.0f - A;
                    A = clampf(A + D, 0.0f, 1.0f);
                    B = clampf(B + D, 0.0f, 1.0f);
                }
#pragma unroll
                for (int c = 0; c < CP; c++) F[c] = F[c] + Phi[c] * c_s;
                timeout += 1;
                if (timeout > kTimeoutIterations) going = false;
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

// one lane's C values w g_c to its particle's row of the feature gradient (grt_features.hip has the same two helpers for its kernel)
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
__global__ __launch_bounds__(kBlock) void k_backward_features_mesh(const RenderArgs a, const BwdArgs b, const FeatMeshArgs f)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    const float* __restrict__ up = f.up;
    const float* __restrict__ feat = f.feat;
    float* __restrict__ gfeat = f.gfeat;
    const uint32_t C = f.channels;
    uint32_t lane;
    size_t idx;
    bool has_out; // (unused: nothing is written per ray)
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out) && (a.root_ref != kNoRoot);
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

    const float epsT = 1e-9f;
    const float minT = a.p.minTransmittance;
    const uint64_t key0 = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
    KBuf<K> kb;
    grt::Cnt cnt; // (dead: no counters, no watchdog)
    RayAcc ra;    // (dead: event_terms<., false> does not touch it)
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);

    // the totals of sweep 0 (grt_backward_mesh.hip, with g_C . R_s = P_s = sum_{i in s} w_i phi_i and g_A = 0)
    float W_tot = 0.0f, K0 = 0.0f, TT_e = 0.0f, QT_e = 0.0f, F_tot = 0.0f, D_fin = 0.0f;
    uint32_t e_tot = 0u;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        f3 curO = o, curD = d;
        float A = 0.0f, B = 0.0f, density = 0.0f;
        uint32_t numBounces = 0u, timeout = 0u, step = 0u;
        bool bound = false;  // the A clamp has bound at a Gaussian pass
        uint32_t e = 0u;     // Gaussian passes before it did
        float mW = 0.0f, mQ = 0.0f, mTT = 0.0f, mQT = 0.0f; // prefixes (sweep 1) / totals (end of sweep 0)
        float sig = 0.0f, mF = 0.0f;
        bool going = live;
        // ---- the raygen loop (shaders/tracer.cu:58-106), the whole wave in step ----
        while (true) {
            const bool it = going && (length3(curD) > 0.1f) && (numBounces < a.p.max_bounces);
            going = it;
            if (!__builtin_amdgcn_ballot_w64(it)) break; // wave-uniform
            const f3 ray_o = curO, ray_d = curD;
            int state = LastGaussianPass;
            float seg_tmax = a.p.t_max;
            f3 normal = mk3(0, 0, 0);
            if (it) { // per lane: no wave operation inside
                uint32_t n0 = 0, n1 = 0;
                const MeshHit mh = mesh_closest_t<false, kBlock>(a, stk, ray_o, ray_d, kTraceMeshTmin, kTraceMeshTmax, n0, n1);
                mesh_shade(a, mh, ray_o, ray_d, state, seg_tmax, normal, curO, curD, numBounces);
                step++;
            }
            // ---- this iteration's Gaussian segment [t_min, seg_tmax] on (ray_o, ray_d), T carried on (trace(), tracer.cuh:328-373) ----
            const f3 dn = normalize3(ray_d);
            const rayinv ri = mk_rayinv(ray_o, ray_d);
            const float t_hi = seg_tmax + epsT;
            float T = 1.0f - density, lastT = a.p.t_min;
            uint64_t last_key = key0;
            float P = 0.0f; // P_s = sum_{i in s} w_i phi_i, term by term
            const bool counted = (step >= f.first) && (f.last == 0u || step <= f.last);
            // sweep 1: the segment's weight c_s, and what lies behind it of sum_j gD_j T_end,j
            float c_s = 0.0f, G_s = 0.0f;
            if (pass) {
                c_s = seg_weight(state, A, B, D_fin);
                if constexpr (GEOM) {
                    G_s = F_tot;
                    if (state == GaussianPass && step <= e_tot) G_s += K0 * (TT_e - mTT) + (QT_e - mQT);
                }
            }
            bool act = it && (lastT <= seg_tmax) && (T > minT);
            while (__builtin_amdgcn_ballot_w64(act)) {
                if (act) {
                    gps_round<false, false, K>(a, stk, ray_o, ray_d, ri, last_key, t_hi, kb, cnt, 0xFFFFFFFFu);
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
                                float phi = 0.0f; // an event outside the step range enters with a feature row of zero
                                if (counted) {
                                    const float* fr = feat + (size_t)id * C;
#pragma unroll
                                    for (int c = 0; c < CP; c++) {
                                        if ((uint32_t)c < C) phi = phi + g[c] * fr[c];
                                    }
                                }
                                P = P + w * phi;
                                if (pass) {
                                    // what lies behind the event: W - W_<=i, against sum_{j >= s} gD_j T_end,j; both enter through 1/(1 - alpha)
                                    const float behind = W_tot - (mW + c_s * P);
                                    geom = event_terms<true, false>(a, b, id, ray_o, ray_d, dn, mk3(phi, 0, 0), T, hitAlpha, mk3(0, 0, 0), mk3(c_s, 0, 0),
                                                                    G_s - behind, 1.0f, v, ra);
                                }
                            }
                            ev = pass != 0;
                            T *= (1.0f - hitAlpha);
                        }
                    }
                    if (pass) { // (wave-uniform: the sweep's number)
                        if constexpr (GEOM) scatter<MERGE>(b.acc, ev, id, v, geom, false, lane);
                        if (gfeat) feat_scatter<MERGE, CP>(gfeat, C, ev && counted, id, c_s * w, g, lane); // (wave-uniform: a kernel argument)
                    }
                }
                if (act) {
                    if (kb.key[K - 1] == kKeyInvalid) act = false;
                    else last_key = kb.key[K - 1];
                    act = act && (lastT <= seg_tmax) && (T > minT);
                }
            }
            // ---- the iteration's step of the loop, and the running sums (both sweeps alike; k_backward_mesh with g_A = 0, no ncol) ----
            if (it) {
                density = 1.0f - T;
                const float D = density;
                if (state == Terminate) { // F += Phi_s
                    if constexpr (GEOM) {
                        mW += P;
                        mF = 0.0f;
                    }
                    going = false;
                } else if (state == LastGaussianPass) { // F += Phi_s D (1 - B); A = clamp(A + D)
                    if constexpr (GEOM) {
                        mW += (D * (1.0f - B)) * P;
                        mF = (P * (1.0f - B)) * T;
                        if (!bound) sig = 0.0f - P * D;
                    }
                    A = clampf(A + D, 0.0f, 1.0f);
                } else { // F += Phi_s (1 - A); A = clamp(A + D); B = clamp(B + D)
                    const float x = A + D;
                    if constexpr (GEOM) {
                        mW += (1.0f - A) * P;
                        if (!bound) {
                            if (x > 1.0f || x < 0.0f) {
                                bound = true;
                                sig = 0.0f - P;
                            } else {
                                mQ += P;
                                mTT += T;
                                mQT += mQ * T;
                                e = step;
                            }
                        }
                    }
                    A = clampf(x, 0.0f, 1.0f);
                    B = clampf(B + D, 0.0f, 1.0f);
                }
                timeout += 1;
                if (timeout > kTimeoutIterations) going = false;
            }
        }
        if (pass == 0) {
            D_fin = density;
            if constexpr (GEOM) {
                W_tot = mW; K0 = sig - mQ; TT_e = mTT; QT_e = mQT; F_tot = mF; e_tot = e;
            }
        }
    }
}

} // namespace
} // namespace grt

using namespace grt;

// what the four entry points refuse before they look at their rays: the mesh backward's refusals in the entry point's name, a channel
// count outside 1 .. GRT_MAX_FEATURE_CHANNELS and a step range that ends before it begins
static int fill(grt_ctx* c, const grt_params* p, uint32_t channels, uint32_t step_first, uint32_t step_last, RenderArgs* a, const char* fn)
{
    int rc = bwd_fill_args(c, p, true, a, fn);
    if (rc != GRT_OK) return rc;
    if (channels == 0 || channels > GRT_MAX_FEATURE_CHANNELS) {
        c->err = std::string(fn) + ": channels must be 1.." + std::to_string(GRT_MAX_FEATURE_CHANNELS) + ", not " + std::to_string(channels);
        return GRT_ERR_INVALID;
    }
    return check_step_range(c, step_first, step_last, fn);
}

static int launch_forward(grt_ctx* c, const RenderArgs& a, const float* d_feat, uint32_t channels, float* d_out, uint32_t step_first,
                          uint32_t step_last, void* stream, const char* fn)
{
    if (!d_feat || !d_out) { c->err = std::string(fn) + ": null pointer (the features and the output are required)"; return GRT_ERR_INVALID; }
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced and its element zero)
    FeatMeshOut f;
    f.feat = d_feat; f.out = d_out; f.channels = channels; f.first = step_first; f.last = step_last;
    static const void* const kernels[3] = {reinterpret_cast<const void*>(k_render_features_mesh<4>), reinterpret_cast<const void*>(k_render_features_mesh<8>),
                                           reinterpret_cast<const void*>(k_render_features_mesh<16>)};
    const void* fnk = kernels[channels <= 4u ? 0 : (channels <= 8u ? 1 : 2)];
    void* args[2] = {const_cast<RenderArgs*>(&a), &f};
    int rc = lane_launch(c, a, fnk, args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

// bwd_launch's kernel table of one CP: [0] no geometry group (nothing goes through the gradient buffer), [1] plain atomics, [2] merged
template <int CP>
static void backward_kernels(bool plain, const void* k[3])
{
    k[0] = plain ? reinterpret_cast<const void*>(k_backward_features_mesh<false, CP, false>)
                 : reinterpret_cast<const void*>(k_backward_features_mesh<true, CP, false>);
    k[1] = reinterpret_cast<const void*>(k_backward_features_mesh<false, CP, true>);
    k[2] = reinterpret_cast<const void*>(k_backward_features_mesh<true, CP, true>);
}

static int launch_backward(grt_ctx* c, const grt_params* p, const RenderArgs& a, const float* d_feat, uint32_t channels, const float* d_grad_out,
                           const grt_feature_grads* g, uint32_t step_first, uint32_t step_last, void* stream, const char* fn)
{
    if (!d_feat || !d_grad_out) { c->err = std::string(fn) + ": null pointer (the features and the upstream gradient are required)"; return GRT_ERR_INVALID; }
    if (!g || (!g->pos && !g->scale && !g->quat && !g->opacity && !g->feat)) {
        c->err = std::string(fn) + ": no output (pos, scale, quat, opacity and feat are all NULL)";
        return GRT_ERR_INVALID;
    }
    const grt_ctx* sc = scene_of(c);
    // no ray, no particle or an empty tree: nothing is composited, nothing is written
    if (a.n_blocks == 0 || sc->n == 0 || sc->gbvh.root_ref == kNoRoot) { c->have_timing = false; return GRT_OK; }
    FeatMeshArgs f;
    f.up = d_grad_out; f.feat = d_feat; f.gfeat = g->feat; f.channels = channels; f.first = step_first; f.last = step_last;
    const grt_gaussian_grads gg = {g->pos, g->scale, g->quat, g->opacity, nullptr}; // (no SH group: the higher-SH buffer is never made)
    const bool plain = c->opt_bwd_plain != 0;
    const void* kernels[3];
    if (channels <= 4u) backward_kernels<4>(plain, kernels);
    else if (channels <= 8u) backward_kernels<8>(plain, kernels);
    else backward_kernels<16>(plain, kernels);
    return bwd_launch(c, p, a, nullptr, nullptr, &gg, BwdUnit{kernels, &f, g->feat != nullptr}, stream, fn); // (no upstream on (rgbf, alpha): BwdArgs' stay null)
}

extern "C" {

int grt_render_features_mesh_frame(grt_ctx* c, const grt_params* p, const float* d_feat, uint32_t channels, float* d_out, uint32_t step_first,
                                   uint32_t step_last, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_render_features_mesh_frame";
    RenderArgs a;
    int rc = fill(c, p, channels, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, d_feat, channels, d_out, step_first, step_last, stream, fn);
}

int grt_render_features_mesh_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_feat, uint32_t channels,
                                  float* d_out, uint32_t step_first, uint32_t step_last, void* stream)
{
    const char* fn = "grt_render_features_mesh_rays";
    RenderArgs a;
    int rc = fill(c, p, channels, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, d_feat, channels, d_out, step_first, step_last, stream, fn);
}

int grt_backward_features_mesh_frame(grt_ctx* c, const grt_params* p, const float* d_feat, uint32_t channels, const float* d_grad_out,
                                     const grt_feature_grads* grads, uint32_t step_first, uint32_t step_last, uint32_t x0, uint32_t y0,
                                     uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_backward_features_mesh_frame";
    RenderArgs a;
    int rc = fill(c, p, channels, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, d_feat, channels, d_grad_out, grads, step_first, step_last, stream, fn);
}

int grt_backward_features_mesh_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_feat, uint32_t channels,
                                    const float* d_grad_out, const grt_feature_grads* grads, uint32_t step_first, uint32_t step_last,
                                    void* stream)
{
    const char* fn = "grt_backward_features_mesh_rays";
    RenderArgs a;
    int rc = fill(c, p, channels, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, d_feat, channels, d_grad_out, grads, step_first, step_last, stream, fn);
}

} // extern "C"
