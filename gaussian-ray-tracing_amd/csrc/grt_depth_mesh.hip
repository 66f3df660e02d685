// grt_depth_mesh.hip — differentiable ray depth through mirror, glass and normal-shaded meshes (include/grt.h: grt_ray_depth_mesh_frame /
// _rays, grt_backward_depth_mesh_frame / _rays): what grt_depth.hip computes for a Gaussian-only ray, for rays that bounce.
// A ray has ONE event list with ONE running transmittance, cut into the segments of its iterations (grt_backward_mesh.hip).  The path
// prefix P_1 = 0, P_{s+1} = P_s + tmax_s (the iteration's segment end: the mesh hit distance, or t_max) is a float32 running sum per lane
// and is DATA; an event i of segment s lies at x_i = P_s + tau_i, tau_i its key distance (KEY) or peak_tau on the step's own ray (PEAK),
// and enters with w_i = T_i alpha_i and the segment's colour weight c_s (grt_features_mesh.hip):
//     m0_s = sum w_i,  m1_s = sum w_i x_i,  m2_s = sum (w_i x_i) x_i;     weight += m0_s c_s,  dist += m1_s c_s,  dist2 += m2_s c_s.
// GRT_DEPTH_SURFACE: a terminating (GRT_NORMAL) hit adds its surface with u = 1 - D_S at x_S = P_S + tmax_S, as the colour adds ncol u.
// The step filter (step_first, step_last) is a per-lane predicate on the iteration's number: an event outside the range is composited —
// T, A and B run through it — and enters no output; it changes no control flow.  The surface flag likewise touches only the step.
//
// Both kernels: one ray per lane, an 8x8 tile or 64 buffer rays per wave (grt_mesh_walk.h: the raygen loop, its convergence contract
// and why it cannot hang).  peak_tau / tau_terms (grt_depth.h) run per lane and hold no wave operation.
//   k_ray_depth_mesh<PEAK>              on mesh_walk, ONE sweep, with three moment accumulators per segment.  Plain stores at the end; no
//                                       atomic, no wave operation.
//   k_backward_depth_mesh<MERGE, PEAK>  keeps the loop WRITTEN OUT as it had it, its own step filter included, statement for statement mesh_walk's and sweep_events' (a change there
//                                       is a change here): on mesh_walk its merged PEAK instantiation ran 2 % behind the parent's
//                                       (DESIGN.md 5.27).  Two sweeps: k_backward_features_mesh<MERGE, ., true>'s with the one-channel radiance
//                                       phi_i = g_D x_i + (g_D2 x_i) x_i + g_W (0 outside the step range), no feature scatter; the
//                                       surface enters sweep 0's F total as -phi_surf T_end,S (k_backward_mesh's ncol term); under PEAK
//                                       a counted event adds dloss/dtau_i = c_s w_i (g_D + 2 g_D2 x_i) through tau_terms<false> on the
//                                       step's ray, NOT gated by the 0.99 clamp.  scatter<MERGE> (DPP, v_readlane; outside
//                                       every per-lane `if`) writes the 11 geometry / opacity values into the slot's gradient buffer.
#include <string>

#include "grt_depth.h"
#include "grt_mesh_walk.h"

namespace grt {
namespace {

// steps / first..last: the iterations whose events are counted, 1-based, inclusive (last = 0: open).  surface: GRT_DEPTH_SURFACE
struct DepthMeshFwd {
    const float* pos;   // [n][3] by original id (the uploaded attributes; read under PEAK alone)
    const float* scale; // [n][3]
    const float* quat;  // [n][4]
    grt_depth_mesh_out o;
    StepRange steps;
    uint32_t surface;
};
struct DepthMeshBwd {
    const float* g_dist;   // [N] or null: 0
    const float* g_dist2;  // [N] or null: 0
    const float* g_weight; // [N] or null: 0
    uint32_t first, last;
    uint32_t surface;
};

template <bool PEAK>
__global__ __launch_bounds__(kBlock) void k_ray_depth_mesh(const RenderArgs a, const DepthMeshFwd k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    const bool live = lane_ray(a, lane, o, d, idx, has_out) && (a.root_ref != kNoRoot);
    float dist = 0.0f, dist2 = 0.0f, weight = 0.0f;
    uint32_t n = 0u;

    if (__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        float Pfx = 0.0f; // the path prefix P_s
        float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
        bool counted = false;
        mesh_walk(
            a, stk, o, d, live,
            [&](const MeshSeg& s) {
                counted = k.steps.counted(s.step);
                m0 = 0.0f; m1 = 0.0f; m2 = 0.0f;
            },
            [&](const MeshSeg& s, bool hit, uint32_t id, float T, float hitAlpha, uint64_t key) {
                if (hit && counted) {
                    float tau = key_t(key);
                    if (PEAK) {
                        PeakFrame f;
                        tau = peak_tau(k.pos, k.scale, k.quat, id, s.ray_o, s.ray_d, f);
                    }
                    const float x = Pfx + tau;
                    const float w = T * hitAlpha; // T: the transmittance before the event
                    const float wt = w * x;
                    m0 = m0 + w;
                    m1 = m1 + wt;
                    m2 = m2 + wt * x;
                    n++;
                }
            },
            [&](const MeshSeg& s, float, float D) { // the segment's moments enter with c_s
                const float c_s = seg_weight(s.state, s.A, s.B, D);
                weight = weight + m0 * c_s;
                dist = dist + m1 * c_s;
                dist2 = dist2 + m2 * c_s;
                if (s.state == Terminate && counted && k.surface != 0u) { // the surface itself, as the colour's ncol (1 - D)
                    const float u = 1.0f - D;
                    const float xs = Pfx + s.seg_tmax;
                    const float ux = u * xs;
                    weight = weight + u;
                    dist = dist + ux;
                    dist2 = dist2 + ux * xs;
                }
                Pfx = Pfx + s.seg_tmax;
            });
    }
    if (has_out) { // every element of the window or of the buffer once per requested array: zeros for a ray that was not traced
        if (k.o.dist) k.o.dist[idx] = dist;
        if (k.o.dist2) k.o.dist2[idx] = dist2;
        if (k.o.weight) k.o.weight[idx] = weight;
        if (k.o.count) k.o.count[idx] = n;
    }
}

template <bool MERGE, bool PEAK>
__global__ __launch_bounds__(kBlock) void k_backward_depth_mesh(const RenderArgs a, const BwdArgs b, const DepthMeshBwd k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out; // (unused: nothing is written per ray)
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out) && (a.root_ref != kNoRoot);
    float gD = 0.0f, gD2 = 0.0f, gW = 0.0f;
    if (live) { // a ray whose three upstream values are exactly 0 is not traced
        if (k.g_dist) gD = k.g_dist[idx];
        if (k.g_dist2) gD2 = k.g_dist2[idx];
        if (k.g_weight) gW = k.g_weight[idx];
        live = (gD != 0.0f) || (gD2 != 0.0f) || (gW != 0.0f);
    }
    if (!__builtin_amdgcn_ballot_w64(live)) return; // wave-uniform
    // A lane without a ray to differentiate takes a zero direction: the raygen loop's own guard |d| > 0.1 then keeps it out of both
    // sweeps, and `live` need not be held across them (as a lane mask it was the one SGPR pair the plain-atomics kernels kept in VGPR
    // lanes: tests/test_mesh_depth_isa.py holds them to no lane move).
    if (!live) d = mk3(0, 0, 0);

    const float epsT = 1e-9f;
    const float minT = a.p.minTransmittance;
    const uint64_t key0 = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
    KBuf<K> kb;
    grt::Cnt cnt; // (dead: no counters, no watchdog)
    RayAcc ra;    // (dead: event_terms<., false> and tau_terms<false> do not touch it)
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);

    // the totals of sweep 0 (grt_backward_mesh.hip, with g_C . R_s = P_s = sum_{i in s} w_i phi_i, g_A = 0 and phi_surf for g_C . ncol)
    float W_tot = 0.0f, K0 = 0.0f, TT_e = 0.0f, QT_e = 0.0f, F_tot = 0.0f, D_fin = 0.0f;
    uint32_t e_tot = 0u;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        f3 curO = o, curD = d;
        float A = 0.0f, B = 0.0f, density = 0.0f;
        float Pfx = 0.0f;    // the path prefix P_s
        uint32_t numBounces = 0u, timeout = 0u, step = 0u;
        bool bound = false;  // the A clamp has bound at a Gaussian pass
        uint32_t e = 0u;     // Gaussian passes before it did
        float mW = 0.0f, mQ = 0.0f, mTT = 0.0f, mQT = 0.0f; // prefixes (sweep 1) / totals (end of sweep 0)
        float sig = 0.0f, mF = 0.0f;
        bool going = true; // (a lane that is not live: d = 0, see above)
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
            const bool counted = (step >= k.first) && (k.last == 0u || step <= k.last);
            // sweep 1: the segment's weight c_s, and what lies behind it of sum_j gD_j T_end,j
            float c_s = 0.0f, G_s = 0.0f;
            if (pass) {
                c_s = seg_weight(state, A, B, D_fin);
                G_s = F_tot;
                if (state == GaussianPass && step <= e_tot) G_s += K0 * (TT_e - mTT) + (QT_e - mQT);
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
                    float v[kVals];
#pragma unroll
                    for (int q = 0; q < kVals; q++) v[q] = 0.0f;
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
                            const float w = T * hitAlpha; // T: the transmittance before the event
                            float phi = 0.0f, x = 0.0f;   // an event outside the step range enters with a radiance of zero
                            if (counted) {
                                float tau = key_t(key);
                                if (PEAK) {
                                    PeakFrame f;
                                    tau = peak_tau(b.pos, b.scale, b.quat, id, ray_o, ray_d, f);
                                }
                                x = Pfx + tau;
                                phi = (gD * x + (gD2 * x) * x) + gW;
                            }
                            P = P + w * phi;
                            if (pass) {
                                // what lies behind the event: W - W_<=i, against sum_{j >= s} gD_j T_end,j; both enter through 1/(1 - alpha)
                                const float behind = W_tot - (mW + c_s * P);
                                // (GAUSS = false: the template flag guards the SH block alone, which a depth call never enters — bwd_launch
                                //  is handed no sh, so want_sh is 0 — and whose 45 atomics and three scalars the text then does not hold)
                                geom = event_terms<false, false>(a, b, id, ray_o, ray_d, dn, mk3(phi, 0, 0), T, hitAlpha, mk3(0, 0, 0), mk3(c_s, 0, 0),
                                                                G_s - behind, 1.0f, v, ra);
                                if (PEAK) {
                                    if (counted) { // tau does not pass through the 0.99 clamp.  The frame is formed again behind event_terms:
                                                   // held across it, it would be live through the whole chain below alpha
                                        PeakFrame f;
                                        const float tau = peak_tau(b.pos, b.scale, b.quat, id, ray_o, ray_d, f);
                                        tau_terms<false>(b, id, ray_d, f, tau, (c_s * w) * (gD + (2.0f * gD2) * x), v, ra);
                                        geom = true;
                                    }
                                }
                                ev = true;
                            }
                            T *= (1.0f - hitAlpha);
                        }
                    }
                    if (pass) scatter<MERGE>(b.acc, ev, id, v, geom, false, lane); // (wave-uniform: the sweep's number)
                }
                if (act) {
                    if (kb.key[K - 1] == kKeyInvalid) act = false;
                    else last_key = kb.key[K - 1];
                    act = act && (lastT <= seg_tmax) && (T > minT);
                }
            }
            // ---- the iteration's step of the loop, and the running sums (both sweeps alike; k_backward_mesh with g_A = 0) ----
            if (it) {
                density = 1.0f - T;
                const float D = density;
                if (state == Terminate) { // F += Phi_s, and under GRT_DEPTH_SURFACE the surface: gD_S = -phi_surf
                    mW += P;
                    mF = 0.0f;
                    if (counted && k.surface != 0u) {
                        const float xs = Pfx + seg_tmax;
                        const float phis = (gD * xs + (gD2 * xs) * xs) + gW;
                        mF = (0.0f - phis) * T;
                    }
                    going = false;
                } else if (state == LastGaussianPass) { // F += Phi_s D (1 - B); A = clamp(A + D)
                    mW += (D * (1.0f - B)) * P;
                    mF = (P * (1.0f - B)) * T;
                    if (!bound) sig = 0.0f - P * D;
                    A = clampf(A + D, 0.0f, 1.0f);
                } else { // F += Phi_s (1 - A); A = clamp(A + D); B = clamp(B + D)
                    const float xx = A + D;
                    mW += (1.0f - A) * P;
                    if (!bound) {
                        if (xx > 1.0f || xx < 0.0f) {
                            bound = true;
                            sig = 0.0f - P;
                        } else {
                            mQ += P;
                            mTT += T;
                            mQT += mQ * T;
                            e = step;
                        }
                    }
                    A = clampf(xx, 0.0f, 1.0f);
                    B = clampf(B + D, 0.0f, 1.0f);
                }
                Pfx = Pfx + seg_tmax;
                timeout += 1;
                if (timeout > kTimeoutIterations) going = false;
            }
        }
        if (pass == 0) {
            D_fin = density;
            W_tot = mW; K0 = sig - mQ; TT_e = mTT; QT_e = mQT; F_tot = mF; e_tot = e;
        }
    }
}

} // namespace
} // namespace grt

using namespace grt;

// what the four entry points refuse before they look at their rays: the mesh backward's refusals in the entry point's name, an unknown
// kind, unknown flag bits and a step range that ends before it begins
static int fill(grt_ctx* c, const grt_params* p, int kind, uint32_t flags, uint32_t step_first, uint32_t step_last, RenderArgs* a, const char* fn)
{
    int rc = bwd_fill_args(c, p, true, a, fn);
    if (rc != GRT_OK) return rc;
    if (kind != GRT_DEPTH_KEY && kind != GRT_DEPTH_PEAK) {
        c->err = std::string(fn) + ": unknown kind " + std::to_string(kind) + " (GRT_DEPTH_KEY = 0, GRT_DEPTH_PEAK = 1)";
        return GRT_ERR_INVALID;
    }
    if (flags & ~(uint32_t)GRT_DEPTH_SURFACE) {
        c->err = std::string(fn) + ": unknown flag bits " + std::to_string(flags & ~(uint32_t)GRT_DEPTH_SURFACE) + " (GRT_DEPTH_SURFACE = 1)";
        return GRT_ERR_INVALID;
    }
    return check_step_range(c, step_first, step_last, fn);
}

static int check_forward(grt_ctx* c, const grt_depth_mesh_out* o, const char* fn)
{
    if (o && (o->dist || o->dist2 || o->weight || o->count)) return GRT_OK;
    c->err = std::string(fn) + ": no output (dist, dist2, weight and count are all NULL)";
    return GRT_ERR_INVALID;
}

// the backward's arguments, checked in the header's order
static int check_backward(grt_ctx* c, const grt_depth_mesh_upstream* up, const grt_feature_grads* g, const char* fn)
{
    if (!up || (!up->g_dist && !up->g_dist2 && !up->g_weight)) {
        c->err = std::string(fn) + ": no upstream (g_dist, g_dist2 and g_weight are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (!g || (!g->pos && !g->scale && !g->quat && !g->opacity)) {
        c->err = std::string(fn) + ": no output (pos, scale, quat and opacity are all NULL; feat is not a depth gradient)";
        return GRT_ERR_INVALID;
    }
    return GRT_OK;
}

static int launch_forward(grt_ctx* c, const RenderArgs& a, int kind, uint32_t flags, const grt_depth_mesh_out* out, uint32_t step_first,
                          uint32_t step_last, void* stream, const char* fn)
{
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced and its elements zero)
    const grt_ctx* sc = scene_of(c);
    DepthMeshFwd k;
    k.pos = sc->d_pos; k.scale = sc->d_scale; k.quat = sc->d_quat;
    k.o = *out;
    k.steps = StepRange(step_first, step_last);
    k.surface = (flags & GRT_DEPTH_SURFACE) ? 1u : 0u;
    void* args[2] = {const_cast<RenderArgs*>(&a), &k};
    const void* kernel = kind == GRT_DEPTH_PEAK ? reinterpret_cast<const void*>(k_ray_depth_mesh<true>)
                                                : reinterpret_cast<const void*>(k_ray_depth_mesh<false>);
    int rc = lane_launch(c, a, kernel, args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

static int launch_backward(grt_ctx* c, const grt_params* p, const RenderArgs& a, int kind, uint32_t flags, const grt_depth_mesh_upstream* up,
                           const grt_feature_grads* g, uint32_t step_first, uint32_t step_last, void* stream, const char* fn)
{
    DepthMeshBwd k;
    k.g_dist = up->g_dist; k.g_dist2 = up->g_dist2; k.g_weight = up->g_weight;
    k.first = step_first; k.last = step_last;
    k.surface = (flags & GRT_DEPTH_SURFACE) ? 1u : 0u;
    const grt_gaussian_grads gg = {g->pos, g->scale, g->quat, g->opacity, nullptr}; // (no SH group; feat is left untouched and is no request)
    // ([0] null: a call without a geometry group was refused, and own_work is false — an empty scene launches nothing)
    static const void* const key_kernels[3] = {nullptr, reinterpret_cast<const void*>(k_backward_depth_mesh<false, false>),
                                               reinterpret_cast<const void*>(k_backward_depth_mesh<true, false>)};
    static const void* const peak_kernels[3] = {nullptr, reinterpret_cast<const void*>(k_backward_depth_mesh<false, true>),
                                                reinterpret_cast<const void*>(k_backward_depth_mesh<true, true>)};
    // (BwdArgs::g_rgb / g_alpha stay NULL: the upstreams are DepthMeshBwd's)
    return bwd_launch(c, p, a, nullptr, nullptr, &gg, BwdUnit{kind == GRT_DEPTH_PEAK ? peak_kernels : key_kernels, &k, false}, stream, fn);
}

extern "C" {

int grt_ray_depth_mesh_frame(grt_ctx* c, const grt_params* p, int kind, uint32_t flags, const grt_depth_mesh_out* out, uint32_t step_first,
                             uint32_t step_last, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_ray_depth_mesh_frame";
    RenderArgs a;
    int rc = fill(c, p, kind, flags, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = check_forward(c, out, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, kind, flags, out, step_first, step_last, stream, fn);
}

int grt_ray_depth_mesh_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, int kind, uint32_t flags,
                            const grt_depth_mesh_out* out, uint32_t step_first, uint32_t step_last, void* stream)
{
    const char* fn = "grt_ray_depth_mesh_rays";
    RenderArgs a;
    int rc = fill(c, p, kind, flags, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = check_forward(c, out, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, kind, flags, out, step_first, step_last, stream, fn);
}

int grt_backward_depth_mesh_frame(grt_ctx* c, const grt_params* p, int kind, uint32_t flags, const grt_depth_mesh_upstream* up,
                                  const grt_feature_grads* grads, uint32_t step_first, uint32_t step_last, uint32_t x0, uint32_t y0,
                                  uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_backward_depth_mesh_frame";
    RenderArgs a;
    int rc = fill(c, p, kind, flags, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, up, grads, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, kind, flags, up, grads, step_first, step_last, stream, fn);
}

int grt_backward_depth_mesh_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, int kind, uint32_t flags,
                                 const grt_depth_mesh_upstream* up, const grt_feature_grads* grads, uint32_t step_first, uint32_t step_last,
                                 void* stream)
{
    const char* fn = "grt_backward_depth_mesh_rays";
    RenderArgs a;
    int rc = fill(c, p, kind, flags, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, up, grads, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, kind, flags, up, grads, step_first, step_last, stream, fn);
}

} // extern "C"
