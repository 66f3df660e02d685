// grt_backward_mesh.hip — the backward pass of mesh frames (include/grt.h: grt_backward_mesh / grt_backward_rays_mesh; DESIGN.md
// 5.11): gradients of a loss on (rgbf, alpha) of a frame whose rays bounce off mirror, glass or normal-shaded meshes, with respect
// to the activated attributes of the Gaussians.  Meshes and every discrete decision are held fixed.
//
// k_backward_mesh<MERGE>, on the shared device text of grt_bwd.h: a lane's ray and upstream gradient, event_terms and scatter.
//
// One ray per lane.  The two sweeps of k_backward, each wrapped in the raygen bounce loop (grt_render.hip: shade_ray):
//   sweep 0  runs the whole loop — mesh hit, next ray, the iteration's Gaussian segment with the transmittance carried on — and
//            derives a handful of per-ray totals;
//   sweep 1  walks the same loop and the same events and forms every composited event's terms, its two suffix quantities
//            (the weighted radiance behind it, sum_{j >= s} gD_j T_end,j) as total minus prefix.
// Nothing is stored per segment or per iteration: a glass ray may take 1001 iterations.
// The bounce loop stays WRITTEN OUT here, as backward_body's sweep does (this kernel runs under every training step
// through a mirror).  Its one other text is mesh_walk of grt_mesh_walk.h, which every other mesh unit stands on: a
// change here is a change there, and the colour weight c_s below is seg_weight's.
//
// The totals (iterations 1..S; every iteration but the last is a Gaussian pass, and in Gaussian passes B follows A step by step):
//   e     the last Gaussian pass before the A clamp binds (all of them when it never binds)
//   W     sum_s c_s (g_C . R_s)                       the weighted radiance of the whole ray
//   sig   dloss/dA_e at fixed R: -(g_C . R_{s*}) when the clamp binds at Gaussian pass s*, else g_A through the last iteration
//   Q     sum_{s <= e} g_C . R_s       TT  sum_{s <= e} T_end,s       QT  sum_{s <= e} Q_s T_end,s  (Q_s: the prefix of Q)
//   F     gD_S T_end,S of a last pass or a terminating iteration
// so that, for s <= e, gD_s = sig - (Q - Q_s) and sum_{j >= s} gD_j T_end,j = (sig - Q)(TT - TT_{s-1}) + (QT - QT_{s-1}) + F; for s > e
// it is F alone (a Gaussian pass behind a binding clamp has gD = 0).
//
// Wave convergence: scatter<MERGE> (DPP, v_readlane) is reached by every lane of the wave for every slot of every round of every
// iteration.  The three nested loops (iterations, rounds, slots) are each entered and left on a wave-uniform condition — a ballot
// over the lanes' own conditions, or a constant trip count — and a lane whose own condition is false idles inside them with
// `it` / `act` cleared.  The mesh walk is the per-lane mesh_closest_t and the k-nearest round the per-lane gps_round, both inside
// `if (it)` / `if (act)` and neither with a wave operation in it.  A lane's iterations are bounded by max_bounces and the
// 1000-iteration timeout, its rounds by lastT rising past the segment's end: every ballot becomes zero.
#include <string>

#include "grt_bwd.h"
#include "grt_mesh.h"

namespace grt {
namespace {

// what the bounce loop carries from iteration to iteration, and the running sums both sweeps form the same way
struct MeshLoop {
    f3 curO, curD;
    float A, B, density;
    uint32_t numBounces, timeout, step;
    bool bound;          // the A clamp has bound at a Gaussian pass
    uint32_t e;          // Gaussian passes before it did
    float W, Q, TT, QT;  // prefixes (sweep 1) / totals (end of sweep 0)
    float sig, F;
};

template <bool MERGE>
__global__ __launch_bounds__(kBlock) void k_backward_mesh(const RenderArgs a, const BwdArgs b)
{
    constexpr bool GAUSS = true, RAYS = false;
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out; // (unused: nothing is written per ray)
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out) && (a.root_ref != kNoRoot);
    f3 gC;
    float gA;
    live = load_upstream(b, idx, live, gC, gA);
    if (!__builtin_amdgcn_ballot_w64(live)) return; // wave-uniform

    const float epsT = 1e-9f;
    const float minT = a.p.minTransmittance;
    const uint64_t key0 = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
    KBuf<K> kb;
    grt::Cnt cnt; // (dead: no counters, no watchdog)
    RayAcc ra; // (dead: RAYS = false)
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);

    // the totals of sweep 0
    float W_tot = 0.0f, K0 = 0.0f, TT_e = 0.0f, QT_e = 0.0f, F_tot = 0.0f, D_fin = 0.0f;
    uint32_t e_tot = 0u;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        MeshLoop m;
        m.curO = o; m.curD = d;
        m.A = m.B = m.density = 0.0f;
        m.numBounces = m.timeout = m.step = 0u;
        m.bound = false; m.e = 0u;
        m.W = m.Q = m.TT = m.QT = 0.0f;
        m.sig = gA; m.F = 0.0f;
        bool going = live;
        // ---- the raygen loop (shaders/tracer.cu:58-106), the whole wave in step ----
        while (true) {
            const bool it = going && (length3(m.curD) > 0.1f) && (m.numBounces < a.p.max_bounces);
            going = it;
            if (!__builtin_amdgcn_ballot_w64(it)) break; // wave-uniform
            const f3 ray_o = m.curO, ray_d = m.curD;
            int state = LastGaussianPass;
            float seg_tmax = a.p.t_max;
            f3 normal = mk3(0, 0, 0);
            if (it) { // per lane: no wave operation inside
                uint32_t n0 = 0, n1 = 0;
                const MeshHit mh = mesh_closest_t<false, kBlock>(a, stk, ray_o, ray_d, kTraceMeshTmin, kTraceMeshTmax, n0, n1);
                mesh_shade(a, mh, ray_o, ray_d, state, seg_tmax, normal, m.curO, m.curD, m.numBounces);
                m.step++;
            }
            // ---- this iteration's Gaussian segment [t_min, seg_tmax] on (ray_o, ray_d), T carried on (trace(), tracer.cuh:328-373) ----
            const f3 dn = normalize3(ray_d);
            const rayinv ri = mk_rayinv(ray_o, ray_d);
            const float t_hi = seg_tmax + epsT;
            float T = 1.0f - m.density, lastT = a.p.t_min;
            uint64_t last_key = key0;
            f3 C = mk3(0, 0, 0);
            // sweep 1: the segment's weight c_s, and what lies behind it of sum_j gD_j T_end,j
            float c_s = 0.0f, G_s = 0.0f;
            if (pass) {
                c_s = (state == Terminate) ? 1.0f : (state == LastGaussianPass ? D_fin * (1.0f - m.B) : 1.0f - m.A);
                G_s = F_tot;
                if (state == GaussianPass && m.step <= e_tot) G_s += K0 * (TT_e - m.TT) + (QT_e - m.QT);
            }
            const f3 g_rad = mul3s(gC, c_s);
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
                            const f3 L = event_radiance(a, id, dn);
                            C = add3(C, mul3s(mul3s(L, T), hitAlpha)); // R_s, term by term as the forward adds it
                            if (pass) {
                                ev = true;
                                // what lies behind the event: W - W_<=i, against sum_{j >= s} gD_j T_end,j; both enter through 1/(1 - alpha)
                                const float behind = W_tot - (m.W + c_s * dot3(gC, C));
                                geom = event_terms<GAUSS, RAYS>(a, b, id, ray_o, ray_d, dn, L, T, hitAlpha, mk3(0, 0, 0), g_rad, G_s - behind, 1.0f, v, ra);
                            }
                            T *= (1.0f - hitAlpha);
                        }
                    }
                    if (pass) scatter<MERGE>(b.acc, ev, id, v, geom, b.want_sh != 0u, lane);
                }
                if (act) {
                    if (kb.key[K - 1] == kKeyInvalid) act = false;
                    else last_key = kb.key[K - 1];
                    act = act && (lastT <= seg_tmax) && (T > minT);
                }
            }
            // ---- the iteration's step of the loop, and the running sums (both sweeps alike) ----
            if (it) {
                m.density = 1.0f - T;
                const float D = m.density;
                const float q = dot3(gC, C);
                if (state == Terminate) { // renderNormal: C += R + ncol (1 - D); A += D + (1 - D)
                    const f3 ncol = mul3s(add3(normal, mk3(1.0f, 1.0f, 1.0f)), 0.5f);
                    m.W += q;
                    m.F = (0.0f - dot3(gC, ncol)) * T;
                    going = false;
                } else if (state == LastGaussianPass) { // C += R D (1 - B); A = clamp(A + D)
                    const float x = m.A + D;
                    const float uA = (x > 1.0f || x < 0.0f) ? 0.0f : 1.0f;
                    m.W += (D * (1.0f - m.B)) * q;
                    m.F = (q * (1.0f - m.B) + uA * gA) * T;
                    if (!m.bound) m.sig = uA * gA - q * D;
                    m.A = clampf(x, 0.0f, 1.0f);
                } else { // C += R (1 - A); A = clamp(A + D); B = clamp(B + D)
                    const float x = m.A + D;
                    m.W += (1.0f - m.A) * q;
                    if (!m.bound) {
                        if (x > 1.0f || x < 0.0f) {
                            m.bound = true;
                            m.sig = 0.0f - q;
                        } else {
                            m.Q += q;
                            m.TT += T;
                            m.QT += m.Q * T;
                            m.e = m.step;
                        }
                    }
                    m.A = clampf(x, 0.0f, 1.0f);
                    m.B = clampf(m.B + D, 0.0f, 1.0f);
                }
                m.timeout += 1;
                if (m.timeout > kTimeoutIterations) going = false;
            }
        }
        if (pass == 0) {
            W_tot = m.W; K0 = m.sig - m.Q; TT_e = m.TT; QT_e = m.QT; F_tot = m.F; D_fin = m.density; e_tot = m.e;
        }
    }
}

} // namespace
} // namespace grt

using namespace grt;

static int launch(grt_ctx* c, const grt_params* p, const RenderArgs& a, const float* d_grad_rgbf, const float* d_grad_alpha, const grt_gaussian_grads* g,
                  void* stream, const char* fn)
{
    if (!d_grad_rgbf || !g) { c->err = std::string(fn) + ": null pointer (d_grad_rgbf and the grads structure are required)"; return GRT_ERR_INVALID; }
    static const void* const kernels[3] = {nullptr, reinterpret_cast<const void*>(k_backward_mesh<false>), reinterpret_cast<const void*>(k_backward_mesh<true>)};
    return bwd_launch(c, p, a, d_grad_rgbf, d_grad_alpha, g, BwdUnit{kernels, nullptr, false}, stream, fn);
}

extern "C" {

int grt_backward_mesh(grt_ctx* c, const grt_params* p, const float* d_grad_rgbf, const float* d_grad_alpha, const grt_gaussian_grads* g,
                      uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_backward_mesh";
    RenderArgs a;
    int rc = bwd_fill_args(c, p, true, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, p, a, d_grad_rgbf, d_grad_alpha, g, stream, fn);
}

int grt_backward_rays_mesh(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_grad_rgbf,
                           const float* d_grad_alpha, const grt_gaussian_grads* g, void* stream)
{
    const char* fn = "grt_backward_rays_mesh";
    RenderArgs a;
    int rc = bwd_fill_args(c, p, true, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    if (n == 0) { // (no ray: nothing to read either)
        if (!g) { c->err = "grt_backward_rays_mesh: null grads structure"; return GRT_ERR_INVALID; }
        c->have_timing = false;
        return GRT_OK;
    }
    return launch(c, p, a, d_grad_rgbf, d_grad_alpha, g, stream, fn);
}

} // extern "C"
