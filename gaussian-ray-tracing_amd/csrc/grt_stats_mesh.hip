// grt_stats_mesh.hip — per-particle contribution statistics of a mesh frame (include/grt.h: grt_particle_stats_mesh_frame /
// grt_particle_stats_mesh_rays): what grt_stats.hip computes for a Gaussian-only frame, for rays that bounce off
// mirror, glass or normal-shaded meshes.  A ray has ONE event list with ONE running transmittance, cut into the segments of its
// iterations; every composited event i of segment s has the weight w_i = T_i alpha_i and the colour weight cw_i = c_s w_i with which its
// radiance enters the pixel (c_s: 1 - A_{s-1} of a Gaussian pass, D_S (1 - B_{S-1}) of the last pass, 1 of a terminating hit).
//
// k_particle_stats_mesh<MERGE, COLOUR>: one ray per lane, an 8x8 tile or 64 buffer rays per wave.  Its skeleton is the raygen loop of
// k_backward_mesh (grt_backward_mesh.hip), statement for statement: the per-lane mesh walk, the iteration's Gaussian segment with the
// transmittance carried on through `density`, the step of A and B.  Per slot of the k-buffers the wave scatters through
// stats_scatter (grt_stats.h).
//   COLOUR = false  (neither colour output asked for): ONE sweep.
//   COLOUR = true   the last pass's c_S needs D_S, known only at the end of that segment: the loop runs twice, as k_backward_mesh's
//                   does.  Sweep 0 scatters nothing and keeps D_fin, sweep 1 scatters.
// Nothing is stored per segment or per iteration.  The step filter (step_first, step_last) is a per-lane predicate on the
// iteration's number: it clears `ev` before the scatter and changes no control flow — T, A and B run through the events it leaves out.
//
// Wave convergence: stats_scatter<MERGE> (DPP, v_readlane) is reached by every lane of the wave for every slot of every round of every
// iteration.  The three nested loops (iterations, rounds, slots) are each entered and left on a wave-uniform condition — a ballot
// over the lanes' own conditions, or a constant trip count — and a lane whose own condition is false idles inside them with
// `it` / `act` cleared, as the header of grt_backward_mesh.hip states.  The mesh walk is the per-lane mesh_closest_t and the k-nearest
// round the per-lane gps_round, both inside `if (it)` / `if (act)` and neither with a wave operation in it.  A lane's iterations are
// bounded by max_bounces and the 1000-iteration timeout, its rounds by lastT rising past the segment's end: every ballot becomes zero.
#include <string>

#include "grt_bwd.h"
#include "grt_mesh.h"
#include "grt_stats.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "k_particle_stats_mesh runs gps_round (grt_kround.h): its per-lane stack stride is the launch block size");

// the iterations whose events are counted: first..last, 1-based, inclusive; last = 0: open
struct StepRange {
    uint32_t first, last;
};

template <bool MERGE, bool COLOUR>
__global__ __launch_bounds__(kBlock) void k_particle_stats_mesh(const RenderArgs a, const StatsArgs s, const StepRange r)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out; // (unused: nothing is written per ray)
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out) && (a.root_ref != kNoRoot);
    float wr = 1.0f;
    if (live && s.ray_weight) {
        wr = s.ray_weight[idx];
        live = wr != 0.0f; // a ray of weight exactly 0 is not traced
    }
    if (!__builtin_amdgcn_ballot_w64(live)) return; // wave-uniform

    const float epsT = 1e-9f;
    const float minT = a.p.minTransmittance;
    const uint64_t key0 = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
    KBuf<K> kb;
    grt::Cnt cnt; // (dead: no counters, no watchdog)

    float D_fin = 0.0f; // sweep 0: the density behind the ray's last iteration
#pragma unroll 1
    for (int pass = COLOUR ? 0 : 1; pass < 2; pass++) {
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
            // the segment's colour weight c_s, in float32 as shade_ray forms it, and whether the step filter counts the segment
            float c_s = 0.0f;
            if (COLOUR && pass) c_s = (state == Terminate) ? 1.0f : (state == LastGaussianPass ? D_fin * (1.0f - B) : 1.0f - A);
            const bool counted = (step >= r.first) && (r.last == 0u || step <= r.last);
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
                    if (pass) { // (wave-uniform: the sweep's number)
                        const bool ev = hit && counted;
                        float w = 0.0f, cw = 0.0f;
                        if (ev) {
                            w = T * hitAlpha; // T: the transmittance before the event
                            cw = c_s * w;
                        } else {
                            id = 0;
                        }
                        stats_scatter<MERGE, COLOUR>(s, ev, id, wr * w, w, wr * cw, cw, lane);
                    }
                    if (hit) T *= (1.0f - hitAlpha);
                }
                if (act) {
                    if (kb.key[K - 1] == kKeyInvalid) act = false;
                    else last_key = kb.key[K - 1];
                    act = act && (lastT <= seg_tmax) && (T > minT);
                }
            }
            // ---- the iteration's step of the loop (shade_ray, grt_render.hip) ----
            if (it) {
                density = 1.0f - T;
                const float D = density;
                if (state == Terminate) {
                    going = false;
                } else if (state == LastGaussianPass) { // A = clamp(A + D)
                    A = clampf(A + D, 0.0f, 1.0f);
                } else { // A = clamp(A + D); B = clamp(B + D)
                    A = clampf(A + D, 0.0f, 1.0f);
                    B = clampf(B + D, 0.0f, 1.0f);
                }
                timeout += 1;
                if (timeout > kTimeoutIterations) going = false;
            }
        }
        if (pass == 0) D_fin = density;
    }
}

} // namespace
} // namespace grt

using namespace grt;

static int launch(grt_ctx* c, const RenderArgs& a, const float* d_ray_weight, const grt_particle_stats_mesh* out, void* stream, const char* fn)
{
    if (!out || (!out->weight_sum && !out->weight_max && !out->count && !out->colour_sum && !out->colour_max)) {
        c->err = std::string(fn) + ": no output (weight_sum, weight_max, count, colour_sum and colour_max are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (out->step_last != 0u && out->step_first > out->step_last) {
        c->err = std::string(fn) + ": step_first > step_last (iterations are counted from 1; step_last = 0 leaves the range open)";
        return GRT_ERR_INVALID;
    }
    const grt_ctx* sc = scene_of(c);
    // no ray, no particle or an empty tree: nothing is composited, nothing is written
    if (a.n_blocks == 0 || sc->n == 0 || sc->gbvh.root_ref == kNoRoot) { c->have_timing = false; return GRT_OK; }
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    StatsArgs sa;
    sa.ray_weight = d_ray_weight;
    sa.weight_sum = out->weight_sum; sa.weight_max = out->weight_max; sa.count = out->count;
    sa.colour_sum = out->colour_sum; sa.colour_max = out->colour_max;
    StepRange sr;
    sr.first = out->step_first; sr.last = out->step_last;
    const bool colour = out->colour_sum || out->colour_max;
    static const void* const kernels[2][2] = {
        {reinterpret_cast<const void*>(k_particle_stats_mesh<true, false>), reinterpret_cast<const void*>(k_particle_stats_mesh<true, true>)},
        {reinterpret_cast<const void*>(k_particle_stats_mesh<false, false>), reinterpret_cast<const void*>(k_particle_stats_mesh<false, true>)}};
    void* args[3] = {const_cast<RenderArgs*>(&a), &sa, &sr};
    int rc = lane_launch(c, a, kernels[c->opt_bwd_plain ? 1 : 0][colour ? 1 : 0], args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

extern "C" {

int grt_particle_stats_mesh_frame(grt_ctx* c, const grt_params* p, const float* d_ray_weight, const grt_particle_stats_mesh* out, uint32_t x0,
                                  uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_particle_stats_mesh_frame";
    RenderArgs a;
    int rc = bwd_fill_args(c, p, true, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, a, d_ray_weight, out, stream, fn);
}

int grt_particle_stats_mesh_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_ray_weight,
                                 const grt_particle_stats_mesh* out, void* stream)
{
    const char* fn = "grt_particle_stats_mesh_rays";
    RenderArgs a;
    int rc = bwd_fill_args(c, p, true, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, a, d_ray_weight, out, stream, fn);
}

} // extern "C"
