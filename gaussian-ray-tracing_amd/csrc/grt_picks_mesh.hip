// grt_picks_mesh.hip — per-ray picks of a mesh frame (include/grt.h: grt_ray_picks_mesh_frame / grt_ray_picks_mesh_rays; DESIGN.md
// 5.24): what grt_picks.hip computes for a Gaussian-only frame, for rays that bounce off mirror, glass or normal-shaded meshes.  A ray
// has ONE event list with ONE running transmittance, cut into the segments of its iterations; among the events of the iterations
// step_first .. step_last the FIRST one, the one of largest weight w_i = T_i alpha_i (PEAK) and the first behind which the ray's own
// transmittance has fallen to cross_T (CROSS), each as the particle's original id, the key distance along the iteration's own ray, the
// weight, the iteration's 1-based number and the world position o_s + t d_s.
//
// k_ray_picks_mesh: one ray per lane, an 8x8 tile or 64 buffer rays per wave.  Its skeleton is the raygen loop of k_particle_stats_mesh
// (grt_stats_mesh.hip) with no colour output, statement for statement: the per-lane mesh walk, the iteration's Gaussian segment with
// the transmittance carried on through `density`, the step of A and B — ONE sweep.  The picks are selections among the lane's own
// events: twenty-one registers per lane, no wave operation, no atomic; at the end every lane that owns an element of the window or of
// the buffer stores the requested ones by plain vector stores — "none" for a ray that was not traced or met no such event.  A NULL
// output is a wave-uniform branch on a kernel argument.  The context owns no buffer for this.  The step filter is a per-lane predicate
// on the iteration's number: it keeps an event from being a candidate and changes no control flow — T, A and B run through the events
// it leaves out, and CROSS tests the ray's own T, not one restarted at the range.
//
// Wave convergence: no wave operation is in the kernel but the ballots of its loop conditions.  The two outer loops (iterations,
// rounds) are each entered and left on a wave-uniform condition — a ballot over the lanes' own conditions — and the slot loop has a
// constant trip count; a lane whose own condition is false idles inside them with `it` / `act` cleared, as the header of
// grt_backward_mesh.hip states.  A lane's iterations are bounded by max_bounces and the 1000-iteration timeout, its rounds by lastT
// rising past the segment's end (a round that finds nothing clears `act`): every ballot becomes zero.  Only vector stores write memory.
#include <string>

#include "grt_bwd.h"
#include "grt_mesh.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "k_ray_picks_mesh runs gps_round (grt_kround.h): its per-lane stack stride is the launch block size");

// one rule's pick, in registers
struct PickM {
    uint32_t id;
    float t, w;
    uint32_t step;
    f3 pt; // o_s + t d_s on the iteration's own ray
};

__device__ __forceinline__ void pick_store(const grt_pick_mesh_out& out, size_t idx, const PickM& k)
{
    if (out.id) out.id[idx] = k.id;
    if (out.t) out.t[idx] = k.t;
    if (out.weight) out.weight[idx] = k.w;
    if (out.step) out.step[idx] = k.step;
    if (out.point) {
        float* q = out.point + idx * 3;
        q[0] = k.pt.x; q[1] = k.pt.y; q[2] = k.pt.z;
    }
}

__global__ __launch_bounds__(kBlock) void k_ray_picks_mesh(const RenderArgs a, const grt_ray_picks_mesh k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    const bool live = lane_ray(a, lane, o, d, idx, has_out) && (a.root_ref != kNoRoot);
    const PickM none = {GRT_PICK_NONE, 0.0f, 0.0f, 0u, mk3(0, 0, 0)};
    PickM first = none, peak = none, cross = none;

    if (__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        const float epsT = 1e-9f;
        const float minT = a.p.minTransmittance;
        const float cross_T = k.cross_T;
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
            const bool counted = (step >= k.step_first) && (k.step_last == 0u || step <= k.step_last);
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
                        const float te = key_t(key);
                        // T: the transmittance before the event; the point o_s[k] + t * d_s[k]: one float32 multiplication and one
                        // addition per component (the unit is built without contraction)
                        const PickM e = {id, te, T * hitAlpha, step, mk3(ray_o.x + te * ray_d.x, ray_o.y + te * ray_d.y, ray_o.z + te * ray_d.z)};
                        if (first.id == GRT_PICK_NONE) first = e;
                        if (peak.id == GRT_PICK_NONE || e.w > peak.w) peak = e; // strictly greater: the earliest event wins a tie
                        // the walk's own T behind the event (T *= 1 - hitAlpha follows: the same float32 product)
                        if (cross.id == GRT_PICK_NONE && T * (1.0f - hitAlpha) <= cross_T) cross = e;
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
    }
    if (has_out) { // every element of the window or of the buffer once per requested array
        pick_store(k.first, idx, first);
        pick_store(k.peak, idx, peak);
        pick_store(k.cross, idx, cross);
    }
}

} // namespace
} // namespace grt

using namespace grt;

static bool wanted(const grt_pick_mesh_out& o) { return o.id || o.t || o.weight || o.step || o.point; }

static int launch(grt_ctx* c, const RenderArgs& a, const grt_ray_picks_mesh* out, void* stream, const char* fn)
{
    if (!out || (!wanted(out->first) && !wanted(out->peak) && !wanted(out->cross))) {
        c->err = std::string(fn) + ": no output (id, t, weight, step and point of first, peak and cross are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (wanted(out->cross) && !(out->cross_T > 0.0f && out->cross_T < 1.0f)) { // (NaN fails both comparisons)
        c->err = std::string(fn) + ": cross_T must lie in (0, 1), not " + std::to_string(out->cross_T);
        return GRT_ERR_INVALID;
    }
    if (out->step_last != 0u && out->step_first > out->step_last) {
        c->err = std::string(fn) + ": step_first > step_last (iterations are counted from 1; step_last = 0 leaves the range open)";
        return GRT_ERR_INVALID;
    }
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced and its elements "none")
    grt_ray_picks_mesh k = *out;
    void* args[2] = {const_cast<RenderArgs*>(&a), &k};
    int rc = lane_launch(c, a, reinterpret_cast<const void*>(k_ray_picks_mesh), args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

extern "C" {

int grt_ray_picks_mesh_frame(grt_ctx* c, const grt_params* p, const grt_ray_picks_mesh* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                             void* stream)
{
    const char* fn = "grt_ray_picks_mesh_frame";
    RenderArgs a;
    int rc = bwd_fill_args(c, p, true, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, a, out, stream, fn);
}

int grt_ray_picks_mesh_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const grt_ray_picks_mesh* out, void* stream)
{
    const char* fn = "grt_ray_picks_mesh_rays";
    RenderArgs a;
    int rc = bwd_fill_args(c, p, true, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, a, out, stream, fn);
}

} // extern "C"
