// grt_mesh_walk.h — the ONE text of the raygen loop of a mesh frame for kernels with one ray per lane, on grt_bwd.h
// (sweep_events) and grt_mesh.h (mesh_closest_t, mesh_shade).  grt_stats_mesh.hip, grt_features_mesh.hip, grt_picks_mesh.hip,
// grt_events_mesh.hip and grt_depth_mesh.hip include it: k_particle_stats_mesh, k_ray_picks_mesh, k_backward_events_mesh and
// k_ray_depth_mesh call mesh_walk; every mesh kernel but k_backward_mesh takes its colour weight from seg_weight, and every unit
// its step-range refusal from check_step_range (grt_internal.h).
// Five kernels keep the loop WRITTEN OUT as they had it before this header, statement for statement mesh_walk's around sweep_events'
// and with their own step filter — a change here is a change there:
//   k_backward_mesh<MERGE> (grt_backward_mesh.hip)     runs under every training step through a mirror;
//   k_ray_events_mesh (grt_events_mesh.hip)            folded, it read two more spilled SGPRs back per iteration than its ISA test allows;
//   k_render_features_mesh<CP>, k_backward_features_mesh<MERGE, CP, GEOM> (grt_features_mesh.hip)
//                                                      folded, the 16-channel forward and feat-only backward ran 1.4 and 0.9 % behind;
//   k_backward_depth_mesh<MERGE, PEAK> (grt_depth_mesh.hip)   folded, its merged PEAK instantiation ran 2 % behind.
//
// mesh_walk runs shade_ray's loop (grt_render.hip; shaders/tracer.cu:58-106) for the whole wave in step.  Per iteration: the per-lane
// mesh hit and the next ray, then the iteration's Gaussian segment [t_min, seg_tmax] on the iteration's own ray as ONE call of
// sweep_events with the transmittance T = 1 - density carried in and out, then the step of A, B and density by the mesh hit's state.
// Nothing is stored per segment or per iteration: a glass ray may take 1001 iterations.  A kernel that needs a total of the whole ray
// before it can form its terms (D_fin, the backward's sums) calls mesh_walk twice and forms the same events in the same order.
//
// The callables and who reaches them:
//   begin(seg)                                  the WHOLE wave, once per iteration, before the segment; per-lane work under seg.it.
//   on_slot(seg, ev, id, Tb, hitAlpha, key)     the WHOLE wave, for every slot of every round of every iteration (sweep_events' own
//                                               contract).  It MAY hold wave operations (scatter<MERGE>, stats_scatter: DPP, v_readlane).
//   end(seg, T, D)                              per lane, inside `if (seg.it)`, behind the segment and before A and B move: T the
//                                               transmittance behind the segment, D = 1 - T.  It must hold NO wave operation.
//   leave()                                     optional, per lane, between two rounds of a lane that is still in the segment: true takes the
//                                               lane out of the walk for good (it idles like a lane whose ray has ended).  No wave operation.
//
// Wave convergence.  Three nested loops: iterations (here), rounds and slots (sweep_events).  The iteration loop is left on a ballot over
// the lanes' own `it`, the round loop on a ballot over the lanes' own `act`, and the slot loop has the constant trip count K; a lane
// whose own condition is false idles inside them with `it` / `act` cleared.  So begin and on_slot are reached by every lane of a wave
// that is in the loop at all.  The mesh walk (mesh_closest_t, mesh_shade) and the k-nearest round (gps_round) are per lane, inside
// `if (it)` / `if (act)`, with no wave operation in them.  A caller that loops around mesh_walk (its sweeps) does so with a constant
// trip count, and returns early only on a ballot.
//
// Why it cannot hang: a lane's iterations are bounded by max_bounces and by the 1000-iteration timeout; its rounds by lastT rising past
// the segment's end (a round that finds nothing clears `act`); the slot loop runs K times; and the group loop of wave_groups inside a
// merged scatter clears at least its leader's bit of a ballot per turn.  Every ballot becomes zero.
#pragma once

#include "grt_bwd.h"
#include "grt_mesh.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "mesh_walk runs gps_round (grt_kround.h): its per-lane stack stride is the launch block size");

// What an iteration hands its callables: the iteration's own ray, the mesh hit's normal, state and segment end, the iteration's
// 1-based number, A and B as they stand BEFORE this iteration's step, and whether this lane takes part.
struct MeshSeg {
    f3 ray_o, ray_d, normal;
    float seg_tmax;
    int state;
    uint32_t step;
    float A, B;
    bool it;
};

// The iterations whose events are counted by a kernel on mesh_walk: step_first .. step_last as the entry points take them, 1-based,
// inclusive, step_last = 0 for an open end.  The only way to make one is the constructor, which keeps the open end as the largest
// number: hoisted out of the loops, a test `last == 0u` is a lane mask in two scalar registers, and the merged kernels at the 106-SGPR
// limit have none to spare.  Trivially copyable: it travels as (part of) a kernel argument.
class StepRange {
    uint32_t first_, last_;

public:
    StepRange() = default;
    __host__ __device__ StepRange(uint32_t step_first, uint32_t step_last) : first_(step_first), last_(step_last == 0u ? 0xFFFFFFFFu : step_last) {}
    __device__ __forceinline__ bool counted(uint32_t step) const { return (step >= first_) && (step <= last_); }
};

// The colour weight c_s with which a segment's events enter the pixel, in float32 as shade_ray forms it: 1 of a terminating hit,
// D_S (1 - B_{S-1}) of the last pass (D_fin: the density behind the ray's last iteration), 1 - A_{s-1} of a Gaussian pass.
__device__ __forceinline__ float seg_weight(int state, float A, float B, float D_fin)
{
    return (state == Terminate) ? 1.0f : (state == LastGaussianPass ? D_fin * (1.0f - B) : 1.0f - A);
}

// part: this lane has a ray to walk.  Returns the density behind the lane's last iteration (D_fin; 0 for a lane that took no part).
template <class Begin, class OnSlot, class End, class Leave = NeverLeave>
__device__ __forceinline__ float mesh_walk(const RenderArgs& a, uint32_t* stk, f3 o, f3 d, bool part, Begin&& begin, OnSlot&& on_slot, End&& end,
                                           Leave&& leave = Leave())
{
    f3 curO = o, curD = d;
    float A = 0.0f, B = 0.0f, density = 0.0f;
    uint32_t numBounces = 0u, timeout = 0u, step = 0u;
    bool going = part;
    while (true) {
        MeshSeg s;
        s.it = going && (length3(curD) > 0.1f) && (numBounces < a.p.max_bounces);
        going = s.it;
        if (!__builtin_amdgcn_ballot_w64(s.it)) break; // wave-uniform
        s.ray_o = curO; s.ray_d = curD;
        s.state = LastGaussianPass;
        s.seg_tmax = a.p.t_max;
        s.normal = mk3(0, 0, 0);
        if (s.it) { // per lane: no wave operation inside
            uint32_t n0 = 0, n1 = 0;
            const MeshHit mh = mesh_closest_t<false, kBlock>(a, stk, s.ray_o, s.ray_d, kTraceMeshTmin, kTraceMeshTmax, n0, n1);
            mesh_shade(a, mh, s.ray_o, s.ray_d, s.state, s.seg_tmax, s.normal, curO, curD, numBounces);
            step++;
        }
        s.step = step; s.A = A; s.B = B;
        begin(s);
        // ---- this iteration's Gaussian segment [t_min, seg_tmax] on (ray_o, ray_d), T carried on (trace(), tracer.cuh:328-373) ----
        float T = 1.0f - density;
        sweep_events(
            a, stk, s.ray_o, s.ray_d, mk_rayinv(s.ray_o, s.ray_d), s.seg_tmax, s.it, T,
            [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t key) { on_slot(s, ev, id, Tb, hitAlpha, key); },
            [&]() {
                const bool out = leave();
                if (out) going = false;
                return out;
            });
        // ---- the iteration's step of the loop (shade_ray, grt_render.hip) ----
        if (s.it) {
            density = 1.0f - T;
            const float D = density;
            end(s, T, D);
            if (s.state == Terminate) {
                going = false;
            } else if (s.state == LastGaussianPass) { // A = clamp(A + D)
                A = clampf(A + D, 0.0f, 1.0f);
            } else { // A = clamp(A + D); B = clamp(B + D)
                A = clampf(A + D, 0.0f, 1.0f);
                B = clampf(B + D, 0.0f, 1.0f);
            }
            timeout += 1;
            if (timeout > kTimeoutIterations) going = false;
        }
    }
    return density;
}

} // namespace
} // namespace grt
