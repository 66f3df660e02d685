// grt_picks_mesh.hip — per-ray picks of a mesh frame (include/grt.h: grt_ray_picks_mesh_frame / grt_ray_picks_mesh_rays; DESIGN.md
// 5.24): what grt_picks.hip computes for a Gaussian-only frame, for rays that bounce off mirror, glass or normal-shaded meshes.  A ray
// has ONE event list with ONE running transmittance, cut into the segments of its iterations; among the events of the iterations
// step_first .. step_last the FIRST one, the one of largest weight w_i = T_i alpha_i (PEAK) and the first behind which the ray's own
// transmittance has fallen to cross_T (CROSS), each as the particle's original id, the key distance along the iteration's own ray, the
// weight, the iteration's 1-based number and the world position o_s + t d_s.
//
// k_ray_picks_mesh: one ray per lane, an 8x8 tile or 64 buffer rays per wave, ONE sweep of mesh_walk (grt_mesh_walk.h: the raygen loop,
// its convergence contract and why it cannot hang).  The picks are selections among the lane's own events: twenty-one registers per
// lane, no wave operation, no atomic; at the end every lane that owns an element of the window or of the buffer stores the requested
// ones by plain vector stores — "none" for a ray that was not traced or met no such event.  A NULL output is a wave-uniform branch on a
// kernel argument.  The context owns no buffer for this.  The step filter is a per-lane predicate on the iteration's number: it keeps
// an event from being a candidate and changes no control flow — T, A and B run through the events it leaves out, and CROSS tests the
// ray's own T, not one restarted at the range.
#include <string>

#include "grt_mesh_walk.h"

namespace grt {
namespace {

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

__global__ __launch_bounds__(kBlock, 3) void k_ray_picks_mesh(const RenderArgs a, const grt_ray_picks_mesh k, const StepRange r)
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
        const float cross_T = k.cross_T;
        bool counted = false;
        mesh_walk(
            a, stk, o, d, live, [&](const MeshSeg& s) { counted = r.counted(s.step); },
            [&](const MeshSeg& s, bool hit, uint32_t id, float T, float hitAlpha, uint64_t key) {
                if (hit && counted) {
                    const float te = key_t(key);
                    // T: the transmittance before the event; the point o_s[k] + t * d_s[k]: one float32 multiplication and one
                    // addition per component (the unit is built without contraction)
                    const PickM e = {id, te, T * hitAlpha, s.step, mk3(s.ray_o.x + te * s.ray_d.x, s.ray_o.y + te * s.ray_d.y, s.ray_o.z + te * s.ray_d.z)};
                    if (first.id == GRT_PICK_NONE) first = e;
                    if (peak.id == GRT_PICK_NONE || e.w > peak.w) peak = e; // strictly greater: the earliest event wins a tie
                    // the walk's own T behind the event (T *= 1 - hitAlpha follows: the same float32 product)
                    if (cross.id == GRT_PICK_NONE && T * (1.0f - hitAlpha) <= cross_T) cross = e;
                }
            },
            [](const MeshSeg&, float, float) {});
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
    if (int rc = check_step_range(c, out->step_first, out->step_last, fn)) return rc;
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced and its elements "none")
    grt_ray_picks_mesh k = *out;
    StepRange r(out->step_first, out->step_last);
    void* args[3] = {const_cast<RenderArgs*>(&a), &k, &r};
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
