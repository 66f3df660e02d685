// grt_stats_mesh.hip — per-particle contribution statistics of a mesh frame (include/grt.h: grt_particle_stats_mesh_frame /
// grt_particle_stats_mesh_rays): what grt_stats.hip computes for a Gaussian-only frame, for rays that bounce off
// mirror, glass or normal-shaded meshes.  A ray has ONE event list with ONE running transmittance, cut into the segments of its
// iterations; every composited event i of segment s has the weight w_i = T_i alpha_i and the colour weight cw_i = c_s w_i with which its
// radiance enters the pixel (c_s: 1 - A_{s-1} of a Gaussian pass, D_S (1 - B_{S-1}) of the last pass, 1 of a terminating hit).
//
// k_particle_stats_mesh<MERGE, COLOUR>: one ray per lane, an 8x8 tile or 64 buffer rays per wave, on mesh_walk (grt_mesh_walk.h: the
// raygen loop, its convergence contract and why it cannot hang).  Per slot of the k-buffers the wave scatters through stats_scatter
// (grt_stats.h: DPP, v_readlane — it sits in on_slot, which the whole wave reaches).
//   COLOUR = false  (neither colour output asked for): ONE sweep.
//   COLOUR = true   the last pass's c_S needs D_S, known only at the end of that segment: the walk runs twice, as k_backward_mesh's
//                   does.  Sweep 0 scatters nothing and keeps D_fin, sweep 1 scatters.
// The step filter (step_first, step_last) is a per-lane predicate on the iteration's number: it clears `ev` before the scatter and
// changes no control flow — T, A and B run through the events it leaves out.
#include <string>

#include "grt_mesh_walk.h"
#include "grt_stats.h"

namespace grt {
namespace {

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

    float D_fin = 0.0f; // sweep 0: the density behind the ray's last iteration
#pragma unroll 1
    for (int pass = COLOUR ? 0 : 1; pass < 2; pass++) {
        // the segment's colour weight c_s, and whether the step filter counts the segment
        float c_s = 0.0f;
        bool counted = false;
        const float D = mesh_walk(
            a, stk, o, d, live,
            [&](const MeshSeg& g) {
                if (COLOUR && pass) c_s = seg_weight(g.state, g.A, g.B, D_fin);
                counted = r.counted(g.step);
            },
            [&](const MeshSeg&, bool hit, uint32_t id, float T, float hitAlpha, uint64_t) {
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
            },
            [](const MeshSeg&, float, float) {});
        if (pass == 0) D_fin = D;
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
    if (int rc = check_step_range(c, out->step_first, out->step_last, fn)) return rc;
    const grt_ctx* sc = scene_of(c);
    // no ray, no particle or an empty tree: nothing is composited, nothing is written
    if (a.n_blocks == 0 || sc->n == 0 || sc->gbvh.root_ref == kNoRoot) { c->have_timing = false; return GRT_OK; }
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    StatsArgs sa;
    sa.ray_weight = d_ray_weight;
    sa.weight_sum = out->weight_sum; sa.weight_max = out->weight_max; sa.count = out->count;
    sa.colour_sum = out->colour_sum; sa.colour_max = out->colour_max;
    StepRange sr(out->step_first, out->step_last);
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
