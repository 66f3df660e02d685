// grt_stats.hip — per-particle contribution statistics of a Gaussian-only frame (include/grt.h: grt_particle_stats_frame /
// grt_particle_stats_rays): for every particle the sum and the peak of its compositing weights T_i alpha_i and the
// number of its composited events, over the rays of a window or of a ray buffer.
//
// k_particle_stats<MERGE> is ONE sweep_events call (grt_bwd.h) without colour: lane_ray gives the ray, one ray per lane, an 8x8 tile
// per wave, every lane of the wave in step.  Per slot of the k-buffers the wave scatters (stats_scatter, grt_stats.h: shared with the
// mesh frames' unit grt_stats_mesh.hip) through wave_groups as scatter<MERGE>
// does: of the lanes that hold the same particle the group's count is its size, its sum wave_sum, its peak wave_max (grt_wave.h), and
// its leader issues one atomic per requested output; a lane alone with its particle issues its own.  MERGE = false
// (GRT_OPT_BWD_PLAIN_ATOMICS = 1): every lane issues its own.  The atomics go straight into the caller's arrays: float add,
// unsigned max on the bit pattern of a non-negative float, unsigned add.  The context owns no buffer for this.
#include <string>

#include "grt_bwd.h"
#include "grt_stats.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "k_particle_stats runs gps_round (grt_kround.h): its per-lane stack stride is the launch block size");

template <bool MERGE>
__global__ __launch_bounds__(kBlock) void k_particle_stats(const RenderArgs a, const StatsArgs s)
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
    float wr = 1.0f;
    if (live && s.ray_weight) {
        wr = s.ray_weight[idx];
        live = wr != 0.0f; // a ray of weight exactly 0 is not traced
    }
    if (!__builtin_amdgcn_ballot_w64(live)) return; // wave-uniform

    // one sweep over the composited events (sweep_events: the scatter is wave-cooperative, a finished lane idles)
    float T = 1.0f;
    sweep_events(a, stk, o, d, mk_rayinv(o, d), a.p.t_max, live, T, [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t) {
        float w = 0.0f;
        if (ev) w = Tb * hitAlpha; // Tb: the transmittance before the event
        stats_scatter<MERGE, false>(s, ev, id, wr * w, w, 0.0f, 0.0f, lane);
    });
}

} // namespace
} // namespace grt

using namespace grt;

// what both entry points refuse before they look at their rays: the backward's refusals in the entry point's name, a scene with meshes in this unit's words
static int fill(grt_ctx* c, const grt_params* p, RenderArgs* a, const char* fn)
{
    return bwd_fill_args(c, p, false, a, fn, "particle statistics are computed for Gaussian-only frames");
}

static int launch(grt_ctx* c, const RenderArgs& a, const float* d_ray_weight, const grt_particle_stats* out, void* stream, const char* fn)
{
    if (!out || (!out->weight_sum && !out->weight_max && !out->count)) {
        c->err = std::string(fn) + ": no output (weight_sum, weight_max and count are all NULL)";
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
    sa.colour_sum = sa.colour_max = nullptr; // (mesh frames: grt_stats_mesh.hip)
    const void* fnk = c->opt_bwd_plain ? reinterpret_cast<const void*>(k_particle_stats<false>) : reinterpret_cast<const void*>(k_particle_stats<true>);
    void* args[2] = {const_cast<RenderArgs*>(&a), &sa};
    int rc = lane_launch(c, a, fnk, args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

extern "C" {

int grt_particle_stats_frame(grt_ctx* c, const grt_params* p, const float* d_ray_weight, const grt_particle_stats* out, uint32_t x0, uint32_t y0,
                             uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_particle_stats_frame";
    RenderArgs a;
    int rc = fill(c, p, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, a, d_ray_weight, out, stream, fn);
}

int grt_particle_stats_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_ray_weight, const grt_particle_stats* out,
                            void* stream)
{
    const char* fn = "grt_particle_stats_rays";
    RenderArgs a;
    int rc = fill(c, p, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, a, d_ray_weight, out, stream, fn);
}

} // extern "C"
