// grt_picks.hip — per-ray picks of a Gaussian-only frame (include/grt.h: grt_ray_picks_frame / grt_ray_picks_rays):
// for every ray of a window or of a ray buffer the FIRST composited event, the event of largest compositing weight T_i alpha_i (PEAK)
// and the first event behind which the transmittance has fallen to cross_T (CROSS; 0.5: the median depth), each as the particle's
// original id, the event's key distance and its weight.
//
// k_ray_picks is ONE sweep_events call (grt_bwd.h) as k_particle_stats is: lane_ray gives the ray, one ray per lane, an 8x8 tile per
// wave.  The picks are selections among the lane's own events: nine registers per lane, no wave operation, no atomic; at the end every
// lane that owns an element of the window or of the buffer stores the requested ones by plain vector stores — "none" for a ray that
// was not traced or met no such event.  A NULL output is a wave-uniform branch on a kernel argument.  The context owns no buffer for this.
#include <string>

#include "grt_bwd.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "k_ray_picks runs gps_round (grt_kround.h): its per-lane stack stride is the launch block size");

// one rule's pick, in registers
struct Pick {
    uint32_t id;
    float t, w;
};

__device__ __forceinline__ void pick_store(const grt_pick_out& out, size_t idx, const Pick& k)
{
    if (out.id) out.id[idx] = k.id;
    if (out.t) out.t[idx] = k.t;
    if (out.weight) out.weight[idx] = k.w;
}

__global__ __launch_bounds__(kBlock) void k_ray_picks(const RenderArgs a, const grt_ray_picks k)
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
    const Pick none = {GRT_PICK_NONE, 0.0f, 0.0f};
    Pick first = none, peak = none, cross = none;

    if (__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        const float cross_T = k.cross_T;
        float T = 1.0f;
        sweep_events(a, stk, o, d, mk_rayinv(o, d), a.p.t_max, live, T, [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t key) {
            if (ev) {
                const Pick e = {id, key_t(key), Tb * hitAlpha}; // Tb: the transmittance before the event
                if (first.id == GRT_PICK_NONE) first = e;
                if (peak.id == GRT_PICK_NONE || e.w > peak.w) peak = e; // strictly greater: the earliest event wins a tie
                // the sweep's own T behind the event (T *= 1 - hitAlpha follows this call: the same float32 product)
                if (cross.id == GRT_PICK_NONE && Tb * (1.0f - hitAlpha) <= cross_T) cross = e;
            }
        });
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

// what both entry points refuse before they look at their rays: the backward's refusals in the entry point's name, a scene with meshes in this unit's words
static int fill(grt_ctx* c, const grt_params* p, RenderArgs* a, const char* fn)
{
    return bwd_fill_args(c, p, false, a, fn, "ray picks are computed for Gaussian-only frames");
}

static bool wanted(const grt_pick_out& o) { return o.id || o.t || o.weight; }

static int launch(grt_ctx* c, const RenderArgs& a, const grt_ray_picks* out, void* stream, const char* fn)
{
    if (!out || (!wanted(out->first) && !wanted(out->peak) && !wanted(out->cross))) {
        c->err = std::string(fn) + ": no output (id, t and weight of first, peak and cross are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (wanted(out->cross) && !(out->cross_T > 0.0f && out->cross_T < 1.0f)) { // (NaN fails both comparisons)
        c->err = std::string(fn) + ": cross_T must lie in (0, 1), not " + std::to_string(out->cross_T);
        return GRT_ERR_INVALID;
    }
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced and its elements "none")
    grt_ray_picks k = *out;
    void* args[2] = {const_cast<RenderArgs*>(&a), &k};
    int rc = lane_launch(c, a, reinterpret_cast<const void*>(k_ray_picks), args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

extern "C" {

int grt_ray_picks_frame(grt_ctx* c, const grt_params* p, const grt_ray_picks* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_ray_picks_frame";
    RenderArgs a;
    int rc = fill(c, p, &a, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, a, out, stream, fn);
}

int grt_ray_picks_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const grt_ray_picks* out, void* stream)
{
    const char* fn = "grt_ray_picks_rays";
    RenderArgs a;
    int rc = fill(c, p, &a, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch(c, a, out, stream, fn);
}

} // extern "C"
