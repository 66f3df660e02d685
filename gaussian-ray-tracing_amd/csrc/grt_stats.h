// grt_stats.h — the scatter the two statistics units share (grt_stats.hip: k_particle_stats, Gaussian-only frames, DESIGN.md 5.12;
// grt_stats_mesh.hip: k_particle_stats_mesh, mesh frames): the kernels' output arguments, one atomic per requested
// output, and the wave merge of the lanes that hold the same particle in the same slot of their k-buffers.
//
// COLOUR: the two colour outputs of a mesh frame (colour_sum, colour_max) are in the text at all.  k_particle_stats instantiates
// COLOUR = false: its text is what it was when this header was part of grt_stats.hip, instruction for instruction.
#pragma once

#include "grt_bwd.h"

namespace grt {
namespace {

struct StatsArgs {
    const float* ray_weight; // [pixels or rays] or null (= 1)
    float* weight_sum;       // [n] by original id, or null
    float* weight_max;       // [n] or null
    uint32_t* count;         // [n] or null
    float* colour_sum;       // [n] or null (mesh frames; COLOUR)
    float* colour_max;       // [n] or null (mesh frames; COLOUR)
};

// one atomic per requested output (the branches are wave-uniform: kernel arguments)
template <bool COLOUR>
__device__ __forceinline__ void stats_add(const StatsArgs& s, uint32_t id, float sum, float peak, uint32_t n, float csum, float cpeak)
{
    if (s.weight_sum) atomicAdd(s.weight_sum + id, sum);
    if (s.weight_max) atomicMax(reinterpret_cast<unsigned int*>(s.weight_max) + id, __float_as_uint(peak)); // (peak >= 0: its bits order as it does)
    if (s.count) atomicAdd(s.count + id, n);
    if constexpr (COLOUR) {
        if (s.colour_sum) atomicAdd(s.colour_sum + id, csum);
        if (s.colour_max) atomicMax(reinterpret_cast<unsigned int*>(s.colour_max) + id, __float_as_uint(cpeak)); // (cpeak >= 0)
    }
}

// Called by the WHOLE wave (ev: this lane has an event of particle id with weight w = T alpha; ws = w_ray * w; COLOUR: its colour
// weight cw = c_s w and cs = w_ray * cw).
template <bool MERGE, bool COLOUR>
__device__ __forceinline__ void stats_scatter(const StatsArgs& s, bool ev, uint32_t id, float ws, float w, float cs, float cw, uint32_t lane)
{
    if (!MERGE) {
        if (ev) stats_add<COLOUR>(s, id, ws, w, 1u, cs, cw);
        return;
    }
    const bool solo = wave_groups(ev, id, [&](uint32_t lid, bool mine, uint32_t n, uint32_t leader) {
        float sum = 0.0f, peak = 0.0f, csum = 0.0f, cpeak = 0.0f;
        if (s.weight_sum) sum = wave_sum(mine ? ws : 0.0f);
        if (s.weight_max) peak = wave_max(mine ? w : 0.0f);
        if constexpr (COLOUR) {
            if (s.colour_sum) csum = wave_sum(mine ? cs : 0.0f);
            if (s.colour_max) cpeak = wave_max(mine ? cw : 0.0f);
        }
        if (lane == leader) stats_add<COLOUR>(s, lid, sum, peak, n, csum, cpeak);
    });
    if (solo) stats_add<COLOUR>(s, id, ws, w, 1u, cs, cw);
}

} // namespace
} // namespace grt
