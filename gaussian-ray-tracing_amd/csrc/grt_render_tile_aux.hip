// grt_render_tile_aux.hip — the tile kernel's camera-ray mode for aux frames (grt_render_aux: per-pixel alpha, expected depth
// and hit count beside colour) as a translation unit of its own: the same source as grt_render_tile.hip, its kernel named
// k_render_tile_aux<SH, PIECES> (MODE 0, no meshes, no counters: four instantiations), the aux pointers as a second kernel
// argument so that RenderArgs — and with it every other kernel's code — stays as it is.  Definitions: include/grt.h
// (grt_aux_out), DESIGN.md 5.7.
#define GRT_TILE_AUX_TU 1
// the ray's first (here: only) Gaussian segment: sum of (T_i alpha_i) t_i and the number of its terms, over the events that
// change T (alpha_min < alpha, repeats of a split particle dropped: the compositing step's own condition).  The expression,
// evaluated before T is updated, is the per-lane kernel's (grt_render.hip: trace_gaussians), term by term: the same bits.
#define GRT_AUX_DECL                                                                                       \
    float aux_depth = 0.0f;                                                                                \
    uint32_t aux_count = 0u;
#define GRT_AUX_EVENT(t, T_, ea_)                                                                          \
    {                                                                                                      \
        aux_depth += ((T_) * (ea_)) * (t);                                                                 \
        aux_count++;                                                                                       \
    }
// alpha: accumAlpha of the raygen loop, clamp(0 + (1 - T), 0, 1) for a frame without meshes (shaders/tracer.cu:81,
// shaders/tracer.cuh:372); a pixel without a ray (fisheye r > 1) gets 0, 0, 0
#define GRT_AUX_WRITE(idx, have_, dens_)                                                                   \
    {                                                                                                      \
        if (ax.alpha) ax.alpha[idx] = (have_) ? clampf(0.0f + (dens_), 0.0f, 1.0f) : 0.0f;                 \
        if (ax.depth) ax.depth[idx] = aux_depth;                                                           \
        if (ax.count) ax.count[idx] = aux_count;                                                           \
    }
#include "grt_render_tile.hip"
