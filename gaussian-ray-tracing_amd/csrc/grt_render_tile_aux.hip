// grt_render_tile_aux.hip — the tile kernel's camera-ray mode for aux frames (grt_render_aux: per-pixel alpha, expected depth and
// hit count beside colour): the head k_render_tile_aux<SH, PIECES> of grt_tile.h (MODE 0, no meshes, no counters: 4 instantiations),
// the aux pointers as a second kernel argument so that RenderArgs — and with it every other kernel's code — stays as it is, and
// launch_render_tile_aux.  Definitions: include/grt.h (grt_aux_out), DESIGN.md 5.7.
#define GRT_TILE_AUX 1
#include "grt_tile.h"

namespace grt {

// What launch_render_tile runs for mode 0 without meshes, plus per-pixel alpha / depth / count.  The four-way parts of heavy tiles
// run as part waves of this kernel (no quad kernel beside it: as with GRT_OPT_QUAD_PARTS = 0, the same pixels).
int launch_render_tile_aux(const RenderArgs& a, const AuxOut& x, hipStream_t stream, std::string* err)
{
    if (a.n_blocks == 0) return GRT_OK;
    if (const int r = tile_layout_check(a, true, err)) return r;
    if (a.mode != 0 || a.mroot != kNoRoot || a.counters) {
        if (err) *err = "tile aux kernel: camera-ray windows without meshes or counters only";
        return GRT_ERR_INVALID;
    }
    const bool sh = a.p.sh_degree_max > 0, pieces = a.has_pieces != 0u;
    RenderArgs b = a;
    b.quad_parts = 0u;
    void (*k)(const RenderArgs, const AuxOut) = sh ? (pieces ? k_render_tile_aux<true, true> : k_render_tile_aux<true, false>)
                                                   : (pieces ? k_render_tile_aux<false, true> : k_render_tile_aux<false, false>);
    const uint32_t grid = (a.order && a.n_launch) ? a.n_launch : a.n_blocks * 4u;
    return tile_launch(k, grid, stream, b, "k_render_tile_aux", err, x);
}

} // namespace grt
