// grt_render_tile_quad.hip — the tile kernel's quad mode (grt_tile.h MODE 3: one 4x4 quadrant of a heavy tile per wave, lanes =
// rays x slots): 4 instantiations, compiled for 3 waves per SIMD (the exact test holds its particle's record per lane), and
// launch_render_tile_quad.  See the note at `constexpr bool QUAD` in grt_tile.h, and launch_render_tile (grt_render_tile.hip) for
// why this kernel is dispatched first on the frame's stream.
#include "grt_tile.h"

namespace grt {

int launch_render_tile_quad(const RenderArgs& a, bool count, hipStream_t stream, std::string* err)
{
    if (!a.qparts || !a.qpart_count) return GRT_OK;
    const bool sh = a.p.sh_degree_max > 0;
    TileKernel k = count ? (sh ? k_render_tile<true, true, false, 3, false> : k_render_tile<true, false, false, 3, false>)
                         : (sh ? k_render_tile<false, true, false, 3, false> : k_render_tile<false, false, false, 3, false>);
    // (one wave per entry of the list when the host knows its length, else per entry it can hold: the waves past its end exit at once)
    return tile_launch(k, a.quad_known ? a.quad_known - 1u : kQuadListCap, stream, a, "k_render_tile (quad parts)", err);
}

} // namespace grt
