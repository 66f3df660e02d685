// grt_render_tile_single.hip — the tile kernel's one-ray-per-wave mode (grt_tile.h MODE 2: the rays of mesh frames whose bundle
// gave up, and the retry queue of k_bounce): 8 instantiations and launch_render_tile_single.  The mode is compiled with an 8-key
// window: its LDS per wave is 14 KB instead of 19 KB (the window's payload cells carry the events' radiance there) and it fits 168
// VGPRs, so 11 waves per CU are resident instead of 8.  The mode waits on memory for 46 % of its wave cycles
// (profiles/r03_C4_counters.json): C4 3.98 -> 3.82 ms.  The camera-ray and bundle kernels keep 12 keys (with 8 they lose 4-10 %).
#define GRT_TILE_KS 8
#define GRT_TILE_WAVES2 3
#include "grt_tile.h"

// the resident grid that draws from the heavy list: 256 CUs x 11 waves (profiles/tools/mkvar_single.sh builds variants with -D)
#ifndef GRT_TILE_GRID2
#define GRT_TILE_GRID2 2816u
#endif

namespace grt {

static TileKernel pick_single(bool count, bool sh, bool pieces)
{
#define GRT_PICK2(C, S) (pieces ? k_render_tile<C, S, true, 2, true> : k_render_tile<C, S, true, 2, false>)
    return count ? (sh ? GRT_PICK2(true, true) : GRT_PICK2(true, false)) : (sh ? GRT_PICK2(false, true) : GRT_PICK2(false, false));
#undef GRT_PICK2
}

int launch_render_tile_single(const RenderArgs& a, bool count, hipStream_t stream, std::string* err)
{
    const bool sh = a.p.sh_degree_max > 0;
    return tile_launch(pick_single(count, sh, a.has_pieces != 0u), GRT_TILE_GRID2, stream, a, "k_render_tile (one ray per wave)", err);
}

} // namespace grt
