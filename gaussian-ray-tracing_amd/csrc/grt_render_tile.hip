// grt_render_tile.hip — the tile kernel's camera-ray and bundle modes (grt_tile.h: MODE 0, with or without the mesh pipeline, and
// MODE 1), 12 keys per window, 4 waves per SIMD: 24 instantiations, and launch_render_tile, the entry of every mode but the aux
// frames'.  The other modes are units of their own (grt_render_tile_single.hip, grt_render_tile_quad.hip,
// grt_render_tile_aux.hip), each compiled for the occupancy it needs.
#include "grt_tile.h"

namespace grt {

static TileKernel pick_tile(bool count, bool sh, bool mesh, int mode, bool pieces)
{
#define GRT_PICK3(C, S, P)                                                                                 \
    (mode == 1 ? k_render_tile<C, S, true, 1, P> : (mesh ? k_render_tile<C, S, true, 0, P> : k_render_tile<C, S, false, 0, P>))
#define GRT_PICK2(C, S) (pieces ? GRT_PICK3(C, S, true) : GRT_PICK3(C, S, false))
    return count ? (sh ? GRT_PICK2(true, true) : GRT_PICK2(true, false)) : (sh ? GRT_PICK2(false, true) : GRT_PICK2(false, false));
#undef GRT_PICK2
#undef GRT_PICK3
}

// mode 0: camera rays (mesh = stage 2 of the wavefront pipeline: up to their mesh hit); mode 1: stage 3, one wave per
// chunk of a.queue_in (grid = the most chunks there can be: one per 8x8 tile of the launch); mode 2: one wave per ray of
// the heavy list, a resident grid drawing from it (grt_render_tile_single.hip)
int launch_render_tile(const RenderArgs& a, bool count, bool mesh, int mode, hipStream_t stream, std::string* err, const LaunchAux* aux)
{
    if (a.n_blocks == 0) return GRT_OK;
    if (const int r = tile_layout_check(a, mode == 0, err)) return r;
    if (mode != 0 && (!a.queue_in || !a.qcount_in || !a.prec || !a.queue || !a.qcount || (!a.heavy && mode == 1) || !a.hcount || !a.fqueue ||
                      !a.fcount || !a.hnext)) {
        if (err) *err = "tile kernel: continuation queues missing";
        return GRT_ERR_INVALID;
    }
    if (mode == 2) return launch_render_tile_single(a, count, stream, err);
    const bool sh = a.p.sh_degree_max > 0;
    RenderArgs b = a;
    b.heavy_role = 0;
    // mode 0: one wave per entry of the launch order (tiles + the parts of split tiles, padded) or per tile; mode 1: one wave per
    // chunk the queue can hold (launch_render passes it as n_launch)
    const uint32_t grid = ((mode == 1 || a.order) && a.n_launch) ? a.n_launch : a.n_blocks * 4u;
    // The four-way parts of heavy tiles run on the quad kernel BESIDE this launch (camera rays without meshes or pieces).  The quad
    // kernel goes on the frame's own stream, this kernel on the second one behind a fork event: the parts are the frame's longest waves
    // and must be dispatched FIRST — launched the other way round (or with the second stream at high priority) they found the machine
    // already full of this kernel's waves and waited 0.2-0.4 ms for registers (a 720p frame: 0.76 -> 0.9-1.0 ms).
    const bool quad = mode == 0 && !mesh && a.quad_parts && a.order && a.n_launch && a.qparts && a.qpart_count && aux && aux->aux && aux->fork && aux->join;
    b.quad_parts = quad ? 1u : 0u;
    hipStream_t main_stream = stream;
    if (quad) {
        hipError_t eq = hipEventRecord(aux->fork, stream);
        if (eq == hipSuccess) eq = hipStreamWaitEvent(aux->aux, aux->fork, 0);
        if (eq != hipSuccess) {
            if (err) *err = std::string("tile kernel: fork to the second stream: ") + hipGetErrorString(eq);
            return GRT_ERR_HIP;
        }
        const int rq = launch_render_tile_quad(b, count, stream, err);
        if (rq != GRT_OK) return rq;
        main_stream = aux->aux;
    }
    // (not tile_launch: the join stands between this launch and the look at its status)
    hipLaunchKernelGGL(pick_tile(count, sh, mesh || mode != 0, mode, a.has_pieces != 0u), dim3(grid), dim3(kWG), 0, main_stream, b);
    if (quad) {
        hipError_t eq = hipEventRecord(aux->join, aux->aux);
        if (eq == hipSuccess) eq = hipStreamWaitEvent(stream, aux->join, 0);
        if (eq != hipSuccess) {
            if (err) *err = std::string("tile kernel: join of the second stream: ") + hipGetErrorString(eq);
            return GRT_ERR_HIP;
        }
    }
    return tile_launch_status("k_render_tile", err);
}

} // namespace grt
