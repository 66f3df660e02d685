// grt_frame.hip — the frame slot's unit: what lies between a render entry point of include/grt.h and launch_render (grt_render.hip), and
// the work queued behind a frame.  The slot's kernels, the arguments every frame shares, the work mappings, the scheduling feedback, the
// overflow pool, do_launch as a list of stages, the render entry points, the synchronising calls.
// Context and options: grt_api.hip; the scene: grt_scene.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "grt_device.h"
#include "grt_internal.h"

using namespace grt;

// ---- kernels of the frame slot ----

// Eye records: everything in the proxy test that depends on the ray ORIGIN only.  Camera rays share one origin,
// so the streaming kernel reads these (wave-uniform, scalar loads) instead of recomputing them on every lane:
//   (o_g.x o_g.y o_g.z cc)      o_g = A (eye - mu), cc = |o_g|^2 - R^2 of the pre-test sphere
// — each by the very operation sequence the kernels use per lane (grt_device.h), so results are bit-identical.
// Rebuilt only when the eye moves or the records change: one pass over the particles (~20 us per million).
__global__ void k_eye_records(const float4* __restrict__ rec, uint32_t m, float ex, float ey, float ez,
                              float4* __restrict__ erec)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const float4 r0 = rec[(size_t)j * 4], r1 = rec[(size_t)j * 4 + 1], r2 = rec[(size_t)j * 4 + 2],
                 r3 = rec[(size_t)j * 4 + 3];
    m33 A;
    A.a[0] = r1.x; A.a[1] = r1.y; A.a[2] = r1.z;
    A.a[3] = r2.x; A.a[4] = r2.y; A.a[5] = r2.z;
    A.a[6] = r3.x; A.a[7] = r3.y; A.a[8] = r3.z;
    const f3 o_g = matvec(A, sub3(mk3(ex, ey, ez), mk3(r0.x, r0.y, r0.z)));
    erec[j] = make_float4(o_g.x, o_g.y, o_g.z, proxy_sphere_cc(o_g, r0.w));
}

// Wide eye records for the tile kernel, 64 B: the same (o_g, cc) plus the ten slab projections of o_g
// (slab_project, grt_device.h) that the exact proxy test otherwise forms on every lane from wave-uniform inputs:
//   (o_g.x o_g.y o_g.z cc) (a0 a1 a2 a3) (a4 a5 a6 a7) (a8 a9 cc_a 0)
// cc_a = |o_g|^2 - R_a^2 of the alpha sphere (proxy_alpha_sphere_cc): the pre-test value of the uncounted instantiations, which skip
// the particles no ray of the tile can see above alpha_min; counted frames read cc.  alpha_sphere = 0: the frame's alpha_min lies below
// the one the proxies were sized with, the insphere is then not the frame's alpha sphere, and cc_a = cc.
__global__ void k_eye_records_wide(const float4* __restrict__ rec, uint32_t m, float ex, float ey, float ez, uint32_t alpha_sphere,
                                   float4* __restrict__ erec)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const float4 r0 = rec[(size_t)j * 4], r1 = rec[(size_t)j * 4 + 1], r2 = rec[(size_t)j * 4 + 2],
                 r3 = rec[(size_t)j * 4 + 3];
    m33 A;
    A.a[0] = r1.x; A.a[1] = r1.y; A.a[2] = r1.z;
    A.a[3] = r2.x; A.a[4] = r2.y; A.a[5] = r2.z;
    A.a[6] = r3.x; A.a[7] = r3.y; A.a[8] = r3.z;
    const f3 o_g = matvec(A, sub3(mk3(ex, ey, ez), mk3(r0.x, r0.y, r0.z)));
    float pa[10];
    slab_project(o_g, pa);
    float4* e = erec + (size_t)j * 4;
    const float cc = proxy_sphere_cc(o_g, r0.w);
    e[0] = make_float4(o_g.x, o_g.y, o_g.z, cc);
    e[1] = make_float4(pa[0], pa[1], pa[2], pa[3]);
    e[2] = make_float4(pa[4], pa[5], pa[6], pa[7]);
    e[3] = make_float4(pa[8], pa[9], alpha_sphere ? proxy_alpha_sphere_cc(o_g, r0.w) : cc, 0.0f);
}

// Cold-start scheduling estimate: how many particle centres project into each 8x8 tile (scheduling unit).  Used ONLY to
// order the launch of a frame that has no previous-frame costs (first frame, camera cut, new size): dense tiles first.
// The projection inverts getRay / getFishEyeRay (shaders/tracer.cuh:115-165) for a point instead of a pixel; it never
// touches a pixel value.
// the pixel a world point projects to (the inverse of getRay / getFishEyeRay, shaders/tracer.cuh:115-165); false: behind the camera,
// outside the fisheye circle or outside the image
__device__ __forceinline__ bool project_point(const grt_params& p, f3 x, float& fx, float& fy)
{
    const f3 v = sub3(x, mk3(p.eye[0], p.eye[1], p.eye[2]));
    const f3 U = mk3(p.U[0], p.U[1], p.U[2]), V = mk3(p.V[0], p.V[1], p.V[2]), W = mk3(p.W[0], p.W[1], p.W[2]);
    // components of v in the (-U, -V, W) basis the ray generators use (the three are mutually orthogonal)
    const float su = -dot3(v, U) / fmaxf(dot3(U, U), 1e-30f), sv = -dot3(v, V) / fmaxf(dot3(V, V), 1e-30f),
                sw = dot3(v, W) / fmaxf(dot3(W, W), 1e-30f);
    float dx, dy;
    if (!p.mode_fisheye) {
        if (!(sw > 1e-6f)) return false; // behind the camera
        dx = su / sw; dy = sv / sw;
    } else {
        const float len = sqrtf(su * su + sv * sv + sw * sw);
        if (!(len > 0.0f)) return false;
        const float ct = fminf(fmaxf(sw / len, -1.0f), 1.0f);
        const float r = sqrtf(2.0f) * sqrtf(fmaxf(0.5f * (1.0f - ct), 0.0f)); // sqrt(2) sin(theta / 2)
        const float rho = sqrtf(su * su + sv * sv);
        if (!(r <= 1.0f) || !(rho > 0.0f)) return false;
        dx = r * su / rho; dy = r * sv / rho;
    }
    fx = (dx + 1.0f) * 0.5f * (float)p.width; fy = (dy + 1.0f) * 0.5f * (float)p.height;
    return fx >= 0.0f && fy >= 0.0f && fx < (float)p.width && fy < (float)p.height;
}

__global__ void k_estimate_costs(const float* __restrict__ pos, uint32_t n, uint32_t stride, const RenderArgs a,
                                 uint32_t* __restrict__ cost)
{
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) * stride; // a sample of the particles is enough for an ORDER
    if (i >= n) return;
    float fx, fy;
    if (!project_point(a.p, mk3(pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]), fx, fy)) return;
    const uint32_t px = (uint32_t)fx, py = (uint32_t)fy;
    uint32_t blk, lx, ly;
    if (a.mode == 0) {
        if (px < a.x0 || py < a.y0 || px >= a.x1 || py >= a.y1) return;
        lx = px - a.x0; ly = py - a.y0;
        blk = (ly / 16u) * a.nbx + lx / 16u;
    } else {
        const uint32_t tile = (py / a.tile_h) * a.tiles_x + px / a.tile_w;
        if (tile < a.first_tile || (tile - a.first_tile) % a.tile_stride) return;
        const uint32_t j = (tile - a.first_tile) / a.tile_stride;
        if (j >= a.n_tiles) return;
        lx = px % a.tile_w; ly = py % a.tile_h;
        blk = j * (a.nbx * a.nby) + (ly / 16u) * a.nbx + lx / 16u;
    }
    atomicAdd(&cost[blk * 4u + (((ly % 16u) / 8u) << 1) + ((lx % 16u) / 8u)], 1u);
}

// The tile kernel's give-up reasons travel in the per-tile cost words (see the watchdog in grt_tile.h): a cost
// above the step watchdog = the watchdog fired, high bits = stack guard / two passes without progress.  One pass over
// the costs right behind the frame ORs them into the context's sticky error word.
// behind every frame (do_launch): error word and overflow demand to their pinned host words, overflow counter reset
// (d_ovf_next[0] = chunks this frame asked for, [1] = the largest demand since the host last took one: the pinned word is written
//  only when the host is not waiting for an earlier value — h_ovf_used == nullptr otherwise — so a peak between two reads is kept)
__global__ void k_frame_tail(const uint32_t* __restrict__ d_err, uint32_t* __restrict__ h_err, uint32_t* __restrict__ d_ovf_next,
                             uint32_t* __restrict__ h_ovf_used, const uint32_t* __restrict__ d_qpcount, uint32_t* __restrict__ h_qpcount)
{
    *h_err = *d_err;
    if (d_qpcount) *h_qpcount = d_qpcount[0]; // how many four-way parts the quad kernel's list holds (a launch that knows it is none skips that kernel)
    if (d_ovf_next) {
        const uint32_t peak = max(d_ovf_next[1], d_ovf_next[0]);
        d_ovf_next[0] = 0u;
        d_ovf_next[1] = h_ovf_used ? 0u : peak;
        if (h_ovf_used) *h_ovf_used = peak;
    }
    __threadfence_system();
}

__global__ void k_check_costs(const uint32_t* __restrict__ cost, uint32_t n, uint32_t max_iters, uint32_t* __restrict__ err_word)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cost[i];
    uint32_t e = 0;
    if (c & kCostStackBit) e |= kErrStack;
    if (c & kCostStallBit) e |= kErrStall;
    if ((c & kCostStepsMask) > max_iters) e |= kErrWatchdog; // (bits 27-28: the tile ran as parts, grt_internal.h)
    if (e) atomicOr(err_word, e);
}

// ---- arguments and work mappings ----
static int fill_common(grt_ctx* c, const grt_params* p, RenderArgs* a)
{
    if (!c || !p) return GRT_ERR_INVALID;
    const grt_ctx* sc = scene_of(c);
    if (!sc->built) { c->err = "render: grt_build_bvh has not been called after the last upload"; return GRT_ERR_INVALID; }
    if (p->sh_degree_max > 3) { c->err = "render: sh_degree_max must be 0..3"; return GRT_ERR_INVALID; }
    if (p->type < 0 || p->type > 2) { c->err = "render: type must be MIRROR/NORMAL/GLASS"; return GRT_ERR_INVALID; }
    if (!(p->t_min > 0.0f)) { c->err = "render: t_min must be > 0"; return GRT_ERR_INVALID; }
    memset(a, 0, sizeof(*a));
    a->p = *p;
    a->rec = sc->d_rec;
    a->nodes = sc->gbvh.nodes;
    a->wnodes = sc->gbvh.wnodes;
    a->qnodes = sc->gbvh.qnodes;
    a->pbox = sc->gbvh.pbox;
    a->root_ref = sc->gbvh.root_ref;
    a->n_prox = sc->gbvh.n_prims;
    a->has_pieces = sc->has_pieces ? 1u : 0u; // set by the build that made pieces (not inferred from counts: build_lbvh drops NaN boxes)
    a->color0 = sc->d_color0;
    a->sh = sc->d_sh;
    a->mnodes = sc->mbvh.nodes;
    a->tri = sc->d_tri;
    a->mroot = sc->n_faces ? sc->mbvh.root_ref : kNoRoot;
    a->n_faces = sc->n_faces;
    a->faces = sc->d_faces;
    a->vnormals = sc->d_vnormals;
    a->counters = c->opt_counters ? c->d_counters : nullptr;
    a->swizzle_chunk = (uint32_t)c->opt_swizzle;
    a->err_word = c->d_err;
    a->max_iters = c->opt_max_iters > 0 ? (uint32_t)c->opt_max_iters : kTileMaxItersDefault;
    return GRT_OK;
}

// (grt_internal.h: also the backward and the statistics units' mappings)
int grt::set_window(grt_ctx* c, const grt_params* p, RenderArgs* a, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const char* fn)
{
    if (x1 > p->width || y1 > p->height || x0 > x1 || y0 > y1) { c->err = std::string(fn) + ": window outside the frame"; return GRT_ERR_INVALID; }
    a->mode = 0;
    a->x0 = x0; a->y0 = y0; a->x1 = x1; a->y1 = y1;
    a->nbx = (x1 - x0 + 15) / 16;
    a->nby = (y1 - y0 + 15) / 16;
    a->n_blocks = a->nbx * a->nby;
    return GRT_OK;
}

// the tile list of grt_render_tiles (has_out: the caller has somewhere to put the pixels; refused between the two geometry tests, where
// that entry point has always refused it)
static int set_tiles(grt_ctx* c, const grt_params* p, RenderArgs* a, uint32_t tile_w, uint32_t tile_h, uint32_t first_tile, uint32_t tile_stride,
                     uint32_t n_tiles, bool has_out, const char* fn)
{
    if (!tile_w || !tile_h || (tile_w % 16) || (tile_h % 16)) { c->err = std::string(fn) + ": tile size must be a multiple of 16"; return GRT_ERR_INVALID; }
    if (!has_out) { c->err = std::string(fn) + ": no output buffer"; return GRT_ERR_INVALID; }
    const uint32_t tiles_x = (p->width + tile_w - 1) / tile_w, tiles_y = (p->height + tile_h - 1) / tile_h;
    if (n_tiles && (!tile_stride || (uint64_t)first_tile + (uint64_t)(n_tiles - 1) * tile_stride >= (uint64_t)tiles_x * tiles_y)) {
        c->err = std::string(fn) + ": tile range outside the frame's tile grid";
        return GRT_ERR_INVALID;
    }
    a->mode = 1;
    a->tile_w = tile_w; a->tile_h = tile_h; a->first_tile = first_tile; a->tile_stride = tile_stride; a->n_tiles = n_tiles;
    a->tiles_x = tiles_x;
    a->nbx = tile_w / 16; a->nby = tile_h / 16;
    a->n_blocks = n_tiles * a->nbx * a->nby;
    return GRT_OK;
}

int grt::set_rays(grt_ctx* c, RenderArgs* a, const float* d_rays, uint64_t n, const char* fn)
{
    if (n && !d_rays) { c->err = std::string(fn) + ": null ray buffer"; return GRT_ERR_INVALID; }
    if (n > 0xFFFFFFFFull * 64) { c->err = std::string(fn) + ": too many rays"; return GRT_ERR_LIMIT; }
    a->mode = 2;
    a->rays = d_rays; a->n_rays = n;
    a->n_blocks = (uint32_t)((n + 255) / 256);
    return GRT_OK;
}

// ---- scheduling feedback ----

// Frame-to-frame scheduling feedback: every render records each 16x16 block's cost (the largest number of
// traversal iterations among its waves); the next render with the same frame geometry launches the blocks
// heaviest-first, so the long-running tiles (10x the mean on the benchmark scenes) no longer form the tail of the
// launch.  Pure scheduling: pixels do not depend on the order.  A viewer's consecutive frames are nearly identical,
// which is what makes last frame's cost a good predictor; the first frame (or any change of size / mode) runs in
// the default XCD-chunked order.

// launch entries beyond one per tile (the parts of split tiles): a quarter of the tiles — and, for a launch that does not fill the
// machine, whatever fills it (a 256^2 frame is 1024 tiles on 4096 wave slots, its tiles' costs lie close together, and with room for
// 106 split tiles the 107th, whole, bounded the frame)
static uint32_t parts_extra_cap(uint32_t n_units)
{
    const uint32_t base = n_units / 4u + 64u;
    return n_units < kTileResidentWaves ? std::max(base, std::min(3u * n_units, kTileResidentWaves - n_units)) : base;
}
// is a frame of another slot of this scene still running?  (its frame-end event, recorded on its stream behind its last kernels)
static bool sibling_frames_in_flight(const grt_ctx* c)
{
    grt_ctx* sc = const_cast<grt_ctx*>(scene_of(c));
    std::lock_guard<std::mutex> lk(sc->views_mu); // (views come and go on other threads: grt_create_view / grt_destroy take the same lock)
    if (sc->n_views == 0) return false;
    auto busy = [&](const grt_ctx* s) { return s != c && s->have_timing && s->ev1 && hipEventQuery(s->ev1) == hipErrorNotReady; };
    if (busy(sc)) return true;
    for (const grt_ctx* v : sc->views) if (busy(v)) return true;
    return false;
}
// four-way parts on the quad kernel: camera rays without meshes or pieces (that kernel has no mesh stage and no piece bookkeeping; such
// frames keep part waves of the camera-ray kernel)
// — and launches that the parts of their heaviest tiles BOUND: up to three times the machine's resident waves (measured,
// profiles/r05_experiments_log.md 4: a 256^2 frame, 1024 tiles, 0.46 -> 0.27 ms; a rank's share of a 1080p frame, 4050 / 8100 tiles,
// 0.77 -> 0.55 / 0.75 -> 0.61 ms; a 720p frame of 14 400 tiles is bound by its total work and loses 5 % to the second kernel).
// GRT_OPT_QUAD_PARTS = 2 forces it on whatever the size (tests).
static bool quad_parts_ok(const grt_ctx* c, uint32_t n_units)
{
    const grt_ctx* sc = scene_of(c);
    if (!c->opt_quad_parts || sc->n_faces || sc->has_pieces) return false;
    // (while frames of the scene's OTHER slots are in flight the machine is shared, the frames are bound by their total work and the quad
    //  kernel — a latency tool — only takes capacity: a rank of 8 with eight frames in flight 0.26 -> 0.33 ms per frame with it)
    return c->opt_quad_parts >= 2 || (n_units <= 3u * kTileResidentWaves && !sibling_frames_in_flight(c));
}
// the four-way threshold such launches use: parts on the quad kernel cost a third of what part waves of the camera-ray kernel cost, so
// more tiles are worth splitting the fewer tiles there are per resident wave — pct4 at two tiles per wave, half of it at one and below
static uint32_t quad_pct4_of(uint32_t p, uint32_t n_units) // (p: GRT_OPT_TILE_PARTS4_PCT)
{
    return std::min(p, std::max(p / 2u, (uint32_t)((uint64_t)p * n_units / (2u * kTileResidentWaves))));
}
static uint32_t quad_pct4(const grt_ctx* c, uint32_t n_units) { return quad_pct4_of((uint32_t)c->opt_tile_parts4_pct, n_units); }

// what a slot's costs, its order and its bundle verdicts belong to: the launch geometry, as six words
static void launch_geometry_sig(const RenderArgs& a, uint32_t n_units, uint64_t sig[6])
{
    const uint64_t g[6] = {a.mode | ((uint64_t)n_units << 8), a.n_blocks, ((uint64_t)a.p.width << 32) | a.p.height,
                           ((uint64_t)a.x0 << 48) ^ ((uint64_t)a.y0 << 32) ^ ((uint64_t)a.x1 << 16) ^ a.y1,
                           ((uint64_t)a.first_tile << 32) | a.tile_stride, ((uint64_t)a.tile_w << 32) | a.tile_h};
    memcpy(sig, g, sizeof(g));
}

// The launch order with the heaviest tiles as parts (n_units + parts_extra_cap entries) and, when `quad`, its four-way parts as a list for
// the quad kernel (one more small kernel behind the ordering).  cost_src orders the tiles, cost_raw holds their own cost words; pct2 / pct4:
// the two- and four-way thresholds; d_zero: see order_units_by_cost; bag_class: what the size classes are read from — 1 cost words, 2
// particle counts (every whole tile "not known": it starts in one chunk).
static int order_with_parts(grt_ctx* c, const uint32_t* cost_src, const uint32_t* cost_raw, uint32_t n_units, uint32_t pct2, uint32_t pct4,
                            uint32_t* d_zero, uint32_t bag_class, bool quad, hipStream_t s)
{
    const uint32_t cap = parts_extra_cap(n_units);
    int rc = order_units_with_parts(cost_src, cost_raw, c->d_order, n_units, cap, pct2, pct4, (uint32_t)c->opt_tile_parts_load_pct, kTileResidentWaves,
                                    d_zero, c->d_ord_scratch, (uint32_t)c->opt_order_multi_min, c->opt_ovf_classes ? bag_class : 0u, s, &c->err);
    c->order_classes = rc == GRT_OK && c->opt_ovf_classes != 0;
    if (rc != GRT_OK) return rc;
    c->order_launch = n_units + cap;
    c->qparts_valid = false;
    if (quad) {
        rc = quad_part_list(c->d_order, c->order_launch, c->d_qparts, c->d_qpcount, (uint32_t)c->opt_quad_parts > 2u ? (uint32_t)c->opt_quad_parts : kQuadListCap, s, &c->err);
        c->qparts_valid = rc == GRT_OK;
        c->qlist_epoch++;
    }
    return rc;
}

// this launch runs with the order in hand
static void launch_with_order(const grt_ctx* c, RenderArgs& a)
{
    a.order = c->d_order;
    a.n_launch = c->order_launch;
    if (c->order_split) a.n_heavy = c->d_n_heavy;
}

// launch order of the units from the costs the last frame left in d_cost (dilated for full-frame launches)
static int order_from_costs(grt_ctx* c, const RenderArgs& a, uint32_t n_units, hipStream_t s, bool* used_split, bool zero_costs = false)
{
    uint32_t* d_zero = zero_costs ? c->d_cost : nullptr; // (the ordering kernel zeroes the consumed costs itself: one packet less)
    const bool split = c->opt_heavy_split == 1 || (c->opt_heavy_split == 2 && a.n_blocks <= 3072u);
    const uint32_t* cost_src = c->d_cost;
    // (the dilation is for a camera that MOVES: a heavy tile of the last frame is a slightly different tile of the next.  When this
    //  frame ran with an order that was made for exactly this view — the camera stood still for two frames — the next order is made
    //  from the tiles' own costs: a dilated map orders a standing view worse, C2 0.86 -> 0.80 ms, C3 -1.3 %; if the camera then moves,
    //  one frame runs with an undilated order)
    //  (camera-ray frames without meshes: on C4 the undilated order costs 2 % — the stages behind the primary one take the tiles'
    //   continuation rays in the order the primary waves finish)
    const bool dilate = c->opt_cost_radius > 0 && !(c->launch_order_matched && c->opt_static_sharp && !scene_of(c)->n_faces);
    if (dilate && a.mode == 0 && n_units == a.n_blocks * 4u && !split) {
        int rcd = dilate_unit_costs(c->d_cost, c->d_cost_dil, a.nbx, a.nby, c->opt_cost_radius, s, &c->err);
        if (rcd != GRT_OK) return rcd;
        cost_src = c->d_cost_dil;
    }
    c->order_launch = 0;
    if (c->parts_ok && (c->opt_tile_parts2_pct > 0 || c->opt_tile_parts4_pct > 0) && n_units == a.n_blocks * 4u) {
        // tile kernel, camera rays, no meshes: the heaviest tiles of this frame run as 2 / 4 waves in the next one
        *used_split = false;
        const bool quad = quad_parts_ok(c, n_units) && c->d_qparts;
        return order_with_parts(c, cost_src, c->d_cost, n_units, (uint32_t)c->opt_tile_parts2_pct,
                                quad ? quad_pct4(c, n_units) : (uint32_t)c->opt_tile_parts4_pct, d_zero, 1u, quad, s);
    }
    *used_split = split;
    c->order_classes = false; // (entries of this order are bare unit numbers)
    return order_units_by_cost(cost_src, c->d_order, n_units, std::max(1u, n_units / (uint32_t)c->opt_heavy_cap_div),
                               (uint32_t)c->opt_heavy_thr_x2, split ? c->d_n_heavy : nullptr, d_zero, s, &c->err);
}

static int prepare_feedback(grt_ctx* c, RenderArgs& a, hipStream_t s, uint32_t n_units, bool need_cost)
{
    a.order = nullptr;
    a.n_launch = 0;
    a.cost = nullptr;
    a.n_heavy = nullptr;
    a.heavy_role = 0;
    a.n_units = n_units;
    if ((!c->opt_feedback && !need_cost) || n_units == 0) return GRT_OK;
    uint64_t sig[6];
    launch_geometry_sig(a, n_units, sig);
    if (c->cost_cap < n_units) {
        (void)hipFree(c->d_cost); (void)hipFree(c->d_order); (void)hipFree(c->d_cost_dil); (void)hipFree(c->d_qparts);
        c->d_cost = c->d_order = c->d_cost_dil = c->d_qparts = nullptr;
        c->qparts_valid = false;
        c->cost_cap = 0;
        c->cost_valid = false;
        CHK(c, hipMalloc(&c->d_cost, sizeof(uint32_t) * n_units));
        CHK(c, hipMalloc(&c->d_order, sizeof(uint32_t) * ((size_t)n_units + parts_extra_cap(n_units) + 4u))); // (+ 3 diagnostic words)
        // (every entry starts as padding: an entry the ordering kernels ever failed to write would make its wave exit instead of
        //  indexing costs, queues and pixels with whatever the allocation held — the likely cause of round 4's one unexplained abort,
        //  profiles/r05_experiments_log.md 1)
        // (on the FRAME'S stream, as everything below: a null-stream hipMemset is not ordered against a non-blocking stream and
        //  may land after the kernels of this very frame have written the array)
        CHK(c, hipMemsetAsync(c->d_order, 0xFF, sizeof(uint32_t) * ((size_t)n_units + parts_extra_cap(n_units) + 4u), s));
        if (!c->d_ord_scratch) { // counts and cursors of the several-workgroup ordering (grt_bvh.hip: k_ord_a); zero once, phase C keeps it so
            CHK(c, hipMalloc(&c->d_ord_scratch, order_scratch_bytes()));
            CHK(c, hipMemsetAsync(c->d_ord_scratch, 0, order_scratch_bytes(), s));
        }
        CHK(c, hipMalloc(&c->d_cost_dil, sizeof(uint32_t) * n_units));
        CHK(c, hipMalloc(&c->d_qparts, sizeof(uint32_t) * kQuadListCap));
        if (!c->d_qpcount) {
            CHK(c, hipMalloc(&c->d_qpcount, 2 * sizeof(uint32_t)));
            CHK(c, hipMemsetAsync(c->d_qpcount, 0, 2 * sizeof(uint32_t), s));
        }
        c->cost_cap = n_units;
    }
    c->sched_units = n_units; // (grt_debug_copy_schedule: the units d_cost and d_order are for, whatever the feedback option)
    if (!c->opt_feedback) { // no scheduling feedback: the cost words are only collected for k_check_costs (tile kernel)
        CHK(c, hipMemsetAsync(c->d_cost, 0, sizeof(uint32_t) * n_units, s));
        a.cost = c->d_cost;
        c->cost_valid = false;
        c->order_ready = false;
        c->cost_zeroed = false;
        return GRT_OK;
    }
    const bool same = c->cost_valid && memcmp(sig, c->cost_sig, sizeof(sig)) == 0;
    const grt_ctx* sc = scene_of(c);
    // was the order this frame is launched with made for THIS frame (same scene, camera, options)?  Remembered for the order that
    // will be made from this frame's costs: costs measured under another view's part waves — its heavy tiles split, this view's not —
    // make an order that is one feedback step short of the fixed point (a 256^2 frame after a camera move: 0.61 instead of 0.53 ms,
    // for as long as the view stands still), so such an order is used but not KEPT: the next identical frame collects once more.
    const bool order_is_for_this_frame = c->order_valid && c->order_epoch == sc->scene_epoch && memcmp(&c->order_params, &a.p, sizeof(grt_params)) == 0;
    c->launch_order_matched = same && order_is_for_this_frame; // (a frame without usable costs runs in the cold order: no match)
    if (same && c->order_ready && c->order_settled && order_is_for_this_frame) {
        // the very frame the order was made from: a tile's cost does not depend on the launch order (nor, once settled, on which
        // tiles run as parts), so this frame would measure the same costs and make the same order again — keep it, collect nothing
        launch_with_order(c, a);
        return GRT_OK;
    }
    if (same) {
        // (normally already there: do_launch orders the units for the next frame right behind this frame's kernels,
        //  where it fills the gap between two frames instead of delaying the next one)
        if (!c->order_ready && !c->cost_zeroed) { // the costs of the last frame are still in d_cost
            int rc = order_from_costs(c, a, n_units, s, &c->order_split);
            if (rc != GRT_OK) return rc;
            c->order_valid = true;
        }
        // (an option was changed after the costs were consumed and zeroed: the order made from them is still the best
        //  there is — this frame collects costs again)
        if (c->order_valid) launch_with_order(c, a);
    } else if (c->opt_cold_estimate && n_units == a.n_blocks * 4u && sc->n && (a.mode == 0 || a.mode == 1)) {
        // no costs of a previous frame with this geometry: order the tiles by the number of particle centres that
        // project into them (dense tiles first), so that the first frame's long tiles do not start last
        CHK(c, hipMemsetAsync(c->d_cost_dil, 0, sizeof(uint32_t) * n_units, s));
        const uint32_t stride = sc->n > 400000 ? 4u : 1u; // original (unsorted) order: every 4th particle is a fair sample
        const uint32_t ns = ((uint32_t)sc->n + stride - 1) / stride;
        hipLaunchKernelGGL(k_estimate_costs, dim3((ns + 255) / 256), dim3(256), 0, s, sc->d_pos, (uint32_t)sc->n, stride, a, c->d_cost_dil);
        const uint32_t* src = c->d_cost_dil;
        if (a.mode == 0) { // proxies are a few tiles wide: a tile next to a dense one is heavy too
            int rcd = dilate_unit_costs(c->d_cost_dil, c->d_cost, a.nbx, a.nby, 1, s, &c->err);
            if (rcd != GRT_OK) return rcd;
            src = c->d_cost;
        }
        c->order_launch = 0;
        int rc;
        if (c->opt_cold_estimate >= 2 && c->parts_ok && a.mode == 0 && c->opt_tile_parts4_pct > 0 && !sc->n_faces) {
            // (not on mesh frames: a split tile queues four thin bundles of continuation rays — C4's cold frame 3.30 -> 3.90 ms)
            // (GRT_OPT_COLD_ESTIMATE = 2, the default since round 4: the estimate also decides which tiles of the cold frame run as part
            //  waves — above GRT_OPT_COLD_PARTS_PCT % of the heaviest estimate: C1's cold frame 0.637 -> 0.553 ms, C2 1.048 -> 1.012, C3 -1.3 %)
            rc = order_with_parts(c, src, c->d_cost_dil, n_units, 0u, (uint32_t)c->opt_cold_parts_pct, nullptr, 2u /* (particle counts, not cost words) */,
                                  quad_parts_ok(c, n_units) && c->d_qparts, s);
            a.n_launch = c->order_launch; // (at once, and 0 when the ordering failed)
        } else {
            c->order_classes = false;
            rc = order_units_by_cost(src, c->d_order, n_units, 1u, (uint32_t)c->opt_heavy_thr_x2, nullptr, nullptr, s, &c->err);
        }
        if (rc != GRT_OK) return rc;
        a.order = c->d_order;
        c->order_valid = true;
        c->order_split = false;
    } else {
        c->order_valid = false; // nothing in d_order is meant for this launch geometry
    }
    if (!(same && c->cost_zeroed)) CHK(c, hipMemsetAsync(c->d_cost, 0, sizeof(uint32_t) * n_units, s));
    a.cost = c->d_cost;
    memcpy(c->cost_sig, sig, sizeof(sig));
    c->cost_valid = true;
    c->order_ready = false;
    c->cost_zeroed = false;
    return GRT_OK;
}

// The tile kernel's pool of window-overflow bags, in chunks of kTileOvfChunkBytes = 32 KiB (32 entries x 64 lanes): a tile that
// overflows takes one to three in a row, by how deep its bags got in the frame before (grt_tile.h kSub).  A tile that
// finds the pool empty falls back to another pass (never wrong; a pool for a quarter of the tiles ran dry on the default 1 M scene and
// cost that frame 12 %, and on the needle scene C3a a pool of 3/8 of the tiles made the first frames 2.3 x slower).  Round 2 held a full
// bag for EVERY tile of the launch for good (3.1 GB at 1080p, 12.4 GB at 4K, per frame slot); rounds 3-4 sized the pool from the
// largest demand ever seen, in whole 96-entry bags (1.3 GB at 1080p).  Now the pool follows the DEMAND both ways: every frame's chunk
// counter is read back behind it (pinned word, no sync; the device keeps the peak between two reads) and the last eight readings are
// kept.  The pool is 1.25 x their MEDIAN + 64 (one cold frame — a camera cut: no size classes, every tile asks for more — does not move
// it); it GROWS when the median comes within 10 % of it and SHRINKS when it is more than 1.2 x what the LARGEST of the eight would ask
// for (so a spike only delays a shrink, and a demand that wanders does not re-make the pool every frame).  A re-size does not wait for
// the device: the new pool is allocated beside the old one, which is freed once the frames that may use it have drained (hipFree
// synchronises: it is called when nothing of this scene is in flight, or at the latest when a third pool would pile up).  The first
// frame of a launch geometry still gets three chunks per tile (or what a sibling frame slot of the same scene has learnt).  An
// allocation that fails is retried at half the size down to nothing and not asked for again: rendering never fails for want of an
// optimisation buffer.
static void overflow_demand_stats(const grt_ctx* c, uint32_t* median, uint32_t* largest)
{
    *median = *largest = 0u;
    if (!c->ovf_hist_n) return;
    uint32_t v[8];
    const uint32_t n = std::min(c->ovf_hist_n, 8u);
    for (uint32_t i = 0; i < n; i++) v[i] = c->ovf_hist[i];
    std::sort(v, v + n);
    *median = v[n / 2u]; // (the upper median of an even count)
    *largest = v[n - 1u];
}

// old pools whose last users may still run: freed when their event has passed and no frame of the scene is in flight (force: now)
static void reap_old_pools(grt_ctx* c, bool force, hipStream_t s = nullptr)
{
    if (c->ovf_old.empty()) return;
    // (hipFree waits for the whole device: not while frames of this slot are queued on its stream — a loop that queues its frames
    //  without waiting would drain, and the head of such a loop would pay for the free — nor while a sibling slot has frames in flight; a
    //  third pool piling up is freed regardless)
    (void)s;
    if (!force && c->ovf_old.size() < 3u && (sibling_frames_in_flight(c) || c->ovf_idle_run < 2u)) return;
    for (size_t i = 0; i < c->ovf_old.size();) {
        auto& o = c->ovf_old[i];
        if (force || c->ovf_old.size() >= 3u || hipEventQuery(o.second) == hipSuccess) {
            if (hipEventQuery(o.second) != hipSuccess) (void)hipEventSynchronize(o.second);
            (void)hipFree(o.first);
            (void)hipEventDestroy(o.second);
            c->ovf_old.erase(c->ovf_old.begin() + (long)i);
        } else {
            i++;
        }
    }
}

static int size_overflow_pool(grt_ctx* c, uint32_t n_tiles, hipStream_t s)
{
    grt_ctx* sc = scene_of(c);
    // (does the application wait for its frames?  Two frames in a row that find their stream idle: the first frame behind a synchronisation
    //  point may be the head of a loop that does not wait)
    c->ovf_idle_run = (hipStreamQuery(s) == hipSuccess) ? std::min(c->ovf_idle_run + 1u, 8u) : 0u;
    (void)hipGetLastError();
    reap_old_pools(c, false, s);
    if (c->ovf_units != n_tiles) { c->ovf_hist_n = 0; c->ovf_demand = 0; c->ovf_short = false; c->ovf_sized = false; c->ovf_units = n_tiles; c->ovf_stale = c->ovf_pending; } // another launch geometry: start over
    if (c->ovf_pending && hipEventQuery(c->ev_ovf) == hipSuccess) {
        if (!c->ovf_stale) { // (a reading asked for under the geometry before says nothing about this one)
            if (*c->h_ovf_used != 0u) { // (0: nothing but frames that do not count since the last reading)
                c->ovf_hist[c->ovf_hist_n % 8u] = *c->h_ovf_used;
                c->ovf_hist_n++;
                overflow_demand_stats(c, &c->ovf_demand, &c->ovf_demand_max);
                sc->ovf_hint_units = c->ovf_units;
                sc->ovf_hint = c->ovf_demand;
            }
        }
        c->ovf_stale = false;
        c->ovf_pending = false;
    }
    const uint32_t cap = (uint32_t)((16ull << 30) / kTileOvfChunkBytes);
    const uint32_t most = (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>((uint64_t)n_tiles * kTileOvfChunksPerTile, 1u));
    uint32_t want;
    bool resize;
    if (c->opt_ovf_chunks != 0) {
        want = c->opt_ovf_chunks > 0 ? (uint32_t)c->opt_ovf_chunks : 0u;
        resize = c->ovf_chunks != want;
    } else {
        const bool own = c->ovf_demand != 0u;
        const uint32_t d = own ? c->ovf_demand : ((sc->ovf_hint_units == n_tiles) ? sc->ovf_hint : 0u);
        const uint32_t dmax = own ? c->ovf_demand_max : d;
        if (d == 0u) { // nothing known yet
            want = most;
            resize = c->ovf_chunks < want && !c->ovf_short;
        } else {
                want = std::min(most, d + d / 4u + 64u);
            const uint32_t keep = std::min(most, dmax + dmax / 4u + 64u); // what the largest recent demand would ask for
            // WHEN: a re-size costs milliseconds of host time (hipMalloc of half a gigabyte: ~5 ms), during which a loop that queues its
            // frames without waiting runs dry.  So the pool is re-made only at a frame the application waited for (nothing queued on
            // the frame's stream) — except the first sizing from a known demand (the pool still holds three chunks for every tile: it
            // happens in the first frames of a view) and a pool that ran DRY (the last frame asked for more than there is)
            const bool idle = c->ovf_idle_run >= 2u;
            const uint32_t last = c->ovf_hist_n ? c->ovf_hist[(c->ovf_hist_n - 1u) % 8u] : d;
            const bool first = !c->ovf_sized;
            const bool grow = c->ovf_chunks < std::min(most, d + d / 10u) && !c->ovf_short && (idle || first || last > c->ovf_chunks);
            const bool shrink = c->ovf_chunks > keep + keep / 5u && (idle || first);
            resize = grow || shrink;
            if (shrink && !grow) want = keep;
            if (resize) c->ovf_sized = true;
        }
    }
    if (resize) {
        if (c->d_ovf) { // frames in flight may still use it: it goes when they have drained
            hipEvent_t ev = nullptr;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, s) == hipSuccess) {
                c->ovf_old.emplace_back(c->d_ovf, ev);
            } else {
                if (ev) (void)hipEventDestroy(ev);
                (void)hipGetLastError();
                (void)hipDeviceSynchronize();
                (void)hipFree(c->d_ovf);
            }
        }
        c->d_ovf = nullptr;
        c->ovf_chunks = 0;
        for (uint32_t n = want; n >= 1u; n /= 2u) {
            if (hipMalloc(&c->d_ovf, (size_t)n * kTileOvfChunkBytes) == hipSuccess) { c->ovf_chunks = n; break; }
            c->ovf_short = true; // (the memory is not there: growing is not tried again for this launch geometry)
            (void)hipGetLastError(); // out of memory is not an error of the frame: a smaller pool, or none
            c->d_ovf = nullptr;
            reap_old_pools(c, true, nullptr); // (what waits to be freed may be what is missing)
            if (c->opt_ovf_chunks > 0) break;
        }
    }
    return GRT_OK;
}

// everything a frame slot owns (a view has nothing else)
void grt::free_slot_state(grt_ctx* c)
{
    (void)hipFree(c->d_erec); (void)hipFree(c->d_erec_wide);
    (void)hipFree(c->d_counters);
    (void)hipFree(c->d_cost); (void)hipFree(c->d_order); (void)hipFree(c->d_cost_dil); (void)hipFree(c->d_ord_scratch); (void)hipFree(c->d_qparts); (void)hipFree(c->d_qpcount);
    (void)hipFree(c->d_prec); (void)hipFree(c->d_queue); (void)hipFree(c->d_qcount); (void)hipFree(c->d_heavy); (void)hipFree(c->d_fqueue);
    (void)hipFree(c->d_bverdict); (void)hipFree(c->d_qunit); (void)hipFree(c->d_qskip); (void)hipFree(c->d_heavy_a);
    reap_old_pools(c, true, nullptr);
    (void)hipFree(c->d_ovf); (void)hipFree(c->d_ovf_next);
    (void)hipFree(c->d_gacc); (void)hipFree(c->d_gacc_sh);
    if (c->ev_bwd) (void)hipEventDestroy(c->ev_bwd);
    (void)hipFree(c->d_err);
    if (c->h_ovf_used) (void)hipHostFree(c->h_ovf_used);
    if (c->h_err) (void)hipHostFree(c->h_err);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_ovf) (void)hipEventDestroy(c->ev_ovf);
    if (c->ev_tail) (void)hipEventDestroy(c->ev_tail);
    (void)hipFree(c->d_n_heavy);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
}

// ---- the launch: do_launch and its stages, in the order they run ----

// GRT_DEBUG_LAUNCH, read once: 0 = unset; 1 = one line per frame on stderr (what the launch is made of; mesh frames: what went through
// the wavefront stages); 2 = and the launch order's parts and the frame's heaviest tiles
static int debug_launch_level()
{
    static const int level = [] { const char* e = getenv("GRT_DEBUG_LAUNCH"); return !e ? 0 : (e[0] == '2' ? 2 : 1); }();
    return level;
}
// 1. the slot catches up with its scene and with the work queued behind its last frame
static int slot_catch_up(grt_ctx* c, hipStream_t s)
{
    const grt_ctx* sc = scene_of(c);
    if (c->seen_epoch != sc->scene_epoch) { // the scene changed under this slot (a view learns of it here)
        c->erec_valid = false;
        c->cost_valid = false;
        c->order_ready = false;
        c->seen_epoch = sc->scene_epoch;
    }
    // the zeroing / ordering queued behind the last frame ran on THAT frame's stream: a launch on another stream waits
    // for it (else it could start before its counters are reset — two tiles taking the same overflow chunk)
    if (c->tail_pending && c->tail_stream != s) CHK(c, hipStreamWaitEvent(s, c->ev_tail, 0));
    // (has the work behind the last frame finished?  then the pinned words it wrote are current: the error word, and how many parts
    //  the quad kernel's list holds)
    const bool tail_done = !c->tail_pending || hipEventQuery(c->ev_tail) == hipSuccess;
    if (tail_done && c->tail_qepoch != ~0ull) { c->qknown_epoch = c->tail_qepoch; c->qknown_count = c->h_err[1]; } // (the list that tail saw, and its length)
    c->tail_pending = false;
    return GRT_OK;
}
// 3. the counters zeroed; the wavefront pipeline's arguments as a frame without meshes has them
static int wavefront_defaults(grt_ctx* c, RenderArgs& a, hipStream_t s)
{
    const grt_ctx* sc = scene_of(c);
    if (c->opt_counters) CHK(c, hipMemsetAsync(c->d_counters, 0, kNumCounters * sizeof(unsigned long long), s));
    a.prec = nullptr; a.queue = nullptr; a.qcount = nullptr;
    a.queue_in = nullptr; a.qcount_in = nullptr; a.queue_alt = nullptr;
    a.heavy = nullptr; a.hcount = nullptr; a.hnext = nullptr; a.fqueue = nullptr; a.fcount = nullptr;
    a.bundle_rounds = (uint32_t)c->opt_bundle_rounds;
    // (rays that went through a glass body are defocused but each of them light: their bundles are worth twice the work
    //  before they are given up — 1 M scene + glass sphere 8.2 -> 5.9 ms; a mirror's limb bundles are not: 4.0 -> 4.5)
    a.bundle_budget = (uint32_t)c->opt_bundle_budget * (a.p.type == GRT_GLASS ? 2u : 1u);
    a.lane_budget = (uint32_t)c->opt_lane_budget;
    a.single_own_mesh = 0;
    a.mstack_depth = sc->mbvh.height + 2u;
    // (2 = fused into the tile kernel's primary stage, on its depth-first stack: only when the mesh tree's walk fits it)
    a.mesh_primary_wave = (uint32_t)c->opt_mesh_primary_wave;
    if (a.mesh_primary_wave == 2u && a.mstack_depth > kTileStack) a.mesh_primary_wave = 1u;
    a.single_look = (float)c->opt_single_look / 1024.0f;
    a.single_band = (float)c->opt_single_band / 1024.0f;
    return GRT_OK;
}
// 4. mesh frame: buffers of the wavefront pipeline (one record per launched thread)
static int wavefront_buffers(grt_ctx* c, RenderArgs& a)
{
    if (!scene_of(c)->n_faces || a.mode == 2) return GRT_OK;
    // (entries of the continuation queues: one 64-entry chunk per wave of the primary stage — per 8x8 tile, and per PART of a
    //  heavy tile when the launch order splits some)
    const size_t need = ((size_t)a.n_blocks * 4 + parts_extra_cap(a.n_blocks * 4u)) * 64;
    if (c->wf_cap < need) {
        (void)hipFree(c->d_prec); (void)hipFree(c->d_queue); (void)hipFree(c->d_heavy); (void)hipFree(c->d_fqueue);
        (void)hipFree(c->d_qunit); (void)hipFree(c->d_qskip); (void)hipFree(c->d_heavy_a); // (sized by the queues: re-made with the verdicts below)
        c->d_qunit = c->d_qskip = c->d_heavy_a = nullptr;
        c->d_prec = c->d_queue = c->d_fqueue = nullptr;
        c->d_heavy = nullptr;
        c->wf_cap = 0;
        CHK(c, hipMalloc(&c->d_prec, need * 3 * sizeof(float4)));
        CHK(c, hipMalloc(&c->d_queue, 2 * need * 4 * sizeof(float4))); // two queues: the stages ping-pong
        CHK(c, hipMalloc(&c->d_heavy, need * sizeof(uint32_t)));
        CHK(c, hipMalloc(&c->d_fqueue, need * 4 * sizeof(float4)));
        c->wf_cap = need;
    }
    if (!c->d_qcount) CHK(c, hipMalloc(&c->d_qcount, sizeof(uint32_t) * kWfCounters));
    a.prec = c->d_prec; a.queue = c->d_queue; a.qcount = c->d_qcount;
    a.queue_alt = c->d_queue + c->wf_cap * 4;
    a.heavy = c->d_heavy; a.fqueue = c->d_fqueue;
    return GRT_OK;
}
// 5. bundle verdicts (RenderArgs::bverdict): one word per 8x8 tile of the launch; they belong to a launch geometry and a scene —
// anything else starts from "every tile is a bundle" — and are used up under a view that changes
static int bundle_verdicts(grt_ctx* c, RenderArgs& a, hipStream_t s, bool tile_kernel)
{
    const grt_ctx* sc = scene_of(c);
    a.bverdict = nullptr; a.qunit = nullptr; a.qunit_out = nullptr; a.qunit_cap = 0; a.qskip = nullptr; a.heavy_a = nullptr; a.hcount_a = nullptr; a.bverdict_epoch = 0;
    if (!(sc->n_faces && a.mode != 2 && tile_kernel && c->opt_bundle_predict && c->opt_bundle_rounds > 0 && c->wf_cap)) return GRT_OK;
    const uint32_t nu = a.n_blocks * 4u;
    uint64_t sig[6];
    launch_geometry_sig(a, nu, sig);
    const size_t chunks = c->wf_cap / 64;
    bool fresh = false;
    if (c->bv_cap < nu || !c->d_qunit) {
        (void)hipFree(c->d_bverdict); (void)hipFree(c->d_qunit); (void)hipFree(c->d_qskip); (void)hipFree(c->d_heavy_a);
        c->d_bverdict = c->d_qunit = c->d_qskip = c->d_heavy_a = nullptr;
        c->bv_cap = 0;
        CHK(c, hipMalloc(&c->d_bverdict, sizeof(uint32_t) * (size_t)nu * kMaxBundleRounds)); // (a set of verdicts per bundle round)
        CHK(c, hipMalloc(&c->d_qunit, sizeof(uint32_t) * 2 * chunks));                       // (tile numbers of the chunks of either queue)
        CHK(c, hipMalloc(&c->d_qskip, sizeof(uint32_t) * chunks));
        CHK(c, hipMalloc(&c->d_heavy_a, sizeof(uint32_t) * c->wf_cap));
        c->bv_cap = nu;
        fresh = true;
    }
    if (fresh || memcmp(sig, c->bv_sig, sizeof(sig)) != 0 || c->bv_epoch != sc->scene_epoch) {
        CHK(c, hipMemsetAsync(c->d_bverdict, 0, sizeof(uint32_t) * (size_t)nu * kMaxBundleRounds, s)); // (on the frame's stream: ordered against its kernels)
        memcpy(c->bv_sig, sig, sizeof(sig));
        c->bv_epoch = sc->scene_epoch;
        c->bv_params_valid = false;
    }
    a.bverdict = c->d_bverdict; a.qunit = c->d_qunit; a.qunit_cap = (uint32_t)chunks; a.qskip = c->d_qskip; a.heavy_a = c->d_heavy_a;
    if (!(c->bv_params_valid && memcmp(&c->bv_params, &a.p, sizeof(grt_params)) == 0)) c->bv_view = (c->bv_view + 1u) ? c->bv_view + 1u : 1u; // another view (never 0: a cleared word is no verdict)
    a.bverdict_epoch = c->bv_view;
    c->bv_params = a.p;
    c->bv_params_valid = true;
    return GRT_OK;
}
// 6. eye records of this slot: the buffer of the kernel family that runs (allocations come first: they may synchronise)
static int eye_record_buffers(grt_ctx* c, bool tile_kernel)
{
    const uint32_t m = scene_of(c)->gbvh.n_prims;
    float4*& d_erec = tile_kernel ? c->d_erec_wide : c->d_erec; // (64 B per proxy for the tile kernel, 16 B for the streaming kernel)
    size_t& cap = tile_kernel ? c->cap_erec_wide : c->cap_erec;
    if (cap >= m) return GRT_OK;
    (void)hipFree(d_erec);
    d_erec = nullptr;
    cap = 0;
    CHK(c, hipMalloc(&d_erec, (size_t)m * (tile_kernel ? 4 : 1) * sizeof(float4) + 256));
    cap = m;
    c->erec_valid = false;
    return GRT_OK;
}
// 7. the overflow pool of a tile-kernel launch, sized, and its counter words
static int overflow_pool(grt_ctx* c, RenderArgs& a, hipStream_t s, bool tile_kernel)
{
    a.ovf_pool = nullptr; a.ovf_next = nullptr; a.ovf_chunks = 0;
    a.ovf_entries = c->opt_ovf_entries > 0 ? (uint32_t)c->opt_ovf_entries : kTileOvfEntries;
    // (an order whose entries carry size classes: a whole tile without one — no cost word yet — starts in one chunk and moves when it
    //  outgrows it; an order of bare unit numbers, or none: a full bag, as ever)
    //  (a scene whose tiles are nearly all deep — the needle scene: 2.8 chunks asked for per tile of the launch — gains nothing from the
    //   small start and pays a move per tile on every cold frame, 16.5 -> 18.5 ms: there a tile without a class starts with a full bag too)
    a.ovf_cls0 = (a.order && c->order_classes && !(c->ovf_units == a.n_blocks * 4u && (uint64_t)c->ovf_demand * 2u > (uint64_t)a.n_blocks * 4u * 3u)) ? 1u : 3u;
    if (!tile_kernel) return GRT_OK;
    int rco = size_overflow_pool(c, a.n_blocks * 4u, s);
    if (rco != GRT_OK) return rco;
    if (!c->d_ovf_next) { // [0] next free chunk, [1] running peak of the demand (k_frame_tail)
        CHK(c, hipMalloc(&c->d_ovf_next, 2 * sizeof(uint32_t)));
        CHK(c, hipMemsetAsync(c->d_ovf_next, 0, 2 * sizeof(uint32_t), s));
        c->ovf_zeroed = true;
    }
    return GRT_OK;
}
// The alpha-sphere pre-test (grt_device.h: proxy_alpha_sphere_cc) rests on the proxies' inradius being the frame's alpha sphere: true
// when the frame's alpha_min is the one the scene was built with, or larger (the sphere is then merely not tight).  A frame with a
// smaller alpha_min keeps the circumsphere: its eye records say so, and its four-way parts stay on the camera-ray kernel.
static bool alpha_sphere_ok(const grt_ctx* c, const grt_params& p) { return p.alpha_min >= scene_of(c)->alpha_min; }
// 9. wave-per-tile kernels on camera rays: refresh the eye records when the eye moved (part of the timed frame)
static void refresh_eye_records(grt_ctx* c, RenderArgs& a, hipStream_t s, bool tile_kernel)
{
    const grt_ctx* sc = scene_of(c);
    const uint32_t m = sc->gbvh.n_prims;
    const bool wide = tile_kernel;
    const bool tight = alpha_sphere_ok(c, a.p); // (wide records only: the narrow ones hold no alpha-sphere value)
    if (!c->erec_valid || c->erec_is_wide != wide || (wide && c->erec_alpha_sphere != tight) ||
        memcmp(c->erec_eye, a.p.eye, sizeof(c->erec_eye)) != 0) {
        if (wide)
            hipLaunchKernelGGL(k_eye_records_wide, dim3((m + 255) / 256), dim3(256), 0, s, sc->d_rec, m, a.p.eye[0],
                               a.p.eye[1], a.p.eye[2], tight ? 1u : 0u, c->d_erec_wide);
        else
            hipLaunchKernelGGL(k_eye_records, dim3((m + 255) / 256), dim3(256), 0, s, sc->d_rec, m, a.p.eye[0], a.p.eye[1],
                               a.p.eye[2], c->d_erec);
        memcpy(c->erec_eye, a.p.eye, sizeof(c->erec_eye));
        c->erec_valid = true;
        c->erec_is_wide = wide;
        c->erec_alpha_sphere = tight;
    }
    a.erec = wide ? c->d_erec_wide : c->d_erec;
}
// 10. what launch_render takes beside the arguments; the tile kernel's tuning; whether the quad kernel runs; the overflow counter at zero
static int tile_tuning(grt_ctx* c, RenderArgs& a, hipStream_t s, bool tile_kernel, const AuxOut* px, LaunchAux& aux)
{
    const grt_ctx* sc = scene_of(c);
    aux.aux = c->aux_stream; aux.fork = c->ev_fork; aux.join = c->ev_join;
    aux.heavy_cap = a.n_heavy ? std::max(1u, a.n_units / (uint32_t)c->opt_heavy_cap_div) : 0u; // in scheduling units
    aux.force_big = c->opt_kernel == 4;
    aux.px = px; // aux frame: launch_render takes the aux kernels (tile aux kernel or per-lane)
    if (tile_kernel) { a.n_heavy = nullptr; aux.heavy_cap = 0; } // no big-window split on the tile kernel
    a.tile_ready_min = (uint32_t)c->opt_tile_ready;
    a.tile_band = (float)c->opt_tile_band / 1024.0f;
    a.tile_look = (float)c->opt_tile_look / 1024.0f;
    // (auto: 16 — C2 -4.5 %, C1 -2 % against 24, C3 / C5 / the dense-core camera unchanged — but 24 for trees with pieces, whose frontier
    //  is crowded with far ranges: the needle scene C3a 14.5 ms at 24, 15.1 at 20, 16.4 at 16, 24.1 at 14)
    a.tile_reserve = c->opt_tile_reserve >= 0 ? (uint32_t)c->opt_tile_reserve : (sc->has_pieces ? 24u : 16u);
    a.tile_band_abs = (float)c->opt_band_abs / 64.0f * sc->gm_diag;
    a.tile_prio_div = (uint32_t)c->opt_tile_prio;
    a.quad_parts = (quad_parts_ok(c, a.n_units) && alpha_sphere_ok(c, a.p) && tile_kernel && c->parts_ok && a.mode != 2 && a.order && a.n_launch && c->qparts_valid) ? 1u : 0u;
    a.qparts = c->d_qparts; a.qpart_count = c->d_qpcount;
    // the list's length when the host knows it (a frame tail that ran behind the list's making has copied it to the pinned word; frames of
    // a standing view keep their order and their list, so frames queued without a host synchronisation between them know it too): a launch
    // without parts skips the quad kernel and its fork / join, one with parts launches exactly that many waves; else kQuadListCap waves,
    // the idle ones exit
    a.quad_known = (a.quad_parts && c->qknown_epoch == c->qlist_epoch) ? (c->qknown_count + 1u) : 0u;
    if (a.quad_known == 1u) a.quad_parts = 0u; // (known to be empty; the order then holds no code-3 entry either)
    if (tile_kernel) {
        if (!c->ovf_zeroed) CHK(c, hipMemsetAsync(c->d_ovf_next, 0, sizeof(uint32_t), s));
        c->ovf_zeroed = false;
        a.ovf_pool = c->d_ovf; a.ovf_next = c->d_ovf_next; a.ovf_chunks = c->ovf_chunks;
    }
    return GRT_OK;
}
// 10b. GRT_OPT_ALPHA_CULL: the launches whose pre-test reads the alpha sphere (cc_a of the wide eye records: the uncounted camera-ray
// kernel with or without the mesh walk, SH and pieces, its aux instantiation, the quad kernel — all of them the PRIMARY stage of a frame
// on the tile kernel) cull their leaf ranges with the alpha radius.  The stages behind it (bundles, single rays; they may start from a
// copy of this argument block) pre-test on the circumsphere and take aux.pbox_bundles; counted frames run the full event stream and keep
// gbvh.pbox, as a frame does whose alpha_min lies below the scene's (alpha_sphere_ok: its cc_a is the circumsphere's).
static void alpha_cull_boxes(const grt_ctx* c, RenderArgs& a, bool tile_camera_rays, LaunchAux& aux)
{
    const grt_ctx* sc = scene_of(c);
    if (!tile_camera_rays || !c->opt_alpha_cull || c->opt_counters || !sc->gbvh.pbox_a || !alpha_sphere_ok(c, a.p) || !c->erec_alpha_sphere) return;
    aux.pbox_bundles = a.pbox;
    a.pbox = sc->gbvh.pbox_a;
}
// 11. GRT_DEBUG_LAUNCH: one line per frame on stderr, what the launch is made of; at level 2 the launch order's parts
static void debug_print_launch(const grt_ctx* c, const RenderArgs& a)
{
    if (!debug_launch_level()) return;
    uint32_t d3[3] = {0, 0, 0}; // entries in use, four-way threshold, heaviest tile (as the ordering kernel left them)
    if (a.order && a.n_launch) { (void)hipDeviceSynchronize(); (void)hipMemcpy(d3, c->d_order + a.n_launch, sizeof(d3), hipMemcpyDeviceToHost); }
    fprintf(stderr, "grt launch: ctx %p mode %u units %u order %s entries %u cost %s parts_ok %d cost_valid %d order_ready %d used %u thr4 %u max %u\n",
            (void*)c, a.mode, a.n_units, a.order ? "yes" : "no", a.n_launch, a.cost ? "collect" : "-", (int)c->parts_ok, (int)c->cost_valid,
            (int)c->order_ready, d3[0], d3[1], d3[2]);
    if (debug_launch_level() >= 2 && a.order && a.n_launch) {
        std::vector<uint32_t> ord(a.n_launch);
        (void)hipMemcpy(ord.data(), c->d_order, sizeof(uint32_t) * a.n_launch, hipMemcpyDeviceToHost);
        uint32_t n4 = 0, n2 = 0;
        std::string head;
        for (uint32_t i = 0; i < d3[0] && i < a.n_launch; i++) {
            const uint32_t e = ord[i], code = e >> 30, part = (e >> 28) & 3u, unit = e & kOrderUnitMask;
            if (part == 0u) { n4 += code == 2u; n2 += code == 1u; }
            if (part == 0u && head.size() < 300) head += " " + std::to_string(unit) + (code ? "/" + std::to_string(code) : "");
        }
        fprintf(stderr, "grt order: four-way %u two-way %u first:%s\n", n4, n2, head.c_str());
    }
}
// 15. GRT_DEBUG_LAUNCH, mesh frames: what went through the wavefront stages (grt_internal.h: kWfCounters)
static void debug_print_wavefront(const RenderArgs& a, hipStream_t s)
{
    if (!debug_launch_level() || !a.qcount) return;
    uint32_t q[kWfCounters];
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(q, a.qcount, sizeof(q), hipMemcpyDeviceToHost);
    std::string t = "grt wavefront: chunks after primary / bundle rounds:";
    for (int k = 0; k <= kMaxBundleRounds; k++) t += " " + std::to_string(q[k]);
    t += " | heavy rays per round:";
    for (int k = 0; k < kMaxBundleRounds; k++) t += " " + std::to_string(q[kMaxBundleRounds + 1 + k]);
    t += " | retry queue: " + std::to_string(q[2 * kMaxBundleRounds + 1]) + " | early lists per round (tiles known not to be bundles):";
    for (int k = 0; k < kMaxBundleRounds; k++) t += " " + std::to_string(q[3 * kMaxBundleRounds + 3 + 2 * k]);
    fprintf(stderr, "%s\n", t.c_str());
}
// GRT_DEBUG_LAUNCH=2: the heaviest tiles of the frame just rendered (steps / part code) before the costs are consumed
static void debug_print_costs(const grt_ctx* c, const RenderArgs& a, hipStream_t s)
{
    if (debug_launch_level() < 2) return;
    (void)hipStreamSynchronize(s);
    std::vector<uint32_t> h(a.n_units);
    (void)hipMemcpy(h.data(), c->d_cost, sizeof(uint32_t) * a.n_units, hipMemcpyDeviceToHost);
    std::vector<uint32_t> idx(a.n_units);
    for (uint32_t i = 0; i < a.n_units; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return (h[x] & kCostStepsMask) > (h[y] & kCostStepsMask); });
    std::string t;
    for (uint32_t k = 0; k < 24 && k < a.n_units; k++)
        t += " " + std::to_string(idx[k]) + ":" + std::to_string(h[idx[k]] & kCostStepsMask) + "/" + std::to_string((h[idx[k]] >> kCostPartShift) & 3u);
    fprintf(stderr, "grt costs (unit:steps/code, by raw steps):%s\n", t.c_str());
}
// 16. behind the frame, outside its timing (grt_last_kernel_ms brackets ev0..ev1; the feedback kernels below are ~60 us per frame under a
// moving camera and are what `frame ms - kernel ms` of bench.py's orbit leg shows): the give-up check, the next frame's order, the tail
static void behind_the_frame(grt_ctx* c, const RenderArgs& a, hipStream_t s, int rc, bool tile_kernel)
{
    bool tail = false;
    if (rc == GRT_OK && tile_kernel && a.cost) { // the tiles' give-up reasons -> sticky error word (a frame that repeats the
        // last one exactly collects no costs and is not checked again: it is the same computation)
        hipLaunchKernelGGL(k_check_costs, dim3((a.n_units + 255u) / 256u), dim3(256), 0, s, c->d_cost, a.n_units, a.max_iters, c->d_err);
        tail = true;
    }
    if (rc == GRT_OK && a.cost && c->cost_valid) debug_print_costs(c, a, s);
    if (rc == GRT_OK && a.cost && c->cost_valid) { // the next frame's launch order
        if (order_from_costs(c, a, a.n_units, s, &c->order_split, true) == GRT_OK) {
            c->order_ready = true;
            c->order_valid = true;
            // (settled: this frame itself ran with an order made for it — or no tile is ever split, and costs do not depend on the order)
            c->order_settled = c->launch_order_matched || c->order_launch == 0;
            c->order_params = a.p;
            c->order_epoch = scene_of(c)->scene_epoch;
            // ... and the zeroing the next frame needs before its first wave: done by the ordering kernel itself (costs consumed)
            c->cost_zeroed = true;
            tail = true;
        }
    }
    // ONE single-thread kernel behind the frame (it was two copies and a memset, each a packet of its own on the queue): the sticky
    // error word as the frame and k_check_costs left it -> pinned host word (grt_sync reads it behind ev_tail: no blocking
    // null-stream copy, which waited for every other frame slot's stream too); the overflow chunks this frame asked for -> pinned
    // host word (sizes the pool of the frames to come), and their counter reset for the next frame
    uint32_t* ovf = (rc == GRT_OK) ? a.ovf_next : nullptr;
    hipLaunchKernelGGL(k_frame_tail, dim3(1), dim3(1), 0, s, c->d_err, c->h_err, ovf, c->ovf_pending ? (uint32_t*)nullptr : c->h_ovf_used, c->d_qpcount, c->h_err + 1);
    c->tail_qepoch = c->qlist_epoch;
    if (hipGetLastError() == hipSuccess) {
        tail = true;
        if (ovf) {
            c->ovf_zeroed = true;
            if (!c->ovf_pending && hipEventRecord(c->ev_ovf, s) == hipSuccess) c->ovf_pending = true;
        }
    }
    if (tail && hipEventRecord(c->ev_tail, s) == hipSuccess) { c->tail_pending = true; c->tail_stream = s; }
}


static int do_launch(grt_ctx* c, RenderArgs& a, void* stream, const AuxOut* px = nullptr)
{
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const grt_ctx* sc = scene_of(c);
    CHK(c, hipSetDevice(c->device));
    // decided once, for every stage: the depth the kernels size their stacks by, and which kernel family runs (the same tests as
    // launch_render's; the streaming kernel is scheduled per 8x8 tile, one wave per workgroup, the other kernels per 16x16 block)
    const uint32_t depth = std::max(std::max(sc->gbvh.height, sc->n_faces ? sc->mbvh.height : 0u), 1u);
    const bool stream_kernel = uses_stream_kernel(c->opt_kernel, a.mode, depth);
    const bool tile_kernel = uses_tile_kernel(c->opt_kernel, a.mode, depth, sc->built_leaf_max, sc->gbvh.n_prims);
    int rc = slot_catch_up(c, s);                                                                                      // 1
    if (rc != GRT_OK) return rc;
    // (mesh frames too, since round 4: a part wave of the primary stage queues its own chunk of continuation rays, <= 16 of them)
    c->parts_ok = a.mode != 2 && (!sc->n_faces || c->opt_mesh_parts) && tile_kernel;                                   // 2
    if ((rc = prepare_feedback(c, a, s, stream_kernel ? a.n_blocks * 4u : a.n_blocks, tile_kernel)) != GRT_OK) return rc;
    if ((rc = wavefront_defaults(c, a, s)) != GRT_OK) return rc;                                                       // 3
    if ((rc = wavefront_buffers(c, a)) != GRT_OK) return rc;                                                           // 4
    if ((rc = bundle_verdicts(c, a, s, tile_kernel)) != GRT_OK) return rc;                                             // 5
    // allocations first (they may synchronise): eye records of this slot, overflow pool
    const bool want_erec = a.mode != 2 && sc->gbvh.n_prims && c->opt_kernel != 1 && c->opt_kernel != 2;
    if (want_erec && (rc = eye_record_buffers(c, tile_kernel)) != GRT_OK) return rc;                                   // 6
    if ((rc = overflow_pool(c, a, s, tile_kernel)) != GRT_OK) return rc;                                               // 7
    CHK(c, hipEventRecord(c->ev0, s));                                                                                 // 8
    a.erec = nullptr;
    if (want_erec) refresh_eye_records(c, a, s, tile_kernel);                                                          // 9
    LaunchAux aux;
    if ((rc = tile_tuning(c, a, s, tile_kernel, px, aux)) != GRT_OK) return rc;                                        // 10
    alpha_cull_boxes(c, a, tile_kernel && want_erec, aux);
    debug_print_launch(c, a);                                                                                    // 11
    if (px && !(tile_kernel && a.mode == 0 && !sc->n_faces)) {                                                         // 12
        // an aux frame on the per-lane kernel (launch_render_aux): screen order, no cost words — and the feedback of this slot starts
        // afresh with the next frame instead of making an order from costs nobody wrote
        a.order = nullptr; a.n_launch = 0; a.cost = nullptr; a.n_heavy = nullptr;
        c->cost_valid = false;
        c->order_ready = false;
    }
    rc = launch_render(a, c->opt_counters != 0, c->opt_kernel, depth, tile_kernel, s, &aux, &c->err);                  // 13
    CHK(c, hipEventRecord(c->ev1, s));                                                                                 // 14
    if (rc == GRT_OK) debug_print_wavefront(a, s);                                                                     // 15
    c->have_timing = (rc == GRT_OK);
    behind_the_frame(c, a, s, rc, tile_kernel);                                                                        // 16
    return rc;
}

extern "C" {

int grt_render(grt_ctx* c, const grt_params* p, uint8_t* d_rgb8, float* d_rgbf, uint32_t x0, uint32_t y0, uint32_t x1,
               uint32_t y1, void* stream)
{
    RenderArgs a;
    int rc = fill_common(c, p, &a);
    if (rc != GRT_OK) return rc;
    if ((rc = set_window(c, p, &a, x0, y0, x1, y1, "grt_render")) != GRT_OK) return rc;
    if (!d_rgb8 && !d_rgbf) { c->err = "grt_render: no output buffer"; return GRT_ERR_INVALID; }
    a.out8 = d_rgb8; a.outf = d_rgbf;
    return do_launch(c, a, stream);
}

// aux frames: NULL aux (or three NULL pointers) is the plain call itself; counters have no aux kernels
static bool aux_wanted(const grt_aux_out* x) { return x && (x->alpha || x->depth || x->count); }
static int aux_refused(grt_ctx* c, const char* fn)
{
    if (!c) return GRT_ERR_INVALID;
    if (c->opt_counters) {
        c->err = std::string(fn) + ": aux outputs with GRT_OPT_COUNTERS = 1 (the instrumented kernels have no aux variant)";
        return GRT_ERR_INVALID;
    }
    return GRT_OK;
}

int grt_render_aux(grt_ctx* c, const grt_params* p, uint8_t* d_rgb8, float* d_rgbf, const grt_aux_out* aux, uint32_t x0, uint32_t y0,
                   uint32_t x1, uint32_t y1, void* stream)
{
    if (!aux_wanted(aux)) return grt_render(c, p, d_rgb8, d_rgbf, x0, y0, x1, y1, stream);
    int rc = aux_refused(c, "grt_render_aux");
    if (rc != GRT_OK) return rc;
    RenderArgs a;
    rc = fill_common(c, p, &a);
    if (rc != GRT_OK) return rc;
    if ((rc = set_window(c, p, &a, x0, y0, x1, y1, "grt_render_aux")) != GRT_OK) return rc;
    a.out8 = d_rgb8; a.outf = d_rgbf; // (either may be NULL: the aux outputs alone are a frame)
    const AuxOut px{aux->alpha, aux->depth, aux->count};
    return do_launch(c, a, stream, &px);
}

int grt_render_tiles(grt_ctx* c, const grt_params* p, uint8_t* d_rgb8, float* d_rgbf, uint32_t tile_w, uint32_t tile_h,
                     uint32_t first_tile, uint32_t tile_stride, uint32_t n_tiles, void* stream)
{
    RenderArgs a;
    int rc = fill_common(c, p, &a);
    if (rc != GRT_OK) return rc;
    if ((rc = set_tiles(c, p, &a, tile_w, tile_h, first_tile, tile_stride, n_tiles, d_rgb8 || d_rgbf, "grt_render_tiles")) != GRT_OK) return rc;
    a.out8 = d_rgb8; a.outf = d_rgbf;
    return do_launch(c, a, stream);
}

// rank 0 of an N-rank frame: the gathered compact buffers back into screen order ("rank 0 un-permutes tiles
// with a trivial copy kernel").  Tile t of the row-major tile grid was rendered by rank t % world as its tile t / world.
__global__ void k_assemble_tiles(const uint8_t* __restrict__ g, uint32_t world, uint32_t max_cnt, uint32_t tile_w, uint32_t tile_h,
                                 uint32_t tiles_x, uint32_t width, uint32_t height, uint8_t* __restrict__ out)
{
    const uint32_t px = blockIdx.x * blockDim.x + threadIdx.x, py = blockIdx.y;
    if (px >= width || py >= height) return;
    const uint32_t t = (py / tile_h) * tiles_x + px / tile_w;
    const uint32_t r = t % world, j = t / world;
    const size_t src = ((((size_t)r * max_cnt + j) * tile_h + py % tile_h) * tile_w + px % tile_w) * 3;
    const size_t dst = ((size_t)py * width + px) * 3;
    out[dst] = g[src]; out[dst + 1] = g[src + 1]; out[dst + 2] = g[src + 2];
}

int grt_assemble_tiles(grt_ctx* c, const uint8_t* d_gathered, uint32_t world, uint32_t max_cnt, uint32_t tile_w, uint32_t tile_h,
                       uint32_t width, uint32_t height, uint8_t* d_rgb8, void* stream)
{
    if (!c) return GRT_ERR_INVALID;
    if (!d_gathered || !d_rgb8 || !world || !tile_w || !tile_h || !width || !height) { c->err = "grt_assemble_tiles: bad arguments"; return GRT_ERR_INVALID; }
    const uint32_t tiles_x = (width + tile_w - 1) / tile_w, tiles_y = (height + tile_h - 1) / tile_h;
    if ((uint64_t)max_cnt * world < (uint64_t)tiles_x * tiles_y) { c->err = "grt_assemble_tiles: world x max_cnt tiles do not cover the frame"; return GRT_ERR_INVALID; }
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    hipLaunchKernelGGL(k_assemble_tiles, dim3((width + 255) / 256, height), dim3(256), 0, s, d_gathered, world, max_cnt, tile_w, tile_h,
                       tiles_x, width, height, d_rgb8);
    CHK(c, hipGetLastError());
    return GRT_OK;
}

int grt_render_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, float* d_rgbf, void* stream)
{
    RenderArgs a;
    int rc = fill_common(c, p, &a);
    if (rc != GRT_OK) return rc;
    if (n && (!d_rays || !d_rgbf)) { c->err = "grt_render_rays: null buffer"; return GRT_ERR_INVALID; } // (the output too: in front of the shared refusals)
    if ((rc = set_rays(c, &a, d_rays, n, "grt_render_rays")) != GRT_OK) return rc;
    a.outf = d_rgbf;
    return do_launch(c, a, stream);
}

int grt_render_rays_aux(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, float* d_rgbf, const grt_aux_out* aux,
                        void* stream)
{
    if (!aux_wanted(aux)) return grt_render_rays(c, p, d_rays, n, d_rgbf, stream);
    int rc = aux_refused(c, "grt_render_rays_aux");
    if (rc != GRT_OK) return rc;
    RenderArgs a;
    rc = fill_common(c, p, &a);
    if (rc != GRT_OK) return rc;
    if ((rc = set_rays(c, &a, d_rays, n, "grt_render_rays_aux")) != GRT_OK) return rc;
    a.outf = d_rgbf; // (may be NULL)
    const AuxOut px{aux->alpha, aux->depth, aux->count};
    return do_launch(c, a, stream, &px);
}

// The sticky device error word (RenderArgs::err_word): a wave that had to give up on a ray — watchdog, depth-first stack
// guard, two passes without progress — ORs its reason in, in EVERY kernel variant (counters on or off).  Read (and
// cleared) at the synchronising entry points; the reference turns traversal trouble into exceptions the same way
// (OptiX exception flags, src/GaussianTracer.cpp:114-119; src/Exception.h:31-80).
static int check_device_error(grt_ctx* c)
{
    // the last frame may have gone to ANY stream (the caller's, a view's): what ran behind it — k_check_costs, which
    // turns the tile kernel's give-up reasons into the error word, and the copy of the word to h_err — is finished once
    // ev_tail is.  (Waiting for c->stream and ev1 alone returned GRT_OK for a frame on a non-blocking side stream whose
    // tiles had given up: ADVICE r03.)
    if (c->tail_pending) CHK(c, hipEventSynchronize(c->ev_tail));
    const uint32_t w = *(volatile uint32_t*)c->h_err;
    if (!w) return GRT_OK;
    hipStream_t s = c->tail_stream ? c->tail_stream : c->stream;
    CHK(c, hipMemsetAsync(c->d_err, 0, sizeof(w), s)); // stream-ordered before the next frame's kernels (do_launch waits on ev_tail)
    *c->h_err = 0;
    if (hipEventRecord(c->ev_tail, s) == hipSuccess) { c->tail_pending = true; c->tail_stream = s; }
    c->err = std::string("render: a wave gave up on live rays (pixels are missing hits):") +
             ((w & kErrWatchdog) ? " step watchdog expired;" : "") + ((w & kErrStack) ? " depth-first overflow stack full;" : "") +
             ((w & kErrStall) ? " two passes without progress;" : "");
    return GRT_ERR_LIMIT;
}

int grt_sync(grt_ctx* c)
{
    if (!c) return GRT_ERR_INVALID;
    CHK(c, hipSetDevice(c->device));
    CHK(c, hipStreamSynchronize(c->stream));
    // (renders go to the caller's stream: the last frame is finished once the event recorded behind its kernels is)
    if (c->have_timing) CHK(c, hipEventSynchronize(c->ev1));
    CHK(c, hipGetLastError());
    return check_device_error(c);
}

int grt_get_counters(grt_ctx* c, grt_counters* out)
{
    if (!c || !out) return GRT_ERR_INVALID;
    CHK(c, hipSetDevice(c->device));
    CHK(c, hipDeviceSynchronize());
    unsigned long long h[kNumCounters];
    CHK(c, hipMemcpy(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost));
    out->rays = h[0]; out->segments = h[1]; out->hit_evals = h[2]; out->rounds = h[3];
    out->node_visits = h[4]; out->proxy_tests = h[5]; out->rec_fetches = h[6]; out->stall_exits = h[7];
    return check_device_error(c);
}

int grt_last_kernel_ms(grt_ctx* c, float* ms)
{
    if (!c || !ms) return GRT_ERR_INVALID;
    if (!c->have_timing) { c->err = "grt_last_kernel_ms: no render has been launched"; return GRT_ERR_INVALID; }
    CHK(c, hipSetDevice(c->device));
    CHK(c, hipEventSynchronize(c->ev1));
    CHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return GRT_OK;
}

// ---- (testing) the launch-order kernels on the caller's arrays, and the slot's schedule as it stands (include/grt.h; tests/order_check.py) ----
// Never on a render path.  The kernels are reached through the host functions do_launch reaches them by, with the caller's arguments.
int grt_debug_order_units(grt_ctx* c, grt_debug_order* o)
{
    if (!c) return GRT_ERR_INVALID;
    if (!o) { c->err = "grt_debug_order_units: null arguments"; return GRT_ERR_INVALID; }
    auto refuse = [&](const char* what) { c->err = std::string("grt_debug_order_units: ") + what; return GRT_ERR_INVALID; };
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    switch (o->op) {
    case GRT_DEBUG_ORDER_PARTS: {
        if (o->n == 0) return refuse("n must be > 0");
        if (o->n > kOrderUnitMask) return refuse("n does not fit an entry's unit field");
        if (!o->d_cost || !o->d_cost_raw || !o->d_order) return refuse("null array");
        if (o->bag_classes > 2u) return refuse("bag_classes must be 0, 1 or 2");
        const uint32_t cap = o->extra_cap == 0xFFFFFFFFu ? parts_extra_cap(o->n) : o->extra_cap;
        if ((uint64_t)o->n + cap + 3u > 0xFFFFFFFFull) return refuse("n + extra_cap too large");
        const uint32_t pct4 = o->quad_pct4 ? quad_pct4_of(o->pct4, o->n) : o->pct4;
        o->extra_cap_used = cap;
        o->pct4_used = pct4;
        return order_units_with_parts(o->d_cost, o->d_cost_raw, o->d_order, o->n, cap, o->pct2, pct4, o->pct_load, o->resident_waves, o->d_zero,
                                      o->d_scratch, o->multi_min, o->bag_classes, s, &c->err);
    }
    case GRT_DEBUG_ORDER_PLAIN:
        if (o->n == 0) return refuse("n must be > 0");
        if (!o->d_cost || !o->d_order) return refuse("null array");
        return order_units_by_cost(o->d_cost, o->d_order, o->n, o->heavy_cap, o->thr_x2, o->d_out, o->d_zero, s, &c->err);
    case GRT_DEBUG_ORDER_QUAD_LIST:
        if (o->n == 0) return refuse("n must be > 0");
        if (!o->d_order || !o->d_out || !o->d_count) return refuse("null array");
        return quad_part_list(o->d_order, o->n, o->d_out, o->d_count, o->cap, s, &c->err);
    case GRT_DEBUG_ORDER_DILATE:
        if (o->nbx == 0 || o->nby == 0 || (uint64_t)o->nbx * o->nby * 4u != o->n) return refuse("n must be nbx x nby x 4 > 0");
        if (!o->d_cost || !o->d_out || o->d_cost == o->d_out) return refuse("null array, or the output is the input");
        if (o->radius < 0 || o->radius > 64) return refuse("radius must be 0..64");
        return dilate_unit_costs(o->d_cost, o->d_out, o->nbx, o->nby, o->radius, s, &c->err);
    }
    return refuse("unknown op");
}

uint32_t grt_debug_order_scratch_bytes(void) { return order_scratch_bytes(); }

int grt_debug_estimate_costs(grt_ctx* c, const grt_params* p, uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                             uint32_t stride, uint32_t* d_cost, uint32_t n_units)
{
    if (!c) return GRT_ERR_INVALID;
    if (!p) { c->err = "grt_debug_estimate_costs: null parameters"; return GRT_ERR_INVALID; }
    RenderArgs a;
    int rc = fill_common(c, p, &a);
    if (rc != GRT_OK) return rc;
    if (tile_w || tile_h) rc = set_tiles(c, p, &a, tile_w, tile_h, x0, y0, x1, true, "grt_debug_estimate_costs");
    else rc = set_window(c, p, &a, x0, y0, x1, y1, "grt_debug_estimate_costs");
    if (rc != GRT_OK) return rc;
    const grt_ctx* sc = scene_of(c);
    if (!d_cost) { c->err = "grt_debug_estimate_costs: null array"; return GRT_ERR_INVALID; }
    if (n_units == 0 || n_units != a.n_blocks * 4u) { c->err = "grt_debug_estimate_costs: n_units is not 4 per 16x16 block of the launch geometry"; return GRT_ERR_INVALID; }
    if (stride == 0 || sc->n == 0) { c->err = "grt_debug_estimate_costs: stride must be > 0 and a scene uploaded"; return GRT_ERR_INVALID; }
    CHK(c, hipSetDevice(c->device));
    const uint32_t ns = ((uint32_t)sc->n + stride - 1) / stride;
    hipLaunchKernelGGL(k_estimate_costs, dim3((ns + 255) / 256), dim3(256), 0, c->stream, sc->d_pos, (uint32_t)sc->n, stride, a, d_cost);
    CHK(c, hipGetLastError());
    return GRT_OK;
}

int grt_debug_copy_schedule(grt_ctx* c, grt_debug_schedule* o)
{
    if (!c) return GRT_ERR_INVALID;
    if (!o) { c->err = "grt_debug_copy_schedule: null arguments"; return GRT_ERR_INVALID; }
    CHK(c, hipSetDevice(c->device));
    if (hipDeviceSynchronize() != hipSuccess) { c->err = "grt_debug_copy_schedule: hipDeviceSynchronize failed"; return GRT_ERR_HIP; }
    const uint32_t n_units = c->d_cost ? std::min(c->sched_units, c->cost_cap) : 0u;
    // (an order is for the units of cost_sig's launch geometry; after frames without feedback the arrays may be another geometry's)
    const bool order = c->order_valid && c->d_order && n_units && (uint32_t)(c->cost_sig[0] >> 8) == n_units;
    const bool quad = order && c->order_launch && c->qparts_valid && c->d_qparts && c->d_qpcount;
    uint32_t n_quad = 0;
    if (quad && hipMemcpy(&n_quad, c->d_qpcount, sizeof(n_quad), hipMemcpyDeviceToHost) != hipSuccess) {
        c->err = "grt_debug_copy_schedule: copy of the quad list's count failed";
        return GRT_ERR_HIP;
    }
    const uint32_t n_order = !order ? 0u : (c->order_launch ? c->order_launch + 3u : n_units);
    // (the second call copies what the first one counted: a caller's buffers are sized by those counts)
    const bool counted = o->n_units == n_units && o->n_order == n_order && o->n_quad == n_quad;
    o->n_units = n_units;
    o->order_launch = order ? c->order_launch : 0u;
    o->order_valid = order ? 1u : 0u;
    o->order_classes = (order && c->order_launch && c->order_classes) ? 1u : 0u;
    o->quad_valid = quad ? 1u : 0u;
    o->n_order = n_order;
    o->n_quad = n_quad;
    if (!o->order && !o->quad && !o->cost) return GRT_OK;
    if (!counted) { c->err = "grt_debug_copy_schedule: the counts have changed since the buffers were sized"; return GRT_ERR_INVALID; }
    if (n_quad > kQuadListCap) { c->err = "grt_debug_copy_schedule: the quad list's count exceeds its capacity"; return GRT_ERR_LIMIT; }
    struct Part { void* dst; const void* src; size_t words; };
    const Part parts[] = {{o->order, c->d_order, n_order}, {o->quad, c->d_qparts, n_quad}, {o->cost, c->d_cost, n_units}};
    for (const Part& q : parts) {
        if (!q.dst || !q.words) continue;
        if (hipMemcpy(q.dst, q.src, q.words * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) {
            c->err = "grt_debug_copy_schedule: copy of the schedule failed";
            return GRT_ERR_HIP;
        }
    }
    return GRT_OK;
}

} // extern "C"
