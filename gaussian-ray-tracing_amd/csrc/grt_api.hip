// grt_api.hip — C ABI of libgrt_hip.so (include/grt.h), the part that is neither a frame nor the scene: the context's life cycle
// (create, view, destroy), the options, info and debug getters.  No kernel lives here.  The scene entry points and their kernels are
// grt_scene.hip's, the render entry points and everything a frame slot does grt_frame.hip's.  No CPU fallback: every entry point that
// needs the GPU fails loudly without one.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "grt_device.h"
#include "grt_internal.h"

using namespace grt;

static thread_local std::string g_create_err;

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
extern "C" {

int grt_create(grt_ctx** out, int device)
{
    if (!out) return GRT_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_err = "grt_create: no HIP device available (" + std::string(e != hipSuccess ? hipGetErrorString(e) : "0 devices") +
                       "); libgrt_hip has no CPU fallback";
        return GRT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        g_create_err = "grt_create: device index out of range";
        return GRT_ERR_INVALID;
    }
    if ((e = hipSetDevice(device)) != hipSuccess) {
        g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return GRT_ERR_HIP;
    }
    grt_ctx* c = new grt_ctx();
    c->device = device;
    if ((e = hipStreamCreate(&c->stream)) != hipSuccess || (e = hipEventCreate(&c->ev0)) != hipSuccess ||
        (e = hipEventCreate(&c->ev1)) != hipSuccess ||
        (e = hipMalloc(&c->d_counters, kNumCounters * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipStreamCreate(&c->aux_stream)) != hipSuccess || (e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming)) != hipSuccess ||
        (e = hipMalloc(&c->d_n_heavy, sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&c->d_err, sizeof(uint32_t))) != hipSuccess || (e = hipMemset(c->d_err, 0, sizeof(uint32_t))) != hipSuccess ||
        (e = hipHostMalloc(&c->h_ovf_used, sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc(&c->h_err, 2 * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess || // [0] error word, [1] parts in the quad list
        (e = hipEventCreateWithFlags(&c->ev_ovf, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming)) != hipSuccess) {
        g_create_err = std::string("grt_create: ") + hipGetErrorString(e);
        free_slot_state(c);
        delete c;
        return GRT_ERR_HIP;
    }
    *c->h_ovf_used = 0;
    *c->h_err = 0;
    *out = c;
    return GRT_OK;
}

// A second frame slot on the SAME scene: its own eye records, scheduling feedback, overflow pool, queues, counters and
// events, the parent's Gaussians / BVHs / meshes.  What D frames in flight need (bench.py, a double-buffering viewer)
// without D scene replicas.  Scene calls (upload, build, meshes) go to the parent; the parent must outlive its use by
// the view's renders (grt_destroy of a parent with live views is deferred until the last of them is destroyed).
int grt_create_view(grt_ctx* parent, grt_ctx** out)
{
    if (!out) return GRT_ERR_INVALID;
    *out = nullptr;
    if (!parent || parent->parent) {
        g_create_err = "grt_create_view: the parent must be a context made by grt_create";
        return GRT_ERR_INVALID;
    }
    grt_ctx* v = nullptr;
    const int rc = grt_create(&v, parent->device);
    if (rc != GRT_OK) return rc;
    v->parent = parent;
    {
        std::lock_guard<std::mutex> lk(parent->views_mu);
        parent->n_views++;
        parent->views.push_back(v);
    }
    *out = v;
    return GRT_OK;
}

static void destroy_now(grt_ctx* c)
{
    if (!c->parent) free_scene_state(c);
    free_slot_state(c);
    delete c;
}

void grt_destroy(grt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize(); // renders of this slot (and, for a scene, of its views) may be in flight on any stream
    if (c->parent) {
        grt_ctx* p = c->parent;
        bool last;
        {   // (a sibling's launch may be looking at this view's frame-end event: off the list first, under the lock, then destroyed)
            std::lock_guard<std::mutex> lk(p->views_mu);
            p->views.erase(std::remove(p->views.begin(), p->views.end(), c), p->views.end());
            last = --p->n_views == 0;
        }
        destroy_now(c);
        if (last && p->zombie) destroy_now(p);
        return;
    }
    if (c->n_views > 0) { c->zombie = true; return; } // its views still render this scene
    destroy_now(c);
}

const char* grt_last_error(const grt_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int grt_set_option(grt_ctx* c, int option, int value)
{
    if (!c) return GRT_ERR_INVALID;
    c->order_ready = false; // prepared with the old options
    if (option == GRT_OPT_COUNTERS) c->opt_counters = value ? 1 : 0;
    else if (option == GRT_OPT_KERNEL) {
        if (value < 0 || value > GRT_KERNEL_MAX) { c->err = "GRT_OPT_KERNEL must be 0.." + std::to_string(GRT_KERNEL_MAX); return GRT_ERR_INVALID; }
        c->opt_kernel = value;
        c->cost_valid = false; // scheduling units differ between kernels
    }
    else if (option == GRT_OPT_FEEDBACK) { c->opt_feedback = value ? 1 : 0; c->opt_heavy_split = (value & 4) ? 1 : ((value & 2) ? 0 : 2); c->cost_valid = false;
                                             c->bv_epoch = ~0ull; /* (what the frames before taught — costs, and the bundle verdicts of mesh frames — is forgotten) */ }
    else if (option == GRT_OPT_HEAVY_THRESHOLD_X2) { c->opt_heavy_thr_x2 = std::max(2, value); }
    else if (option == GRT_OPT_HEAVY_CAP_DIV) { c->opt_heavy_cap_div = std::max(1, value); }
    else if (option == GRT_OPT_SWIZZLE) {
        if (value < 0) { c->err = "GRT_OPT_SWIZZLE must be >= 0"; return GRT_ERR_INVALID; }
        c->opt_swizzle = value;
    }
    else if (option == GRT_OPT_TILE_READY_MIN) { c->opt_tile_ready = std::min(64, std::max(1, value)); }
    else if (option == GRT_OPT_TILE_BAND) { c->opt_tile_band = std::max(0, value); }
    else if (option == GRT_OPT_TILE_LOOKAHEAD) { c->opt_tile_look = std::max(0, value); }
    else if (option == GRT_OPT_COLD_ESTIMATE) { c->opt_cold_estimate = std::min(2, std::max(0, value)); c->cost_valid = false; }
    else if (option == GRT_OPT_COLD_PARTS_PCT) { c->opt_cold_parts_pct = std::max(0, value); c->cost_valid = false; }
    else if (option == GRT_OPT_BUNDLE_ROUNDS) {
        if (value < 0 || value > kMaxBundleRounds) { c->err = "GRT_OPT_BUNDLE_ROUNDS must be 0.." + std::to_string(kMaxBundleRounds); return GRT_ERR_INVALID; }
        c->opt_bundle_rounds = value;
    }
    else if (option == GRT_OPT_BUNDLE_BUDGET) { c->opt_bundle_budget = std::max(1, value); c->bv_epoch = ~0ull; /* (a verdict is a statement about THIS budget) */ }
    else if (option == GRT_OPT_LANE_BUDGET) { c->opt_lane_budget = std::max(1, value); }
    else if (option == GRT_OPT_MESH_PRIMARY_WAVE) { c->opt_mesh_primary_wave = value < 0 ? 0 : (value > 2 ? 2 : value); }
    else if (option == GRT_OPT_BUNDLE_PREDICT) { c->opt_bundle_predict = value ? 1 : 0; c->bv_epoch = ~0ull; /* (verdicts start afresh) */ }
    else if (option == GRT_OPT_SINGLE_LOOKAHEAD) { c->opt_single_look = std::max(0, value); }
    else if (option == GRT_OPT_SINGLE_BAND) { c->opt_single_band = std::max(0, value); }
    else if (option == GRT_OPT_SIZE_CLASSES) { NOT_A_VIEW(c, "GRT_OPT_SIZE_CLASSES"); c->opt_size_classes = value ? 1 : 0; }
    else if (option == GRT_OPT_BVH_ROTATIONS) { NOT_A_VIEW(c, "GRT_OPT_BVH_ROTATIONS"); c->opt_bvh_rotations = value < 0 ? -1 : (value > 8 ? 8 : value); }
    else if (option == GRT_OPT_SPLIT_VOL_PCT) { NOT_A_VIEW(c, "GRT_OPT_SPLIT_VOL_PCT"); c->opt_split_vol_pct = std::max(1, value); }
    else if (option == GRT_OPT_SPLIT) { NOT_A_VIEW(c, "GRT_OPT_SPLIT"); c->opt_split = value < 0 ? -1 : std::min(1024, value); }
    else if (option == GRT_OPT_TILE_BAND_ABS) { c->opt_band_abs = std::max(0, value); }
    else if (option == GRT_OPT_OVF_CHUNKS) { c->opt_ovf_chunks = value; c->ovf_demand = 0; c->ovf_hist_n = 0; c->ovf_short = false; c->ovf_sized = false; }
    else if (option == GRT_OPT_OVF_ENTRIES) {
        if (value < 0 || value > (int)kTileOvfEntries) { c->err = "GRT_OPT_OVF_ENTRIES must be 0.." + std::to_string(kTileOvfEntries); return GRT_ERR_INVALID; }
        c->opt_ovf_entries = value;
    }
    else if (option == GRT_OPT_MAX_ITERS) { // (the steps travel in 27 bits of the tile's cost word: a limit the word cannot exceed could never be reported)
        if (value < 0 || (uint32_t)value > kCostStepsMask - 1u) { c->err = "GRT_OPT_MAX_ITERS: 0 (default) .. 2^27 - 2"; return GRT_ERR_INVALID; }
        c->opt_max_iters = value;
    }
    else if (option == GRT_OPT_COST_RADIUS) { c->opt_cost_radius = std::min(8, std::max(0, value)); }
    else if (option == GRT_OPT_TILE_PARTS2_PCT) { c->opt_tile_parts2_pct = std::min(100, std::max(0, value)); c->cost_valid = false; c->order_ready = false; }
    else if (option == GRT_OPT_TILE_PARTS4_PCT) { c->opt_tile_parts4_pct = std::min(100, std::max(0, value)); c->cost_valid = false; c->order_ready = false; }
    else if (option == GRT_OPT_STATIC_SHARP) { c->opt_static_sharp = value != 0; c->cost_valid = false; c->order_ready = false; }
    else if (option == GRT_OPT_ORDER_MULTI_MIN) { c->opt_order_multi_min = std::max(1, value); }
    else if (option == GRT_OPT_MESH_PARTS) { c->opt_mesh_parts = value != 0; c->cost_valid = false; c->order_ready = false; }
    else if (option == GRT_OPT_OVF_CLASSES) { c->opt_ovf_classes = value ? 1 : 0; c->cost_valid = false; c->order_ready = false; }
    else if (option == GRT_OPT_QUAD_PARTS) { c->opt_quad_parts = std::max(0, value); c->cost_valid = false; c->order_ready = false; } // (2: whatever the launch's size; > 2: and that many parts at most — testing)
    else if (option == GRT_OPT_TILE_PARTS_LOAD_PCT) { c->opt_tile_parts_load_pct = std::min(100000, std::max(0, value)); c->cost_valid = false; c->order_ready = false; }
    else if (option == GRT_OPT_TILE_PRIO_DIV) { c->opt_tile_prio = std::max(0, value); }
    else if (option == GRT_OPT_BWD_PLAIN_ATOMICS) { c->opt_bwd_plain = value ? 1 : 0; }
    else if (option == GRT_OPT_REFIT_MAX_AREA_PCT) { NOT_A_VIEW(c, "GRT_OPT_REFIT_MAX_AREA_PCT"); c->opt_refit_max_area_pct = std::max(0, value); }
    else if (option == GRT_OPT_ALPHA_CULL) { c->opt_alpha_cull = value ? 1 : 0; }
    else if (option == GRT_OPT_TILE_RESERVE) { c->opt_tile_reserve = std::min(63, std::max(-1, value)); }
    else if (option == GRT_OPT_LEAF_MAX) {
        if (value < 1 || value > (int)kLeafMaxPrims) { c->err = "GRT_OPT_LEAF_MAX must be 1..8"; return GRT_ERR_INVALID; }
        NOT_A_VIEW(c, "GRT_OPT_LEAF_MAX");
        c->opt_leaf_max = value; // takes effect at the next grt_build_bvh / grt_set_meshes
    }
    else { c->err = "grt_set_option: unknown option"; return GRT_ERR_INVALID; }
    return GRT_OK;
}

int grt_get_bvh_info(const grt_ctx* c, grt_bvh_info* o)
{
    if (!c || !o) return GRT_ERR_INVALID;
    const grt_ctx* sc = scene_of(c);
    memset(o, 0, sizeof(*o));
    o->n_particles = sc->n;
    o->n_proxies = sc->n_hittable;
    o->n_primitives = sc->gbvh.n_prims;
    o->n_nodes = sc->gbvh.n_prims ? sc->gbvh.n_prims - 1 : 0;
    o->height = sc->gbvh.height;
    o->mesh_faces = sc->n_faces;
    o->mesh_height = sc->mbvh.height;
    o->build_ms = sc->build_ms;
    o->mesh_update_ms = sc->mesh_update_ms;
    for (int k = 0; k < 3; k++) { o->scene_lo[k] = sc->gbvh.lo[k]; o->scene_hi[k] = sc->gbvh.hi[k]; }
    return GRT_OK;
}

// (testing) The depth of the Gaussian LBVH as a traversal meets it, WALKED on the host over a copy of the binary node records — independent
// of the level bookkeeping of the build, whose root level grt_get_bvh_info reports as `height` and the kernels size their stacks by.
int grt_debug_bvh_depth(grt_ctx* c, uint32_t* out_depth)
{
    if (!c || !out_depth) return GRT_ERR_INVALID;
    grt_ctx* sc = scene_of(c);
    *out_depth = 0;
    const uint32_t m = sc->gbvh.n_prims;
    if (m == 0 || (sc->gbvh.root_ref & kLeafBit) || !sc->gbvh.nodes) return GRT_OK;
    (void)hipSetDevice(sc->device);
    std::vector<float4> h((size_t)(m - 1) * 4);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h.data(), sc->gbvh.nodes, h.size() * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) {
        c->err = "grt_debug_bvh_depth: copy of the node records failed";
        return GRT_ERR_HIP;
    }
    std::vector<std::pair<uint32_t, uint32_t>> stack; // (node, depth counted in internal nodes)
    stack.emplace_back(0u, 1u);
    uint64_t visited = 0;
    while (!stack.empty()) {
        const auto [i, d] = stack.back();
        stack.pop_back();
        if (i >= m - 1 || ++visited > (uint64_t)m) { c->err = "grt_debug_bvh_depth: the node records are not a tree"; return GRT_ERR_LIMIT; }
        *out_depth = std::max(*out_depth, d);
        uint32_t ch[2];
        memcpy(&ch[0], &h[(size_t)i * 4 + 3].x, 4);
        memcpy(&ch[1], &h[(size_t)i * 4 + 3].y, 4);
        for (int k = 0; k < 2; k++)
            if (!(ch[k] & kLeafBit)) stack.emplace_back(ch[k], d + 1u);
    }
    return GRT_OK;
}

// (testing) Copy of a built tree as it lies in device memory, for tests/bvh_check.py; never on a render path.
int grt_debug_copy_tree(grt_ctx* c, int which, grt_debug_tree* o)
{
    if (!c || !o || (which != 0 && which != 1)) return GRT_ERR_INVALID;
    grt_ctx* sc = scene_of(c);
    if (which == 0 && !sc->built) { c->err = "grt_debug_copy_tree: no Gaussian BVH has been built"; return GRT_ERR_INVALID; }
    const DevBvh& b = which == 0 ? sc->gbvh : sc->mbvh;
    const uint32_t m = (which == 1 && sc->n_faces == 0) ? 0u : b.n_prims;
    const uint32_t n_nodes = (m > 0 && !(b.root_ref & kLeafBit) && b.nodes) ? m - 1u : 0u;
    const uint32_t rec_floats = which == 0 ? 16u : 12u;
    const float4* rec = which == 0 ? sc->d_rec : sc->d_tri;
    o->n_prims = m;
    o->n_nodes = n_nodes;
    o->height = m ? b.height : 0u;
    o->root_ref = m ? b.root_ref : kNoRoot;
    o->leaf_max = b.leaf_max;
    o->has_pieces = (which == 0 && sc->has_pieces) ? 1u : 0u;
    o->n_qnodes = (which == 0 && b.qnodes) ? n_nodes : 0u;
    o->n_pbox = (which == 0 && b.pbox) ? m : 0u;
    o->wide = kTileWide;
    o->rec_floats = rec_floats;
    (void)hipSetDevice(sc->device);
    if (hipDeviceSynchronize() != hipSuccess) { c->err = "grt_debug_copy_tree: hipDeviceSynchronize failed"; return GRT_ERR_HIP; }
    struct Part { void* dst; const void* src; size_t bytes; };
    const Part parts[] = {
        {o->nodes, b.nodes, (size_t)n_nodes * 4 * sizeof(float4)},
        {o->wnodes, b.wnodes, (size_t)n_nodes * 8 * sizeof(float4)},
        {o->qnodes, b.qnodes, (size_t)o->n_qnodes * 2 * kTileWide * sizeof(float4)},
        {o->pbox, b.pbox, (size_t)o->n_pbox * 2 * sizeof(float4)},
        {o->order, b.order, (size_t)m * sizeof(uint32_t)},
        {o->rec, rec, (size_t)m * rec_floats * sizeof(float)},
    };
    for (const Part& p : parts) {
        if (!p.dst || !p.bytes) continue;
        if (!p.src || hipMemcpy(p.dst, p.src, p.bytes, hipMemcpyDeviceToHost) != hipSuccess) {
            c->err = "grt_debug_copy_tree: copy of the tree failed";
            return GRT_ERR_HIP;
        }
    }
    return GRT_OK;
}

// Device memory held: by the scene this context renders (shared by a context and its views) and by this frame slot.
int grt_get_memory_info(const grt_ctx* c, grt_memory_info* o)
{
    if (!c || !o) return GRT_ERR_INVALID;
    const grt_ctx* sc = scene_of(c);
    memset(o, 0, sizeof(*o));
    const uint64_t n = sc->n, m = sc->gbvh.n_prims, nf = sc->n_faces, nv = sc->n_verts;
    uint64_t b = n * (3 + 3 + 4 + 1 + 48) * 4 + n * 16;                     // raw attributes + color0
    b += sc->cap_rec * 64;                                                    // proxy records
    b += sc->gbvh.cap_nodes * 64 + sc->gbvh.cap_order * 4;                    // binary nodes, order
    if (sc->gbvh.wnodes && m > 1) b += (m - 1) * 128;                         // 4-wide view
    if (sc->gbvh.qnodes && m > 1) b += (m - 1) * 32ull * kTileWide;           // 8-wide per-child view
    if (sc->gbvh.pbox) b += m * 32;
    if (sc->gbvh.level && m > 1) b += (m - 1) * 4;                            // levels, kept from the first refit on
    b += sc->upd_cap_n * (4 + 16 + 16 + 1) + sc->upd_cap_m * 32;              // scratch of grt_update_gaussians_device ...
    b += (sc->upd_flag ? 4 : 0) + (sc->upd_part ? kAreaParts * 8 : 0);
    b += nf * (48 + 12) + nv * 12 + sc->mbvh.cap_nodes * 64 + sc->mbvh.cap_order * 4 + (sc->mbvh.wnodes && nf > 1 ? (nf - 1) * 128 : 0) +
         (sc->mbvh.level && nf > 1 ? (nf - 1) * 4 : 0);
    o->scene_bytes = b;
    o->alpha_cull_bytes = sc->gbvh.pbox_a ? m * 32 : 0;                       // (beside scene_bytes, whose sum stays the one of the arrays above)
    uint64_t v = (uint64_t)c->cap_erec * 16 + (uint64_t)c->cap_erec_wide * 64;
    v += (uint64_t)c->ovf_chunks * kTileOvfChunkBytes;
    v += (uint64_t)c->cost_cap * 12;
    v += (uint64_t)c->wf_cap * (48 + 128 + 4 + 64);
    v += (uint64_t)c->gacc_cap * 64 + (uint64_t)c->gacc_sh_cap * 180; // backward pass: gradient rows, higher-SH buffer
    o->slot_bytes = v;
    o->overflow_pool_bytes = (uint64_t)c->ovf_chunks * kTileOvfChunkBytes;
    o->overflow_chunks = c->ovf_chunks;
    o->overflow_demand = c->ovf_demand;
    return GRT_OK;
}

} // extern "C"
