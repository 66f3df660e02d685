// grt_points.hip — point queries: density, occupancy and owner at 3-D points, with gradients (include/grt.h: grt_query_points,
// grt_backward_points).  The first unit that asks about a point of space and not about a ray.
//
// The proxy of particle i has Gaussian-space inradius s = sqrt(2 log(opacity / alpha_min)) (grt_device.h, above
// proxy_alpha_sphere_cc), so a point where opacity * response > alpha_min lies inside the insphere, the insphere inside the
// icosahedron, the icosahedron inside the leaf box: a depth-first walk of the binary tree (RenderArgs::nodes / rec, the loop of
// gps_round in grt_kround.h) with point-in-box tests visits every contributing particle and very little else.  A split particle
// has exactly one owning piece at a point (piece_owns at t = 0), and the cells overlap by a hair, so the owner's box holds the point.
//
// One point per lane, block kRoundBlock, the per-lane LDS stack stk[level * kRoundBlock] as deep as the tree (lane_launch).  The walk
// (walk_point) is written once and called with a functor, as sweep_events is:
//   k_query_points                 one walk; the five outputs by plain stores behind it.  No atomic, no wave operation, no buffer of the
//                                  context.  A NULL output is a wave-uniform branch on a kernel argument.
//   k_backward_points<GAUSS, POINTS> two walks through ONE call site: walk 0 forms V = prod (1 - a_j) (skipped when g_occupancy is NULL),
//                                  walk 1 forms dloss/da = g_D + g_O V / (1 - a) of every contributing particle below the 0.99 clamp
//                                  and its terms by alpha_terms<POINTS>(o = x, d = 0): d_val is -0, vv = mu - x exactly, ra.go collects
//                                  sum m and ra.gd stays 0 — no second text of the quaternion chain.  The walk is not
//                                  wave-convergent, so the Gaussians' terms go through scatter_own (per-lane float atomics into the
//                                  slot's gradient buffer; bwd_launch's set-up and k_bwd_flush stay the only ones).  GAUSS = false is
//                                  the points-only call: no atomic in its text, no buffer, no flush.
// The walks' order is the tree's, the same for every call on one tree: the forward and dloss/dx repeat bit for bit.
#include <cmath>
#include <cstring>
#include <string>

#include "grt_bwd.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "the point kernels keep gps_round's per-lane stack (grt_kround.h): its stride is the launch block size");

// The unit's arrays: the kernels' last argument (behind RenderArgs; behind RenderArgs and BwdArgs in the backward).
struct PointArgs {
    const float* points;   // [n][3]
    uint64_t n;
    float alpha_min;       // the call's (>= the scene's)
    grt_point_out out;     // forward
    const float* g_density;   // backward: upstreams [n], each may be null
    const float* g_occupancy;
    float* g_points;       // backward: [n][3] written, or null
};

// The depth-first walk of the Gaussian tree for the point x: on_hit(id, alpha) for every particle with alpha = min(0.99, opacity r) >
// alpha_min at x, once per particle (pieces: the owner's), in the tree's order.  Per lane, no wave operation.  a.root_ref != kNoRoot.
// NaN compares false: a NaN point descends nowhere and, in a tree that is one leaf, contributes nowhere.
template <class OnHit>
__device__ __forceinline__ void walk_point(const RenderArgs& a, uint32_t* __restrict__ stk, f3 x, float alpha_min, OnHit&& on_hit)
{
    uint32_t sp = 0;
    uint32_t cur = a.root_ref;
    while (true) {
        if (cur & kLeafBit) {
            const uint32_t first = leaf_first(cur), cnt = leaf_count(cur);
            for (uint32_t j = 0; j < cnt; j++) {
                const float4* __restrict__ r = a.rec + (size_t)(first + j) * 4;
                const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
                const f3 mu = mk3(r0.x, r0.y, r0.z);
                m33 A;
                A.a[0] = r1.x; A.a[1] = r1.y; A.a[2] = r1.z;
                A.a[3] = r2.x; A.a[4] = r2.y; A.a[5] = r2.z;
                A.a[6] = r3.x; A.a[7] = r3.y; A.a[8] = r3.z;
                const f3 y = matvec(A, sub3(x, mu));
                // (a piece of a split proxy answers only for the points of its cell)
                const uint32_t cellb = __float_as_uint(r3.w);
                if (!cellb || piece_owns(cellb, r0.w, y, mk3(0, 0, 0), 0.0f)) {
                    // response_from at d = 0: p_g = A (mu - x) = -y, term for term
                    const float alpha = fminf(0.99f, exp_nonpos(-0.5f * dot3(y, y)) * r1.w);
                    if (alpha > alpha_min) on_hit(__float_as_uint(r2.w), alpha);
                }
            }
            if (sp == 0) break;
            cur = stk[(--sp) * kRoundBlock];
        } else {
            const float4* __restrict__ q = a.nodes + (size_t)cur * 4;
            const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            const bool h0 = (x.x >= q0.x) && (x.x <= q0.w) && (x.y >= q0.y) && (x.y <= q1.x) && (x.z >= q0.z) && (x.z <= q1.y);
            const bool h1 = (x.x >= q1.z) && (x.x <= q2.y) && (x.y >= q1.w) && (x.y <= q2.z) && (x.z >= q2.x) && (x.z <= q2.w);
            const uint32_t c0 = __float_as_uint(q3.x), c1 = __float_as_uint(q3.y);
            if (h0 && h1) {
                stk[(sp++) * kRoundBlock] = c1;
                cur = c0;
            } else if (h0) {
                cur = c0;
            } else if (h1) {
                cur = c1;
            } else {
                if (sp == 0) break;
                cur = stk[(--sp) * kRoundBlock];
            }
        }
    }
}

// This lane's point (block blk of the swizzled grid); returns whether the lane owns an element.  live: there is something to walk.
__device__ __forceinline__ bool lane_point(const RenderArgs& a, const PointArgs& k, size_t& idx, f3& x, bool& live)
{
    const uint32_t blk = xcd_swizzle(blockIdx.x, a.n_blocks, a.swizzle_chunk);
    const uint64_t i = (uint64_t)blk * kBlock + threadIdx.x;
    idx = (size_t)i;
    x = mk3(0, 0, 0);
    live = false;
    if (i >= k.n) return false;
    x = mk3(k.points[i * 3], k.points[i * 3 + 1], k.points[i * 3 + 2]);
    const float big = 3.402823466e+38f; // (|v| <= FLT_MAX is false for NaN and for +-inf)
    live = (fabsf(x.x) <= big) && (fabsf(x.y) <= big) && (fabsf(x.z) <= big) && (a.root_ref != kNoRoot);
    return true;
}

__global__ __launch_bounds__(kBlock) void k_query_points(const RenderArgs a, const PointArgs k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    size_t idx;
    f3 x;
    bool live;
    const bool has_out = lane_point(a, k, idx, x, live);
    float dens = 0.0f, V = 1.0f, peak = 0.0f;
    uint32_t peak_id = GRT_PICK_NONE, n = 0;
    if (live) {
        walk_point(a, stk, x, k.alpha_min, [&](uint32_t id, float alpha) {
            dens += alpha;
            V *= (1.0f - alpha);
            if (alpha > peak || (alpha == peak && id < peak_id)) { // (of equal maxima the lowest id: the walk's order does not show)
                peak = alpha;
                peak_id = id;
            }
            n++;
        });
    }
    if (has_out) { // every element once per requested array
        if (k.out.density) k.out.density[idx] = dens;
        if (k.out.occupancy) k.out.occupancy[idx] = 1.0f - V;
        if (k.out.peak) k.out.peak[idx] = peak;
        if (k.out.peak_id) k.out.peak_id[idx] = peak_id;
        if (k.out.count) k.out.count[idx] = n;
    }
}

template <bool GAUSS, bool POINTS>
__global__ __launch_bounds__(kBlock) void k_backward_points(const RenderArgs a, const BwdArgs b, const PointArgs k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    size_t idx;
    f3 x;
    bool live;
    const bool has_out = lane_point(a, k, idx, x, live);
    float gD = 0.0f, gO = 0.0f;
    if (has_out) {
        if (k.g_density) gD = k.g_density[idx];
        if (k.g_occupancy) gO = k.g_occupancy[idx];
    }
    live = live && ((gD != 0.0f) || (gO != 0.0f)); // a point whose two upstream values are exactly 0 is not walked
    RayAcc ra;
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);
    float V = 1.0f;
    if (live) {
        // walk 0: V (nothing reads it without g_occupancy: a wave-uniform skip on a kernel argument); walk 1: the terms
#pragma unroll 1
        for (int pass = k.g_occupancy ? 0 : 1; pass < 2; pass++) {
            walk_point(a, stk, x, k.alpha_min, [&](uint32_t id, float alpha) {
                if (pass == 0) {
                    V *= (1.0f - alpha);
                } else if (alpha < 0.99f) { // (where the 0.99 clamp binds nothing goes into opacity, geometry or the point)
                    const float dLda = gD + (gO * V) / (1.0f - alpha);
                    float v[kVals];
                    alpha_terms<POINTS>(b, id, x, mk3(0, 0, 0), dLda, v, ra);
                    if constexpr (GAUSS) scatter_own(b.acc, id, v, true, false);
                }
            });
        }
    }
    if constexpr (POINTS) {
        if (has_out) { // dloss/dx = -sum m (a point that was not walked holds zeros)
            float* g = k.g_points + idx * 3;
            g[0] = 0.0f - ra.go.x; g[1] = 0.0f - ra.go.y; g[2] = 0.0f - ra.go.z;
        }
    }
}

} // namespace
} // namespace grt

using namespace grt;

// What both entry points refuse before they look at their outputs, and the arguments of the walk: the Gaussian side of the scene
// (meshes are ignored: the mesh side stays empty, and lane_launch sizes the stack by the Gaussian tree alone), the points as the work
// mapping, alpha_min resolved.
static int fill(grt_ctx* c, const float* d_points, uint64_t n, float alpha_min, RenderArgs* a, PointArgs* k, const char* fn)
{
    if (!c) return GRT_ERR_INVALID;
    if (n && !d_points) { c->err = std::string(fn) + ": null point buffer"; return GRT_ERR_INVALID; }
    if (n > 0xFFFFFFFFull * 64) { c->err = std::string(fn) + ": too many points"; return GRT_ERR_LIMIT; }
    const grt_ctx* sc = scene_of(c);
    if (!sc->built) { c->err = std::string(fn) + ": grt_build_bvh has not been called after the last upload"; return GRT_ERR_INVALID; }
    if (!std::isfinite(alpha_min)) { c->err = std::string(fn) + ": alpha_min is not finite"; return GRT_ERR_INVALID; }
    if (alpha_min != 0.0f && alpha_min < sc->alpha_min) {
        c->err = std::string(fn) + ": alpha_min " + std::to_string(alpha_min) + " is below the scene's " + std::to_string(sc->alpha_min) +
                 " (the proxies do not cover that set; build the tree at the smaller value)";
        return GRT_ERR_INVALID;
    }
    memset(a, 0, sizeof(*a));
    a->rec = sc->d_rec;
    a->nodes = sc->gbvh.nodes;
    a->root_ref = sc->gbvh.root_ref;
    a->n_prox = sc->gbvh.n_prims;
    a->has_pieces = sc->has_pieces ? 1u : 0u;
    a->mroot = kNoRoot;
    a->mode = 2;
    a->n_rays = n;
    a->n_blocks = (uint32_t)((n + kBlock - 1) / kBlock);
    a->swizzle_chunk = (uint32_t)c->opt_swizzle;
    a->err_word = c->d_err;
    memset(k, 0, sizeof(*k));
    k->points = d_points;
    k->n = n;
    k->alpha_min = alpha_min != 0.0f ? alpha_min : sc->alpha_min;
    return GRT_OK;
}

extern "C" {

int grt_query_points(grt_ctx* c, const float* d_points, uint64_t n, float alpha_min, const grt_point_out* out, void* stream)
{
    const char* fn = "grt_query_points";
    RenderArgs a;
    PointArgs k;
    int rc = fill(c, d_points, n, alpha_min, &a, &k, fn);
    if (rc != GRT_OK) return rc;
    if (!out || (!out->density && !out->occupancy && !out->peak && !out->peak_id && !out->count)) {
        c->err = std::string(fn) + ": no output (density, occupancy, peak, peak_id and count are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no point: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: no point is live and every element gets the zeros row)
    k.out = *out;
    void* args[2] = {&a, &k};
    rc = lane_launch(c, a, reinterpret_cast<const void*>(k_query_points), args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

int grt_backward_points(grt_ctx* c, const float* d_points, uint64_t n, float alpha_min, const grt_point_upstream* up,
                        const grt_point_grads* grads, void* stream)
{
    const char* fn = "grt_backward_points";
    RenderArgs a;
    PointArgs k;
    int rc = fill(c, d_points, n, alpha_min, &a, &k, fn);
    if (rc != GRT_OK) return rc;
    if (!grads || (!grads->pos && !grads->scale && !grads->quat && !grads->opacity && !grads->points)) {
        c->err = std::string(fn) + ": no output (pos, scale, quat, opacity and points are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (!up || (!up->g_density && !up->g_occupancy)) {
        c->err = std::string(fn) + ": no upstream (g_density and g_occupancy are both NULL)";
        return GRT_ERR_INVALID;
    }
    k.g_density = up->g_density;
    k.g_occupancy = up->g_occupancy;
    k.g_points = grads->points;
    grt_gaussian_grads g;
    g.pos = grads->pos; g.scale = grads->scale; g.quat = grads->quat; g.opacity = grads->opacity; g.sh = nullptr;
    // [0]: the points-only kernel (also what writes the zeros on an empty scene or an empty tree); the walk is not wave-convergent, so
    // plain and merged atomics are one kernel
    static const void* const with_points[3] = {reinterpret_cast<const void*>(k_backward_points<false, true>),
                                               reinterpret_cast<const void*>(k_backward_points<true, true>),
                                               reinterpret_cast<const void*>(k_backward_points<true, true>)};
    static const void* const gauss_only[3] = {nullptr, reinterpret_cast<const void*>(k_backward_points<true, false>),
                                              reinterpret_cast<const void*>(k_backward_points<true, false>)};
    const bool pts = grads->points != nullptr;
    // (a.p: zeros — bwd_launch looks at sh_degree_max alone, and no sh array is asked for)
    return bwd_launch(c, &a.p, a, nullptr, nullptr, &g, BwdUnit{pts ? with_points : gauss_only, &k, pts}, stream, fn);
}

} // extern "C"
