// grt_bwd.h — the device text the units that walk a ray's composited events share (grt_backward.hip, grt_backward_rays.hip,
// grt_backward_mesh.hip, grt_stats.hip, grt_features.hip, grt_picks.hip, grt_events.hip, grt_segments.hip, and through grt_mesh_walk.h the
// five *_mesh feature units): the kernels' arguments, a
// lane's ray and upstream gradient, the sweep over a ray segment's composited events as a helper (sweep_events: the statistics, the
// feature, the pick and the event-list kernels call it, and mesh_walk of grt_mesh_walk.h once per iteration of a mesh frame's raygen
// loop; backward_body and k_backward_mesh keep the same loop written out, DESIGN.md 5.18 says why), the ONE
// grouping of a wave's lanes by particle (wave_groups), the terms of one composited event (event_terms, and below one alpha: alpha_terms),
// the scatter into the gradient buffer, and the ONE body of k_backward<MERGE> and k_backward_rays<MERGE, GAUSS>.
//
// One ray per lane, an 8x8 tile per wave, k = 7 rounds of gps_round (grt_kround.h: the round trace_gaussians of grt_render.hip
// runs, without its watchdog and counters), twice per ray:
//   sweep 0  re-derives rad and T_end (the forward's own arithmetic, so the same events in the same order);
//   sweep 1  walks the same events again and forms every composited event's terms with S_i = rad - C_<=i.
// (d_rgbf / d_alpha are not read: rad = rgbf / A and T_end = 1 - alpha lose what the float32 subtraction 1 - T lost — an absolute
//  6e-8 on a T_end that may be 1e-5.  The second sweep costs a traversal and keeps the float32 error at the formulas' own.)
// Scatter: float atomics into a context-owned AoS buffer (one 64-B row per particle: pos 3, scale 3, quat 4, opacity 1, degree-0
// colour 3, pad 2; the 45 higher SH floats in a second buffer touched only at degree >= 1), added into the caller's arrays by one
// streaming kernel that also zeroes the buffer.  MERGE: the lanes of the wave that composite the same particle in the same slot
// of their k-buffers reduce their 14 values over the wave first (DPP inside rows of 16, v_readlane across) and 14 lanes add one
// float each to the particle's contiguous row; a lane alone with its particle adds its own.  Only vector atomics write memory.
//
// Everything here is a template or __forceinline__ in an unnamed namespace: a unit holds the kernels it instantiates, nothing else.
#pragma once

#include <hip/hip_runtime.h>

#include "grt_device.h"
#include "grt_internal.h"
#include "grt_kround.h"
#include "grt_wave.h"

namespace grt {
namespace {

constexpr int K = 7;       // MaxNumHitPerTrace, shaders/tracer.cuh:11
constexpr int kBlock = 256;
static_assert(kBlock == kRoundBlock, "the per-lane stack stride of gps_round (grt_kround.h) is the launch block size");
constexpr int kRow = 16;   // floats per particle row of the gradient buffer
constexpr int kShHi = 45;  // floats per particle of the higher-SH buffer
constexpr int kVals = 14;  // pos 3, scale 3, quat 4, opacity 1, sh0 3

struct BwdArgs {
    const float* pos;      // [n][3] by original id (the uploaded attributes)
    const float* scale;    // [n][3]
    const float* quat;     // [n][4]
    const float* opacity;  // [n]
    const float* g_rgb;    // upstream [pixels or rays][3]
    const float* g_alpha;  // upstream [pixels or rays] or null
    float* acc;            // [n][kRow]
    float* acc_sh;         // [n][kShHi] (degree >= 1) or null
    uint32_t want_geom;    // pos / scale / quat / opacity asked for (else their terms are not formed)
    uint32_t want_sh;
};

// What one ray collects for grt_backward_ex (RAYS): -dloss/do, the geometry part of dloss/dd, and g_dn (include/grt.h)
struct RayAcc {
    f3 go, gd, gdn;
};
struct RayOut {
    float* rays;           // [pixels or rays][6], written
    uint32_t scatter_geom; // the caller asked for pos / scale / quat / opacity (b.want_geom is set for the rays' sake as well)
};
// sum_k (dY_k/dn)(dn) c_k with c_k = sh_k . gL: the polynomials of sh_basis differentiated in x, y, z (deg >= 1)
__device__ __forceinline__ f3 sh_basis_grad(const float* __restrict__ sh, f3 gL, f3 d, uint32_t deg)
{
#define GRT_SHC(i) (sh[(i) * 3] * gL.x + sh[(i) * 3 + 1] * gL.y + sh[(i) * 3 + 2] * gL.z)
    const float x = d.x, y = d.y, z = d.z;
    f3 g = mk3(-GRT_SH_C1 * GRT_SHC(3), -GRT_SH_C1 * GRT_SHC(1), GRT_SH_C1 * GRT_SHC(2));
    if (deg < 2u) return g;
    {
        const float c4 = GRT_SH_C2_0 * GRT_SHC(4), c5 = GRT_SH_C2_1 * GRT_SHC(5), c6 = GRT_SH_C2_2 * GRT_SHC(6);
        const float c7 = GRT_SH_C2_3 * GRT_SHC(7), c8 = GRT_SH_C2_4 * GRT_SHC(8);
        g.x += ((c4 * y + c7 * z) + 2.0f * (c8 - c6) * x);
        g.y += ((c4 * x + c5 * z) - 2.0f * (c8 + c6) * y);
        g.z += ((c5 * y + c7 * x) + 4.0f * c6 * z);
    }
    if (deg < 3u) return g;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
    const float c9 = GRT_SH_C3_0 * GRT_SHC(9), c10 = GRT_SH_C3_1 * GRT_SHC(10), c11 = GRT_SH_C3_2 * GRT_SHC(11);
    const float c12 = GRT_SH_C3_3 * GRT_SHC(12), c13 = GRT_SH_C3_4 * GRT_SHC(13), c14 = GRT_SH_C3_5 * GRT_SHC(14);
    const float c15 = GRT_SH_C3_6 * GRT_SHC(15);
    g.x += (((6.0f * c9 - 2.0f * c11) * xy + c10 * yz) + ((2.0f * c14 - 6.0f * c12) * xz + c13 * (4.0f * zz - 3.0f * xx - yy))) +
           3.0f * c15 * (xx - yy);
    g.y += (((3.0f * c9) * (xx - yy) + c10 * xz) + (c11 * (4.0f * zz - xx - 3.0f * yy) - (6.0f * c12 + 2.0f * c14) * yz)) -
           (2.0f * c13 + 6.0f * c15) * xy;
    g.z += ((c10 * xy + 8.0f * (c11 * yz + c13 * xz)) + (3.0f * c12) * (2.0f * zz - xx - yy)) + c14 * (xx - yy);
#undef GRT_SHC
    return g;
}

// the basis of sh_radiance (grt_device.h): L = max(0, 0.5 + sum_k Y[k] sh_k); Y[1 .. (deg + 1)^2 - 1] are filled (deg >= 1)
__device__ __forceinline__ void sh_basis(f3 d, uint32_t deg, float Y[16])
{
    const float x = d.x, y = d.y, z = d.z;
    Y[1] = -GRT_SH_C1 * y; Y[2] = GRT_SH_C1 * z; Y[3] = -GRT_SH_C1 * x;
    if (deg < 2u) return;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
    Y[4] = GRT_SH_C2_0 * xy; Y[5] = GRT_SH_C2_1 * yz; Y[6] = GRT_SH_C2_2 * (2.0f * zz - xx - yy);
    Y[7] = GRT_SH_C2_3 * xz; Y[8] = GRT_SH_C2_4 * (xx - yy);
    if (deg < 3u) return;
    Y[9] = (GRT_SH_C3_0 * y) * (3.0f * xx - yy);
    Y[10] = (GRT_SH_C3_1 * xy) * z;
    Y[11] = (GRT_SH_C3_2 * y) * (4.0f * zz - xx - yy);
    Y[12] = (GRT_SH_C3_3 * z) * (2.0f * zz - 3.0f * xx - 3.0f * yy);
    Y[13] = (GRT_SH_C3_4 * x) * (4.0f * zz - xx - yy);
    Y[14] = (GRT_SH_C3_5 * z) * (xx - yy);
    Y[15] = (GRT_SH_C3_6 * x) * (xx - 3.0f * yy);
}

// one lane's 14 values to its particle's row (geom: the 11 geometry / opacity values were formed; colour: the 3 colour values were)
__device__ __forceinline__ void scatter_own(float* __restrict__ acc, uint32_t id, const float v[kVals], bool geom, bool colour)
{
    float* row = acc + (size_t)id * kRow;
    if (geom) {
#pragma unroll
        for (int k = 0; k < 11; k++) atomicAdd(row + k, v[k]);
    }
    if (colour) {
#pragma unroll
        for (int k = 11; k < kVals; k++) atomicAdd(row + k, v[k]);
    }
}

// The wave merge, called by the WHOLE wave (ev: this lane has an event of particle id).  The lanes with an event are grouped by id
// (the lowest lane left leads, v_readlane hands its id round, a ballot finds its group); for every group of two or more lanes the
// whole wave calls on_group(id, mine, n, leader) — the group's id, whether this lane belongs to it, its size and its leader's lane —
// so on_group may hold wave operations.  Returns whether this lane is alone with its id: its own adds are the caller's, once the
// groups are done.  The loop is wave-uniform: todo is a ballot.
template <class OnGroup>
__device__ __forceinline__ bool wave_groups(bool ev, uint32_t id, OnGroup&& on_group)
{
    uint64_t todo = __builtin_amdgcn_ballot_w64(ev);
    bool solo = false;
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t lid = (uint32_t)__builtin_amdgcn_readlane((int)id, leader);
        const bool mine = ev && id == lid;
        const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
        todo &= ~m;
        const uint32_t n = (uint32_t)__builtin_popcountll(m);
        if (n == 1u) {
            solo = solo || mine;
            continue;
        }
        on_group(lid, mine, n, (uint32_t)leader);
    }
    return solo;
}

// Called by the WHOLE wave (ev: this lane has an event).  MERGE: lanes with the same particle add once.
template <bool MERGE>
__device__ __forceinline__ void scatter(float* __restrict__ acc, bool ev, uint32_t id, const float v[kVals], bool geom, bool colour, uint32_t lane)
{
    if (!MERGE) {
        if (ev) scatter_own(acc, id, v, geom, colour);
        return;
    }
    const bool solo = wave_groups(ev, id, [&](uint32_t lid, bool mine, uint32_t, uint32_t) {
        float out = 0.0f;
#pragma unroll
        for (int k = 0; k < kVals; k++) {
            const float s = wave_sum(mine ? v[k] : 0.0f);
            out = (lane == (uint32_t)k) ? s : out;
        }
        if (lane < (uint32_t)kVals && out != 0.0f) atomicAdd(acc + (size_t)lid * kRow + lane, out);
    });
    if (solo) scatter_own(acc, id, v, geom, colour);
}

// The chain below one event's alpha = min(0.99, opacity r): v[0..10] = dLda * d alpha / d (pos 3, scale 3, quat 4, opacity) of particle
// id for the ray (o, d), where the 0.99 clamp does not bind (the caller's test).  dLda: dloss/dalpha of the event — event_terms forms it
// from the radiance and the density behind the event, k_backward_events (grt_events.hip) is handed it.  RAYS: m = A^T g_p (v[0..2])
// goes to the origin's and d_val m to the direction's gradient in ra.
template <bool RAYS>
__device__ __forceinline__ void alpha_terms(const BwdArgs& b, uint32_t id, f3 o, f3 d, float dLda, float v[kVals], RayAcc& ra)
{
    const f3 mu = mk3(b.pos[id * 3], b.pos[id * 3 + 1], b.pos[id * 3 + 2]);
    const float opac = b.opacity[id];
    const float is[3] = {1.0f / b.scale[id * 3], 1.0f / b.scale[id * 3 + 1], 1.0f / b.scale[id * 3 + 2]};
    const float qw = b.quat[id * 4], qx = b.quat[id * 4 + 1], qy = b.quat[id * 4 + 2], qz = b.quat[id * 4 + 3];
    float Rg[9];
    mat3_cast(qw, qx, qy, qz, Rg);
    m33 A; // as k_gather_records forms it (grt_scene.hip)
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) A.a[r * 3 + c] = is[r] * Rg[r * 3 + c];
    }
    // computeResponse (grt_device.h: response_from), keeping v = mu - (o + d_val d) and p_g = A v
    const f3 o_g = matvec(A, sub3(o, mu));
    const f3 d_g = matvec(A, d);
    const float d_val = -dot3(o_g, d_g) / fmaxf(1e-6f, dot3(d_g, d_g));
    const f3 vv = sub3(mu, add3(o, mul3s(d, d_val)));
    const f3 p_g = matvec(A, vv);
    const float r = exp_nonpos(-0.5f * dot3(p_g, p_g));
    v[10] = dLda * r;                 // d alpha / d opacity = r
    const float gr = -(dLda * opac) * r; // d r / d p_g = -r p_g
    const f3 gp = mk3(gr * p_g.x, gr * p_g.y, gr * p_g.z);
    // d/d mu = A^T g_p
    v[0] = A.a[0] * gp.x + A.a[3] * gp.y + A.a[6] * gp.z;
    v[1] = A.a[1] * gp.x + A.a[4] * gp.y + A.a[7] * gp.z;
    v[2] = A.a[2] * gp.x + A.a[5] * gp.y + A.a[8] * gp.z;
    if (RAYS) { // d p_g / d o = -A, d p_g / d d = -d_val A (at fixed d_val)
        ra.go = add3(ra.go, mk3(v[0], v[1], v[2]));
        ra.gd = add3(ra.gd, mk3(d_val * v[0], d_val * v[1], d_val * v[2]));
    }
    // d/d s_k = -g_p,k (R^T v)_k / s_k^2 = -g_p,k p_g,k / s_k
    v[3] = -(gp.x * p_g.x) * is[0];
    v[4] = -(gp.y * p_g.y) * is[1];
    v[5] = -(gp.z * p_g.z) * is[2];
    // d/d R_jk = v_j g_p,k / s_k, then through glm::mat3_cast
    const float h[3] = {gp.x * is[0], gp.y * is[1], gp.z * is[2]};
    const float vj[3] = {vv.x, vv.y, vv.z};
    float G[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
#pragma unroll
        for (int k = 0; k < 3; k++) G[j][k] = vj[j] * h[k];
    }
    v[6] = 2.0f * (((qz * (G[1][0] - G[0][1])) + (qy * (G[0][2] - G[2][0]))) + (qx * (G[2][1] - G[1][2])));
    v[7] = 2.0f * ((((qy * (G[0][1] + G[1][0])) + (qz * (G[0][2] + G[2][0]))) + (qw * (G[2][1] - G[1][2]))) -
                   2.0f * qx * (G[1][1] + G[2][2]));
    v[8] = 2.0f * ((((qx * (G[0][1] + G[1][0])) + (qz * (G[1][2] + G[2][1]))) + (qw * (G[0][2] - G[2][0]))) -
                   2.0f * qy * (G[0][0] + G[2][2]));
    v[9] = 2.0f * ((((qx * (G[0][2] + G[2][0])) + (qy * (G[1][2] + G[2][1]))) + (qw * (G[1][0] - G[0][1]))) -
                   2.0f * qz * (G[0][0] + G[1][1]));
}

// The terms of one composited event (sweep 1): v[0..13] = what it adds to pos 3, scale 3, quat 4, opacity, sh_0 3 of particle id (the
// higher SH coefficients go to their buffer from here: one lane, one direction — nothing to merge across the wave).  T: the
// transmittance before the event; S: what lies behind it (rad - C_<=i).  Returns whether the geometry / opacity terms were formed.
// GAUSS: the Gaussians' gradients are wanted at all (else no atomic is in the text); RAYS: the event's part of the ray's gradient
// goes to ra — m = A^T g_p (v[0..2]) to the origin, d_val m to the direction, the colour's direction derivative to g_dn.
// GAUSS guards the SH block and NOTHING else: grt_depth_mesh.hip calls event_terms<false, false> for its geometry / opacity terms.
template <bool GAUSS, bool RAYS>
__device__ __forceinline__ bool event_terms(const RenderArgs& a, const BwdArgs& b, uint32_t id, f3 o, f3 d, f3 dn, f3 L, float T, float hitAlpha,
                                            f3 S, f3 g_rad, float gAp, float Tend, float v[kVals], RayAcc& ra)
{
    bool geom = false;
    const float w = T * hitAlpha;
    const float inv1 = 1.0f / (1.0f - hitAlpha);
    const float dLda = (g_rad.x * (T * L.x - S.x * inv1) + g_rad.y * (T * L.y - S.y * inv1) + g_rad.z * (T * L.z - S.z * inv1)) +
                       gAp * Tend * inv1;
    // colour: dloss/dL_c = T alpha g_rad_c where L_c > 0
    const f3 gL = mk3(L.x > 0.0f ? w * g_rad.x : 0.0f, L.y > 0.0f ? w * g_rad.y : 0.0f, L.z > 0.0f ? w * g_rad.z : 0.0f);
    if (GAUSS && b.want_sh) {
        v[11] = GRT_SH_C0 * gL.x; v[12] = GRT_SH_C0 * gL.y; v[13] = GRT_SH_C0 * gL.z;
        if (a.p.sh_degree_max > 0u) { // the higher coefficients: one lane, one direction — no merge across the wave
            float Y[16];
            sh_basis(dn, a.p.sh_degree_max, Y);
            float* hi = b.acc_sh + (size_t)id * kShHi;
            const uint32_t nb = (a.p.sh_degree_max + 1u) * (a.p.sh_degree_max + 1u);
#pragma unroll
            for (uint32_t k = 1; k < 16; k++) {
                if (k < nb) {
                    atomicAdd(hi + (k - 1) * 3 + 0, Y[k] * gL.x);
                    atomicAdd(hi + (k - 1) * 3 + 1, Y[k] * gL.y);
                    atomicAdd(hi + (k - 1) * 3 + 2, Y[k] * gL.z);
                }
            }
        }
    }
    if constexpr (RAYS) {
        if (a.p.sh_degree_max > 0u) ra.gdn = add3(ra.gdn, sh_basis_grad(a.sh + (size_t)id * 48, gL, dn, a.p.sh_degree_max));
    }
    if (b.want_geom && hitAlpha < 0.99f) { // (where the 0.99 clamp binds nothing goes into opacity or geometry)
        geom = true;
        alpha_terms<RAYS>(b, id, o, d, dLda, v, ra);
    }
    return geom;
}

// This lane's ray: from the ray buffer, or of its pixel of the window (block blk of the swizzled grid, 16x16 pixels, an 8x8 tile per
// wave).  idx: the element of the upstream arrays and of the per-ray output; has_out: the lane owns that element (a ray of the
// buffer, a pixel of the window).  Returns whether there is a ray to trace (a fisheye pixel outside the image circle has none).
__device__ __forceinline__ bool lane_ray(const RenderArgs& a, uint32_t& lane, f3& o, f3& d, size_t& idx, bool& has_out)
{
    const uint32_t blk = xcd_swizzle(blockIdx.x, a.n_blocks, a.swizzle_chunk);
    const uint32_t wave = threadIdx.x >> 6;
    lane = threadIdx.x & 63u;
    const uint32_t lx = (wave & 1u) * 8u + (lane & 7u), ly = (wave >> 1) * 8u + (lane >> 3);
    idx = 0;
    has_out = false;
    bool live = false;
    o = mk3(0, 0, 0); d = mk3(0, 0, 1);
    if (a.mode == 2) { // ray buffer
        const uint64_t i = (uint64_t)blk * kBlock + threadIdx.x;
        if (i < a.n_rays) {
            const float* r = a.rays + i * 6;
            o = mk3(r[0], r[1], r[2]);
            d = mk3(r[3], r[4], r[5]);
            idx = (size_t)i;
            live = has_out = true;
        }
    } else { // window of the full frame
        const uint32_t px = a.x0 + (blk % a.nbx) * 16u + lx;
        const uint32_t py = a.y0 + (blk / a.nbx) * 16u + ly;
        idx = (size_t)py * a.p.width + px;
        if ((px < a.x1) && (py < a.y1)) {
            const f3 nU = mk3(-a.p.U[0], -a.p.U[1], -a.p.U[2]), nV = mk3(-a.p.V[0], -a.p.V[1], -a.p.V[2]);
            const f3 W = mk3(a.p.W[0], a.p.W[1], a.p.W[2]);
            live = has_out = true;
            if (!a.p.mode_fisheye) get_ray(px, py, nU, nV, W, a.p.width, a.p.height, d);
            else live = get_fisheye_ray(px, py, nU, nV, W, a.p.width, a.p.height, d);
            o = mk3(a.p.eye[0], a.p.eye[1], a.p.eye[2]);
        }
    }
    return live;
}

// The upstream gradient of a live lane's element (else zeros).  Returns live, cleared where the upstream is zero: nothing is added.
__device__ __forceinline__ bool load_upstream(const BwdArgs& b, size_t idx, bool live, f3& gC, float& gA)
{
    gC = mk3(0, 0, 0);
    gA = 0.0f;
    if (live) {
        gC = mk3(b.g_rgb[idx * 3], b.g_rgb[idx * 3 + 1], b.g_rgb[idx * 3 + 2]);
        if (b.g_alpha) gA = b.g_alpha[idx];
        live = (gC.x != 0.0f) || (gC.y != 0.0f) || (gC.z != 0.0f) || (gA != 0.0f);
    }
    return live;
}

// The ONE sweep over the events trace() composites on a ray segment (shaders/tracer.cuh:328-373): rounds of gps_round through its
// single call site until the segment [t_min, t_max] or the transmittance runs out, and per round the K slots of the k-buffer in
// order — the forward's events in the forward's order.  stk: the lane's LDS stack; part: this lane takes part at all; T: the
// transmittance, carried in and out (1, or what the ray's earlier segments left).  For every slot of every round the WHOLE wave calls
// on_slot(ev, id, Tb, hitAlpha, key) once: ev — this lane composites an event in the slot, of particle id with alpha hitAlpha, at
// transmittance Tb before it, under the k-buffer's key (key_t: the event's distance; ev false: id 0, nothing to use); T *= 1 -
// hitAlpha follows the call.
//
// Wave convergence: on_slot may hold wave operations (scatter<MERGE>: DPP, v_readlane), so every lane of the wave reaches it for
// every slot of every round.  The round loop is entered and left on a ballot over the lanes' own `act`, the slot loop has a constant
// trip count, and a lane whose own condition is false idles inside them with `act` cleared.  The round itself is the per-lane
// gps_round inside `if (act)`, with no wave operation in it.  A lane's rounds are bounded by lastT rising past the segment's end:
// the ballot becomes zero.  A caller that loops around the sweep (passes) enters and leaves its loops the same way.
// leave() (optional, per lane, no wave operation): asked between two rounds of a lane that was still in the sweep; true takes the lane
// out of it (`act` cleared).  grt_mesh_walk.h hands it on for k_backward_events_mesh; every other caller leaves it defaulted.
// backward_body, k_backward_mesh and the mesh kernels that grt_mesh_walk.h's head lists as left out (k_ray_events_mesh,
// k_render_features_mesh, k_backward_features_mesh, k_backward_depth_mesh) hold this loop written out, statement for statement: a change
// here is a change there.  The mesh frames' raygen loop around the sweep is mesh_walk of grt_mesh_walk.h.
struct NeverLeave {
    __device__ __forceinline__ bool operator()() const { return false; }
};
template <class OnSlot, class Leave = NeverLeave>
__device__ __forceinline__ void sweep_events(const RenderArgs& a, uint32_t* stk, f3 o, f3 d, const rayinv& ri, float t_max, bool part, float& T,
                                             OnSlot&& on_slot, Leave&& leave = Leave())
{
    const float epsT = 1e-9f;
    const float t_hi = t_max + epsT;
    const float minT = a.p.minTransmittance;
    const uint64_t key0 = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
    KBuf<K> kb;
    grt::Cnt cnt; // (dead: no counters, no watchdog; grt::Cnt is the round's, grt_kround.h — Cnt alone would be grt_wave.h's)
    float lastT = a.p.t_min;
    uint64_t last_key = key0;
    bool act = part && (lastT <= t_max) && (T > minT);
    while (__builtin_amdgcn_ballot_w64(act)) {
        if (act) {
            gps_round<false, false, K>(a, stk, o, d, ri, last_key, t_hi, kb, cnt, 0xFFFFFFFFu);
            if (kb.key[0] == kKeyInvalid) act = false;
        }
#pragma unroll 1
        for (int i = 0; i < K; i++) {
            bool ev = false;
            uint32_t id = 0;
            uint64_t key = kKeyInvalid;
            float hitAlpha = 0.0f;
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (j == i) { key = kb.key[j]; hitAlpha = kb.alpha[j]; }
            }
            if (act && key != kKeyInvalid && T > minT) {
                lastT = fmaxf(key_t(key), lastT);
                if (a.p.alpha_min < hitAlpha) {
                    ev = true;
                    id = key_id(key);
                }
            }
            on_slot(ev, id, T, hitAlpha, key);
            if (ev) T *= (1.0f - hitAlpha);
        }
        if (act) {
            if (kb.key[K - 1] == kKeyInvalid) act = false;
            else last_key = kb.key[K - 1];
            act = act && (lastT <= t_max) && (T > minT);
            if (leave()) act = false;
        }
    }
}

// The body of k_backward<MERGE> (GAUSS = true, RAYS = false; ro unused) and of k_backward_rays<MERGE, GAUSS> (RAYS = true: every
// ray's six floats are written once, by plain stores — zeros for a ray that is not traced or whose upstream is zero; GAUSS = false:
// nothing is scattered).
template <bool MERGE, bool GAUSS, bool RAYS>
__device__ __forceinline__ void backward_body(const RenderArgs& a, const BwdArgs& b, const RayOut& ro)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out; // this lane's six floats are written whatever becomes of the wave
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out);
    // the raygen loop's guard (shaders/tracer.cu:59): such a ray renders, and differentiates, to nothing
    live = live && (length3(d) > 0.1f) && (a.p.max_bounces > 0u) && (a.root_ref != kNoRoot);
    f3 gC;
    float gA;
    live = load_upstream(b, idx, live, gC, gA);
    RayAcc ra;
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);
    if (!__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        if constexpr (RAYS) {
            if (has_out) {
#pragma unroll
                for (int k = 0; k < 6; k++) ro.rays[idx * 6 + k] = 0.0f;
            }
        }
        return;
    }

    const f3 dn = normalize3(d);
    const rayinv ri = mk_rayinv(o, d);
    const float epsT = 1e-9f;
    const float t_max = a.p.t_max;
    const float t_hi = t_max + epsT;
    const float minT = a.p.minTransmittance;
    const uint64_t key0 = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
    KBuf<K> kb;
    grt::Cnt cnt; // (dead: no counters, no watchdog; grt::Cnt is the round's, grt_kround.h — Cnt alone would be grt_wave.h's)

    // ---- two sweeps over the same events through ONE call site of the traversal (every lane of the wave in step: the scatter of
    //      sweep 1 is wave-cooperative).  Sweep 0: rad and T_end, trace() as the forward runs it (shaders/tracer.cuh:328-373);
    //      sweep 1: every composited event's terms ----
    f3 rad = mk3(0, 0, 0), g_rad = mk3(0, 0, 0);
    float Tend = 1.0f, gAp = 0.0f;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        float T = 1.0f, lastT = a.p.t_min;
        uint64_t last_key = key0;
        f3 C = mk3(0, 0, 0);
        bool act = live && (lastT <= t_max) && (T > minT);
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                gps_round<false, false, K>(a, stk, o, d, ri, last_key, t_hi, kb, cnt, 0xFFFFFFFFu);
                if (kb.key[0] == kKeyInvalid) act = false;
            }
#pragma unroll 1
            for (int i = 0; i < K; i++) {
                bool ev = false, geom = false;
                uint32_t id = 0;
                float v[kVals];
#pragma unroll
                for (int k = 0; k < kVals; k++) v[k] = 0.0f;
                uint64_t key = kKeyInvalid;
                float hitAlpha = 0.0f;
#pragma unroll
                for (int j = 0; j < K; j++) {
                    if (j == i) { key = kb.key[j]; hitAlpha = kb.alpha[j]; }
                }
                if (act && key != kKeyInvalid && T > minT) {
                    lastT = fmaxf(key_t(key), lastT);
                    if (a.p.alpha_min < hitAlpha) {
                        id = key_id(key);
                        const f3 L = event_radiance(a, id, dn);
                        C = add3(C, mul3s(mul3s(L, T), hitAlpha)); // (sweep 0: this is rad, term by term as the forward adds it)
                        if (pass == 0) {
                            rad = C;
                        } else {
                            ev = true;
                            geom = event_terms<GAUSS, RAYS>(a, b, id, o, d, dn, L, T, hitAlpha, sub3(rad, C), g_rad, gAp, Tend, v, ra);
                            if constexpr (RAYS) geom = geom && (ro.scatter_geom != 0u);
                        }
                        T *= (1.0f - hitAlpha);
                    }
                }
                if (GAUSS && pass) scatter<MERGE>(b.acc, ev, id, v, geom, b.want_sh != 0u, lane);
            }
            if (act) {
                if (kb.key[K - 1] == kKeyInvalid) act = false;
                else last_key = kb.key[K - 1];
                act = act && (lastT <= t_max) && (T > minT);
            }
        }
        if (pass == 0) {
            Tend = T;
            const float dens = clampf(1.0f - Tend, 0.0f, 1.0f); // grt_aux_out::alpha
            g_rad = mul3s(gC, dens);                            // rgbf = rad * A
            gAp = gA + dot3(gC, rad);                           // A = 1 - T_end enters through alpha and through rgbf
        }
    }
    if constexpr (RAYS) {
        if (has_out) { // dloss/do = -sum m; dloss/dd = -sum d_val m + (I - dn dn^T) g_dn / |d|   (a lane that was not live holds zeros)
            float* r = ro.rays + idx * 6;
            r[0] = 0.0f - ra.go.x; r[1] = 0.0f - ra.go.y; r[2] = 0.0f - ra.go.z;
            f3 pr = mk3(0, 0, 0);
            if (live && a.p.sh_degree_max > 0u) pr = mul3s(sub3(ra.gdn, mul3s(dn, dot3(dn, ra.gdn))), 1.0f / length3(d));
            r[3] = pr.x - ra.gd.x; r[4] = pr.y - ra.gd.y; r[5] = pr.z - ra.gd.z;
        }
    }
}

} // namespace
} // namespace grt
