// grt_scene.hip — the scene of a context (include/grt.h): the Gaussians (upload, BVH build driver, device update) and the meshes (set,
// update), with their kernels.  Each step is written once and each entry point reads as a list of named stages; the
// trees themselves are grt_bvh.hip's.  A view has no scene of its own: every entry point here refuses one.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <omp.h>

#include "grt_device.h"
#include "grt_internal.h"

using namespace grt;

// ------------------------------------------------------------------------------------------------
// scene kernels
// ------------------------------------------------------------------------------------------------

// Radius of a sphere about the box centre that holds the particle's alpha ellipsoid |A (x - mu)|^2 = R_a^2, R_a^2 = s^2 (1 +
// kAlphaSphereRel) + kAlphaSphereAbs being the very sphere the uncounted camera-ray pre-test asks about (grt_device.h:
// proxy_alpha_sphere_cc): its longest half-axis R_a max(scale), the product's rounding, and emax three times over for the distance
// between the box centre and mu, as the circumradius beside it.  A tile whose frustum stays outside this sphere has no ray the pre-test
// would pass, so a leaf step that culls with it (DevBvh::pbox_a) drops only trips that would have ended at the pre-test.
// ONLY the radius shrinks, never the box: the box's near faces bound every event's distance from below (lam, grt_tile.h) and its far
// faces decide what a later pass may skip, and the events are the ICOSAHEDRON's — a box fitted to the ellipsoid would let an event of
// a ray that does pass inside the sphere lie in front of its box, and a pass would call final what is not.
__device__ __forceinline__ float alpha_cull_radius(float s, const float* __restrict__ scale3, float emax)
{
    const float smax = fmaxf(fabsf(scale3[0]), fmaxf(fabsf(scale3[1]), fabsf(scale3[2])));
    return sqrtf((s * s) * (1.0f + kAlphaSphereRel) + kAlphaSphereAbs) * smax * (1.0f + 1e-5f) + 3.0f * emax;
}

// World AABB of the proxy icosahedron M = T * (R * diag(scale*s)) (src/GaussianTracer.cpp:304-311,
// src/geometry/Icosahedron.h:13-37).  opacity <= alpha_min gives s = NaN/0 in the reference, i.e. an
// unhittable instance: such particles get an inverted box and are left out of the BVH.
__global__ void k_proxy_boxes(const float* __restrict__ pos, const float* __restrict__ scale,
                              const float* __restrict__ quat, const float* __restrict__ s_arr, uint32_t n,
                              float4* __restrict__ lo, float4* __restrict__ hi)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float s = s_arr[i];
    if (!(s > 0.0f)) {
        lo[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
        hi[i] = make_float4(-1.0f, -1.0f, -1.0f, 0.0f);
        return;
    }
    const float rr = (3.0f + sqrtf(5.0f)) / (2.0f * sqrtf(3.0f));
    const float ss = 1.0f / rr;
    const float tt = (1.0f + sqrtf(5.0f)) / (2.0f * rr);
    const float V[12][3] = {{-ss, tt, 0}, {ss, tt, 0}, {-ss, -tt, 0}, {ss, -tt, 0}, {0, -ss, tt}, {0, ss, tt},
                            {0, -ss, -tt}, {0, ss, -tt}, {tt, 0, -ss}, {tt, 0, ss}, {-tt, 0, -ss}, {-tt, 0, ss}};
    float Rg[9];
    mat3_cast(quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3], Rg);
    const float sx = scale[i * 3] * s, sy = scale[i * 3 + 1] * s, sz = scale[i * 3 + 2] * s;
    float l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
    float r2 = 0.0f; // largest squared distance of a vertex from the centre
#pragma unroll
    for (int v = 0; v < 12; v++) {
        const float lx = sx * V[v][0], ly = sy * V[v][1], lz = sz * V[v][2];
        float q2 = 0.0f;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float wl = (Rg[0 * 3 + r] * lx + Rg[1 * 3 + r] * ly) + Rg[2 * 3 + r] * lz;
            const float w = wl + pos[i * 3 + r];
            l[r] = fminf(l[r], w);
            h[r] = fmaxf(h[r], w);
            q2 += wl * wl;
        }
        r2 = fmaxf(r2, q2);
    }
    float emax = 0.0f;
    bool finite = true;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float e = 1e-5f * (1.0f + fmaxf(fabsf(l[r]), fabsf(h[r])));
        l[r] -= e;
        h[r] += e;
        emax = fmaxf(emax, e);
        finite = finite && fabsf(l[r]) < INFINITY && fabsf(h[r]) < INFINITY;
    }
    // a NaN or infinite position, scale or rotation: the oracle's exact test never reports such a particle, and a box with one
    // finite axis would pass the builder's validity test (lo.x <= hi.x) and carry NaN into the scene bounds and every Morton key
    if (!finite) {
        lo[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
        hi[i] = make_float4(-1.0f, -1.0f, -1.0f, 0.0f);
        return;
    }
    // hi.w: radius of a sphere about the BOX CENTRE that holds the proxy (the vertices come in +- pairs, so the box centre is
    // the particle's position up to the rounding the box margin e covers many times over): what the tile kernel's leaf step
    // culls with besides the box, which for a round proxy reaches 1.5 x as far along an oblique plane normal.
    // lo.w: the alpha radius (alpha_cull_radius), which the builder puts in hi.w's place in its second box array.  Never above hi.w: for
    // s < 0.008 (an opacity within 3e-5 of alpha_min) the absolute part of R_a^2 outgrows the circumsphere, which holds every event there is
    const float r_circ = sqrtf(r2) * (1.0f + 1e-5f) + 3.0f * emax;
    lo[i] = make_float4(l[0], l[1], l[2], fminf(alpha_cull_radius(s, scale + i * 3, emax), r_circ));
    hi[i] = make_float4(h[0], h[1], h[2], r_circ);
}

// ---- spatial splits of large anisotropic proxies -------------------------------------------------------------------
// The LBVH bounds every proxy by its world AABB.  A needle or a sheet that is not axis-aligned fills a vanishing part of
// that box: a tile's thin frustum crosses thousands of such boxes without ever touching the proxies inside, and the
// traversal runs with a frontier that never clears (the C3a scene: 608 child boxes culled and 774 proxies slab-tested
// per ray for 67 composited events).  OptiX meets the same scene with an ORIENTED proxy per particle (an instance
// transform over 20 triangles, src/GaussianTracer.cpp:297-317,401-420).  Here a large proxy whose box is mostly empty
// enters the tree as several PIECES: the proxy-local box [-tt s, tt s]^3 (tt = 1.0705: the icosahedron's extent along
// its principal axes) is cut into p1 x p2 x p3 cells, each bounded by the world AABB of its cell, clipped to the
// proxy's own AABB.  Every piece refers to the WHOLE particle (the record is the particle's; the exact test is
// unchanged), the cells cover the proxy, so the piece that contains a ray's entry (exit) point is reached no later than
// that event: the hits are the same.  A ray that crosses several pieces of one particle meets it several times with
// bit-identical keys (t, id, entry/exit).  An EVENT BELONGS TO THE PIECE WHOSE CELL HOLDS ITS POINT (piece_owns,
// grt_device.h: the cell index of o_g + t d_g, from the descriptor in the record's last word), so each event is
// reported once; where the wave-per-tile kernels carry the exit with the entry a repeat is still possible (the entry
// is composited, then the exit's own piece turns up) and they drop it: an event at or before the last composited key is
// not inserted, and of equal keys that meet in a window only the first is composited.  Pure acceleration-structure
// work, as splitting is inside OptiX: pixels, hit counters and the oracle (which builds its own BVH) are untouched.
constexpr float kIcoTT = 1.0704663f; // (1 + sqrt 5) / (2 rr), rr = (3 + sqrt 5) / (2 sqrt 3): src/geometry/Icosahedron.h:15-17
constexpr uint32_t kMaxPieces = 512u;

struct PieceGrid { uint32_t p[3]; };

// how particle i is cut: pieces per principal axis (1,1,1 = not split).  tau = the piece length aimed at.
__device__ __forceinline__ PieceGrid piece_grid(const float* __restrict__ scale, const float* __restrict__ quat, float s, uint32_t i,
                                                float tau, float4 lo, float4 hi, float volf)
{
    PieceGrid g{{1u, 1u, 1u}};
    if (!(s > 0.0f) || !(tau > 0.0f) || !(lo.x <= hi.x)) return g; // (an unhittable proxy stays one inverted box)
    const float e[3] = {scale[i * 3] * s * kIcoTT, scale[i * 3 + 1] * s * kIcoTT, scale[i * 3 + 2] * s * kIcoTT};
    const float emin = fminf(e[0], fminf(e[1], e[2])), emax = fmaxf(e[0], fmaxf(e[1], e[2]));
    if (!(2.0f * emax > tau)) return g;
    float Rg[9];
    mat3_cast(quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3], Rg);
    float len = fmaxf(tau, 2.0f * emin); // cells about as long as the proxy is thick: their boxes come out compact
    uint32_t p[3];
    for (int it = 0; it < 16; it++) {
        for (int r = 0; r < 3; r++) p[r] = (uint32_t)fminf(fmaxf(ceilf(2.0f * e[r] / len), 1.0f), 32.0f); // (5 bits per axis: piece_desc)
        if (p[0] * p[1] * p[2] <= kMaxPieces) break;
        len *= 1.5f;
    }
    if (p[0] * p[1] * p[2] > kMaxPieces || p[0] * p[1] * p[2] <= 1u) return g;
    // worth it only when the cells' boxes hold much less than the proxy's box does (an axis-aligned needle gains nothing)
    float v1 = (float)(p[0] * p[1] * p[2]);
    for (int k = 0; k < 3; k++) {
        float h = 0.0f; // half-size of a cell's box along world axis k (column c of R = Rg[c*3 + k])
        for (int c = 0; c < 3; c++) h += fabsf(Rg[c * 3 + k]) * (e[c] / (float)p[c]);
        v1 *= fminf(2.0f * h, (k == 0) ? hi.x - lo.x : (k == 1) ? hi.y - lo.y : hi.z - lo.z);
    }
    const float v0 = (hi.x - lo.x) * (hi.y - lo.y) * (hi.z - lo.z);
    if (!(v1 < volf * v0)) return g;
    g.p[0] = p[0]; g.p[1] = p[1]; g.p[2] = p[2];
    return g;
}

// 64-bit sum of a 32-bit array (the piece total: the exclusive scan beside it runs in 32 bits and could wrap)
__global__ void k_sum_u32(const uint32_t* __restrict__ v, uint64_t n, unsigned long long* __restrict__ out)
{
    unsigned long long acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) acc += v[i];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63u) == 0u && acc) atomicAdd(out, acc);
}

__global__ void k_piece_counts(const float* __restrict__ scale, const float* __restrict__ quat, const float* __restrict__ s_arr,
                               const float4* __restrict__ lo, const float4* __restrict__ hi, uint32_t n, float tau, float volf,
                               uint32_t* __restrict__ counts)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PieceGrid g = piece_grid(scale, quat, s_arr[i], i, tau, lo[i], hi[i], volf);
    counts[i] = g.p[0] * g.p[1] * g.p[2];
}

// world box of cell kk of the p[0] x p[1] x p[2] grid over particle i's proxy-local box, clipped to the proxy's own box l .. h
// (k_piece_boxes at the build; k_refit_prim_boxes when the particle has moved: the cell stays, its box follows)
__device__ __forceinline__ void piece_cell_box(const float* __restrict__ pos, const float* __restrict__ scale, const float* __restrict__ quat,
                                               float s, uint32_t i, const uint32_t kk[3], const uint32_t p[3], float4 l, float4 h,
                                               float bl[3], float bh[3])
{
    float Rg[9];
    mat3_cast(quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3], Rg);
    float mid[3], half[3];
    for (int r = 0; r < 3; r++) {
        const float e = scale[i * 3 + r] * s * kIcoTT, w = 2.0f * e / (float)p[r];
        mid[r] = -e + ((float)kk[r] + 0.5f) * w;
        half[r] = 0.5f * w * (1.0f + 1e-5f) + 1e-6f * e; // the cells overlap by a hair: no point of the proxy falls between two
    }
    const float L[3] = {l.x, l.y, l.z}, H[3] = {h.x, h.y, h.z};
    for (int k = 0; k < 3; k++) {
        float c = pos[i * 3 + k], hw = 0.0f;
        for (int r = 0; r < 3; r++) { c += Rg[r * 3 + k] * mid[r]; hw += fabsf(Rg[r * 3 + k]) * half[r]; }
        const float m = 2e-5f * (1.0f + fabsf(c) + hw); // rounding of the nine products above, and then some
        bl[k] = fmaxf(c - hw - m, L[k]);
        bh[k] = fminf(c + hw + m, H[k]);
        if (!(bl[k] <= bh[k])) { bl[k] = L[k]; bh[k] = H[k]; } // (cannot happen: the cell meets the proxy's box)
    }
}

// one thread per piece: its owner by binary search in the offsets, its cell, its box
__global__ void k_piece_boxes(const float* __restrict__ pos, const float* __restrict__ scale, const float* __restrict__ quat,
                              const float* __restrict__ s_arr, const float4* __restrict__ lo, const float4* __restrict__ hi,
                              const uint32_t* __restrict__ offs, uint32_t n, uint32_t n_pieces, float tau, float volf,
                              float4* __restrict__ plo, float4* __restrict__ phi, uint32_t* __restrict__ owner,
                              uint32_t* __restrict__ desc)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pieces) return;
    desc[j] = 0u;
    uint32_t a = 0, b = n; // largest i with offs[i] <= j
    while (b - a > 1u) {
        const uint32_t m = (a + b) >> 1;
        if (offs[m] <= j) a = m; else b = m;
    }
    const uint32_t i = a;
    owner[j] = i;
    const float4 l = lo[i], h = hi[i];
    const PieceGrid g = piece_grid(scale, quat, s_arr[i], i, tau, l, h, volf);
    if (g.p[0] * g.p[1] * g.p[2] <= 1u) { plo[j] = l; phi[j] = h; return; }
    uint32_t q = j - offs[i];
    const uint32_t k0 = q % g.p[0]; q /= g.p[0];
    const uint32_t k1 = q % g.p[1], k2 = q / g.p[1];
    const uint32_t kk[3] = {k0, k1, k2};
    desc[j] = piece_desc(kk, g.p);
    float bl[3], bh[3];
    piece_cell_box(pos, scale, quat, s_arr[i], i, kk, g.p, l, h, bl, bh);
    plo[j] = make_float4(bl[0], bl[1], bl[2], INFINITY); // (a cell has no bounding sphere worth testing, of either kind: see k_proxy_boxes)
    phi[j] = make_float4(bh[0], bh[1], bh[2], INFINITY);
}

// sum over the hittable proxies of log(box diagonal), per workgroup (fixed order; the host adds the partials in double):
// exp(mean) is the typical proxy size the split length is a multiple of
__global__ void k_log_diag_partial(const float4* __restrict__ lo, const float4* __restrict__ hi, uint32_t n, float* __restrict__ part,
                                   uint32_t* __restrict__ cnt)
{
    float sum = 0.0f;
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 l = lo[i], h = hi[i];
        if (l.x <= h.x) {
            sum += logf(fmaxf(sqrtf((h.x - l.x) * (h.x - l.x) + (h.y - l.y) * (h.y - l.y) + (h.z - l.z) * (h.z - l.z)), 1e-30f));
            c++;
        }
    }
    for (int off = 32; off > 0; off >>= 1) { sum += __shfl_xor(sum, off); c += (uint32_t)__shfl_xor((int)c, off); }
    __shared__ float ssum[4];
    __shared__ uint32_t scnt[4];
    if ((threadIdx.x & 63) == 0) { ssum[threadIdx.x >> 6] = sum; scnt[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = ssum[0]; uint32_t k = scnt[0];
        for (uint32_t w = 1; w < (blockDim.x + 63u) / 64u; w++) { t += ssum[w]; k += scnt[w]; }
        part[blockIdx.x] = t; cnt[blockIdx.x] = k;
    }
}

// Proxy record in Morton order, 64 B = 4 x float4:
//   (mu.x mu.y mu.z s) (A00 A01 A02 opacity) (A10 A11 A12 id-bits) (A20 A21 A22 cell-bits)
// A = diag(1/scale) * R^T exactly as computeResponse forms it per hit (shaders/tracer.cuh:191-201).
// (owner / desc: piece -> particle and the piece's cell (piece_desc) when large proxies were split, else nullptr:
//  primitive = particle; the last word of the record is the cell descriptor, 0 for a whole proxy)
__device__ __forceinline__ void write_record(const float* __restrict__ pos, const float* __restrict__ scale, const float* __restrict__ quat,
                                             const float* __restrict__ opacity, const float* __restrict__ s_arr, uint32_t i, uint32_t cd,
                                             float4* rec)
{
    float Rg[9];
    mat3_cast(quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3], Rg);
    float A[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float inv = 1.0f / scale[i * 3 + r];
#pragma unroll
        for (int c = 0; c < 3; c++) A[r * 3 + c] = inv * Rg[r * 3 + c];
    }
    rec[0] = make_float4(pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2], s_arr[i]);
    rec[1] = make_float4(A[0], A[1], A[2], opacity[i]);
    rec[2] = make_float4(A[3], A[4], A[5], __uint_as_float(i));
    rec[3] = make_float4(A[6], A[7], A[8], __uint_as_float(cd));
}
__global__ void k_gather_records(const float* __restrict__ pos, const float* __restrict__ scale,
                                 const float* __restrict__ quat, const float* __restrict__ opacity,
                                 const float* __restrict__ s_arr, const uint32_t* __restrict__ order,
                                 const uint32_t* __restrict__ owner, const uint32_t* __restrict__ desc, uint32_t m,
                                 float4* __restrict__ rec)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = owner ? owner[order[j]] : order[j];
    const uint32_t cd = desc ? desc[order[j]] : 0u;
    write_record(pos, scale, quat, opacity, s_arr, i, cd, rec + (size_t)j * 4);
}

// ---- refit (grt_update_gaussians_device): the tree in hand keeps its sorted order; a sorted primitive's particle and
// cell are read from its OLD record (the id bits and the cell descriptor, which a refit never changes) ----
// boxes of the sorted primitives from the particles' new values: a whole proxy takes its new box (lo / hi by particle: k_proxy_boxes),
// a piece the new box of its old cell
__global__ void k_refit_prim_boxes(const float4* __restrict__ rec, const float* __restrict__ pos, const float* __restrict__ scale,
                                   const float* __restrict__ quat, const float* __restrict__ s_arr, const float4* __restrict__ lo,
                                   const float4* __restrict__ hi, uint32_t m, uint32_t n, float4* __restrict__ lb_lo, float4* __restrict__ lb_hi)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = min(__float_as_uint(rec[(size_t)j * 4 + 2].w), n - 1u); // (an id is < n: the clamp only keeps a damaged record in bounds)
    const uint32_t cd = __float_as_uint(rec[(size_t)j * 4 + 3].w);
    const float4 l = lo[i], h = hi[i];
    if (cd == 0u) { lb_lo[j] = l; lb_hi[j] = h; return; }
    uint32_t kk[3], p[3];
    for (int r = 0; r < 3; r++) { kk[r] = (cd >> (10 * r)) & 31u; p[r] = ((cd >> (10 * r + 5)) & 31u) + 1u; } // (piece_desc, grt_device.h)
    float bl[3], bh[3];
    piece_cell_box(pos, scale, quat, s_arr[i], i, kk, p, l, h, bl, bh);
    lb_lo[j] = make_float4(bl[0], bl[1], bl[2], INFINITY);
    lb_hi[j] = make_float4(bh[0], bh[1], bh[2], INFINITY);
}

// the records again, in place: each thread reads the two words it keeps before it writes its record
__global__ void k_regather_records(const float* __restrict__ pos, const float* __restrict__ scale, const float* __restrict__ quat,
                                   const float* __restrict__ opacity, const float* __restrict__ s_arr, uint32_t m, uint32_t n, float4* rec)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = min(__float_as_uint(rec[(size_t)j * 4 + 2].w), n - 1u);
    const uint32_t cd = __float_as_uint(rec[(size_t)j * 4 + 3].w);
    write_record(pos, scale, quat, opacity, s_arr, i, cd, rec + (size_t)j * 4);
}

// in_tree[i] = 1 for every particle a record names (in_tree zeroed before; the pieces of a particle all write the same byte)
__global__ void k_mark_in_tree(const float4* __restrict__ rec, uint32_t m, uint32_t n, uint8_t* __restrict__ in_tree)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = __float_as_uint(rec[(size_t)j * 4 + 2].w);
    if (i < n) in_tree[i] = 1u;
}

// does the set of particles with a valid new box (hittable and finite: k_proxy_boxes) differ from the set in the tree?
__global__ void k_set_changed(const float4* __restrict__ lo, const float4* __restrict__ hi, const uint8_t* __restrict__ in_tree, uint32_t n,
                              uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool valid = lo[i].x <= hi[i].x;
    if (valid != (in_tree[i] != 0u)) atomicOr(flag, 1u);
}

// degree-0 radiance max(0.5 + SH_C0 * sh[0], 0) (shaders/tracer.cuh:223,263), by original id
__global__ void k_color0(const float* __restrict__ sh, uint32_t n, float4* __restrict__ color0)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* s = sh + (size_t)i * 48;
    color0[i] = make_float4(fmaxf(0.5f + GRT_SH_C0 * s[0], 0.0f), fmaxf(0.5f + GRT_SH_C0 * s[1], 0.0f),
                            fmaxf(0.5f + GRT_SH_C0 * s[2], 0.0f), 0.0f);
}

__global__ void k_tri_boxes(const float* __restrict__ verts, const uint32_t* __restrict__ faces, uint32_t nf,
                            float4* __restrict__ lo, float4* __restrict__ hi)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    float l[3], h[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float a = verts[faces[f * 3] * 3 + k], b = verts[faces[f * 3 + 1] * 3 + k],
                    c = verts[faces[f * 3 + 2] * 3 + k];
        l[k] = fminf(a, fminf(b, c));
        h[k] = fmaxf(a, fmaxf(b, c));
        const float e = 1e-5f * (1.0f + fmaxf(fabsf(l[k]), fabsf(h[k])));
        l[k] -= e;
        h[k] += e;
    }
    lo[f] = make_float4(l[0], l[1], l[2], 0.0f);
    hi[f] = make_float4(h[0], h[1], h[2], 0.0f);
}

__global__ void k_gather_tris(const float* __restrict__ verts, const uint32_t* __restrict__ faces,
                              const uint32_t* __restrict__ order, uint32_t m, float4* __restrict__ tri)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t f = order[j];
    const uint32_t i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    tri[(size_t)j * 3 + 0] = make_float4(verts[i0 * 3], verts[i0 * 3 + 1], verts[i0 * 3 + 2], __uint_as_float(f));
    tri[(size_t)j * 3 + 1] = make_float4(verts[i1 * 3], verts[i1 * 3 + 1], verts[i1 * 3 + 2], 0.0f);
    tri[(size_t)j * 3 + 2] = make_float4(verts[i2 * 3], verts[i2 * 3 + 1], verts[i2 * 3 + 2], 0.0f);
}

// FNV-1a over the face indices of the meshes in the order given (grt_update_meshes checks the topology with it)
static uint64_t faces_hash(uint64_t h, const uint32_t* f, size_t n)
{
    if (h == 0) h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= f[i]; h *= 1099511628211ull; }
    return h;
}

// ---- what a scene owns ----
static void free_gaussians(grt_ctx* c)
{
    (void)hipFree(c->d_pos); (void)hipFree(c->d_scale); (void)hipFree(c->d_quat); (void)hipFree(c->d_opacity);
    (void)hipFree(c->d_sh); (void)hipFree(c->d_color0);
    c->d_pos = c->d_scale = c->d_quat = c->d_opacity = c->d_sh = nullptr;
    c->d_color0 = nullptr;
    c->n = 0;
    c->built = false;
}

// scratch of grt_update_gaussians_device
static void free_update_scratch(grt_ctx* c)
{
    (void)hipFree(c->upd_s); (void)hipFree(c->upd_lo); (void)hipFree(c->upd_hi); (void)hipFree(c->upd_lb_lo); (void)hipFree(c->upd_lb_hi);
    (void)hipFree(c->upd_in_tree); (void)hipFree(c->upd_flag); (void)hipFree(c->upd_part);
    c->upd_s = nullptr; c->upd_lo = c->upd_hi = c->upd_lb_lo = c->upd_lb_hi = nullptr;
    c->upd_in_tree = nullptr; c->upd_flag = nullptr; c->upd_part = nullptr;
    c->upd_cap_n = c->upd_cap_m = 0;
    if (c->ev_upd0) (void)hipEventDestroy(c->ev_upd0);
    if (c->ev_upd1) (void)hipEventDestroy(c->ev_upd1);
    c->ev_upd0 = c->ev_upd1 = nullptr;
}

static void free_meshes(grt_ctx* c)
{
    (void)hipFree(c->d_tri); (void)hipFree(c->d_faces); (void)hipFree(c->d_vnormals);
    c->d_tri = nullptr; c->d_faces = nullptr; c->d_vnormals = nullptr;
    c->n_faces = c->n_verts = 0;
    free_bvh(&c->mbvh);
}

void grt::free_scene_state(grt_ctx* c)
{
    free_gaussians(c); free_update_scratch(c); free_meshes(c); free_bvh(&c->gbvh); (void)hipFree(c->d_rec);
}

// ---- Gaussians: the steps the upload, the build and the device update share ----
// the refusals of the upload and of the update: a null array, more particles than a hit key can name
static int check_gaussian_arrays(grt_ctx* c, const grt_gaussians* g, uint64_t n, const char* fn)
{
    if (n && (!g || !g->pos || !g->scale || !g->quat || !g->opacity || !g->sh)) { c->err = std::string(fn) + ": null argument"; return GRT_ERR_INVALID; }
    if (n >= (1ull << 26)) { c->err = std::string(fn) + ": more than 2^26-1 particles (hit keys carry a 26-bit id)"; return GRT_ERR_LIMIT; }
    return GRT_OK;
}

// the library's own arrays by original particle id (the backward pass reads them) ...
static int alloc_attributes(grt_ctx* c, uint64_t n)
{
    CHK(c, hipMalloc(&c->d_pos, n * 3 * sizeof(float)));
    CHK(c, hipMalloc(&c->d_scale, n * 3 * sizeof(float)));
    CHK(c, hipMalloc(&c->d_quat, n * 4 * sizeof(float)));
    CHK(c, hipMalloc(&c->d_opacity, n * sizeof(float)));
    CHK(c, hipMalloc(&c->d_sh, n * 48 * sizeof(float)));
    CHK(c, hipMalloc(&c->d_color0, n * sizeof(float4)));
    return GRT_OK;
}
// ... filled from the caller's (kind: from the host for the upload, from the device for the update), and the degree-0 radiance from the new SH
static int copy_attributes(grt_ctx* c, const grt_gaussians* g, uint64_t n, hipMemcpyKind kind)
{
    CHK(c, hipMemcpyAsync(c->d_pos, g->pos, n * 3 * sizeof(float), kind, c->stream));
    CHK(c, hipMemcpyAsync(c->d_scale, g->scale, n * 3 * sizeof(float), kind, c->stream));
    CHK(c, hipMemcpyAsync(c->d_quat, g->quat, n * 4 * sizeof(float), kind, c->stream));
    CHK(c, hipMemcpyAsync(c->d_opacity, g->opacity, n * sizeof(float), kind, c->stream));
    CHK(c, hipMemcpyAsync(c->d_sh, g->sh, n * 48 * sizeof(float), kind, c->stream));
    hipLaunchKernelGGL(k_color0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_sh, (uint32_t)n, c->d_color0);
    CHK(c, hipGetLastError());
    return GRT_OK;
}

// Proxy half-width s = sqrtf(2 logf(opacity / alpha_min)) on the HOST, as the reference does (src/GaussianTracer.cpp:306): that keeps
// the libm-dependent value identical to the host libm's.  Counts the hittable particles (s > 0) as it goes.  Each
// element is computed by one thread from its own opacity: the same bits on one thread (under 65 536 particles) as on sixteen.
static void proxy_half_widths(const float* opacity, uint64_t n, float alpha_min, float* out_s, uint32_t* n_hittable)
{
    long long hits = 0;
#pragma omp parallel for num_threads(n < 65536 ? 1 : std::max(1, std::min(16, omp_get_max_threads()))) schedule(static) reduction(+ : hits)
    for (long long i = 0; i < (long long)n; i++) {
        out_s[i] = sqrtf(2.0f * logf(opacity[i] / alpha_min));
        hits += (out_s[i] > 0.0f) ? 1 : 0;
    }
    *n_hittable = (uint32_t)hits;
}

// ---- the Gaussian BVH and the proxy records, in stages (the device is idle when a build starts) ----
// what one build holds between its stages; the arrays are the holder's and go with it, behind finish_build's synchronisation
struct GaussianBuild {
    uint32_t n = 0, n_pieces = 0;                       // particles; primitives the tree is built over
    float* d_s = nullptr;                               // by particle: half-width, proxy box
    float4 *d_lo = nullptr, *d_hi = nullptr;
    uint32_t *d_cnt = nullptr, *d_offs = nullptr;       // pieces per particle at the piece length tau, their exclusive scan
    float tau = 0.0f, volf = 0.0f;
    uint64_t total = 0;                                 // ... and their sum
    float4 *d_plo = nullptr, *d_phi = nullptr;          // by piece, when large proxies are split: box, particle, cell (d_owner != nullptr:
    uint32_t *d_owner = nullptr, *d_desc = nullptr;     //   the tree is built over pieces)
    DevTemps tmp{&d_s, &d_lo, &d_hi, &d_cnt, &d_offs, &d_plo, &d_phi, &d_owner, &d_desc};
};

static int build_failed(grt_ctx* c, const char* what, hipError_t e)
{
    c->err = std::string("grt_build_bvh: ") + what + hipGetErrorString(e);
    return GRT_ERR_HIP;
}

static void reset_build_state(grt_ctx* c, float alpha_min)
{
    c->built = false;
    c->alpha_min = alpha_min;
    c->area_build = 0.0;
    c->gbvh.n_prims = 0;
    c->gbvh.root_ref = kNoRoot;
    c->gbvh.height = 0;
    c->has_pieces = false;
    c->built_opts[0] = c->opt_leaf_max; c->built_opts[1] = c->opt_size_classes; c->built_opts[2] = c->opt_split;
    c->built_opts[3] = c->opt_split_vol_pct; c->built_opts[4] = c->opt_bvh_rotations;
}

// s goes up, the build's clock starts behind it, every particle gets the world box of its proxy
static int proxy_boxes(grt_ctx* c, GaussianBuild& b, const float* s)
{
    hipError_t e;
    if ((e = hipMalloc(&b.d_s, b.n * sizeof(float))) != hipSuccess || (e = hipMalloc(&b.d_lo, b.n * sizeof(float4))) != hipSuccess ||
        (e = hipMalloc(&b.d_hi, b.n * sizeof(float4))) != hipSuccess)
        return build_failed(c, "hipMalloc: ", e);
    (void)hipMemcpyAsync(b.d_s, s, b.n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    (void)hipEventRecord(c->ev0, c->stream);
    hipLaunchKernelGGL(k_proxy_boxes, dim3((b.n + 255) / 256), dim3(256), 0, c->stream, c->d_pos, c->d_scale, c->d_quat, b.d_s, b.n, b.d_lo, b.d_hi);
    return GRT_OK;
}

// pieces at a given piece length: per-proxy counts (d_cnt), their exclusive scan (d_offs) and the total, summed in 64 bits (the scan runs in
// 32 bits: 512 pieces per particle times 2^26 particles could wrap it; a scene whose pieces would not fit the leaf index keeps whole proxies)
static int count_pieces(grt_ctx* c, GaussianBuild& b, float tau)
{
    const uint32_t n = b.n;
    b.tau = tau;
    hipLaunchKernelGGL(k_piece_counts, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_scale, c->d_quat, b.d_s, b.d_lo, b.d_hi, n, tau, b.volf, b.d_cnt);
    if (device_exclusive_scan_u32(b.d_cnt, b.d_offs, n, c->stream, &c->err) != GRT_OK) return GRT_ERR_HIP;
    unsigned long long* d_tot = nullptr;
    DevTemps tmp(&d_tot);
    unsigned long long h_tot = 0;
    hipError_t e = hipMalloc(&d_tot, sizeof(*d_tot));
    if (e == hipSuccess) e = hipMemsetAsync(d_tot, 0, sizeof(*d_tot), c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_sum_u32, dim3(std::min<uint32_t>((uint32_t)((n + 255) / 256), 1024u)), dim3(256), 0, c->stream, b.d_cnt, n, d_tot);
        if ((e = hipMemcpyAsync(&h_tot, d_tot, sizeof(h_tot), hipMemcpyDeviceToHost, c->stream)) == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) return build_failed(c, "piece total: ", e);
    b.total = h_tot;
    return GRT_OK;
}

// Spatial splits (see k_piece_boxes): the piece length tau = GRT_OPT_SPLIT / 4 x the geometric-mean proxy diagonal, and the pieces it gives.
static int choose_piece_length(grt_ctx* c, GaussianBuild& b)
{
    const uint32_t n = b.n;
    float* d_part = nullptr;
    uint32_t* d_pcnt = nullptr;
    DevTemps tmp(&d_part, &d_pcnt);
    const int grid = (int)std::min<uint32_t>((n + 255) / 256, 256u);
    std::vector<float> h_part(grid);
    std::vector<uint32_t> h_pcnt(grid);
    hipError_t e;
    if ((e = hipMalloc(&d_part, grid * sizeof(float))) != hipSuccess || (e = hipMalloc(&d_pcnt, grid * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&b.d_cnt, (size_t)n * sizeof(uint32_t))) != hipSuccess || (e = hipMalloc(&b.d_offs, (size_t)n * sizeof(uint32_t))) != hipSuccess)
        return build_failed(c, "hipMalloc(split): ", e);
    hipLaunchKernelGGL(k_log_diag_partial, dim3(grid), dim3(256), 0, c->stream, b.d_lo, b.d_hi, n, d_part, d_pcnt);
    (void)hipMemcpyAsync(h_part.data(), d_part, grid * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    (void)hipMemcpyAsync(h_pcnt.data(), d_pcnt, grid * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return build_failed(c, "", e);
    double sum = 0.0; uint64_t cnt = 0;
    for (int k = 0; k < grid; k++) { sum += h_part[k]; cnt += h_pcnt[k]; }
    if (!cnt) return GRT_OK; // (no hittable, finite proxy: nothing to cut)
    c->gm_diag = (float)std::exp(sum / (double)cnt);
    const float tau = 0.25f * (float)(c->opt_split < 0 ? 8 : c->opt_split) * c->gm_diag;
    if (!(tau > 0.0f)) return GRT_OK;
    b.volf = 0.01f * (float)c->opt_split_vol_pct;
    int rc = count_pieces(c, b, tau);
    // GRT_OPT_SPLIT < 0 (default): the piece length follows the scene.  Measured on the 1 M scene with per-axis log-scale noise sigma,
    // every proxy longer than the piece length cut (GRT_OPT_SPLIT_VOL_PCT = 400), kernel ms by length in quarters of the typical
    // diagonal (profiles/r06_experiments_log.md 9): sigma 0.7: 2.29 (6) 2.28 (8) 2.57 (12); 0.85: 2.46 (6) 2.50 (8) 2.63 (10); 1.0: 2.97 (6)
    // 3.00 (8) 3.45 (12); 1.2: 4.28 (6) 4.20 (8) 4.42 (10); 1.4: 8.31 (6) 7.67 (8) 7.60 (10) 8.07 (12); 1.6: 9.12 (8) 8.75 (10) 8.62 (12) 9.06
    // (16); 2.0: 70 (8) 59 (12) 53 (16).  Mildly anisotropic proxies want SHORT pieces, scene-sized needles long ones (every piece
    // re-tests its particle).  The primitives per proxy that cutting at 8 gives tell the scenes apart (1.10 / 1.16 / 1.23 / 1.37 /
    // 1.56 / 1.82 / 2.62 for the sigmas above): under 1.25 -> 6, under 1.5 -> 8, under 1.7 -> 10, under 2.2 -> 12, else 16; and a scene
    // that would gain under 2 % of primitives keeps whole proxies and the kernels without the piece logic (the benchmark scenes
    // C1-C5: cut finer they only lose, 1.78 -> 1.86 ms at 3 % of pieces).
    if (rc == GRT_OK && c->opt_split < 0) {
        const double r8 = (double)b.total / (double)n;
        const int q = r8 < 1.02 ? 8 : (r8 < 1.25 ? 6 : (r8 < 1.5 ? 8 : (r8 < 1.7 ? 10 : (r8 < 2.2 ? 12 : 16))));
        if (q != 8) rc = count_pieces(c, b, 0.25f * (float)q * c->gm_diag);
        c->split_used = q;
    } else {
        c->split_used = c->opt_split;
    }
    return rc;
}

// (a scene where splitting adds less than 2 % of primitives has no population of needles and sheets to speak of:
//  it keeps whole proxies — size classes deal with the odd large one — and the kernels without the piece logic)
static int make_pieces(grt_ctx* c, GaussianBuild& b)
{
    if (!(b.total > (uint64_t)b.n + b.n / 50u && b.total <= (uint64_t)kLeafIndexMask)) return GRT_OK;
    b.n_pieces = (uint32_t)b.total;
    hipError_t e;
    if ((e = hipMalloc(&b.d_plo, (size_t)b.n_pieces * sizeof(float4))) != hipSuccess || (e = hipMalloc(&b.d_phi, (size_t)b.n_pieces * sizeof(float4))) != hipSuccess ||
        (e = hipMalloc(&b.d_owner, (size_t)b.n_pieces * sizeof(uint32_t))) != hipSuccess || (e = hipMalloc(&b.d_desc, (size_t)b.n_pieces * sizeof(uint32_t))) != hipSuccess)
        return build_failed(c, "hipMalloc(pieces): ", e);
    hipLaunchKernelGGL(k_piece_boxes, dim3((b.n_pieces + 255) / 256), dim3(256), 0, c->stream, c->d_pos, c->d_scale, c->d_quat, b.d_s,
                       b.d_lo, b.d_hi, b.d_offs, b.n, b.n_pieces, b.tau, b.volf, b.d_plo, b.d_phi, b.d_owner, b.d_desc);
    return GRT_OK;
}

// the proxy records in the tree's order; d_rec grows when the tree holds more primitives than it has room for, and never shrinks
static int gather_records(grt_ctx* c, const GaussianBuild& b)
{
    const uint32_t m = c->gbvh.n_prims;
    if (!m) return GRT_OK;
    if (c->cap_rec < m) {
        (void)hipFree(c->d_rec);
        c->d_rec = nullptr;
        c->cap_rec = 0;
        const hipError_t e = hipMalloc(&c->d_rec, (size_t)m * 4 * sizeof(float4) + 256);
        if (e != hipSuccess) return build_failed(c, "hipMalloc(rec): ", e);
        c->cap_rec = m;
    }
    hipLaunchKernelGGL(k_gather_records, dim3((m + 255) / 256), dim3(256), 0, c->stream, c->d_pos, c->d_scale,
                       c->d_quat, c->d_opacity, b.d_s, c->gbvh.order, b.d_owner, b.d_owner ? b.d_desc : nullptr, m, c->d_rec);
    return GRT_OK;
}

// the build's clock stops, the stream is waited for (the temporaries go after this); what the frames remembered of the old tree is dropped
static int finish_build(grt_ctx* c, const GaussianBuild& b, int rc)
{
    if (rc == GRT_OK) {
        (void)hipEventRecord(c->ev1, c->stream);
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) rc = build_failed(c, "", e);
        else (void)hipEventElapsedTime(&c->build_ms, c->ev0, c->ev1);
    }
    c->have_timing = false;
    c->cost_valid = false;
    c->erec_valid = false;
    if (rc == GRT_OK) { c->built = true; c->built_leaf_max = c->opt_leaf_max; c->has_pieces = b.d_owner != nullptr; }
    return rc;
}

// The Gaussian BVH and the proxy records from the attributes in device memory and the half-widths s [c->n] the host computed, n_hittable
// of them > 0: the body of grt_build_bvh, shared with grt_update_gaussians_device.
static int build_gaussian_bvh(grt_ctx* c, float alpha_min, const float* s, uint32_t n_hittable)
{
    reset_build_state(c, alpha_min);
    if (c->n == 0) { c->built = true; return GRT_OK; }
    c->n_hittable = n_hittable;
    GaussianBuild b;
    b.n = b.n_pieces = (uint32_t)c->n;
    int rc = proxy_boxes(c, b, s);
    if (rc == GRT_OK && c->opt_split != 0 && b.n > 1) rc = choose_piece_length(c, b);
    if (rc == GRT_OK) rc = make_pieces(c, b);
    if (rc == GRT_OK)
        rc = build_lbvh(b.d_owner ? b.d_plo : b.d_lo, b.d_owner ? b.d_phi : b.d_hi, b.n_pieces, (uint32_t)c->opt_leaf_max, true, false,
                        c->opt_size_classes, &c->gbvh, c->stream, &c->err, b.d_owner != nullptr, c->opt_bvh_rotations);
    if (rc == GRT_OK) rc = gather_records(c, b);
    return finish_build(c, b, rc);
}

// ---- the device update, stage by stage (include/grt.h) ----
static int update_scratch_n(grt_ctx* c, uint64_t n)
{
    if (!c->ev_upd0) CHK(c, hipEventCreate(&c->ev_upd0));
    if (!c->ev_upd1) CHK(c, hipEventCreate(&c->ev_upd1));
    if (!c->upd_flag) CHK(c, hipMalloc(&c->upd_flag, sizeof(uint32_t)));
    if (!c->upd_part) CHK(c, hipMalloc(&c->upd_part, kAreaParts * sizeof(double)));
    if (c->upd_cap_n >= n) return GRT_OK;
    (void)hipFree(c->upd_s); (void)hipFree(c->upd_lo); (void)hipFree(c->upd_hi); (void)hipFree(c->upd_in_tree);
    c->upd_s = nullptr; c->upd_lo = c->upd_hi = nullptr; c->upd_in_tree = nullptr;
    c->upd_cap_n = 0;
    CHK(c, hipMalloc(&c->upd_s, n * sizeof(float)));
    CHK(c, hipMalloc(&c->upd_lo, n * sizeof(float4)));
    CHK(c, hipMalloc(&c->upd_hi, n * sizeof(float4)));
    CHK(c, hipMalloc(&c->upd_in_tree, n));
    c->upd_cap_n = n;
    return GRT_OK;
}
static int update_scratch_m(grt_ctx* c, uint64_t m)
{
    if (c->upd_cap_m >= m) return GRT_OK;
    (void)hipFree(c->upd_lb_lo); (void)hipFree(c->upd_lb_hi);
    c->upd_lb_lo = c->upd_lb_hi = nullptr;
    c->upd_cap_m = 0;
    CHK(c, hipMalloc(&c->upd_lb_lo, m * sizeof(float4)));
    CHK(c, hipMalloc(&c->upd_lb_hi, m * sizeof(float4)));
    c->upd_cap_m = m;
    return GRT_OK;
}

static const char* update_reason_text(uint32_t r)
{
    switch (r) {
    case GRT_UPDATE_REASON_FIRST_BUILD: return "no Gaussian BVH has been built";
    case GRT_UPDATE_REASON_N_CHANGED: return "the number of particles changed";
    case GRT_UPDATE_REASON_SET_CHANGED: return "the set of hittable, finite particles is not the one in the tree";
    case GRT_UPDATE_REASON_OPTION_CHANGED: return "a build option changed since the last build";
    case GRT_UPDATE_REASON_AREA: return "the refitted boxes grew past GRT_OPT_REFIT_MAX_AREA_PCT";
    default: return "none";
    }
}

// every array must be device memory of the context's GPU
static int check_device_pointers(grt_ctx* c, const grt_gaussians* g)
{
    const void* ptrs[5] = {g->pos, g->scale, g->quat, g->opacity, g->sh};
    static const char* const names[5] = {"pos", "scale", "quat", "opacity", "sh"};
    for (int k = 0; k < 5; k++) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof(at));
        const hipError_t e = hipPointerGetAttributes(&at, ptrs[k]);
        const bool dev_mem = e == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) && at.device == c->device;
        if (!dev_mem) {
            (void)hipGetLastError(); // (an unregistered host pointer leaves an error behind)
            c->err = std::string("grt_update_gaussians_device: ") + names[k] + " is not device memory of the context's GPU";
            return GRT_ERR_INVALID;
        }
    }
    return GRT_OK;
}

// can the tree in hand be refitted, as far as the host knows? (the last condition, the set of particles in it, is decided on the device)
static uint32_t refit_reason_on_host(const grt_ctx* c, uint64_t n)
{
    if (!c->built) return GRT_UPDATE_REASON_FIRST_BUILD;
    if (n != c->n) return GRT_UPDATE_REASON_N_CHANGED;
    if (c->built_opts[0] != c->opt_leaf_max || c->built_opts[1] != c->opt_size_classes || c->built_opts[2] != c->opt_split ||
        c->built_opts[3] != c->opt_split_vol_pct || c->built_opts[4] != c->opt_bvh_rotations)
        return GRT_UPDATE_REASON_OPTION_CHANGED;
    return GRT_UPDATE_REASON_NONE;
}

// the half-widths as grt_build_bvh computes them: the opacities come down, s goes up; the update's clock starts behind it
static int update_half_widths(grt_ctx* c, const grt_gaussians* g, uint64_t n, float alpha_min, uint32_t* n_hit)
{
    const int rc = update_scratch_n(c, n);
    if (rc != GRT_OK) return rc;
    c->upd_h_opacity.resize(n);
    c->upd_h_s.resize(n);
    CHK(c, hipMemcpy(c->upd_h_opacity.data(), g->opacity, n * sizeof(float), hipMemcpyDeviceToHost));
    proxy_half_widths(c->upd_h_opacity.data(), n, alpha_min, c->upd_h_s.data(), n_hit);
    CHK(c, hipMemcpyAsync(c->upd_s, c->upd_h_s.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    CHK(c, hipEventRecord(c->ev_upd0, c->stream));
    return GRT_OK;
}

// the new proxy boxes, from the CALLER's arrays (nothing of the scene is touched before the refit is known to be possible): is the set of
// particles with a valid box the one in the tree?
static int set_unchanged_on_device(grt_ctx* c, const grt_gaussians* g, uint32_t nn, bool* unchanged)
{
    const uint32_t m = c->gbvh.n_prims;
    uint32_t h_flag = 0;
    hipLaunchKernelGGL(k_proxy_boxes, dim3((nn + 255) / 256), dim3(256), 0, c->stream, g->pos, g->scale, g->quat, c->upd_s, nn, c->upd_lo, c->upd_hi);
    CHK(c, hipMemsetAsync(c->upd_in_tree, 0, nn, c->stream));
    CHK(c, hipMemsetAsync(c->upd_flag, 0, sizeof(uint32_t), c->stream));
    if (m) hipLaunchKernelGGL(k_mark_in_tree, dim3((m + 255) / 256), dim3(256), 0, c->stream, c->d_rec, m, nn, c->upd_in_tree);
    hipLaunchKernelGGL(k_set_changed, dim3((nn + 255) / 256), dim3(256), 0, c->stream, c->upd_lo, c->upd_hi, c->upd_in_tree, nn, c->upd_flag);
    CHK(c, hipMemcpyAsync(&h_flag, c->upd_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipGetLastError());
    *unchanged = h_flag == 0;
    return GRT_OK;
}

// the attributes, into the library's own arrays (the backward pass reads them by original id)
static int take_attributes(grt_ctx* c, const grt_gaussians* g, uint64_t n)
{
    if (n != c->n) {
        free_gaussians(c);
        if (n) { const int rc = alloc_attributes(c, n); if (rc != GRT_OK) return rc; }
    }
    c->h_opacity.assign(c->upd_h_opacity.begin(), c->upd_h_opacity.begin() + (n ? n : 0));
    if (n) { const int rc = copy_attributes(c, g, n, hipMemcpyDeviceToDevice); if (rc != GRT_OK) return rc; }
    c->n = n;
    c->have_timing = false;
    c->erec_valid = false;
    return GRT_OK;
}

// refit: primitive boxes, binary nodes by level, pbox / wnodes / qnodes, records; the child half-areas now against those of the tree as built
static int refit_tree(grt_ctx* c, uint32_t nn, float alpha_min, uint32_t n_hit, float* area_ratio, float* ms)
{
    const uint32_t m = c->gbvh.n_prims;
    double area_now = 0.0;
    if (m) {
        int rc = update_scratch_m(c, m);
        if (rc != GRT_OK) return rc;
        if (!(c->area_build > 0.0) && (rc = lbvh_child_area(&c->gbvh, c->upd_part, &c->area_build, c->stream, &c->err)) != GRT_OK) return rc;
        hipLaunchKernelGGL(k_refit_prim_boxes, dim3((m + 255) / 256), dim3(256), 0, c->stream, c->d_rec, c->d_pos, c->d_scale, c->d_quat, c->upd_s,
                           c->upd_lo, c->upd_hi, m, nn, c->upd_lb_lo, c->upd_lb_hi);
        if ((rc = refit_sorted_lbvh(c->upd_lb_lo, c->upd_lb_hi, &c->gbvh, c->has_pieces, c->stream, &c->err)) != GRT_OK) return rc;
        hipLaunchKernelGGL(k_regather_records, dim3((m + 255) / 256), dim3(256), 0, c->stream, c->d_pos, c->d_scale, c->d_quat, c->d_opacity, c->upd_s,
                           m, nn, c->d_rec);
        CHK(c, hipEventRecord(c->ev_upd1, c->stream));
        if ((rc = lbvh_child_area(&c->gbvh, c->upd_part, &area_now, c->stream, &c->err)) != GRT_OK) return rc;
    } else {
        CHK(c, hipEventRecord(c->ev_upd1, c->stream));
    }
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipGetLastError());
    c->alpha_min = alpha_min;
    c->n_hittable = n_hit;
    *area_ratio = (c->area_build > 0.0 && area_now > 0.0) ? (float)(area_now / c->area_build) : 1.0f;
    (void)hipEventElapsedTime(ms, c->ev_upd0, c->ev_upd1);
    return GRT_OK;
}

// ---- meshes: what grt_set_meshes and grt_update_meshes share ----
// Every primitive flattened into one world-space soup; face indices are offset per mesh in the order given (reference: one instance per
// primitive, instanceId = order of creation, src/GaussianTracer.cpp:592-593; lowest (mesh, face) wins exact-t ties).
struct FlatMeshes {
    std::vector<float> v, nrm;
    std::vector<uint32_t> f, nv, nf; // faces (grt_set_meshes only); per mesh, as given
    uint64_t hash = 0;               // faces_hash of the meshes in the order given
};
static int flatten_meshes(grt_ctx* c, const grt_mesh* meshes, uint32_t n_meshes, bool with_faces, const char* fn, FlatMeshes* o)
{
    for (uint32_t k = 0; k < n_meshes; k++) {
        const grt_mesh& m = meshes[k];
        if ((m.nv && (!m.verts || !m.normals)) || (m.nf && !m.faces)) { c->err = std::string(fn) + ": null array"; return GRT_ERR_INVALID; }
        const uint32_t base = (uint32_t)(o->v.size() / 3);
        o->nv.push_back(m.nv); o->nf.push_back(m.nf);
        o->hash = faces_hash(o->hash, m.faces, (size_t)m.nf * 3);
        o->v.insert(o->v.end(), m.verts, m.verts + (size_t)m.nv * 3);
        o->nrm.insert(o->nrm.end(), m.normals, m.normals + (size_t)m.nv * 3);
        for (size_t i = 0; with_faces && i < (size_t)m.nf * 3; i++) {
            if (m.faces[i] >= m.nv) { c->err = std::string(fn) + ": face index out of range"; return GRT_ERR_INVALID; }
            o->f.push_back(m.faces[i] + base);
        }
    }
    return GRT_OK;
}

// The device half of both calls, timed from ev0 to ev1: vertices and normals up (the set: its arrays made, the faces up as well), the
// triangles' boxes, the tree BUILT over them (the set) or REFITTED to them, the triangles gathered in the tree's order.
static int mesh_tree(grt_ctx* c, const FlatMeshes& fm, uint32_t nv, uint32_t nf, bool build, const char* fn)
{
    float* d_verts = nullptr;
    float4 *d_lo = nullptr, *d_hi = nullptr;
    DevTemps tmp(&d_verts, &d_lo, &d_hi);
    int rc = GRT_OK;
    // the temporaries; the arrays the set makes and the update overwrites; then the copies, the faces with the set only.  Every failure
    // falls through to the synchronisation below: the host vectors are borrowed by the async copies
    hipError_t e = hipMalloc(&d_verts, (size_t)nv * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&d_lo, (size_t)nf * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc(&d_hi, (size_t)nf * sizeof(float4));
    if (e == hipSuccess && build) e = hipMalloc(&c->d_vnormals, (size_t)nv * 3 * sizeof(float));
    if (e == hipSuccess && build) e = hipMalloc(&c->d_faces, (size_t)nf * 3 * sizeof(uint32_t));
    if (e == hipSuccess && build) e = hipMalloc(&c->d_tri, (size_t)nf * 3 * sizeof(float4));
    if (e == hipSuccess) e = hipMemcpyAsync(d_verts, fm.v.data(), (size_t)nv * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_vnormals, fm.nrm.data(), (size_t)nv * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && build) e = hipMemcpyAsync(c->d_faces, fm.f.data(), (size_t)nf * 3 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { c->err = std::string(fn) + ": " + hipGetErrorString(e); rc = GRT_ERR_HIP; }
    if (rc == GRT_OK) {
        (void)hipEventRecord(c->ev0, c->stream);
        hipLaunchKernelGGL(k_tri_boxes, dim3((nf + 255) / 256), dim3(256), 0, c->stream, d_verts, c->d_faces, nf, d_lo, d_hi);
        rc = build ? build_lbvh(d_lo, d_hi, nf, (uint32_t)c->opt_leaf_max, false, true, 0, &c->mbvh, c->stream, &c->err)
                   : refit_lbvh(d_lo, d_hi, nf, &c->mbvh, c->stream, &c->err);
    }
    if (rc == GRT_OK) {
        hipLaunchKernelGGL(k_gather_tris, dim3((nf + 255) / 256), dim3(256), 0, c->stream, d_verts, c->d_faces, c->mbvh.order, nf, c->d_tri);
        (void)hipEventRecord(c->ev1, c->stream);
        e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) { c->err = std::string(fn) + ": " + hipGetErrorString(e); rc = GRT_ERR_HIP; }
        else (void)hipEventElapsedTime(&c->mesh_update_ms, c->ev0, c->ev1);
    } else {
        (void)hipStreamSynchronize(c->stream);
    }
    return rc;
}

// ---- the scene entry points ----
extern "C" {

int grt_upload_gaussians(grt_ctx* c, const grt_gaussians* g, uint64_t n)
{
    if (!c) return GRT_ERR_INVALID;
    c->scene_epoch++; // (a refused call bumps it too)
    const int rc = check_gaussian_arrays(c, g, n, "grt_upload_gaussians");
    if (rc != GRT_OK) return rc;
    NOT_A_VIEW(c, "grt_upload_gaussians");
    CHK(c, hipSetDevice(c->device));
    CHK(c, hipDeviceSynchronize()); // frames of this scene may be in flight on any stream (caller's, views')
    free_gaussians(c);
    c->h_opacity.assign(g ? g->opacity : nullptr, g ? g->opacity + n : nullptr);
    if (n == 0) return GRT_OK;
    if (int e = alloc_attributes(c, n)) return e;
    if (int e = copy_attributes(c, g, n, hipMemcpyHostToDevice)) return e;
    CHK(c, hipStreamSynchronize(c->stream)); // host arrays are only borrowed for the call
    c->n = n;
    return GRT_OK;
}

int grt_build_bvh(grt_ctx* c, float alpha_min)
{
    if (!c) return GRT_ERR_INVALID;
    c->scene_epoch++;
    if (!(alpha_min > 0.0f)) { c->err = "grt_build_bvh: alpha_min must be > 0"; return GRT_ERR_INVALID; }
    NOT_A_VIEW(c, "grt_build_bvh");
    CHK(c, hipSetDevice(c->device));
    CHK(c, hipDeviceSynchronize());
    c->built = false;
    std::vector<float> s(c->n);
    uint32_t n_hittable = 0;
    proxy_half_widths(c->h_opacity.data(), c->n, alpha_min, s.data(), &n_hittable);
    return build_gaussian_bvh(c, alpha_min, s.data(), n_hittable);
}

int grt_update_gaussians_device(grt_ctx* c, const grt_gaussians* g, uint64_t n, float alpha_min, int mode, void* stream, grt_update_info* out)
{
    (void)stream; // (the device is synchronised below: that orders the reads after the work queued on this stream, and on every other)
    if (!c) return GRT_ERR_INVALID;
    if (out) memset(out, 0, sizeof(*out));
    // ---- refusals ----
    if (mode != GRT_UPDATE_AUTO && mode != GRT_UPDATE_REFIT && mode != GRT_UPDATE_REBUILD) { c->err = "grt_update_gaussians_device: unknown mode"; return GRT_ERR_INVALID; }
    if (!(alpha_min > 0.0f)) { c->err = "grt_update_gaussians_device: alpha_min must be > 0"; return GRT_ERR_INVALID; }
    int rc = check_gaussian_arrays(c, g, n, "grt_update_gaussians_device");
    if (rc != GRT_OK) return rc;
    NOT_A_VIEW(c, "grt_update_gaussians_device");
    CHK(c, hipSetDevice(c->device));
    if (n && (rc = check_device_pointers(c, g)) != GRT_OK) return rc;
    CHK(c, hipDeviceSynchronize()); // the caller's stream; frames of this scene in flight on any stream (caller's, views')
    // ---- can the tree in hand be refitted? ----
    uint32_t reason = mode != GRT_UPDATE_REBUILD ? refit_reason_on_host(c, n) : GRT_UPDATE_REASON_NONE;
    bool try_refit = mode != GRT_UPDATE_REBUILD && reason == GRT_UPDATE_REASON_NONE;
    uint32_t n_hit = 0;
    if (n && (rc = update_half_widths(c, g, n, alpha_min, &n_hit)) != GRT_OK) return rc;
    if (n && try_refit) {
        if ((rc = set_unchanged_on_device(c, g, (uint32_t)n, &try_refit)) != GRT_OK) return rc;
        if (!try_refit) reason = GRT_UPDATE_REASON_SET_CHANGED;
    }
    if (mode == GRT_UPDATE_REFIT && !try_refit) {
        c->err = std::string("grt_update_gaussians_device: a refit is not possible: ") + update_reason_text(reason) + " (the scene is unchanged)";
        return GRT_ERR_INVALID;
    }
    // ---- the scene changes from here on ----
    c->scene_epoch++;
    if ((rc = take_attributes(c, g, n)) != GRT_OK) return rc;
    float copy_ms = 0.0f;
    if (try_refit && n) {
        float area_ratio = 1.0f, ms = 0.0f;
        if ((rc = refit_tree(c, (uint32_t)n, alpha_min, n_hit, &area_ratio, &ms)) != GRT_OK) return rc;
        const bool guard = mode == GRT_UPDATE_AUTO && c->opt_refit_max_area_pct > 0 && !(area_ratio * 100.0f <= (float)c->opt_refit_max_area_pct);
        if (!guard) {
            if (out) { out->mode_used = GRT_UPDATE_REFIT; out->reason = GRT_UPDATE_REASON_NONE; out->device_ms = ms; out->area_ratio = area_ratio; }
            return GRT_OK;
        }
        reason = GRT_UPDATE_REASON_AREA; // the boxes of this hierarchy no longer fit the scene: build a new one, in the same call
        copy_ms = ms;
    } else if (try_refit) { // n = 0 then and now: nothing to refit
        if (out) { out->mode_used = GRT_UPDATE_REFIT; out->area_ratio = 1.0f; }
        return GRT_OK;
    } else if (n) {
        CHK(c, hipEventRecord(c->ev_upd1, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
        (void)hipEventElapsedTime(&copy_ms, c->ev_upd0, c->ev_upd1);
    }
    // ---- rebuild: grt_build_bvh's own body, from the s computed above ----
    if ((rc = build_gaussian_bvh(c, alpha_min, c->upd_h_s.data(), n_hit)) != GRT_OK) return rc;
    if (out) { out->mode_used = GRT_UPDATE_REBUILD; out->reason = reason; out->device_ms = copy_ms + (n ? c->build_ms : 0.0f); out->area_ratio = 1.0f; }
    return GRT_OK;
}

int grt_set_meshes(grt_ctx* c, const grt_mesh* meshes, uint32_t n_meshes)
{
    if (c) c->scene_epoch++;
    if (!c || (n_meshes && !meshes)) return GRT_ERR_INVALID;
    NOT_A_VIEW(c, "grt_set_meshes");
    CHK(c, hipSetDevice(c->device));
    CHK(c, hipDeviceSynchronize());
    free_meshes(c);
    FlatMeshes fm;
    int rc = flatten_meshes(c, meshes, n_meshes, true, "grt_set_meshes", &fm);
    c->mesh_nv = fm.nv; c->mesh_nf = fm.nf; c->faces_hash = fm.hash; // (what grt_update_meshes checks its topology against)
    if (rc != GRT_OK) return rc;
    const uint32_t nf = (uint32_t)(fm.f.size() / 3), nv = (uint32_t)(fm.v.size() / 3);
    if (nf == 0) return GRT_OK;
    if ((rc = mesh_tree(c, fm, nv, nf, true, "grt_set_meshes")) != GRT_OK) { free_meshes(c); return rc; }
    c->have_timing = false;
    c->n_faces = nf;
    c->n_verts = nv;
    return GRT_OK;
}

// Same meshes, moved (a gizmo drag: reference updateInstanceTransforms, src/GaussianTracer.cpp:711-736, rebuilds GAS and
// IAS every time and leaks the old ones): new vertex positions / normals for the SAME topology; the mesh LBVH keeps its
// hierarchy and only re-fits its boxes.  Fails with GRT_ERR_INVALID when the counts differ from the last grt_set_meshes.
int grt_update_meshes(grt_ctx* c, const grt_mesh* meshes, uint32_t n_meshes)
{
    if (c) c->scene_epoch++;
    if (!c || (n_meshes && !meshes)) return GRT_ERR_INVALID;
    NOT_A_VIEW(c, "grt_update_meshes");
    CHK(c, hipSetDevice(c->device));
    // the topology must be the one grt_set_meshes built the tree for: per mesh, not just in total (two meshes that swap
    // sizes keep the sums), and the same indices (only positions / normals may move)
    bool same = n_meshes == c->mesh_nv.size() && c->n_faces != 0;
    for (uint32_t k = 0; same && k < n_meshes; k++) same = meshes[k].nv == c->mesh_nv[k] && meshes[k].nf == c->mesh_nf[k];
    if (!same) {
        c->err = "grt_update_meshes: mesh count or per-mesh vertex / face counts differ from the last grt_set_meshes (call that instead)";
        return GRT_ERR_INVALID;
    }
    FlatMeshes fm;
    const int rc = flatten_meshes(c, meshes, n_meshes, false, "grt_update_meshes", &fm);
    if (rc != GRT_OK) return rc;
    if (fm.hash != c->faces_hash) {
        c->err = "grt_update_meshes: face indices differ from the last grt_set_meshes (call that instead)";
        return GRT_ERR_INVALID;
    }
    // the node boxes, triangles and normals are overwritten in place: no frame may still be reading them, on whatever
    // stream it was launched (renders are asynchronous on the caller's stream; views have streams of their own)
    CHK(c, hipDeviceSynchronize());
    const int rc_tree = mesh_tree(c, fm, c->n_verts, c->n_faces, false, "grt_update_meshes");
    c->have_timing = false;
    return rc_tree;
}

} // extern "C"
