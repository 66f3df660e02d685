// grt_depth.h — the device text the two depth units share (grt_depth.hip, grt_depth_mesh.hip): the distance of a
// particle's maximum response along a ray (peak_tau, with the frame it was formed in) and the chain below it (tau_terms).  Everything
// here is __forceinline__ in an unnamed namespace and holds no wave operation: a unit holds the kernels it instantiates, nothing else.
#pragma once

#include "grt_bwd.h"

namespace grt {
namespace {

// computeResponse's frame of particle id for the ray (o, d), term by term as alpha_terms has it: A = diag(1/s) R^T, x = o - mu,
// o_g = A x, d_g = A d, dd = d_g.d_g; returns d_val = -(o_g.d_g) / max(1e-6, dd)
struct PeakFrame {
    m33 A;
    float is[3];
    f3 x, o_g, d_g;
    float dd;
};
__device__ __forceinline__ float peak_tau(const float* __restrict__ pos, const float* __restrict__ scale, const float* __restrict__ quat,
                                          uint32_t id, f3 o, f3 d, PeakFrame& f)
{
    const f3 mu = mk3(pos[id * 3], pos[id * 3 + 1], pos[id * 3 + 2]);
    f.is[0] = 1.0f / scale[id * 3]; f.is[1] = 1.0f / scale[id * 3 + 1]; f.is[2] = 1.0f / scale[id * 3 + 2];
    float Rg[9];
    mat3_cast(quat[id * 4], quat[id * 4 + 1], quat[id * 4 + 2], quat[id * 4 + 3], Rg);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) f.A.a[r * 3 + c] = f.is[r] * Rg[r * 3 + c];
    }
    f.x = sub3(o, mu);
    f.o_g = matvec(f.A, f.x);
    f.d_g = matvec(f.A, d);
    f.dd = dot3(f.d_g, f.d_g);
    return -dot3(f.o_g, f.d_g) / fmaxf(1e-6f, f.dd);
}

// A^T g
__device__ __forceinline__ f3 matvec_t(const m33& A, f3 g)
{
    return mk3(A.a[0] * g.x + A.a[3] * g.y + A.a[6] * g.z, A.a[1] * g.x + A.a[4] * g.y + A.a[7] * g.z,
               A.a[2] * g.x + A.a[5] * g.y + A.a[8] * g.z);
}

// The chain below one event's tau = d_val, ADDED to v[0..9] (pos 3, scale 3, quat 4; tau does not depend on the opacity): with
// q = max(1e-6, dd), a = dtau/do_g = -d_g / q and b = dtau/dd_g = -(o_g + 2 tau d_g) / q (= (p_g - tau d_g) / q; where the max binds
// the denominator is a constant: b = -o_g / q),
//     d/dmu = -A^T a,   d/do = A^T a,   d/dd = A^T b,   d/ds_k = -(a_k o_g,k + b_k d_g,k) / s_k,
//     d/dR_jk = (a_k x_j + b_k d_j) / s_k, then through glm::mat3_cast as alpha_terms takes its own G.
// RAYS: ra.go and ra.gd collect what the ray's output SUBTRACTS (alpha_terms' convention), so the tau terms enter negated.
template <bool RAYS>
__device__ __forceinline__ void tau_terms(const BwdArgs& b, uint32_t id, f3 d, const PeakFrame& f, float tau, float gtau, float v[kVals], RayAcc& ra)
{
    const float iq = 1.0f / fmaxf(1e-6f, f.dd);
    const float two_tau = (f.dd < 1e-6f) ? 0.0f : 2.0f * tau;
    const f3 ga = mul3s(f.d_g, -(gtau * iq));
    const f3 gb = mul3s(add3(f.o_g, mul3s(f.d_g, two_tau)), -(gtau * iq));
    const f3 mo = matvec_t(f.A, ga); // dloss/do of this event; -mo goes to pos
    v[0] -= mo.x; v[1] -= mo.y; v[2] -= mo.z;
    if (RAYS) {
        ra.go = sub3(ra.go, mo);
        ra.gd = sub3(ra.gd, matvec_t(f.A, gb));
    }
    v[3] -= (ga.x * f.o_g.x + gb.x * f.d_g.x) * f.is[0];
    v[4] -= (ga.y * f.o_g.y + gb.y * f.d_g.y) * f.is[1];
    v[5] -= (ga.z * f.o_g.z + gb.z * f.d_g.z) * f.is[2];
    const float ha[3] = {ga.x * f.is[0], ga.y * f.is[1], ga.z * f.is[2]};
    const float hb[3] = {gb.x * f.is[0], gb.y * f.is[1], gb.z * f.is[2]};
    const float xj[3] = {f.x.x, f.x.y, f.x.z};
    const float dj[3] = {d.x, d.y, d.z};
    float G[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
#pragma unroll
        for (int k = 0; k < 3; k++) G[j][k] = xj[j] * ha[k] + dj[j] * hb[k];
    }
    const float qw = b.quat[id * 4], qx = b.quat[id * 4 + 1], qy = b.quat[id * 4 + 2], qz = b.quat[id * 4 + 3];
    v[6] += 2.0f * (((qz * (G[1][0] - G[0][1])) + (qy * (G[0][2] - G[2][0]))) + (qx * (G[2][1] - G[1][2])));
    v[7] += 2.0f * ((((qy * (G[0][1] + G[1][0])) + (qz * (G[0][2] + G[2][0]))) + (qw * (G[2][1] - G[1][2]))) -
                    2.0f * qx * (G[1][1] + G[2][2]));
    v[8] += 2.0f * ((((qx * (G[0][1] + G[1][0])) + (qz * (G[1][2] + G[2][1]))) + (qw * (G[0][2] - G[2][0]))) -
                    2.0f * qy * (G[0][0] + G[2][2]));
    v[9] += 2.0f * ((((qx * (G[0][2] + G[2][0])) + (qy * (G[1][2] + G[2][1]))) + (qw * (G[1][0] - G[0][1]))) -
                    2.0f * qz * (G[0][0] + G[1][1]));
}

} // namespace
} // namespace grt
