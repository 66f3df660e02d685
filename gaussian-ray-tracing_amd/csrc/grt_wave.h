// grt_wave.h — wave64-level building blocks shared by the wave-cooperative render kernels, the backward pass and the particle
// statistics (gfx950 only): scalar (constant-address-space) record fetches, DPP reductions (min, sum, max; signed floats and 64-bit
// keys through integer keys), lane-mask votes, lane reads, slot-key packing.  The one home of such helpers: a unit defines none.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grt_device.h"

namespace grt {
namespace {

constexpr uint64_t kCellMask = 31ull; // payload-cell bits of a slot key
__device__ __forceinline__ uint64_t mk_skey(float t, uint32_t id, uint32_t is_exit)
{
    return ((uint64_t)__float_as_uint(t) << 32) | (uint64_t)((id << 6) | (is_exit << 5));
}
__device__ __forceinline__ uint32_t skey_id(uint64_t k) { return ((uint32_t)k) >> 6; }

struct Cnt {
    uint32_t rays = 0, segments = 0, hit_evals = 0, rounds = 0, node_visits = 0, proxy_tests = 0, fetches = 0, stall_exits = 0;
};

// scalar (SGPR) fetch of one float4 at a wave-uniform index: constant address space => s_load_dwordx4
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 sload4(const float4* base, uint32_t idx)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) v4f* cptr4;
    const v4f v = ((cptr4)(uintptr_t)base)[idx];
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return base[idx];
#endif
}

// one 64-B record by ONE scalar load at base + a 32-bit byte offset (s_load_dwordx16 sdst, sbase, soffset)
typedef float v16f __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void sload64(const float4* base, uint32_t byte_off, float4& q0, float4& q1, float4& q2, float4& q3)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) char* cptr1;
    typedef const __attribute__((address_space(4))) v16f* cptr16;
    const v16f v = *(cptr16)((cptr1)(uintptr_t)base + byte_off);
    q0 = make_float4(v.s0, v.s1, v.s2, v.s3); q1 = make_float4(v.s4, v.s5, v.s6, v.s7);
    q2 = make_float4(v.s8, v.s9, v.sa, v.sb); q3 = make_float4(v.sc, v.sd, v.se, v.sf);
#else
    const float4* p = (const float4*)((const char*)base + byte_off);
    q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3];
#endif
}
// x with bit b cleared, b wave-uniform (s_bitset0_b64: one SALU operation instead of the three of x & (x - 1))
__device__ __forceinline__ uint64_t clear_bit64(uint64_t x, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm("s_bitset0_b64 %0, %1" : "+s"(x) : "s"(b));
    return x;
#else
    return x & ~(1ull << b);
#endif
}

// wave64 min of non-negative floats (or +inf) -> wave-uniform value.  Their bit patterns order like unsigned
// integers, so the reduction is 4 v_min_u32 with DPP operands inside rows of 16, then 4 v_readlane + 3 s_min_u32
// (no NaN canonicalisation, which fminf would add to every step).
__device__ __forceinline__ float wave_min(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t x = __float_as_uint(v);
    // bound_ctrl:1 lets the compiler fold each DPP move into the v_min_u32 itself (one VALU op per step)
    x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true));  // quad_perm [1,0,3,2]
    x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true));  // quad_perm [2,3,0,1]
    x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, true)); // row_half_mirror
    x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, true)); // row_mirror
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)x, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)x, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)x, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
    return __uint_as_float(min(min(a, b), min(c, d)));
#else
    return v;
#endif
}

// sum over the wave of v (lanes outside `mine` hold 0), as a wave-uniform value
__device__ __forceinline__ float wave_sum(float v)
{
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));  // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));  // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true)); // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true)); // row_mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}

// max over the wave of v >= 0 (lanes outside the group hold 0), as a wave-uniform value: wave_sum's ladder with fmaxf
__device__ __forceinline__ float wave_max(float v)
{
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true)));  // quad_perm [1,0,3,2]
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true)));  // quad_perm [2,3,0,1]
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true))); // row_half_mirror
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true))); // row_mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// four independent wave minima in lockstep: the DPP steps of different reductions interleave, so the two wait states a
// DPP operand needs after its producer are filled with useful work instead of s_nop
__device__ __forceinline__ void wave_min4(float a, float b, float c, float d, float& ra, float& rb, float& rc, float& rd)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t x0 = __float_as_uint(a), x1 = __float_as_uint(b), x2 = __float_as_uint(c), x3 = __float_as_uint(d);
#define GRT_DPP_STEP(CTRL)                                                                                 \
    {                                                                                                      \
        const uint32_t y0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x0, CTRL, 0xF, 0xF, true);       \
        const uint32_t y1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x1, CTRL, 0xF, 0xF, true);       \
        const uint32_t y2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x2, CTRL, 0xF, 0xF, true);       \
        const uint32_t y3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x3, CTRL, 0xF, 0xF, true);       \
        x0 = min(x0, y0); x1 = min(x1, y1); x2 = min(x2, y2); x3 = min(x3, y3);                            \
    }
    GRT_DPP_STEP(0xB1)  // quad_perm [1,0,3,2]
    GRT_DPP_STEP(0x4E)  // quad_perm [2,3,0,1]
    GRT_DPP_STEP(0x141) // row_half_mirror
    GRT_DPP_STEP(0x140) // row_mirror
#undef GRT_DPP_STEP
#define GRT_ROWS(x)                                                                                        \
    __uint_as_float(min(min((uint32_t)__builtin_amdgcn_readlane((int)x, 0), (uint32_t)__builtin_amdgcn_readlane((int)x, 16)), \
                        min((uint32_t)__builtin_amdgcn_readlane((int)x, 32), (uint32_t)__builtin_amdgcn_readlane((int)x, 48))))
    ra = GRT_ROWS(x0); rb = GRT_ROWS(x1); rc = GRT_ROWS(x2); rd = GRT_ROWS(x3);
#undef GRT_ROWS
#else
    ra = a; rb = b; rc = c; rd = d;
#endif
}

// Signed-float wave reductions (the tile kernel, grt_tile.h): eleven per frustum fit, and a tile re-fits its frustum every time half of its wanting lanes
// have finished.  As `fminf(v, __shfl_xor(v, off))` each was six dependent LDS round trips (ds_bpermute) and eighteen VALU
// operations with their NaN canonicalisation; here a float goes through an order-preserving integer key (sign bit
// flipped for v >= 0, all bits for v < 0), the DPP integer minimum above (wave_min / wave_min4: no LDS, four
// reductions interleaved) and back.  The result is wave-uniform and the exact minimum / maximum as before.
// NaN: unlike fminf / fmaxf the integer key does not drop it (a NaN would win the reduction and void the frustum for the
// whole tile).  No NaN reaches these reductions: they are fed from the rays of lanes with `alive`, which implies
// have_ray, i.e. length(d) > 0.1 (the reference's loop guard, shaders/tracer.cu:59 — false for a NaN direction, which is
// how a bounce off a zero shading normal ends), with origins that are the eye or a finite mesh hit point
// (tests/test_gpu_parity.py::test_mesh_with_zero_normals_nan_bounce_directions).
__device__ __forceinline__ uint32_t fkey(float f)
{
    const uint32_t b = __float_as_uint(f);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k)
{
    return __uint_as_float(k ^ ((uint32_t)((int32_t)~k >> 31) | 0x80000000u));
}
__device__ __forceinline__ float wave_fmin(float v) { return fkey_inv(__float_as_uint(wave_min(__uint_as_float(fkey(v))))); }
__device__ __forceinline__ float wave_fmax(float v) { return fkey_inv(~__float_as_uint(wave_min(__uint_as_float(~fkey(v))))); }
// (min a, max b, min c, max d) in one go
__device__ __forceinline__ void wave_fminmax4(float a, float b, float c, float d, float& mna, float& mxb, float& mnc, float& mxd)
{
    float ra, rb, rc, rd;
    wave_min4(__uint_as_float(fkey(a)), __uint_as_float(~fkey(b)), __uint_as_float(fkey(c)), __uint_as_float(~fkey(d)), ra, rb, rc, rd);
    mna = fkey_inv(__float_as_uint(ra)); mxb = fkey_inv(~__float_as_uint(rb));
    mnc = fkey_inv(__float_as_uint(rc)); mxd = fkey_inv(~__float_as_uint(rd));
}
__device__ __forceinline__ float uni(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v)));
#else
    return v;
#endif
}
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) // number of set bits of m below this lane
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
#else
    return 0u;
#endif
}
// wave64 minimum of 64-bit keys (two unsigned 32-bit DPP reductions: wave_min works on the bit patterns)
__device__ __forceinline__ uint64_t wave_umin64(uint64_t k)
{
    const uint32_t hi = (uint32_t)(k >> 32);
    const uint32_t mh = __float_as_uint(wave_min(__uint_as_float(hi)));
    const uint32_t lo = (hi == mh) ? (uint32_t)k : 0xFFFFFFFFu;
    const uint32_t ml = __float_as_uint(wave_min(__uint_as_float(lo)));
    return ((uint64_t)mh << 32) | (uint64_t)ml;
}
// minimum of 64-bit keys over the four lanes of a quad (lanes 4 q .. 4 q + 3), in every lane of the quad: the high words by two
// DPP minima, then the low words of the lanes that hold that high word
__device__ __forceinline__ uint64_t quad_umin64(uint64_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t hi = (uint32_t)(k >> 32);
    uint32_t mh = min(hi, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0xB1, 0xF, 0xF, true)); // quad_perm [1,0,3,2]
    mh = min(mh, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mh, 0x4E, 0xF, 0xF, true));           // quad_perm [2,3,0,1]
    const uint32_t lo = (hi == mh) ? (uint32_t)k : 0xFFFFFFFFu;
    uint32_t ml = min(lo, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0xB1, 0xF, 0xF, true));
    ml = min(ml, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ml, 0x4E, 0xF, 0xF, true));
    return ((uint64_t)mh << 32) | (uint64_t)ml;
#else
    return k;
#endif
}
__device__ __forceinline__ float lane_value(float v, int l) // v of lane l (l wave-uniform)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), l));
#else
    return v;
#endif
}
__device__ __forceinline__ void wave_fence()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // compiler ordering of the LDS exchange; no instruction
#endif
}

// votes straight on the lane mask (the __any/__ballot wrappers go through an int and cost two extra VALU ops)
__device__ __forceinline__ uint64_t wave_ballot(bool p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(p);
#else
    return p ? 1ull : 0ull;
#endif
}
__device__ __forceinline__ bool wave_any(bool p) { return wave_ballot(p) != 0ull; }
// votes on ONE compare, as the lane mask the compare instruction writes (v_cmp -> SGPR pair): whatever else uses the
// condition, and wherever it was computed, the vote costs one VALU operation (wave_ballot of a bool that arrives from
// another block costs two on top of its compare)
__device__ __forceinline__ uint64_t vote_eq_u32(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_uicmp(a, b, 32); // ICMP_EQ
#else
    return a == b;
#endif
}
__device__ __forceinline__ uint64_t vote_lt_f32(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fcmpf(a, b, 4); // FCMP_OLT (fcmpf: the float form; fcmp is the double one)
#else
    return a < b;
#endif
}
__device__ __forceinline__ uint64_t vote_nle_f32(float a, float b) // !(a > b): true for a NaN
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fcmpf(a, b, 13); // FCMP_ULE
#else
    return !(a > b);
#endif
}
__device__ __forceinline__ uint64_t vote_lt_u64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_uicmpl(a, b, 36); // ICMP_ULT
#else
    return a < b;
#endif
}
__device__ __forceinline__ uint64_t vote_eq_u64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_uicmpl(a, b, 32); // ICMP_EQ
#else
    return a == b;
#endif
}
__device__ __forceinline__ uint64_t vote_ne_u64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_uicmpl(a, b, 33); // ICMP_NE
#else
    return a != b;
#endif
}
// a lane mask as a per-lane condition: bit `lane` of m (m wave-uniform).  No instruction: the SGPR pair is used as the
// condition of the select or the EXEC narrowing itself — where a bool that was computed per lane and is also needed as a
// mask pays a vote (wave_ballot of a bool: two VALU operations), a mask that is also needed per lane pays nothing
__device__ __forceinline__ bool lane_of(uint64_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_inverse_ballot_w64(m);
#else
    return (m & 1ull) != 0ull;
#endif
}
// max(v, +0) for a non-NaN float as one integer max (negative floats are negative ints)
__device__ __forceinline__ float clamp0(float v) { return __int_as_float(max(__float_as_int(v), 0)); }

typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); } // v_pk_fma_f32

// two wave-uniform floats as one 64-bit scalar (an aligned SGPR pair) and back
__device__ __forceinline__ uint64_t pack2(float a, float b)
{
    return (uint64_t)__float_as_uint(a) | ((uint64_t)__float_as_uint(b) << 32);
}
__device__ __forceinline__ v2f unpack2(uint64_t u)
{
    return v2f{__uint_as_float((uint32_t)u), __uint_as_float((uint32_t)(u >> 32))};
}

} // namespace
} // namespace grt
