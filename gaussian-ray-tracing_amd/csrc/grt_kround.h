// grt_kround.h — the per-lane k-nearest round: the k-buffer, its insert, one BVH round and the radiance of an event.
//
// ONE text for the forward per-lane kernels (grt_render.hip) and the backward pass (grt_bwd.h, the header of the three backward
// units, and grt_backward_mesh.hip): the backward is right only while it builds the same k-buffer in the same order as the
// forward, and here that is a fact of the include.
// (The wave kernel, grt_render_wave.hip with its branch-free kbuf_insert and gps_round_wave, the stream body and the tile kernel
//  stay independent on purpose: "four independent traversals, bit for bit" is a test asset.)
#pragma once

#include "grt_device.h"
#include "grt_internal.h"

namespace grt {

// stride of the per-lane LDS stack (stack[level][thread]): the launch block size of every kernel that calls gps_round
constexpr int kRoundBlock = 256;

struct Cnt {
    uint32_t rays = 0, segments = 0, hit_evals = 0, rounds = 0, node_visits = 0, proxy_tests = 0, iters = 0;
};

template <int KK>
struct KBuf {
    uint64_t key[KK];
    float alpha[KK];
};

template <int KK>
__device__ __forceinline__ void kbuf_insert(KBuf<KK>& kb, uint64_t key, float alpha)
{
    // same effect as the 7 compare-and-swap steps of __anyhit__anyhit (shaders/tracer.cu:124-146)
    if (key >= kb.key[KK - 1]) return;
#pragma unroll
    for (int i = 0; i < KK; i++) {
        if (key == kb.key[i]) return; // the same event again: a split particle met through another of its pieces
        if (key < kb.key[i]) {
            const uint64_t tk = kb.key[i];
            const float ta = kb.alpha[i];
            kb.key[i] = key;
            kb.alpha[i] = alpha;
            key = tk;
            alpha = ta;
        }
    }
}

// one k-nearest round: traceGPs + __anyhit__ (shaders/tracer.cuh:289-326, shaders/tracer.cu:136-153)
// (WATCH: the iteration watchdog; limit: value of c.iters at which the segment gives up; false = gave up.
//  Without WATCH and COUNT c is not touched and the round returns true.)
template <bool COUNT, bool WATCH, int KK>
__device__ __forceinline__ bool gps_round(const RenderArgs& a, uint32_t* __restrict__ stk, f3 o, f3 d,
                                          const rayinv& ri, uint64_t last_key, float t_hi, KBuf<KK>& kb, Cnt& c,
                                          uint32_t limit)
{
#pragma unroll
    for (int i = 0; i < KK; i++) {
        kb.key[i] = kKeyInvalid;
        kb.alpha[i] = 0.0f;
    }
    const float t_lo = key_t(last_key);
    float bound = t_hi; // nothing beyond the current k-th nearest hit can enter the buffer
    uint32_t sp = 0;
    uint32_t cur = a.root_ref;
    while (true) {
        if (WATCH) {
            c.iters++;
            if (c.iters > limit) return false;
        }
        if (cur & kLeafBit) {
            const uint32_t first = leaf_first(cur), cnt = leaf_count(cur);
            for (uint32_t j = 0; j < cnt; j++) {
                const float4* __restrict__ r = a.rec + (size_t)(first + j) * 4;
                const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
                if (COUNT) c.proxy_tests++;
                const f3 mu = mk3(r0.x, r0.y, r0.z);
                m33 A;
                A.a[0] = r1.x; A.a[1] = r1.y; A.a[2] = r1.z;
                A.a[3] = r2.x; A.a[4] = r2.y; A.a[5] = r2.z;
                A.a[6] = r3.x; A.a[7] = r3.y; A.a[8] = r3.z;
                const f3 o_g = matvec(A, sub3(o, mu));
                const f3 d_g = matvec(A, d);
                float te, tx;
                if (proxy_sphere_maybe(o_g, d_g, r0.w) && proxy_slabs(o_g, d_g, r0.w, te, tx)) {
                    // (a piece of a split proxy reports an event only when the event's point lies in its cell)
                    const uint32_t cellb = __float_as_uint(r3.w);
                    const bool in_e = (te >= t_lo) && (te < t_hi) && (!cellb || piece_owns(cellb, r0.w, o_g, d_g, te));
                    const bool in_x = (tx >= t_lo) && (tx < t_hi) && (!cellb || piece_owns(cellb, r0.w, o_g, d_g, tx));
                    if (in_e || in_x) {
                        // alpha does not depend on the hit distance (shaders/tracer.cuh:354-357):
                        // evaluated once, carried by the entry and the exit hit
                        const float alpha = fminf(0.99f, response_from(A, mu, o, d, o_g, d_g) * r1.w);
                        const uint32_t id = __float_as_uint(r2.w);
                        if (in_e) {
                            const uint64_t k = mk_key(te, id, 0);
                            if (k > last_key) kbuf_insert(kb, k, alpha);
                        }
                        if (in_x) {
                            const uint64_t k = mk_key(tx, id, 1);
                            if (k > last_key) kbuf_insert(kb, k, alpha);
                        }
                        if (kb.key[KK - 1] != kKeyInvalid) bound = key_t(kb.key[KK - 1]);
                    }
                }
            }
            if (sp == 0) break;
            cur = stk[(--sp) * kRoundBlock];
        } else {
            const float4* __restrict__ q = a.nodes + (size_t)cur * 4;
            const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            if (COUNT) c.node_visits++;
            float n0, f0, n1, f1;
            box_interval(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, ri, n0, f0);
            box_interval(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, ri, n1, f1);
            const bool h0 = (n0 <= f0) && (f0 >= t_lo) && (n0 <= bound);
            const bool h1 = (n1 <= f1) && (f1 >= t_lo) && (n1 <= bound);
            const uint32_t c0 = __float_as_uint(q3.x), c1 = __float_as_uint(q3.y);
            if (h0 && h1) {
                const bool first0 = n0 <= n1;
                stk[(sp++) * kRoundBlock] = first0 ? c1 : c0;
                cur = first0 ? c0 : c1;
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
    return true;
}

// computeRadiance (shaders/tracer.cuh:260-264) of particle id along the normalised ray direction dn: the degree-0 colours are
// kept evaluated (color0), the higher degrees go through sh_radiance
__device__ __forceinline__ f3 event_radiance(const RenderArgs& a, uint32_t id, f3 dn)
{
    if (a.p.sh_degree_max == 0) {
        const float4 cc = a.color0[id];
        return mk3(cc.x, cc.y, cc.z);
    }
    return sh_radiance(a.sh + (size_t)id * 48, dn, a.p.sh_degree_max);
}

} // namespace grt
