// grt_segments.hip — ray segments of a Gaussian-only scene, with gradients (include/grt.h: grt_trace_segments_frame / _rays,
// grt_backward_segments_frame / _rays): the reference's trace() itself (shaders/tracer.cuh:328-373) — one segment
// [t_near, t_far] of every ray, entered with the transmittance T_in the ray's earlier segments left — as the plain radiance
// R = sum_i T_i alpha_i L_i, the transmittance T_out behind it, the expected distance and the event count; and, given dloss/dR and
// dloss/dT_out, the gradients with respect to pos, scale, quat, opacity and sh.
//
// One ray per lane, an 8x8 tile per wave (lane_ray); range and T_in are per LANE, loaded at the lane's element idx.
//   k_trace_segments          ONE sweep_events call (grt_bwd.h) with T entering as T_in; R, depth and count are accumulated in on_slot in
//                             the forward's own arithmetic (R = R + (L T) alpha; depth += (T alpha) t before T is updated), plain vector
//                             stores behind the sweep.  No atomic, no wave operation, no buffer of the context.  A NULL array is a
//                             wave-uniform branch on a kernel argument.
//   k_backward_segments<MERGE> the two sweeps of backward_body — sweep 0 re-derives R and T_out, sweep 1 forms every composited event's
//                             terms — with the lane's own range, T starting at T_in in both, and the upstream mapping g_rad = g_R,
//                             gAp = -g_T (event_terms: dL/dalpha_i = g_R . (T_i L_i - S_i / (1 - alpha_i)) - g_T T_out / (1 - alpha_i)).
//                             It launches through bwd_launch with SegIn behind (RenderArgs, BwdArgs): gradient buffer and flush.
// The per-lane start: sweep_events reads a.p.t_min, so each kernel hands it a LANE-LOCAL COPY of its arguments with p.t_min
// overwritten (every other member stays the kernel argument it was: the copy is taken apart, one VGPR holds the start); the end is
// sweep_events' own t_max parameter.  grt_bwd.h is untouched, so no other unit's code moves.
#include <string>

#include "grt_bwd.h"

namespace grt {
namespace {

static_assert(kBlock == kRoundBlock, "the segment kernels run gps_round (grt_kround.h): its per-lane stack stride is the launch block size");

struct SegIn {
    const float* t_near; // [N] or null: p.t_min
    const float* t_far;  // [N] or null: p.t_max
    const float* T_in;   // [N] or null: 1
};
struct SegOut {
    grt_segment_out o;
};

// This lane's segment at its element idx (owned: has_out), and whether it is traced at all: every comparison is written so that a NaN
// in t_near, t_far or T_in fails it.
__device__ __forceinline__ bool lane_segment(const RenderArgs& a, const SegIn& s, size_t idx, bool has_out, float& tn, float& tf, float& T0)
{
    tn = a.p.t_min; tf = a.p.t_max; T0 = 1.0f;
    if (has_out) { // (idx of a lane without an element may lie outside the arrays)
        if (s.t_near) tn = s.t_near[idx];
        if (s.t_far) tf = s.t_far[idx];
        if (s.T_in) T0 = s.T_in[idx];
    }
    return (tn > 0.0f) && (tn <= tf) && (fabsf(tf) < INFINITY) && (T0 > a.p.minTransmittance);
}

__global__ __launch_bounds__(kBlock) void k_trace_segments(const RenderArgs a, const SegIn s, const SegOut k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out);
    float tn, tf, T0;
    const bool seg = lane_segment(a, s, idx, has_out, tn, tf, T0);
    // trace() has no bounce: max_bounces is not looked at
    live = live && seg && (length3(d) > 0.1f) && (a.root_ref != kNoRoot);
    f3 R = mk3(0, 0, 0);
    float depth = 0.0f, T = T0; // (an untraced ray keeps T_in's bits: T is stored as it was loaded)
    uint32_t n = 0;

    if (__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        RenderArgs al = a; // the lane's own start (see the head of this file)
        al.p.t_min = live ? tn : a.p.t_min;
        const f3 dn = normalize3(d);
        sweep_events(al, stk, o, d, mk_rayinv(o, d), tf, live, T, [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t key) {
            if (ev) { // Tb: the transmittance before the event
                depth += (Tb * hitAlpha) * key_t(key);
                n++;
                const f3 L = event_radiance(a, id, dn);
                R = add3(R, mul3s(mul3s(L, Tb), hitAlpha));
            }
        });
    }
    if (has_out) { // every element of the window or of the buffer once per requested array
        if (k.o.radiance) {
            float* r = k.o.radiance + idx * 3;
            r[0] = R.x; r[1] = R.y; r[2] = R.z;
        }
        if (k.o.T_out) k.o.T_out[idx] = T;
        if (k.o.depth) k.o.depth[idx] = depth;
        if (k.o.count) k.o.count[idx] = n;
    }
}

template <bool MERGE>
__global__ __launch_bounds__(kBlock) void k_backward_segments(const RenderArgs a, const BwdArgs b, const SegIn s)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out);
    float tn, tf, T0;
    const bool seg = lane_segment(a, s, idx, has_out, tn, tf, T0);
    live = live && seg && (length3(d) > 0.1f) && (a.root_ref != kNoRoot);
    f3 gR;
    float gT;
    live = load_upstream(b, idx, live, gR, gT); // a ray whose four upstream values are exactly 0 is not traced
    if (!__builtin_amdgcn_ballot_w64(live)) return; // wave-uniform

    RenderArgs al = a; // the lane's own start (see the head of this file)
    al.p.t_min = live ? tn : a.p.t_min;
    const f3 dn = normalize3(d);
    const rayinv ri = mk_rayinv(o, d);
    RayAcc ra;    // (dead: event_terms<., false> does not touch it)
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);
    const float gAp = 0.0f - gT; // T_out enters with -g_T where backward_body's A = 1 - T_end enters with gA'

    // two sweeps over the same events, as backward_body has them — sweep 0: R and T_out (the forward's own arithmetic); sweep 1: every
    // composited event's terms with S_i = R - C_<=i.  Every lane of the wave in step: the scatter of sweep 1 is wave-cooperative.
    f3 rad = mk3(0, 0, 0);
    float Tend = T0;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        float T = T0;
        f3 C = mk3(0, 0, 0);
        sweep_events(al, stk, o, d, ri, tf, live, T, [&](bool ev, uint32_t id, float Tb, float hitAlpha, uint64_t) {
            bool geom = false;
            float v[kVals];
#pragma unroll
            for (int i = 0; i < kVals; i++) v[i] = 0.0f;
            if (ev) {
                const f3 L = event_radiance(a, id, dn);
                C = add3(C, mul3s(mul3s(L, Tb), hitAlpha)); // (sweep 0: this is R, term by term as the forward adds it)
                if (pass == 0) rad = C;
                else geom = event_terms<true, false>(a, b, id, o, d, dn, L, Tb, hitAlpha, sub3(rad, C), gR, gAp, Tend, v, ra);
            }
            if (pass) scatter<MERGE>(b.acc, ev, id, v, geom, b.want_sh != 0u, lane);
        });
        if (pass == 0) Tend = T;
    }
}

} // namespace
} // namespace grt

using namespace grt;

// what the four entry points refuse before they look at their rays: the backward's refusals in the entry point's name and a scene with meshes
static int fill(grt_ctx* c, const grt_params* p, RenderArgs* a, const char* fn)
{
    return bwd_fill_args(c, p, false, a, fn, "trace() is the Gaussian-only call: ray segments are traced through the Gaussians alone");
}

static SegIn seg_in(const grt_segments* seg)
{
    SegIn s;
    s.t_near = seg ? seg->t_near : nullptr;
    s.t_far = seg ? seg->t_far : nullptr;
    s.T_in = seg ? seg->T_in : nullptr;
    return s;
}

static bool wanted(const grt_segment_out* o) { return o && (o->radiance || o->T_out || o->depth || o->count); }

static int no_output(grt_ctx* c, const char* fn)
{
    c->err = std::string(fn) + ": no output (radiance, T_out, depth and count are all NULL)";
    return GRT_ERR_INVALID;
}

static int launch_forward(grt_ctx* c, const RenderArgs& a, const grt_segments* seg, const grt_segment_out* out, void* stream, const char* fn)
{
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced)
    SegIn s = seg_in(seg);
    SegOut k;
    k.o = *out;
    void* args[3] = {const_cast<RenderArgs*>(&a), &s, &k};
    int rc = lane_launch(c, a, reinterpret_cast<const void*>(k_trace_segments), args, st, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, st);
}

// the backward's arguments, checked in the header's order
static int check_backward(grt_ctx* c, const float* d_grad_radiance, const grt_gaussian_grads* g, const char* fn)
{
    if (!d_grad_radiance) { c->err = std::string(fn) + ": null pointer (d_grad_radiance is required)"; return GRT_ERR_INVALID; }
    if (!g || (!g->pos && !g->scale && !g->quat && !g->opacity && !g->sh)) {
        c->err = std::string(fn) + ": no output (pos, scale, quat, opacity and sh are all NULL)";
        return GRT_ERR_INVALID;
    }
    return GRT_OK;
}

static int launch_backward(grt_ctx* c, const grt_params* p, const RenderArgs& a, const grt_segments* seg, const float* d_grad_radiance,
                           const float* d_grad_T_out, const grt_gaussian_grads* g, void* stream, const char* fn)
{
    SegIn s = seg_in(seg);
    // ([0]: a call without a gradient group is refused; no ray, no particle or an empty tree: bwd_launch writes nothing)
    static const void* const kernels[3] = {nullptr, reinterpret_cast<const void*>(k_backward_segments<false>),
                                           reinterpret_cast<const void*>(k_backward_segments<true>)};
    return bwd_launch(c, p, a, d_grad_radiance, d_grad_T_out, g, BwdUnit{kernels, &s, false}, stream, fn); // (BwdArgs::g_rgb / g_alpha)
}

extern "C" {

int grt_trace_segments_frame(grt_ctx* c, const grt_params* p, const grt_segments* seg, const grt_segment_out* out, uint32_t x0, uint32_t y0,
                             uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_trace_segments_frame";
    RenderArgs a;
    int rc = fill(c, p, &a, fn);
    if (rc == GRT_OK && !wanted(out)) rc = no_output(c, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, seg, out, stream, fn);
}

int grt_trace_segments_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const grt_segments* seg,
                            const grt_segment_out* out, void* stream)
{
    const char* fn = "grt_trace_segments_rays";
    RenderArgs a;
    int rc = fill(c, p, &a, fn);
    if (rc == GRT_OK && !wanted(out)) rc = no_output(c, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, seg, out, stream, fn);
}

int grt_backward_segments_frame(grt_ctx* c, const grt_params* p, const grt_segments* seg, const float* d_grad_radiance,
                                const float* d_grad_T_out, const grt_gaussian_grads* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                                void* stream)
{
    const char* fn = "grt_backward_segments_frame";
    RenderArgs a;
    int rc = fill(c, p, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, d_grad_radiance, out, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, seg, d_grad_radiance, d_grad_T_out, out, stream, fn);
}

int grt_backward_segments_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const grt_segments* seg,
                               const float* d_grad_radiance, const float* d_grad_T_out, const grt_gaussian_grads* out, void* stream)
{
    const char* fn = "grt_backward_segments_rays";
    RenderArgs a;
    int rc = fill(c, p, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, d_grad_radiance, out, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, seg, d_grad_radiance, d_grad_T_out, out, stream, fn);
}

} // extern "C"
