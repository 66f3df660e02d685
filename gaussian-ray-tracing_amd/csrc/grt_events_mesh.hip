// grt_events_mesh.hip — per-ray event lists of a mesh frame, with gradients (include/grt.h: grt_ray_events_mesh_frame / _rays,
// grt_backward_events_mesh_frame / _rays): what grt_events.hip computes for a Gaussian-only frame, for rays that bounce
// off mirror, glass or normal-shaded meshes.  A ray has ONE event list with ONE running transmittance, cut into the segments of its
// iterations (grt_backward_mesh.hip); the events of the iterations step_first .. step_last are numbered 0, 1, ... in compositing order
// over the whole ray, and the events first .. first + K - 1 go to slot n - first as (original id, key distance on the iteration's own
// ray, alpha, iteration).  Beside them the ray's path: per iteration its ray (o_s, d_s), the end of its segment and its state.
//
// Both kernels: one ray per lane, an 8x8 tile or 64 buffer rays per wave, ONE sweep of the raygen loop each (grt_mesh_walk.h: the loop,
// its convergence contract and why it cannot hang).  The step filter is a per-lane predicate on the iteration's number: an event
// outside the range is composited — T, A and B run through it — and is neither numbered nor listed; it changes no control flow.
//   k_ray_events_mesh            keeps the loop WRITTEN OUT as it had it, its own step filter included, statement for statement mesh_walk's and sweep_events' (a change there is a
//                                change here): its seven NULL tests are seven lane masks, it sits at the 106-SGPR limit, and on mesh_walk
//                                it read two more spilled SGPRs back per iteration than tests/test_picks_events_mesh_isa.py allows
//                                (DESIGN.md 5.27).  A listed event goes to its slot by up to four plain vector stores, an iteration
//                                below P to its path slot; after the loop the lane fills the slots behind its last listed event and
//                                behind its last iteration and stores count, T_in and n_steps.  No atomic, no buffer of the context,
//                                no wave operation but the loops' ballots.  A NULL output is a wave-uniform branch on a kernel argument.
//   k_backward_events_mesh<MERGE> on mesh_walk.  A pre-scan of the lane's column of the upstream leaves a ray whose values are all 0
//                                untraced; a listed event with g != 0 below the 0.99 clamp forms its 11 geometry / opacity values with
//                                dLda = g (alpha_terms) on the ITERATION'S OWN ray (o_s, d_s), and the whole wave calls scatter<MERGE>
//                                for every slot (on_slot).  dloss/dalpha is the caller's, so nothing depends on D_S: one sweep, which a
//                                lane leaves (mesh_walk's `leave`) at the end of the round that holds its last non-zero slot.  It
//                                launches through bwd_launch with EvMeshUp behind (RenderArgs, BwdArgs): gradient buffer and flush.
#include <string>

#include "grt_mesh_walk.h"

namespace grt {
namespace {

static_assert(GRT_STEP_LAST == LastGaussianPass && GRT_STEP_GAUSSIAN == GaussianPass && GRT_STEP_TERMINATE == Terminate,
              "path_state holds the raygen loop's own state numbers");

struct EvMeshOut {
    grt_ray_events_mesh e;
    uint64_t n; // N: elements of a slot plane (width * height, or the rays of the buffer)
};
struct EvMeshUp {
    const float* g; // upstream [K][N]
    uint64_t n;     // N
    uint32_t first, max_events;
    StepRange steps;
};

__global__ __launch_bounds__(kBlock) void k_ray_events_mesh(const RenderArgs a, const EvMeshOut k)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    uint32_t lane;
    size_t idx;
    bool has_out;
    f3 o, d;
    const bool live = lane_ray(a, lane, o, d, idx, has_out) && (a.root_ref != kNoRoot);
    const uint32_t first = k.e.first, Kn = k.e.max_events, P = k.e.max_steps;
    const size_t N = (size_t)k.n;
    uint32_t n = 0;    // this lane's composited events inside the step range so far
    uint32_t step = 0u; // this lane's iterations so far
    float T_end = 1.0f, T_in = 1.0f; // T_end: the running transmittance behind the lane's last segment

    if (__builtin_amdgcn_ballot_w64(live)) { // wave-uniform
        const float epsT = 1e-9f;
        const float minT = a.p.minTransmittance;
        const uint64_t key0 = mk_key(a.p.t_min + epsT, 0x7FFFFFFFu, 1);
        KBuf<K> kb;
        grt::Cnt cnt; // (dead: no counters, no watchdog)

        f3 curO = o, curD = d;
        float A = 0.0f, B = 0.0f, density = 0.0f;
        uint32_t numBounces = 0u, timeout = 0u;
        bool going = live;
        // ---- the raygen loop (shaders/tracer.cu:58-106), the whole wave in step ----
        while (true) {
            const bool it = going && (length3(curD) > 0.1f) && (numBounces < a.p.max_bounces);
            going = it;
            if (!__builtin_amdgcn_ballot_w64(it)) break; // wave-uniform
            const f3 ray_o = curO, ray_d = curD;
            int state = LastGaussianPass;
            float seg_tmax = a.p.t_max;
            f3 normal = mk3(0, 0, 0);
            if (it) { // per lane: no wave operation inside
                uint32_t n0 = 0, n1 = 0;
                const MeshHit mh = mesh_closest_t<false, kBlock>(a, stk, ray_o, ray_d, kTraceMeshTmin, kTraceMeshTmax, n0, n1);
                mesh_shade(a, mh, ray_o, ray_d, state, seg_tmax, normal, curO, curD, numBounces);
                if (step < P) { // the path slot of iteration step + 1 (a lane in an iteration is live, and a live lane owns element idx)
                    const size_t at = (size_t)step * N + idx;
                    if (k.e.path_rays) {
                        float* q = k.e.path_rays + at * 6;
                        q[0] = ray_o.x; q[1] = ray_o.y; q[2] = ray_o.z;
                        q[3] = ray_d.x; q[4] = ray_d.y; q[5] = ray_d.z;
                    }
                    if (k.e.path_t_far) k.e.path_t_far[at] = seg_tmax;
                    if (k.e.path_state) k.e.path_state[at] = (uint32_t)state;
                }
                step++;
            }
            // ---- this iteration's Gaussian segment [t_min, seg_tmax] on (ray_o, ray_d), T carried on (trace(), tracer.cuh:328-373) ----
            const rayinv ri = mk_rayinv(ray_o, ray_d);
            const float t_hi = seg_tmax + epsT;
            float T = 1.0f - density, lastT = a.p.t_min;
            uint64_t last_key = key0;
            const bool counted = (step >= k.e.step_first) && (k.e.step_last == 0u || step <= k.e.step_last);
            bool act = it && (lastT <= seg_tmax) && (T > minT);
            while (__builtin_amdgcn_ballot_w64(act)) {
                if (act) {
                    gps_round<false, false, K>(a, stk, ray_o, ray_d, ri, last_key, t_hi, kb, cnt, 0xFFFFFFFFu);
                    if (kb.key[0] == kKeyInvalid) act = false;
                }
#pragma unroll 1
                for (int i = 0; i < K; i++) {
                    bool hit = false;
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
                            hit = true;
                            id = key_id(key);
                        }
                    }
                    if (hit && counted) {
                        if (n == first) T_in = T; // T: the transmittance before the event
                        const uint32_t s = n - first; // (n < first wraps past K)
                        if (s < Kn) {
                            const size_t at = (size_t)s * N + idx;
                            if (k.e.id) k.e.id[at] = id;
                            if (k.e.t) k.e.t[at] = key_t(key);
                            if (k.e.alpha) k.e.alpha[at] = hitAlpha;
                            if (k.e.step) k.e.step[at] = step;
                        }
                        n++;
                    }
                    if (hit) T *= (1.0f - hitAlpha);
                }
                if (act) {
                    if (kb.key[K - 1] == kKeyInvalid) act = false;
                    else last_key = kb.key[K - 1];
                    act = act && (lastT <= seg_tmax) && (T > minT);
                }
            }
            // ---- the iteration's step of the loop (shade_ray, grt_render.hip) ----
            if (it) {
                T_end = T;
                density = 1.0f - T;
                const float D = density;
                if (state == Terminate) {
                    going = false;
                } else if (state == LastGaussianPass) { // A = clamp(A + D)
                    A = clampf(A + D, 0.0f, 1.0f);
                } else { // A = clamp(A + D); B = clamp(B + D)
                    A = clampf(A + D, 0.0f, 1.0f);
                    B = clampf(B + D, 0.0f, 1.0f);
                }
                timeout += 1;
                if (timeout > kTimeoutIterations) going = false;
            }
        }
    }
    if (has_out) { // every element of the window or of the buffer once per requested array
        if (n <= first) T_in = T_end; // no event `first`: the ray's final transmittance (1 for a ray that was not traced)
        for (uint32_t s = (n > first) ? ((n - first < Kn) ? n - first : Kn) : 0u; s < Kn; s++) { // behind the last listed event
            const size_t at = (size_t)s * N + idx;
            if (k.e.id) k.e.id[at] = GRT_PICK_NONE;
            if (k.e.t) k.e.t[at] = 0.0f;
            if (k.e.alpha) k.e.alpha[at] = 0.0f;
            if (k.e.step) k.e.step[at] = 0u;
        }
        for (uint32_t s = step; s < P; s++) { // behind the last iteration
            const size_t at = (size_t)s * N + idx;
            if (k.e.path_rays) {
                float* q = k.e.path_rays + at * 6;
                q[0] = 0.0f; q[1] = 0.0f; q[2] = 0.0f;
                q[3] = 0.0f; q[4] = 0.0f; q[5] = 0.0f;
            }
            if (k.e.path_t_far) k.e.path_t_far[at] = 0.0f;
            if (k.e.path_state) k.e.path_state[at] = GRT_PICK_NONE;
        }
        if (k.e.count) k.e.count[idx] = n;
        if (k.e.T_in) k.e.T_in[idx] = T_in;
        if (k.e.n_steps) k.e.n_steps[idx] = step;
    }
}

template <bool MERGE>
__global__ __launch_bounds__(kBlock) void k_backward_events_mesh(const RenderArgs a, const BwdArgs b, const EvMeshUp u)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t* stk = lds_stack + threadIdx.x;
    const float* __restrict__ g = u.g;
    const uint32_t first = u.first, Kn = u.max_events;
    const size_t N = (size_t)u.n;
    uint32_t lane;
    size_t idx;
    bool has_out; // (unused: nothing is written per ray)
    f3 o, d;
    bool live = lane_ray(a, lane, o, d, idx, has_out) && (a.root_ref != kNoRoot);
    uint32_t stop_n = 0u; // the number of the event in the lane's last non-zero slot, plus one: nothing behind it is differentiated
    if (live) { // the lane's column of the upstream
        for (uint32_t s = 0; s < Kn; s++) {
            if (g[(size_t)s * N + idx] != 0.0f) stop_n = first + s + 1u; // (first + K does not overflow: the host refuses it)
        }
    }
    live = live && (stop_n != 0u); // a ray whose K upstream values are all exactly 0 is not traced
    if (!__builtin_amdgcn_ballot_w64(live)) return; // wave-uniform

    RayAcc ra;    // (dead: alpha_terms<false> does not touch it)
    ra.go = ra.gd = ra.gdn = mk3(0, 0, 0);

    uint32_t n = 0; // this lane's composited events inside the step range so far
    bool counted = false;
    mesh_walk(
        a, stk, o, d, live, [&](const MeshSeg& s) { counted = u.steps.counted(s.step); },
        [&](const MeshSeg& s, bool hit, uint32_t id, float, float hitAlpha, uint64_t) {
            bool geom = false;
            float v[kVals];
#pragma unroll
            for (int q = 0; q < kVals; q++) v[q] = 0.0f;
            if (hit && counted) {
                const uint32_t slot = n - first; // (n < first wraps past K)
                if (slot < Kn && hitAlpha < 0.99f) { // (where the 0.99 clamp binds nothing goes into opacity or geometry)
                    const float dLda = g[(size_t)slot * N + idx];
                    if (dLda != 0.0f) {
                        geom = true;
                        alpha_terms<false>(b, id, s.ray_o, s.ray_d, dLda, v, ra); // the iteration's own ray
                    }
                }
                n++;
            }
            scatter<MERGE>(b.acc, geom, id, v, geom, false, lane); // every lane of the wave
        },
        [](const MeshSeg&, float, float) {},
        // behind its last non-zero slot the lane has nothing left to differentiate: it leaves the walk between two rounds and idles in
        // the wave's loops like a lane whose ray has ended (a per-lane condition, as the others)
        [&]() { return n >= stop_n; });
}

} // namespace
} // namespace grt

using namespace grt;

// what the four entry points refuse before they look at their rays: the mesh backward's refusals in the entry point's name, a step
// range that ends before it begins, and a slot range that is empty or overflows
static int fill(grt_ctx* c, const grt_params* p, bool have_range, uint32_t first, uint32_t max_events, uint32_t step_first, uint32_t step_last,
                RenderArgs* a, const char* fn)
{
    int rc = bwd_fill_args(c, p, true, a, fn);
    if (rc != GRT_OK || !have_range) return rc;
    if ((rc = check_step_range(c, step_first, step_last, fn)) != GRT_OK) return rc;
    if (max_events == 0) { c->err = std::string(fn) + ": max_events must be >= 1"; return GRT_ERR_INVALID; }
    if (first > 0xFFFFFFFFu - max_events) {
        c->err = std::string(fn) + ": first + max_events overflows (" + std::to_string(first) + " + " + std::to_string(max_events) + ")";
        return GRT_ERR_INVALID;
    }
    return GRT_OK;
}

static bool path_wanted(const grt_ray_events_mesh* o) { return o->path_rays || o->path_t_far || o->path_state; }
static bool wanted(const grt_ray_events_mesh* o)
{
    return o && (o->id || o->t || o->alpha || o->step || o->count || o->T_in || o->n_steps || path_wanted(o));
}

// N: the elements of a slot plane
static uint64_t plane(const RenderArgs& a) { return a.mode == 2 ? a.n_rays : (uint64_t)a.p.width * a.p.height; }

// the forward's own refusals, behind fill's
static int check_forward(grt_ctx* c, const grt_ray_events_mesh* out, const char* fn)
{
    if (!wanted(out)) {
        c->err = std::string(fn) + ": no output (id, t, alpha, step, count, T_in, the path arrays and n_steps are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (out->max_steps == 0 && path_wanted(out)) {
        c->err = std::string(fn) + ": max_steps must be >= 1 when path_rays, path_t_far or path_state is given";
        return GRT_ERR_INVALID;
    }
    return GRT_OK;
}

static int launch_forward(grt_ctx* c, const RenderArgs& a, const grt_ray_events_mesh* out, void* stream, const char* fn)
{
    if (a.n_blocks == 0) { c->have_timing = false; return GRT_OK; } // no ray: nothing to write
    CHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // (no particle or an empty tree: the kernel's guard makes every ray untraced and its elements "none")
    EvMeshOut k;
    k.e = *out; k.n = plane(a);
    if (!path_wanted(out)) k.e.max_steps = 0; // (no path array: no path slot is addressed)
    void* args[2] = {const_cast<RenderArgs*>(&a), &k};
    int rc = lane_launch(c, a, reinterpret_cast<const void*>(k_ray_events_mesh), args, s, fn);
    return rc != GRT_OK ? rc : lane_launch_done(c, s);
}

// the backward's arguments, checked in the header's order
static int check_backward(grt_ctx* c, const float* d_grad_alpha, const grt_gaussian_grads* g, const char* fn)
{
    if (g && g->sh) { c->err = std::string(fn) + ": sh must be NULL (colour does not depend on the listed events' alpha)"; return GRT_ERR_INVALID; }
    if (!g || (!g->pos && !g->scale && !g->quat && !g->opacity)) {
        c->err = std::string(fn) + ": no output (pos, scale, quat and opacity are all NULL)";
        return GRT_ERR_INVALID;
    }
    if (!d_grad_alpha) { c->err = std::string(fn) + ": null pointer (the upstream gradient is required)"; return GRT_ERR_INVALID; }
    return GRT_OK;
}

static int launch_backward(grt_ctx* c, const grt_params* p, const RenderArgs& a, const float* d_grad_alpha, uint32_t first, uint32_t max_events,
                           uint32_t step_first, uint32_t step_last, const grt_gaussian_grads* g, void* stream, const char* fn)
{
    EvMeshUp u;
    u.g = d_grad_alpha; u.n = plane(a); u.first = first; u.max_events = max_events; u.steps = StepRange(step_first, step_last);
    // ([0]: a call without a geometry group is refused; no ray, no particle or an empty tree: bwd_launch writes nothing)
    static const void* const kernels[3] = {nullptr, reinterpret_cast<const void*>(k_backward_events_mesh<false>),
                                           reinterpret_cast<const void*>(k_backward_events_mesh<true>)};
    return bwd_launch(c, p, a, nullptr, nullptr, g, BwdUnit{kernels, &u, false}, stream, fn); // (no upstream on (rgbf, alpha): BwdArgs' stay null)
}

extern "C" {

int grt_ray_events_mesh_frame(grt_ctx* c, const grt_params* p, const grt_ray_events_mesh* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                              void* stream)
{
    const char* fn = "grt_ray_events_mesh_frame";
    RenderArgs a;
    int rc = fill(c, p, wanted(out), out ? out->first : 0u, out ? out->max_events : 0u, out ? out->step_first : 0u, out ? out->step_last : 0u, &a, fn);
    if (rc == GRT_OK) rc = check_forward(c, out, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, out, stream, fn);
}

int grt_ray_events_mesh_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const grt_ray_events_mesh* out, void* stream)
{
    const char* fn = "grt_ray_events_mesh_rays";
    RenderArgs a;
    int rc = fill(c, p, wanted(out), out ? out->first : 0u, out ? out->max_events : 0u, out ? out->step_first : 0u, out ? out->step_last : 0u, &a, fn);
    if (rc == GRT_OK) rc = check_forward(c, out, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_forward(c, a, out, stream, fn);
}

int grt_backward_events_mesh_frame(grt_ctx* c, const grt_params* p, const float* d_grad_alpha, uint32_t first, uint32_t max_events,
                                   uint32_t step_first, uint32_t step_last, const grt_gaussian_grads* out, uint32_t x0, uint32_t y0,
                                   uint32_t x1, uint32_t y1, void* stream)
{
    const char* fn = "grt_backward_events_mesh_frame";
    RenderArgs a;
    int rc = fill(c, p, true, first, max_events, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, d_grad_alpha, out, fn);
    if (rc == GRT_OK) rc = set_window(c, p, &a, x0, y0, x1, y1, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, d_grad_alpha, first, max_events, step_first, step_last, out, stream, fn);
}

int grt_backward_events_mesh_rays(grt_ctx* c, const grt_params* p, const float* d_rays, uint64_t n, const float* d_grad_alpha, uint32_t first,
                                  uint32_t max_events, uint32_t step_first, uint32_t step_last, const grt_gaussian_grads* out, void* stream)
{
    const char* fn = "grt_backward_events_mesh_rays";
    RenderArgs a;
    int rc = fill(c, p, true, first, max_events, step_first, step_last, &a, fn);
    if (rc == GRT_OK) rc = check_backward(c, d_grad_alpha, out, fn);
    if (rc == GRT_OK) rc = set_rays(c, &a, d_rays, n, fn);
    if (rc != GRT_OK) return rc;
    return launch_backward(c, p, a, d_grad_alpha, first, max_events, step_first, step_last, out, stream, fn);
}

} // extern "C"
