// grt_render_stream_body.inc — body of the streaming kernel, included once per window size (GRT_KS = 12: the
// default kernel at 4 waves/SIMD; GRT_KS = 32: the "big window" kernel at 2 waves/SIMD used for the few blocks the
// scheduling feedback marks as heavy, where a 12-particle window overflows and forces extra passes).
//
// ---- per-lane particle slots.  Registers hold only the GRT_KS sorted 64-bit keys k0.. (~0 = free); each key
// carries, in its 5 lowest bits, the index of its payload cell in LDS (exit t while the key is the entry event —
// +inf = no exit event — and alpha), so sorting moves 2 registers per slot and the window is GRT_KS particles
// (2 hits each) for fewer registers than 7 register-resident (key, other, alpha) slots.
//   key = t bits << 32 | particle id << 6 | exit << 5 | payload cell          (particle ids < 2^26)
#define KS GRT_KS
#if GRT_KS == 12
#define KLAST k11
#define SLOT_DECL                                                                                          \
    uint64_t k0 = kKeyInvalid, k1 = kKeyInvalid, k2 = kKeyInvalid, k3 = kKeyInvalid, k4 = kKeyInvalid,   \
             k5 = kKeyInvalid, k6 = kKeyInvalid, k7 = kKeyInvalid, k8 = kKeyInvalid, k9 = kKeyInvalid,   \
             k10 = kKeyInvalid, k11 = kKeyInvalid;                                                         \
    uint32_t pmask = 0; /* payload cells in use */
#define SLOT_CLEAR                                                                                         \
    k0 = k1 = k2 = k3 = k4 = k5 = k6 = k7 = k8 = k9 = k10 = k11 = kKeyInvalid;                            \
    pmask = 0;
#elif GRT_KS == 32
#define KLAST k31
#define SLOT_DECL                                                                                          \
    uint64_t k0 = kKeyInvalid, k1 = kKeyInvalid, k2 = kKeyInvalid, k3 = kKeyInvalid, k4 = kKeyInvalid,   \
             k5 = kKeyInvalid, k6 = kKeyInvalid, k7 = kKeyInvalid, k8 = kKeyInvalid, k9 = kKeyInvalid,   \
             k10 = kKeyInvalid, k11 = kKeyInvalid, k12 = kKeyInvalid, k13 = kKeyInvalid, k14 = kKeyInvalid, \
             k15 = kKeyInvalid, k16 = kKeyInvalid, k17 = kKeyInvalid, k18 = kKeyInvalid, k19 = kKeyInvalid, \
             k20 = kKeyInvalid, k21 = kKeyInvalid, k22 = kKeyInvalid, k23 = kKeyInvalid, k24 = kKeyInvalid, \
             k25 = kKeyInvalid, k26 = kKeyInvalid, k27 = kKeyInvalid, k28 = kKeyInvalid, k29 = kKeyInvalid, \
             k30 = kKeyInvalid, k31 = kKeyInvalid;                                                         \
    uint32_t pmask = 0; /* payload cells in use */
#define SLOT_CLEAR                                                                                         \
    k0 = k1 = k2 = k3 = k4 = k5 = k6 = k7 = k8 = k9 = k10 = k11 = k12 = k13 = k14 = k15 = k16 = k17 = k18 = \
        k19 = k20 = k21 = k22 = k23 = k24 = k25 = k26 = k27 = k28 = k29 = k30 = k31 = kKeyInvalid;         \
    pmask = 0;
#else
#error "GRT_KS must be 12 or 32"
#endif
// SLOT_INSERT(KEY): sorted insert (KEY == ~0 is a no-op; the largest key falls off a full window);
// SLOT_SHIFT_ALL(MASK): lanes in MASK pop their smallest key.  Generated inline assembly — one v_mov_b64 under
// EXEC per conditional move instead of two v_cndmask_b32 (see gen_slots.py).
#include "grt_slots_gen.inc"
#define PL_OTHER(cell) pl_other[(cell) * kWG + lane]
#define PL_ALPHA(cell) pl_alpha[(cell) * kWG + lane]

// ---- wave-level frontier: slot i (0..63) = lane i of (fl0, fr0); fu0 = wave-uniform occupancy mask ----
#define FRONTIER_PUSH(LAMBDA, REF, OK)                                                                     \
    {                                                                                                      \
        const uint64_t free_ = ~fu0;                                                                       \
        OK = free_ != 0ull;                                                                                \
        const uint32_t slot_ = OK ? (uint32_t)__builtin_ctzll(free_) : 64u; /* 64 matches no lane */       \
        const bool me_ = lane == slot_;                                                                    \
        fl0 = me_ ? (LAMBDA) : fl0;                                                                        \
        fr0 = me_ ? (REF) : fr0;                                                                           \
        fu0 |= OK ? (1ull << (slot_ & 63u)) : 0ull;                                                        \
    }

// depth-first overflow stack: rarely used, so it lives in LDS (256 entries per wave) and costs no registers
#define DFS_PUSH(REF)                                                                                      \
    {                                                                                                      \
        if (lane == 0u) dstack[dsp] = (REF);                                                               \
        ++dsp;                                                                                             \
    }

template <bool COUNT, bool SH, bool MESH>
__global__ __launch_bounds__(kWG, GRT_WAVES) void GRT_KERNEL_NAME(const RenderArgs a)
{
    // rank of this workgroup in the launch order; runs of 4 * chunk consecutive ranks execute on one XCD (one L2)
    const uint32_t rank = xcd_swizzle(blockIdx.x, gridDim.x, a.swizzle_chunk * 4u);
    if (a.heavy_role) { // split launch: this kernel only owns one side of the cost-sorted order
        const uint32_t nh = *a.n_heavy;
        if ((a.heavy_role == 1u) != (rank < nh)) return;
    }
    __shared__ float pl_other[KS * kWG], pl_alpha[KS * kWG];
    __shared__ uint32_t dstack[256]; // depth <= 3 per wide level + 3: covers every tree the launcher sends here (height <= 120)
    Cnt c;
    GRT_W_DECL
    // one workgroup = one wave = one 8x8 tile (scheduling unit u); units 4b..4b+3 cover the 16x16 screen block b
    const uint32_t unit = [&] { // workgroup -> tile: heaviest-first order, or XCD-contiguous blocks (speed only)
        return a.order ? a.order[rank] : rank;
    }();
    const uint32_t blk = unit >> 2, wave = unit & 3u, lane = threadIdx.x;
    const uint32_t lx = (wave & 1u) * 8u + (lane & 7u), ly = (wave >> 1) * 8u + (lane >> 3);
    uint32_t px, py;
    size_t out_idx;
    bool in_frame;
    if (a.mode == 0) {
        px = a.x0 + (blk % a.nbx) * 16u + lx;
        py = a.y0 + (blk / a.nbx) * 16u + ly;
        in_frame = (px < a.x1) && (py < a.y1);
        out_idx = (size_t)py * a.p.width + px;
    } else {
        const uint32_t per_tile = a.nbx * a.nby;
        const uint32_t j = blk / per_tile, sub = blk % per_tile;
        const uint32_t tile = a.first_tile + j * a.tile_stride;
        const uint32_t tx_ = tile % a.tiles_x, ty_ = tile / a.tiles_x;
        const uint32_t ox = (sub % a.nbx) * 16u + lx, oy = (sub / a.nbx) * 16u + ly;
        px = tx_ * a.tile_w + ox;
        py = ty_ * a.tile_h + oy;
        in_frame = (px < a.p.width) && (py < a.p.height);
        out_idx = ((size_t)j * a.tile_h + oy) * a.tile_w + ox;
    }
    const bool write = in_frame || (a.mode == 1);
    const f3 nU = mk3(-a.p.U[0], -a.p.U[1], -a.p.U[2]), nV = mk3(-a.p.V[0], -a.p.V[1], -a.p.V[2]);
    const f3 W = mk3(a.p.W[0], a.p.W[1], a.p.W[2]);
    const f3 o = mk3(a.p.eye[0], a.p.eye[1], a.p.eye[2]); // wave-uniform origin (camera rays)
    f3 d = mk3(0.0f, 0.0f, -1.0f);
    bool have_ray = in_frame;
    if (in_frame) {
        if (!a.p.mode_fisheye) get_ray(px, py, nU, nV, W, a.p.width, a.p.height, d);
        else have_ray = get_fisheye_ray(px, py, nU, nV, W, a.p.width, a.p.height, d);
    }
    if (COUNT && have_ray && !MESH) c.rays++;
    have_ray = have_ray && (length3(d) > 0.1f) && (a.p.max_bounces > 0u); // loop guard, shaders/tracer.cu:59
    // MESH: stage 1 (k_primary_mesh) already traced the mesh for this pixel
    float seg_tmax = a.p.t_max;
    uint32_t pflags = 0;
    f3 nextO = mk3(0, 0, 0), nextD = mk3(0, 0, 0), hitN = mk3(0, 0, 0);
    if (MESH) {
        const size_t pi = ((size_t)blk * kBlock + wave * 64u + lane) * 3;
        const float4 pr0 = a.prec[pi], pr1 = a.prec[pi + 1], pr2 = a.prec[pi + 2];
        seg_tmax = pr0.x;
        pflags = __float_as_uint(pr0.y);
        nextO = mk3(pr0.z, pr0.w, pr1.x);
        nextD = mk3(pr1.y, pr1.z, pr1.w);
        hitN = mk3(pr2.x, pr2.y, pr2.z);
        have_ray = have_ray && ((pflags >> 16) & 1u);
    }

    // ---- trace() for the whole wave (shaders/tracer.cuh:328-373), density starts at 0 ----
    const float minT = a.p.minTransmittance;
    float T = 1.0f;
    f3 radiance = mk3(0.0f, 0.0f, 0.0f);
    if (COUNT && have_ray) c.segments++;
    if (a.root_ref != kNoRoot) {
        const float epsT = 1e-9f;
        const f3 dn = normalize3(d);
        const rayinv ri = mk_rayinv(o, d);
        const float t_hi = seg_tmax + epsT; // per lane when MESH (segment ends at the mesh hit)
        const float t_hi_m = __uint_as_float(__float_as_uint(t_hi) - 1u); // largest float below t_hi (t_hi > 0)
        // Box tests: when every ray of the wave has the same direction signs (all but the few tiles that straddle
        // an axis), the near/far plane of each slab is picked on the scalar unit and the six products run as three
        // packed FMAs; otherwise the general min/max form is used.  Culling only — never decides a hit.
        const v2f inv_xy = {ri.inv.x, ri.inv.y}, inv_zz = {ri.inv.z, ri.inv.z};
        const v2f oiv_xy = {ri.oinv.x, ri.oinv.y}, oiv_zz = {ri.oinv.z, ri.oinv.z};
        const uint64_t raym = wave_ballot(have_ray);
        const uint64_t ngx = wave_ballot(have_ray && ri.inv.x < 0.0f), ngy = wave_ballot(have_ray && ri.inv.y < 0.0f);
        const bool coh = (ngx == 0ull || ngx == raym) && (ngy == 0ull || ngy == raym);
        // x/y swap mask for the (lo, hi) pairs of a box, applied with 64-bit scalar ops
        const uint64_t mxy = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(ngy ? -1 : 0) << 32) |
                             (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(ngx ? -1 : 0);
        uint64_t last_key = mk_skey(a.p.t_min + epsT, 0x03FFFFFFu, 1) | kCellMask; // last composited event (exclusive bound)
        bool alive = have_ray && (T > minT);
        uint32_t stalls = 0;
        SLOT_DECL
        uint32_t iters = 0; // wave-uniform work measure for the scheduling feedback
        while (wave_any(alive)) { // one iteration = one front-to-back pass
            if (COUNT && alive) c.rounds++;
            const uint64_t pass_lo = last_key; // events with key <= pass_lo were composited by an earlier pass
            const float t_lo = key_t(pass_lo);
            uint64_t cutoff = kKeyInvalid;     // smallest key this lane had to drop in this pass
            SLOT_CLEAR
            float fl0 = INFINITY;
            uint32_t fr0 = 0, dsp = 0;
            uint64_t fu0 = 0;
            {
                bool ok_;
                FRONTIER_PUSH(0.0f, a.root_ref, ok_)
                (void)ok_;
            }
            float F = 0.0f;
            bool final_sweep = false;
            uint32_t bypass = kNoRoot; // a child whose key equals F is a frontier minimum: expand it next, no push/pop
            while (true) {
                uint32_t cur = 0;
                if (!final_sweep) {
                    if (bypass != kNoRoot && wave_any(alive)) {
                        cur = bypass;
                        bypass = kNoRoot;
                    } else if (!wave_any(alive) || (dsp == 0 && !fu0)) {
                        // frontier exhausted (or every lane done): everything still buffered is final
                        F = INFINITY;
                        final_sweep = true;
                    } else if (dsp) { // depth-first overflow entries first; the finality bound F is unchanged
                        --dsp;
                        cur = dstack[dsp]; // same address for the whole wave: an LDS broadcast
                    } else { // pop the frontier minimum
                        F = wave_min(fl0);
                        const uint32_t slot = (uint32_t)__builtin_ctzll(wave_ballot(fl0 == F));
                        cur = (uint32_t)__builtin_amdgcn_readlane((int)fr0, (int)slot);
                        fl0 = (lane == slot) ? INFINITY : fl0;
                        fu0 &= ~(1ull << slot);
                    }
                }
                cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);
                ++iters;
                GRT_W(rays)
                // issue the popped record's 64-B scalar fetch now: its latency overlaps the compositing below
                const bool is_leaf = (cur & kLeafBit) != 0u;
                // the final sweep pops nothing (cur = 0): its (unused) prefetch reads record 0, which always exists —
                // a scene of <= leaf_max proxies has a leaf root and NO wide-node array at all
                const bool ld_leaf = is_leaf || final_sweep;
                const float4* pbase = ld_leaf ? a.rec : a.wnodes;
                const uint32_t pidx = ld_leaf ? leaf_first(cur) * 4u : cur * 8u;
                const float4 p0 = sload4(pbase, pidx), p1 = sload4(pbase, pidx + 1), p2 = sload4(pbase, pidx + 2),
                             p3 = sload4(pbase, pidx + 3), p4 = sload4(pbase, pidx + 4), p5 = sload4(pbase, pidx + 5),
                             p6 = sload4(pbase, pidx + 6); // 128-B wide node (a leaf uses the first 64 B)
                const float4 p7 = sload4(a.erec, is_leaf ? leaf_first(cur) : 0u); // first particle's eye record

                // ---- composite every buffered event with t < F (and key < cutoff), in key order ----
                while (true) {
                    const bool can_ = alive && (k0 != kKeyInvalid) && (key_t(k0) < F) && (k0 < cutoff);
                    const uint64_t cm_ = wave_ballot(can_);
                    if (!cm_) break;
                    GRT_W(hit_evals)
                    const uint64_t ek = k0;
                    const uint32_t cell = (uint32_t)(ek & kCellMask);
                    const uint32_t id = skey_id(ek);
                    float ea = 0.0f, eo = INFINITY;
                    float4 cc = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (can_) { // payload from LDS and (degree 0) the colour, both in flight while the window is popped
                        ea = PL_ALPHA(cell); eo = PL_OTHER(cell);
                        if (!SH) cc = a.color0[id];
                    }
                    SLOT_SHIFT_ALL(cm_)
                    // (equal keys: a split particle met through two of its pieces — the repeat only gives its cell back)
                    const bool dup_ = can_ && ((ek | kCellMask) == last_key);
                    if (can_ && !dup_) { // shaders/tracer.cuh:352-367
                        if (COUNT) c.hit_evals++;
                        last_key = ek | kCellMask; // nothing with the same (t, id, exit) can compare above it
                        if (a.p.alpha_min < ea) {
                            f3 L;
                            if (!SH) {
                                L = mk3(cc.x, cc.y, cc.z);
                            } else {
                                // the SH basis depends on the ray only: left alone, the compiler hoists its ~20 terms out
                                // of the traversal loop and spills them; recomputing them per hit is far cheaper
                                f3 dl = dn;
                                asm volatile("" : "+v"(dl.x), "+v"(dl.y), "+v"(dl.z));
                                L = sh_radiance(a.sh + (size_t)id * 48, dl, a.p.sh_degree_max);
                            }
                            radiance = add3(radiance, mul3s(mul3s(L, T), ea));
                            T *= (1.0f - ea);
                        }
                        if (!(T > minT)) alive = false;
                    }
                    // pop slot 0; an entry whose exit lies inside the segment is re-keyed to its exit event and
                    // keeps its payload cell, otherwise the cell is released
                    const bool rekey = can_ && !dup_ && ((((uint32_t)ek) & 32u) == 0u) && (eo < t_hi);
                    const uint64_t nk = rekey ? (mk_skey(eo, id, 1) | (uint64_t)cell) : kKeyInvalid;
                    pmask = (can_ && !rekey) ? (pmask & ~(1u << cell)) : pmask;
                    if (wave_any(rekey)) { // wave-uniform branch
                        GRT_W(rounds)
                        if (rekey) PL_OTHER(cell) = INFINITY;
                        SLOT_INSERT(nk) // a slot was just freed: it fits
                    }
                }
                if (final_sweep) break;

                const float cut_t = (cutoff != kKeyInvalid) ? key_t(cutoff) : t_hi_m;
                if (is_leaf) {
                    const uint32_t first = leaf_first(cur), cnt = leaf_count(cur);
                    float4 r0 = p0, r1 = p1, r2 = p2, r3 = p3, e0 = p7;
                    for (uint32_t j = 0; j < cnt; j++) {
                        if (j) {
                            const uint32_t idx = (first + j) * 4u;
                            r0 = sload4(a.rec, idx); r1 = sload4(a.rec, idx + 1); r2 = sload4(a.rec, idx + 2);
                            r3 = sload4(a.rec, idx + 3);
                            e0 = sload4(a.erec, first + j);
                        }
                        if (COUNT) c.fetches += 5; // 64-B record + 16-B eye record, in 16-B units
                        GRT_W(fetches)
                        const f3 mu = mk3(r0.x, r0.y, r0.z);
                        m33 A;
                        A.a[0] = r1.x; A.a[1] = r1.y; A.a[2] = r1.z;
                        A.a[3] = r2.x; A.a[4] = r2.y; A.a[5] = r2.z;
                        A.a[6] = r3.x; A.a[7] = r3.y; A.a[8] = r3.z;
                        // o_g = A (o - mu) and what derives from it alone come from the eye record (wave-uniform)
                        const f3 o_g = mk3(e0.x, e0.y, e0.z);
                        const f3 d_g = matvec(A, d);
                        {   // conservative sphere pre-test (proxy_sphere_maybe_pre) as lane masks: no lane can touch it -> skip
                            const float b_ = dot3(o_g, d_g), aa_ = dot3(d_g, d_g);
                            const uint64_t m_ = (wave_ballot(e0.w <= 0.0f) | wave_ballot(b_ * b_ * (1.0f + 4e-6f) >= aa_ * e0.w)) &
                                                wave_ballot(alive);
                            if (!m_) continue;
                        }
                        if (COUNT && alive) c.proxy_tests++;
                        GRT_W(proxy_tests)
                        float te, tx;
                        const bool hit = proxy_slabs(o_g, d_g, r0.w, te, tx) && alive;
                        const uint32_t id = __float_as_uint(r2.w);
                        const uint64_t ke = mk_skey(te, id, 0), kx = mk_skey(tx, id, 1);
                        // float compares first: te/tx may be negative or NaN, the unsigned key compares assume t > 0
                        // (> last_key: what was composited already is not taken again when another piece of it turns up)
                        bool in_e = hit && (te >= t_lo) && (te < t_hi) && (ke > last_key);
                        bool in_x = hit && (tx >= t_lo) && (tx < t_hi) && (kx > last_key);
                        const uint32_t cellb = __float_as_uint(r3.w);
                        if (cellb) { // piece of a split proxy: reports the particle only when the first pending event lies in its cell
                            const bool own_ = piece_owns(cellb, r0.w, o_g, d_g, in_e ? te : tx);
                            in_e = in_e && own_;
                            in_x = in_x && own_;
                        }
                        const uint64_t k_first = in_e ? ke : (in_x ? kx : kKeyInvalid); // the slot's first pending event
                        const bool ins = (k_first != kKeyInvalid) && (k_first < cutoff);
                        if (wave_any(ins)) { // wave-uniform branch
                            GRT_W(segments)
                            // alpha does not depend on the hit distance (shaders/tracer.cuh:354-357)
                            const float alpha = fminf(0.99f, response_from(A, mu, o, d, o_g, d_g) * r1.w);
                            const float other = (in_e && in_x) ? tx : INFINITY;
                            // window full: the largest pending key is dropped (the new one or slot 11's) and the lane
                            // becomes lossy beyond it
                            const bool full = KLAST != kKeyInvalid;
                            const bool take = ins && (!full || k_first < KLAST);
                            const uint64_t dropped = (ins && full) ? (take ? (KLAST | kCellMask) : k_first) : kKeyInvalid;
                            cutoff = (dropped < cutoff) ? dropped : cutoff;
                            const uint32_t cell = full ? (uint32_t)(KLAST & kCellMask) : (uint32_t)__builtin_ctz(~pmask);
                            KLAST = (take && full) ? kKeyInvalid : KLAST;
                            pmask = take ? (pmask | (1u << cell)) : pmask;
                            if (take) { PL_OTHER(cell) = other; PL_ALPHA(cell) = alpha; }
                            SLOT_INSERT(take ? (k_first | (uint64_t)cell) : kKeyInvalid)
                        }
                    }
                } else {
                    // 4-wide node: boxes of up to four (grand)children in one 128-B fetch
                    if (COUNT) { c.fetches += 8; if (alive) c.node_visits++; } // 128-B wide node
                    GRT_W(node_visits)
                    // a lane wants a child when its box interval [n, f] overlaps the lane's open interval: from the
                    // last composited t (lo) up to the cutoff (or the segment end).  N = max(n, lo), Fx = min(f, limit)
                    // (integer min/max: lo > 0, so the bit patterns order correctly and a negative f stays negative);
                    // N is also the lane's lower bound for any unseen hit in the child.
                    const int lo_i = __float_as_int(key_t(last_key)), lim_i = __float_as_int(cut_t);
                    float N0, N1, N2, N3, F0, F1, F2, F3;
#define GRT_BOX_COH(LX, LY, HX, HY, LZ, HZ, NN, FF)                                                        \
                    {                                                                                      \
                        const uint64_t l_ = pack2(LX, LY), h_ = pack2(HX, HY), t_ = (l_ ^ h_) & mxy;       \
                        const v2f nxy = fma2(unpack2(l_ ^ t_), inv_xy, oiv_xy);                            \
                        const v2f fxy = fma2(unpack2(h_ ^ t_), inv_xy, oiv_xy);                            \
                        const v2f zz = fma2(v2f{LZ, HZ}, inv_zz, oiv_zz);                                  \
                        NN = __int_as_float(max(__float_as_int(fmaxf(fmaxf(nxy.x, nxy.y), fminf(zz.x, zz.y))), lo_i)); \
                        FF = __int_as_float(min(__float_as_int(fminf(fminf(fxy.x, fxy.y), fmaxf(zz.x, zz.y))), lim_i)); \
                    }
#define GRT_BOX_GEN(LX, LY, HX, HY, LZ, HZ, NN, FF)                                                        \
                    {                                                                                      \
                        float n_, f_;                                                                      \
                        box_interval(LX, LY, LZ, HX, HY, HZ, ri, n_, f_);                                  \
                        NN = __int_as_float(max(__float_as_int(n_), lo_i));                                \
                        FF = __int_as_float(min(__float_as_int(f_), lim_i));                               \
                    }
#define GRT_BOX4(B)                                                                                        \
                    B(p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, N0, F0)                                          \
                    B(p1.z, p1.w, p2.x, p2.y, p2.z, p2.w, N1, F1)                                          \
                    B(p3.x, p3.y, p3.z, p3.w, p4.x, p4.y, N2, F2)                                          \
                    B(p4.z, p4.w, p5.x, p5.y, p5.z, p5.w, N3, F3)
                    if (coh) { GRT_BOX4(GRT_BOX_COH) } else { GRT_BOX4(GRT_BOX_GEN) }
#undef GRT_BOX4
#undef GRT_BOX_GEN
#undef GRT_BOX_COH
                    const uint32_t c0 = __float_as_uint(p6.x), c1 = __float_as_uint(p6.y), c2 = __float_as_uint(p6.z),
                                   c3 = __float_as_uint(p6.w);
                    const bool h0 = alive && (N0 <= F0);
                    const bool h1 = alive && (N1 <= F1);
                    const bool h2 = alive && (c2 != kNoRoot) && (N2 <= F2);
                    const bool h3 = alive && (c3 != kNoRoot) && (N3 <= F3);
                    // the four reductions back to back (independent chains overlap)
                    float lam0, lam1, lam2, lam3;
                    wave_min4(h0 ? N0 : INFINITY, h1 ? N1 : INFINITY, h2 ? N2 : INFINITY, h3 ? N3 : INFINITY, lam0, lam1, lam2,
                              lam3);
                    // some lane wants the child <=> its reduced key is finite (a scalar compare)
                    const bool any0 = lam0 < INFINITY, any1 = lam1 < INFINITY, any2 = lam2 < INFINITY, any3 = lam3 < INFINITY;
                    if (dsp) { // already depth-first below a full frontier: stay depth-first
                        if (any3) DFS_PUSH(c3)
                        if (any2) DFS_PUSH(c2)
                        if (any1) DFS_PUSH(c1)
                        if (any0) DFS_PUSH(c0)
                    } else {
                        // a child whose key equals the bound F just popped is a minimum of the frontier (every entry
                        // is >= F): expand it right away instead of pushing and popping it
                        const bool by0 = any0 && (lam0 <= F);
                        const bool by1 = any1 && !by0 && (lam1 <= F);
                        const bool by2 = any2 && !by0 && !by1 && (lam2 <= F);
                        const bool by3 = any3 && !by0 && !by1 && !by2 && (lam3 <= F);
                        bypass = by0 ? c0 : (by1 ? c1 : (by2 ? c2 : (by3 ? c3 : kNoRoot)));
#define PUSH_CHILD(ANY, BY, LAM, REF)                                                                      \
                        if ((ANY) && !(BY)) {                                                              \
                            bool ok = false;                                                               \
                            if (!dsp) FRONTIER_PUSH(LAM, REF, ok)                                          \
                            if (!ok) DFS_PUSH(REF)                                                         \
                        }
                        PUSH_CHILD(any0, by0, lam0, c0)
                        PUSH_CHILD(any1, by1, lam1, c1)
                        PUSH_CHILD(any2, by2, lam2, c2)
                        PUSH_CHILD(any3, by3, lam3, c3)
#undef PUSH_CHILD
                    }
                }
            }
            // a lane goes again only if it dropped something and still has transmittance left
            const bool progressed = last_key != pass_lo;
            stalls = progressed ? 0u : stalls + 1u;
            const bool again = alive && (cutoff != kKeyInvalid);
            // giving up on a lane that still has transmittance and dropped hits would lose part of a pixel: counted, and
            // the tests assert it never happens (grt_counters::stall_exits)
            if (COUNT && again && stalls >= 2u) c.stall_exits++;
            if (wave_any(again && stalls >= 2u) && lane == 0) atomicOr(a.err_word, kErrStall); // always on, counters or not
            alive = again && (stalls < 2u);
        }
        // the big-window kernel needs ~4x fewer iterations for the same block (no extra passes): scale its cost so
        // that a block keeps its class from frame to frame instead of oscillating between the two kernels
        if (a.cost && lane == 0) atomicMax(&a.cost[unit], GRT_KS > 12 ? iters * 4u : iters);
    }
    const float density = 1.0f - T;

    f3 col = mk3(0.0f, 0.0f, 0.0f);
    bool cont = false; // MESH: the ray goes on bouncing (stage 3)
    f3 accumColor = mk3(0, 0, 0);
    float accumAlpha = 0.0f, blocking = 0.0f;
    const uint32_t numBounces = (pflags >> 8) & 0xFFu;
    if (have_ray) {
        const float alpha = density;
        if (!MESH) {
            const f3 directLight = mul3s(radiance, alpha);     // shaders/tracer.cu:80
            col = add3(col, mul3s(directLight, 1.0f - 0.0f));  // shaders/tracer.cu:101 with blocking == 0
        } else {
            // first iteration of the bounce loop (shaders/tracer.cu:58-106) with all accumulators at zero
            const uint32_t state = pflags & 0xFFu;
            f3 directLight = mk3(0, 0, 0);
            if (state == 3u) { // Terminate: renderNormal, shaders/tracer.cuh:417-428
                accumColor = add3(accumColor, radiance);
                accumAlpha += alpha;
                const f3 normalColor = mul3s(add3(hitN, mk3(1.0f, 1.0f, 1.0f)), 0.5f);
                accumColor = add3(accumColor, mul3s(normalColor, 1.0f - alpha));
            } else {
                if (state == 0u) { // LastGaussianPass, shaders/tracer.cu:68-82
                    directLight = mul3s(radiance, alpha);
                    accumAlpha = clampf(accumAlpha + alpha, 0.0f, 1.0f);
                } else {           // shaders/tracer.cu:84-98
                    accumColor = add3(accumColor, mul3s(radiance, 1.0f - accumAlpha));
                    accumAlpha = clampf(accumAlpha + alpha, 0.0f, 1.0f);
                    blocking = clampf(blocking + alpha, 0.0f, 1.0f);
                }
                accumColor = add3(accumColor, mul3s(directLight, 1.0f - blocking)); // shaders/tracer.cu:101
                cont = (length3(nextD) > 0.1f) && (numBounces < a.p.max_bounces);
            }
            col = accumColor;
        }
    }
    if (MESH) {
        // ---- the rays that go on: the wave takes ONE 64-entry chunk of the queue (one atomic), every lane writes its own
        //      slot; bit 31 of the timeout word marks the slots that carry a ray (same layout as grt_tile.h) ----
        const uint64_t mask = wave_ballot(cont);
        if (mask) { // wave-uniform
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(a.qcount, 1u);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            float4* q = a.queue + ((size_t)base * 64u + lane) * 4;
            if (cont) {
                q[0] = make_float4(nextO.x, nextO.y, nextO.z, nextD.x);
                q[1] = make_float4(nextD.y, nextD.z, accumColor.x, accumColor.y);
                q[2] = make_float4(accumColor.z, accumAlpha, blocking, density);
            }
            q[3] = make_float4(__uint_as_float(numBounces), __uint_as_float(1u | (cont ? 0x80000000u : 0u)), // timeout after one iteration
                               __uint_as_float((uint32_t)out_idx), __uint_as_float((uint32_t)(out_idx >> 32)));
        }
    }
    const bool write_px = write && !cont; // queued rays write their pixel in stage 3
    if (write_px) {
        if (a.outf) {
            a.outf[out_idx * 3] = col.x; a.outf[out_idx * 3 + 1] = col.y; a.outf[out_idx * 3 + 2] = col.z;
        }
        if (a.out8) {
            a.out8[out_idx * 3] = quantize8(col.x);
            a.out8[out_idx * 3 + 1] = quantize8(col.y);
            a.out8[out_idx * 3 + 2] = quantize8(col.z);
        }
    }
    GRT_W_FLUSH
    if (COUNT) {
        uint32_t v0 = c.rays, v1 = c.segments, v2 = c.hit_evals, v3 = c.rounds, v4 = c.node_visits, v5 = c.proxy_tests;
        for (int off = 32; off > 0; off >>= 1) {
            v0 += (uint32_t)__shfl_xor((int)v0, off); v1 += (uint32_t)__shfl_xor((int)v1, off);
            v2 += (uint32_t)__shfl_xor((int)v2, off); v3 += (uint32_t)__shfl_xor((int)v3, off);
            v4 += (uint32_t)__shfl_xor((int)v4, off); v5 += (uint32_t)__shfl_xor((int)v5, off);
        }
        if (lane == 0) {
            if (v0) atomicAdd(&a.counters[0], (unsigned long long)v0);
            if (v1) atomicAdd(&a.counters[1], (unsigned long long)v1);
            if (v2) atomicAdd(&a.counters[2], (unsigned long long)v2);
            if (v3) atomicAdd(&a.counters[3], (unsigned long long)v3);
            if (v4) atomicAdd(&a.counters[4], (unsigned long long)v4);
            if (v5) atomicAdd(&a.counters[5], (unsigned long long)v5);
            if (c.fetches) atomicAdd(&a.counters[6], (unsigned long long)c.fetches);
        }
        if (c.stall_exits) atomicAdd(&a.counters[7], (unsigned long long)c.stall_exits); // per lane; expected never
    }
}


#undef KS
#undef KLAST
#undef SLOT_DECL
#undef SLOT_CLEAR
#undef SLOT_INSERT
#undef SLOT_SHIFT_ALL
#undef PL_OTHER
#undef PL_ALPHA
#undef FRONTIER_PUSH
#undef DFS_PUSH
