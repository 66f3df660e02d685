"""CPU checker of the aux outputs (grt_render_aux / grt_render_rays_aux: alpha, depth, count; definitions in include/grt.h).

It restates one Gaussian segment — trace(), shaders/tracer.cuh:328-373 — on top of the PINNED oracle primitives, which it
calls through oracle.lib() and never modifies: grto_trace_gps for the k nearest events of a round, grto_compute_response and
the particle's opacity for an event's alpha (fminf(0.99, r * opacity) in float32), grto_compute_radiance for its colour.  Per
ray it returns radiance, T, depth (float64, summed from the float32 terms (T alpha) and t) and count.  Mesh frames follow
grto_render_pixel's state machine (shaders/tracer.cu:17-110) with grto_tri_hit over the faces, grto_reflect / grto_refract and
the per-segment densities.

The checker proves its own event sequence: segment() compares its radiance and density with grto_trace bit for bit, and
pixel() its colour with grto_render_pixel.  Its rounds continue from a float tmin (just below the 7th event's t, skipping the
events at that t it has composited); an exact-t tie that this cannot restate — grto_trace continues from the 7th event's full
key — changes what it composites and shows up as a mismatch: CheckerMismatch, never skipped.
"""
import ctypes as C

import numpy as np

import oracle as O

f32 = np.float32
EPS_T = f32(1e-9)
TRACE_MESH_TMIN, TRACE_MESH_TMAX = f32(1e-5), f32(1e5)
REFRACTION_EPS_SHIFT = f32(1e-5)
TIMEOUT_ITERATIONS = 1000
MIRROR, NORMAL, GLASS = 0, 1, 2


class CheckerMismatch(AssertionError):
    """The checker's restatement disagrees with the pinned oracle (an event sequence it could not restate)."""


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _normalize(v):
    v = np.asarray(v, f32)
    inv = f32(1.0) / np.sqrt(f32(f32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
    return (v * inv).astype(f32)


def _dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def _length(v):
    return np.sqrt(_dot(v, v))


class Checker:
    """particles: oracle PARTICLE_DTYPE array; params: oracle.Params; scene: oracle.Scene of the same particles (meshes set on it
    when the frame has any: pass verts / normals / faces too)."""

    def __init__(self, particles, params, scene, mesh=None):
        self.parts = np.ascontiguousarray(particles, dtype=O.PARTICLE_DTYPE)
        self.p = params
        self.sc = scene
        self.L = O.lib()
        if mesh is not None:
            v, n, f = mesh
            self.mv = np.ascontiguousarray(v, f32)
            self.mn = np.ascontiguousarray(n, f32)
            self.mf = np.ascontiguousarray(f, np.uint32)
        else:
            self.mv = None
        self._ids = np.zeros(7, np.uint32)
        self._ts = np.zeros(7, f32)
        self._rgb = np.zeros(3, f32)

    def _part(self, i):
        return C.c_void_p(self.parts.ctypes.data + int(i) * O.PARTICLE_DTYPE.itemsize)

    # ---- one Gaussian segment (trace(), tracer.cuh:328-373) ----
    def _segment(self, o, d, t_min, t_max, density):
        o = np.ascontiguousarray(o, f32); d = np.ascontiguousarray(d, f32)
        op, dp = _fp(o), _fp(d)
        p = self.p
        minT, amin = f32(p.min_transmittance), f32(p.alpha_min)
        T = f32(f32(1.0) - f32(density))
        t_max = f32(t_max)
        lastT = f32(t_min)
        rad = np.zeros(3, f32)
        depth, count = 0.0, 0
        dn = _normalize(d)
        tmin_q = f32(lastT + EPS_T)
        t_hi = f32(t_max + EPS_T)
        t_last, skip = None, 0  # the previous round's last distance; how many events at it were composited already
        while lastT <= t_max and T > minT:
            n = self.L.grto_trace_gps(self.sc._h, op, dp, float(tmin_q), float(t_hi), self._ids.ctypes.data, self._ts.ctypes.data)
            if n == 0:
                break
            start = 0
            while start < n and skip and self._ts[start] == t_last:  # repeats of what the last round composited
                start += 1
                skip -= 1
            if start == n == 7:
                raise CheckerMismatch("seven events at one distance: the float continuation cannot restate them")
            for i in range(start, n):
                if not T > minT:
                    continue
                t = self._ts[i]
                lastT = max(t, lastT)
                pid = int(self._ids[i])
                r = f32(self.L.grto_compute_response(self._part(pid), op, dp))
                alpha = f32(min(f32(0.99), f32(r * f32(self.parts["opacity"][pid]))))
                if amin < alpha:
                    self.L.grto_compute_radiance(self._part(pid), _fp(dn), self.p.sh_degree_max, _fp(self._rgb))
                    rad = (rad + (self._rgb * T).astype(f32) * alpha).astype(f32)
                    term = f32(T * alpha)
                    depth += float(term) * float(t)
                    count += 1
                    T = f32(T * f32(f32(1.0) - alpha))
            if n < 7:
                break
            # the next round starts just below the 7th event's distance (grto_trace_gps takes a float tmin: every event AT that
            # distance comes back, a grazing ray's entry and exit at one t included) and skips those this round composited
            t_last = self._ts[6]
            skip = int(np.count_nonzero(self._ts[:n] == t_last))
            tmin_q = np.nextafter(t_last, f32(-np.inf), dtype=f32)
        return rad, f32(f32(1.0) - T), T, depth, count

    def segment(self, o, d, t_min, t_max, density=0.0, check=True):
        """(radiance f32[3], density, T, depth float64, count) of one segment; check: radiance and density equal grto_trace's bits."""
        rad, dens, T, depth, count = self._segment(o, d, t_min, t_max, density)
        if check:
            ref_rad, ref_dens = self.sc.trace(self.p, np.asarray(o, f32), np.asarray(d, f32), float(f32(t_min)), float(f32(t_max)),
                                              float(f32(density)))
            if not (np.array_equal(ref_rad.view(np.uint32), rad.view(np.uint32)) and f32(ref_dens) == dens):
                raise CheckerMismatch(f"segment o={list(o)} d={list(d)}: checker radiance {rad} density {dens!r} != grto_trace "
                                      f"{ref_rad} {ref_dens!r} (an exact-t tie the float tmin continuation cannot restate?)")
        return rad, dens, T, depth, count

    # ---- mesh closest hit (grt_oracle.c mesh_closest: lowest t in (tmin, tmax), ties to the lowest face) ----
    def _mesh_hit(self, o, d):
        if self.mv is None or len(self.mf) == 0:
            return None
        v0 = self.mv[self.mf[:, 0]].astype(np.float64); v1 = self.mv[self.mf[:, 1]].astype(np.float64)
        v2 = self.mv[self.mf[:, 2]].astype(np.float64)
        od, dd = np.asarray(o, np.float64), np.asarray(d, np.float64)
        e1, e2 = v1 - v0, v2 - v0
        pv = np.cross(dd[None], e2)
        det = np.einsum("ij,ij->i", e1, pv)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = od[None] - v0
            u = np.einsum("ij,ij->i", tv, pv) * inv
            q = np.cross(tv, e1)
            v = (q @ dd) * inv
        m = 1e-3  # float64 prefilter with a margin; the float32 test below decides
        cand = np.nonzero((det != 0) & (u >= -m) & (u <= 1 + m) & (v >= -m) & (u + v <= 1 + m))[0]
        best = None
        t_, u_, v_ = C.c_float(), C.c_float(), C.c_float()
        o32, d32 = np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)
        for f in cand:
            fc = self.mf[f]
            if not self.L.grto_tri_hit(_fp(self.mv[fc[0]]), _fp(self.mv[fc[1]]), _fp(self.mv[fc[2]]), _fp(o32), _fp(d32),
                                       C.byref(t_), C.byref(u_), C.byref(v_)):
                continue
            t = f32(t_.value)
            if not (t > TRACE_MESH_TMIN and t < TRACE_MESH_TMAX):
                continue
            if best is None or t < best[0] or (t == best[0] and f < best[3]):
                best = (t, f32(u_.value), f32(v_.value), int(f))
        return best

    def _bary_normal(self, hit):
        _, u, v, f = hit
        fc = self.mf[f]
        n0, n1, n2 = self.mn[fc[0]], self.mn[fc[1]], self.mn[fc[2]]
        w0 = f32(f32(f32(1.0) - u) - v)
        s = ((n0 * w0).astype(f32) + (n1 * u).astype(f32)).astype(f32)
        s = (s + (n2 * v).astype(f32)).astype(f32)
        return _normalize(s)

    # ---- the raygen loop (shaders/tracer.cu:58-106) ----
    def ray(self, o, d):
        """(rgb f32[3] pre-clamp accumColor, alpha = accumAlpha, depth, count of the first segment) of one ray."""
        p = self.p
        curO, curD = np.asarray(o, f32).copy(), np.asarray(d, f32).copy()
        accum = np.zeros(3, f32); direct = np.zeros(3, f32)
        accumAlpha, blocking, density = f32(0), f32(0), f32(0)
        nb, timeout = 0, 0
        first = None
        while _length(curD) > f32(0.1) and nb < p.max_bounces:
            ray_o, ray_d = curO, curD
            hit = self._mesh_hit(ray_o, ray_d)
            if hit is not None:
                t_hit = hit[0]
                normal = self._bary_normal(hit)
                state = 1
                newDir = np.zeros(3, f32)
                if p.type == MIRROR:
                    out = np.zeros(3, f32)
                    self.L.grto_reflect(_fp(np.ascontiguousarray(ray_d, f32)), _fp(normal), _fp(out))
                    newDir = out
                    nb += 1
                elif p.type == NORMAL:
                    rad, density, _, dep, cnt = self.segment(ray_o, ray_d, p.t_min, t_hit, density)
                    if first is None:
                        first = (dep, cnt)
                    alpha = density
                    accum = (accum + rad).astype(f32)
                    accumAlpha = f32(accumAlpha + alpha)
                    ncol = ((normal + f32(1.0)).astype(f32) * f32(0.5)).astype(f32)
                    accum = (accum + (ncol * f32(f32(1.0) - alpha)).astype(f32)).astype(f32)
                    accumAlpha = f32(accumAlpha + f32(f32(1.0) - alpha))
                    break
                else:
                    out = np.zeros(3, f32)
                    if self.L.grto_refract(_fp(np.ascontiguousarray(ray_d, f32)), _fp(normal), C.c_float(f32(1.5) / f32(1.0003)), _fp(out)):
                        t_hit = f32(t_hit + REFRACTION_EPS_SHIFT)
                    else:
                        nb += 1
                    newDir = out
                seg_t = t_hit
                curO = (ray_o + (ray_d * t_hit).astype(f32)).astype(f32)
                curD = newDir
            else:
                curO = np.zeros(3, f32); curD = np.zeros(3, f32)
                state = 0
                seg_t = f32(p.t_max)
            rad, density, _, dep, cnt = self.segment(ray_o, ray_d, p.t_min, seg_t, density)
            if first is None:
                first = (dep, cnt)
            alpha = density
            if state == 0:
                direct = (rad * alpha).astype(f32)
                accumAlpha = f32(np.clip(f32(accumAlpha + alpha), 0, 1))
            else:
                accum = (accum + (rad * f32(f32(1.0) - accumAlpha)).astype(f32)).astype(f32)
                accumAlpha = f32(np.clip(f32(accumAlpha + alpha), 0, 1))
                blocking = f32(np.clip(f32(blocking + alpha), 0, 1))
            accum = (accum + (direct * f32(f32(1.0) - blocking)).astype(f32)).astype(f32)
            timeout += 1
            if timeout > TIMEOUT_ITERATIONS:
                break
        dep, cnt = first if first is not None else (0.0, 0)
        return accum, float(accumAlpha), dep, cnt

    def pixel(self, x, y, check=True):
        """(rgb, alpha, depth, count) of pixel (x, y); fisheye r > 1: zeros.  check: rgb equals grto_render_pixel's bits."""
        rays, valid = self._rays()
        if not valid[y, x]:
            return np.zeros(3, f32), 0.0, 0.0, 0
        r = rays[y, x]
        rgb, alpha, dep, cnt = self.ray(r[:3], r[3:])
        if check:
            ref = self.sc.render_pixel(self.p, x, y)
            if not np.array_equal(ref.view(np.uint32), rgb.view(np.uint32)):
                raise CheckerMismatch(f"pixel ({x}, {y}): checker colour {rgb} != grto_render_pixel {ref}")
        return rgb, alpha, dep, cnt

    def _rays(self):
        if not hasattr(self, "_cam"):
            self._cam = O.camera_rays(self.p)
        return self._cam


def compare(name, got, want, tol_alpha=2e-6, rel_depth=1e-5, abs_depth=0.0):
    """got / want: dicts of 'alpha', 'depth', 'count' arrays over the same pixels.  Returns the indices that fail, by output:
    count equal, alpha within tol_alpha, depth within rel_depth relative plus abs_depth."""
    bad = {}
    c_g, c_w = np.asarray(got["count"]).astype(np.int64), np.asarray(want["count"]).astype(np.int64)
    bad["count"] = np.nonzero(c_g != c_w)[0]
    a_g, a_w = np.asarray(got["alpha"], np.float64), np.asarray(want["alpha"], np.float64)
    bad["alpha"] = np.nonzero(~(np.abs(a_g - a_w) <= tol_alpha))[0]
    d_g, d_w = np.asarray(got["depth"], np.float64), np.asarray(want["depth"], np.float64)
    bad["depth"] = np.nonzero(~(np.abs(d_g - d_w) <= rel_depth * np.abs(d_w) + abs_depth))[0]
    return {k: v for k, v in bad.items() if len(v)}
