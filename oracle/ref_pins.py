"""Inputs and reference-side outputs of the bit-exact pins in tests/test_oracle_units.py (TEST INFRASTRUCTURE ONLY).

The pins compare the oracle with functions of the reference compiled in place (oracle/_ref, `make -C oracle ref`).  That
library exists only where the reference checkout does, so what it returns for the pins' seeded inputs is stored as
tests/golden/ref_pins.npz and the tests compare the oracle with the stored values everywhere.  Regenerate (needs oracle/_ref):

  python oracle/ref_pins.py
"""
import ctypes as C
import os

import numpy as np

import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ref_pins.npz")
fp = C.POINTER(C.c_float)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def ptr(a):
    return a.ctypes.data_as(fp)


def unit_quat(rng):
    q = f32(rng.normal(size=4))
    return f32(q / np.float32(np.sqrt(np.float32((q * q).sum()))))


def uvw_inputs():
    """200 cameras: (eye, lookat, up, fovy, aspect)."""
    rng = np.random.default_rng(7)
    for _ in range(200):
        eye = f32(rng.normal(size=3) * 3); look = f32(rng.normal(size=3)); up = f32([0, 1, 0])
        fov = float(rng.uniform(20, 100)); asp = float(rng.uniform(0.5, 2.5))
        yield eye, look, up, fov, asp


def invcov_inputs():
    """300 particles (one-element PARTICLE_DTYPE arrays with quat / scale / pos set)."""
    rng = np.random.default_rng(11)
    for _ in range(300):
        p = np.zeros(1, O.PARTICLE_DTYPE)
        p["quat"] = unit_quat(rng); p["scale"] = f32(np.exp(rng.normal(-3, 1, size=3))); p["pos"] = f32(rng.normal(size=3))
        yield p


def response_inputs():
    """200 (particle, ray origin, unnormalised ray direction)."""
    rng = np.random.default_rng(13)
    for _ in range(200):
        p = np.zeros(1, O.PARTICLE_DTYPE)
        p["quat"] = unit_quat(rng); p["scale"] = f32(np.exp(rng.normal(-2, 0.7, size=3))); p["pos"] = f32(rng.normal(size=3) * 0.3)
        o = f32([0, 0, 3]); d = f32(rng.normal(size=3) * 0.1 + [0, 0, -1])
        yield p, o, d


def vector_inputs():
    """200 (vector, unnormalised normal)."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        yield f32(rng.normal(size=3)), f32(rng.normal(size=3))


def proxy_inputs():
    """50 particles of opacity 0.6."""
    rng = np.random.default_rng(3)
    for _ in range(50):
        p = np.zeros(1, O.PARTICLE_DTYPE)
        p["quat"] = unit_quat(rng); p["scale"] = f32(np.exp(rng.normal(-2, 0.7, size=3))); p["pos"] = f32(rng.normal(size=3))
        p["opacity"] = 0.6
        yield p


def small_scene(n=300, seed=21):
    rng = np.random.default_rng(seed)
    pos = f32(rng.normal(0.0, 0.45, size=(n, 3)))
    f_dc = f32(rng.uniform(-1.5, 1.5, size=(n, 3)))
    f_rest = f32(rng.normal(0.0, 0.1, size=(n, 45)))
    logit = f32(rng.normal(1.0, 2.0, size=n))
    log_scale = f32(rng.normal(np.log(0.12), 0.6, size=(n, 3)))  # anisotropic: axes differ by e^(+-0.6)
    rot = f32(rng.normal(size=(n, 4)))
    return O.activate(pos, f_dc, f_rest, logit, log_scale, rot)


def proxy_scale(opacity, alpha_min=0.01):
    """s = sqrtf(2 logf(opacity / alpha_min)) in float32, as the reference's instance transform computes it."""
    return np.float32(np.sqrt(np.float32(2.0) * np.float32(np.log(np.float32(opacity / np.float32(alpha_min))))))


def compute(R, L):
    """Every reference-side value the pins compare with: R = oracle.ref(), L = oracle.lib() (the pins' own oracle inputs)."""
    g = {}
    uvw = []
    for eye, look, up, fov, asp in uvw_inputs():
        u2 = np.zeros(3, np.float32); v2 = np.zeros(3, np.float32); w2 = np.zeros(3, np.float32)
        R.ref_uvw_frame(ptr(eye), ptr(look), ptr(up), C.c_float(fov), C.c_float(asp), ptr(u2), ptr(v2), ptr(w2))
        uvw.append([u2, v2, w2])
    g["uvw"] = f32(uvw)
    v2 = np.zeros(36, np.float32); i2 = np.zeros(60, np.uint32)
    R.ref_icosahedron(ptr(v2), i2.ctypes.data_as(C.c_void_p))
    g["icosahedron_vertices"], g["icosahedron_indices"] = v2.reshape(12, 3), i2
    inv_cov, mat3 = [], []
    for p in invcov_inputs():
        A2 = np.zeros(9, np.float32); Rg2 = np.zeros(9, np.float32)
        R.ref_inv_cov(ptr(f32(p["scale"][0])), ptr(f32(p["quat"][0])), ptr(A2))
        R.ref_mat3_cast(ptr(f32(p["quat"][0])), ptr(Rg2))
        inv_cov.append(A2); mat3.append(Rg2)
    g["inv_cov"], g["mat3_cast"] = f32(inv_cov), f32(mat3)
    dirs, args = [], []
    for p, o, d in response_inputs():
        # computeResponse rebuilt from the reference's glm pieces (mat*vec, dot): the argument of its expf
        dn = np.zeros(3, np.float32); R.ref_normalize(ptr(d), ptr(dn))
        A = np.zeros(9, np.float32)
        R.ref_inv_cov(ptr(f32(p["scale"][0])), ptr(f32(p["quat"][0])), ptr(A))
        mu = f32(p["pos"][0])
        og = np.zeros(3, np.float32); dg = np.zeros(3, np.float32); pg = np.zeros(3, np.float32)
        R.ref_mat3_vec(ptr(A), ptr(f32(o - mu)), ptr(og)); R.ref_mat3_vec(ptr(A), ptr(dn), ptr(dg))
        dval = np.float32(-np.float32(R.ref_glm_dot(ptr(og), ptr(dg))) / max(np.float32(1e-6), np.float32(R.ref_glm_dot(ptr(dg), ptr(dg)))))
        pos = f32(o + f32(dval * dn))
        R.ref_mat3_vec(ptr(A), ptr(f32(mu - pos)), ptr(pg))
        dirs.append(dn); args.append(np.float32(np.float32(-0.5) * np.float32(R.ref_glm_dot(ptr(pg), ptr(pg)))))
    g["response_dir"], g["response_exp_arg"] = f32(dirs), f32(args)
    normals, reflected = [], []
    for a, n in vector_inputs():
        nn = np.zeros(3, np.float32); R.ref_normalize(ptr(n), ptr(nn))
        r2 = np.zeros(3, np.float32); R.ref_reflect(ptr(a), ptr(nn), ptr(r2))
        normals.append(nn); reflected.append(r2)
    g["normalized"], g["reflected"] = f32(normals), f32(reflected)
    v = np.zeros((12, 3), np.float32); idx = np.zeros(60, np.uint32)
    L.grto_icosahedron(v.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p))
    s = L.grto_proxy_scale(0.6, 0.01)
    verts = []
    for p in proxy_inputs():
        for k in range(12):
            w = np.zeros(3, np.float32)
            R.ref_instance_vertex(ptr(f32(p["pos"][0])), ptr(f32(p["scale"][0])), ptr(f32(p["quat"][0])), C.c_float(s), ptr(v[k]), ptr(w))
            verts.append(w)
    g["proxy_vertices"] = f32(verts).reshape(50, 12, 3)
    # the reference's OWN icosahedron through its OWN instance transform T * (R * S) for every particle of small_scene()
    parts = small_scene()
    base = g["icosahedron_vertices"]
    inst = np.zeros((len(parts), 12, 3), np.float32)
    for i, p in enumerate(parts):
        if not p["opacity"] > 0.01:
            continue  # NaN / zero transform in the reference: unhittable (decision (vi)); the oracle never tests it
        for k in range(12):
            w = np.zeros(3, np.float32)
            R.ref_instance_vertex(ptr(f32(p["pos"])), ptr(f32(p["scale"])), ptr(f32(p["quat"])), C.c_float(float(proxy_scale(p["opacity"]))),
                                  ptr(f32(base[k])), ptr(w))
            inst[i, k] = w
    g["instanced_icosahedra"] = inst
    # the particles those vertices were computed from: the oracle's activate() of small_scene()'s columns on the machine that wrote them
    g["small_scene_particles"] = parts
    return g


if __name__ == "__main__":
    R = O.ref()
    assert R is not None, f"{O._REF} is not built: make -C oracle ref"
    np.savez_compressed(GOLDEN, **compute(R, O.lib()))
    print("wrote", GOLDEN)
