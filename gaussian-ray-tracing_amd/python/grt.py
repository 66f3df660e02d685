"""ctypes binding of libgrt_hip.so (include/grt.h) for bench.py and the tests.

PyTorch is used only as plumbing: device buffers (torch.empty on cuda:N), the current stream and
torch.distributed.  There is NO CPU fallback here: without the HIP library or a GPU every call raises.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (GRT_LIB: a diagnostic build of the same library, e.g. make EXTRA=-DGRT_TILE_DIAG — profiling only)
LIB_PATH = os.environ.get("GRT_LIB") or os.path.join(_PKG, "libgrt_hip.so")


class GrtError(RuntimeError):
    """Mirrors the reference's std::runtime_error on any CUDA/OptiX failure (src/Exception.h:19-80)."""


class Params(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("sh_degree_max", C.c_uint32),
        ("eye", C.c_float * 3), ("U", C.c_float * 3), ("V", C.c_float * 3), ("W", C.c_float * 3),
        ("t_min", C.c_float), ("t_max", C.c_float), ("minTransmittance", C.c_float), ("alpha_min", C.c_float),
        ("mode_fisheye", C.c_int32), ("type", C.c_int32), ("max_bounces", C.c_uint32),
    ]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays", "segments", "hit_evals", "rounds", "node_visits", "proxy_tests",
                                          "rec_fetches", "stall_exits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class BvhInfo(C.Structure):
    _fields_ = [("n_particles", C.c_uint64), ("n_proxies", C.c_uint64), ("n_nodes", C.c_uint32),
                ("height", C.c_uint32), ("mesh_faces", C.c_uint32), ("mesh_height", C.c_uint32),
                ("build_ms", C.c_float), ("mesh_update_ms", C.c_float), ("scene_lo", C.c_float * 3), ("scene_hi", C.c_float * 3),
                ("n_primitives", C.c_uint64)]


class DebugTree(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_prims", "n_nodes", "height", "root_ref", "leaf_max", "has_pieces", "n_qnodes",
                                          "n_pbox", "wide", "rec_floats")] + \
               [(n, C.c_void_p) for n in ("nodes", "wnodes", "qnodes", "pbox", "order", "rec")]


class DebugOrder(C.Structure):
    """grt_debug_order (include/grt.h): arguments of grt_debug_order_units."""
    _fields_ = [("op", C.c_uint32), ("n", C.c_uint32)] + \
               [(n, C.c_void_p) for n in ("d_cost", "d_cost_raw", "d_order", "d_zero", "d_scratch", "d_out", "d_count")] + \
               [(n, C.c_uint32) for n in ("extra_cap", "pct2", "pct4", "pct_load", "resident_waves", "multi_min", "bag_classes", "quad_pct4",
                                          "heavy_cap", "thr_x2", "cap", "nbx", "nby")] + \
               [("radius", C.c_int32), ("extra_cap_used", C.c_uint32), ("pct4_used", C.c_uint32)]


class DebugSchedule(C.Structure):
    """grt_debug_schedule (include/grt.h): what grt_debug_copy_schedule copies."""
    _fields_ = [(n, C.c_uint32) for n in ("n_units", "order_launch", "order_valid", "order_classes", "quad_valid", "n_order", "n_quad")] + \
               [(n, C.c_void_p) for n in ("order", "quad", "cost")]


DEBUG_ORDER_PARTS, DEBUG_ORDER_PLAIN, DEBUG_ORDER_QUAD_LIST, DEBUG_ORDER_DILATE = 0, 1, 2, 3


class MemoryInfo(C.Structure):
    _fields_ = [("scene_bytes", C.c_uint64), ("slot_bytes", C.c_uint64), ("overflow_pool_bytes", C.c_uint64),
                ("overflow_chunks", C.c_uint32), ("overflow_demand", C.c_uint32), ("alpha_cull_bytes", C.c_uint64)]


class AuxOut(C.Structure):
    """grt_aux_out (include/grt.h): device pointers of the per-pixel alpha / depth / count arrays, each may be NULL."""
    _fields_ = [("alpha", C.c_void_p), ("depth", C.c_void_p), ("count", C.c_void_p)]


class Gaussians(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pos", "scale", "quat", "opacity", "sh")]


class GaussianGrads(C.Structure):
    """grt_gaussian_grads (include/grt.h): device pointers of the gradient arrays by original particle id, each may be NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("pos", "scale", "quat", "opacity", "sh")]


class BackwardOut(C.Structure):
    """grt_backward_out (include/grt.h): the Gaussians' gradient arrays (or NULL) and the per-ray gradient array (or NULL)."""
    _fields_ = [("gaussians", C.POINTER(GaussianGrads)), ("rays", C.c_void_p)]


class ParticleStats(C.Structure):
    """grt_particle_stats (include/grt.h): device pointers of the per-particle weight_sum / weight_max / count arrays, each may be NULL."""
    _fields_ = [("weight_sum", C.c_void_p), ("weight_max", C.c_void_p), ("count", C.c_void_p)]


class ParticleStatsMesh(C.Structure):
    """grt_particle_stats_mesh (include/grt.h): device pointers of the per-particle weight_sum / weight_max / count / colour_sum /
    colour_max arrays, each may be NULL, and the iterations whose events are counted (1-based, inclusive; 0, 0 = all)."""
    _fields_ = [("weight_sum", C.c_void_p), ("weight_max", C.c_void_p), ("count", C.c_void_p), ("colour_sum", C.c_void_p),
                ("colour_max", C.c_void_p), ("step_first", C.c_uint32), ("step_last", C.c_uint32)]


class PickOut(C.Structure):
    """grt_pick_out (include/grt.h): device pointers of one rule's id / t / weight arrays, each may be NULL."""
    _fields_ = [("id", C.c_void_p), ("t", C.c_void_p), ("weight", C.c_void_p)]


class RayPicks(C.Structure):
    """grt_ray_picks (include/grt.h): the three rules' outputs and the transmittance the cross rule waits for."""
    _fields_ = [("first", PickOut), ("peak", PickOut), ("cross", PickOut), ("cross_T", C.c_float)]


class RayEvents(C.Structure):
    """grt_ray_events (include/grt.h): device pointers of the slot-major id / t / alpha arrays [K][N] and of count / T_in [N], each may
    be NULL; the first listed event and K = max_events."""
    _fields_ = [("id", C.c_void_p), ("t", C.c_void_p), ("alpha", C.c_void_p), ("count", C.c_void_p), ("T_in", C.c_void_p),
                ("first", C.c_uint32), ("max_events", C.c_uint32)]


class PickMeshOut(C.Structure):
    """grt_pick_mesh_out (include/grt.h): device pointers of one rule's id / t / weight / step / point arrays, each may be NULL."""
    _fields_ = [("id", C.c_void_p), ("t", C.c_void_p), ("weight", C.c_void_p), ("step", C.c_void_p), ("point", C.c_void_p)]


class RayPicksMesh(C.Structure):
    """grt_ray_picks_mesh (include/grt.h): the three rules' outputs, the transmittance the cross rule waits for and the iterations
    whose events are candidates (1-based, inclusive; 0, 0 = all)."""
    _fields_ = [("first", PickMeshOut), ("peak", PickMeshOut), ("cross", PickMeshOut), ("cross_T", C.c_float),
                ("step_first", C.c_uint32), ("step_last", C.c_uint32)]


class RayEventsMesh(C.Structure):
    """grt_ray_events_mesh (include/grt.h): device pointers of the slot-major id / t / alpha / step arrays [K][N], of count / T_in [N],
    of the path arrays [P][N] and of n_steps [N], each may be NULL; the first listed event, K = max_events, the step range, P = max_steps."""
    _fields_ = [("id", C.c_void_p), ("t", C.c_void_p), ("alpha", C.c_void_p), ("step", C.c_void_p), ("count", C.c_void_p), ("T_in", C.c_void_p),
                ("first", C.c_uint32), ("max_events", C.c_uint32), ("step_first", C.c_uint32), ("step_last", C.c_uint32),
                ("path_rays", C.c_void_p), ("path_t_far", C.c_void_p), ("path_state", C.c_void_p), ("n_steps", C.c_void_p),
                ("max_steps", C.c_uint32)]


class Segments(C.Structure):
    """grt_segments (include/grt.h): device pointers of the per-ray t_near / t_far / T_in arrays [N], each may be NULL (p->t_min,
    p->t_max, 1 for every ray)."""
    _fields_ = [("t_near", C.c_void_p), ("t_far", C.c_void_p), ("T_in", C.c_void_p)]


class SegmentOut(C.Structure):
    """grt_segment_out (include/grt.h): device pointers of radiance [N][3] and T_out / depth / count [N], each may be NULL, not all."""
    _fields_ = [("radiance", C.c_void_p), ("T_out", C.c_void_p), ("depth", C.c_void_p), ("count", C.c_void_p)]


class DepthOut(C.Structure):
    """grt_depth_out (include/grt.h): device pointers of dist / dist2 / T_out / count [N], each may be NULL, not all."""
    _fields_ = [("dist", C.c_void_p), ("dist2", C.c_void_p), ("T_out", C.c_void_p), ("count", C.c_void_p)]


class DepthUpstream(C.Structure):
    """grt_depth_upstream (include/grt.h): device pointers of dloss/ddist, dloss/ddist2 and dloss/dT_out [N], each may be NULL, not all."""
    _fields_ = [("dist", C.c_void_p), ("dist2", C.c_void_p), ("T_out", C.c_void_p)]


class DepthMeshOut(C.Structure):
    """grt_depth_mesh_out (include/grt.h): device pointers of dist / dist2 / weight / count [N], each may be NULL, not all."""
    _fields_ = [("dist", C.c_void_p), ("dist2", C.c_void_p), ("weight", C.c_void_p), ("count", C.c_void_p)]


class DepthMeshUpstream(C.Structure):
    """grt_depth_mesh_upstream (include/grt.h): device pointers of dloss/ddist, dloss/ddist2 and dloss/dweight [N], each may be NULL, not all."""
    _fields_ = [("g_dist", C.c_void_p), ("g_dist2", C.c_void_p), ("g_weight", C.c_void_p)]


class PointOut(C.Structure):
    """grt_point_out (include/grt.h): device pointers of density / occupancy / peak / peak_id / count [n], each may be NULL, not all."""
    _fields_ = [(n, C.c_void_p) for n in ("density", "occupancy", "peak", "peak_id", "count")]


class PointUpstream(C.Structure):
    """grt_point_upstream (include/grt.h): device pointers of dloss/ddensity and dloss/doccupancy [n], each may be NULL, not both."""
    _fields_ = [("g_density", C.c_void_p), ("g_occupancy", C.c_void_p)]


class PointGrads(C.Structure):
    """grt_point_grads (include/grt.h): device pointers of the gradient arrays pos, scale, quat, opacity (added to) and points [n][3]
    (written); each may be NULL, not all."""
    _fields_ = [(n, C.c_void_p) for n in ("pos", "scale", "quat", "opacity", "points")]


class FeatureGrads(C.Structure):
    """grt_feature_grads (include/grt.h): device pointers of the gradient arrays pos, scale, quat, opacity, feat; each may be NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("pos", "scale", "quat", "opacity", "feat")]


class UpdateInfo(C.Structure):
    """grt_update_info (include/grt.h): what grt_update_gaussians_device did."""
    _fields_ = [("mode_used", C.c_uint32), ("reason", C.c_uint32), ("device_ms", C.c_float), ("area_ratio", C.c_float)]


UPDATE_AUTO, UPDATE_REFIT, UPDATE_REBUILD = 0, 1, 2
UPDATE_MODES = {"auto": UPDATE_AUTO, "refit": UPDATE_REFIT, "rebuild": UPDATE_REBUILD}
REASON_NONE, REASON_FIRST_BUILD, REASON_N_CHANGED, REASON_SET_CHANGED, REASON_OPTION_CHANGED, REASON_AREA = 0, 1, 2, 3, 4, 5

GRAD_SHAPES = {"pos": (3,), "scale": (3,), "quat": (4,), "opacity": (), "sh": (16, 3)}
STATS_OUTPUTS = ("weight_sum", "weight_max", "count")
MESH_STATS_OUTPUTS = STATS_OUTPUTS + ("colour_sum", "colour_max")
MAX_FEATURE_CHANNELS = 16  # GRT_MAX_FEATURE_CHANNELS
PICK_NONE = 0xFFFFFFFF     # GRT_PICK_NONE
PICK_RULES = ("first", "peak", "cross")
PICK_FIELDS = ("id", "t", "weight")
FEATURE_GROUPS = ("pos", "scale", "quat", "opacity", "feat")
EVENT_FIELDS = ("id", "t", "alpha", "count", "T_in")
EVENT_GROUPS = ("pos", "scale", "quat", "opacity")
MESH_PICK_FIELDS = PICK_FIELDS + ("step", "point")
MESH_EVENT_FIELDS = ("id", "t", "alpha", "step", "count", "T_in")
MESH_PATH_FIELDS = ("path_rays", "path_t_far", "path_state", "n_steps")
STEP_LAST, STEP_GAUSSIAN, STEP_TERMINATE = 0, 1, 3  # GRT_STEP_*: the states in path_state (PICK_NONE: an unused path slot)
SEGMENT_OUTPUTS = ("radiance", "T_out", "depth", "count")
DEPTH_OUTPUTS = ("dist", "dist2", "T_out", "count")
DEPTH_KINDS = {"key": 0, "peak": 1}  # GRT_DEPTH_KEY, GRT_DEPTH_PEAK
DEPTH_GROUPS = ("pos", "scale", "quat", "opacity")
DEPTH_MESH_OUTPUTS = ("dist", "dist2", "weight", "count")
DEPTH_SURFACE = 1  # GRT_DEPTH_SURFACE
POINT_OUTPUTS = ("density", "occupancy", "peak", "peak_id", "count")
POINT_GROUPS = ("pos", "scale", "quat", "opacity")


class Mesh(C.Structure):
    _fields_ = [("verts", C.c_void_p), ("normals", C.c_void_p), ("nv", C.c_uint32), ("faces", C.c_void_p),
                ("nf", C.c_uint32)]


MIRROR, NORMAL, GLASS = 0, 1, 2
OPT_COUNTERS, OPT_KERNEL, OPT_LEAF_MAX, OPT_SWIZZLE, OPT_FEEDBACK = 1, 2, 3, 4, 5
OPT_TILE_READY_MIN, OPT_TILE_BAND, OPT_TILE_LOOKAHEAD, OPT_TILE_RESERVE, OPT_TILE_PRIO_DIV, OPT_COST_RADIUS, OPT_SIZE_CLASSES, OPT_COLD_ESTIMATE = 8, 9, 10, 11, 12, 13, 14, 15
OPT_BUNDLE_ROUNDS, OPT_BUNDLE_BUDGET, OPT_SINGLE_LOOKAHEAD, OPT_SINGLE_BAND, OPT_LANE_BUDGET = 16, 17, 18, 19, 20
OPT_OVF_CHUNKS, OPT_OVF_ENTRIES, OPT_MAX_ITERS, OPT_SPLIT, OPT_TILE_BAND_ABS = 21, 22, 23, 24, 25
OPT_TILE_PARTS2_PCT, OPT_TILE_PARTS4_PCT, OPT_TILE_PARTS_LOAD_PCT = 26, 27, 28
OPT_MESH_PARTS = 29
OPT_ORDER_MULTI_MIN = 30
OPT_STATIC_SHARP = 31
OPT_COLD_PARTS_PCT = 32
OPT_QUAD_PARTS = 33
OPT_OVF_CLASSES = 34
OPT_BVH_ROTATIONS = 35
OPT_BUNDLE_PREDICT = 36
OPT_MESH_PRIMARY_WAVE = 37
OPT_SPLIT_VOL_PCT = 38
OPT_BWD_PLAIN_ATOMICS = 39
OPT_REFIT_MAX_AREA_PCT = 40
OPT_ALPHA_CULL = 41  # the leaf cull of uncounted camera-ray frames takes the alpha radius (include/grt.h); 0: the circumradius, as counted frames do
ERR_LIMIT = -5
KERNEL_AUTO, KERNEL_PERLANE, KERNEL_WAVE, KERNEL_STREAM, KERNEL_STREAM_BIG, KERNEL_TILE = 0, 1, 2, 3, 4, 5

EXPORTS = [
    "grt_create", "grt_create_view", "grt_get_memory_info", "grt_destroy", "grt_last_error", "grt_set_option", "grt_upload_gaussians", "grt_build_bvh",
    "grt_update_gaussians_device",
    "grt_set_meshes", "grt_update_meshes", "grt_get_bvh_info", "grt_debug_bvh_depth", "grt_debug_copy_tree", "grt_debug_order_units",
    "grt_debug_order_scratch_bytes", "grt_debug_estimate_costs", "grt_debug_copy_schedule", "grt_render", "grt_render_tiles", "grt_assemble_tiles", "grt_render_rays", "grt_render_aux",
    "grt_render_rays_aux", "grt_backward", "grt_backward_rays", "grt_backward_ex", "grt_backward_rays_ex", "grt_backward_mesh", "grt_backward_rays_mesh",
    "grt_particle_stats_frame", "grt_particle_stats_rays", "grt_particle_stats_mesh_frame", "grt_particle_stats_mesh_rays", "grt_ray_picks_frame", "grt_ray_picks_rays",
    "grt_ray_events_frame", "grt_ray_events_rays", "grt_backward_events_frame", "grt_backward_events_rays",
    "grt_ray_picks_mesh_frame", "grt_ray_picks_mesh_rays", "grt_ray_events_mesh_frame", "grt_ray_events_mesh_rays",
    "grt_backward_events_mesh_frame", "grt_backward_events_mesh_rays",
    "grt_trace_segments_frame", "grt_trace_segments_rays", "grt_backward_segments_frame", "grt_backward_segments_rays",
    "grt_ray_depth_frame", "grt_ray_depth_rays", "grt_backward_depth_frame", "grt_backward_depth_rays",
    "grt_ray_depth_mesh_frame", "grt_ray_depth_mesh_rays", "grt_backward_depth_mesh_frame", "grt_backward_depth_mesh_rays",
    "grt_render_features_frame", "grt_render_features_rays", "grt_backward_features_frame", "grt_backward_features_rays", "grt_render_features_mesh_frame", "grt_render_features_mesh_rays",
    "grt_backward_features_mesh_frame", "grt_backward_features_mesh_rays", "grt_query_points", "grt_backward_points", "grt_sync",
    "grt_get_counters", "grt_last_kernel_ms", "grt_host_activate", "grt_host_uvw_frame", "grt_host_synth_scene",
    "grt_host_ply_count", "grt_host_ply_read", "grt_host_ply_write", "grt_host_last_error",
    "grt_host_primitive_counts", "grt_host_primitive_fill", "grt_host_obj_count", "grt_host_obj_read", "grt_host_obj_write",
]

_lib = None


def lib():
    """Load libgrt_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        # torch ships its own HIP/HSA runtime (torch/lib/libamdhip64.so); it must be the one the process
        # initialises, so import torch BEFORE libgrt_hip.so resolves libamdhip64 (two runtimes opening the
        # KFD in one process => "no ROCm-capable device is detected").  Stand-alone C/C++ users bind to
        # /opt/rocm as usual.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise GrtError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, u32, u64, fl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        L.grt_create.argtypes = [C.POINTER(vp), C.c_int]
        L.grt_create_view.argtypes = [vp, C.POINTER(vp)]
        L.grt_get_memory_info.argtypes = [vp, C.POINTER(MemoryInfo)]
        L.grt_destroy.argtypes = [vp]
        L.grt_last_error.restype = C.c_char_p
        L.grt_last_error.argtypes = [vp]
        L.grt_set_option.argtypes = [vp, C.c_int, C.c_int]
        L.grt_upload_gaussians.argtypes = [vp, C.POINTER(Gaussians), u64]
        L.grt_build_bvh.argtypes = [vp, fl]
        L.grt_update_gaussians_device.argtypes = [vp, C.POINTER(Gaussians), u64, fl, C.c_int, vp, C.POINTER(UpdateInfo)]
        L.grt_set_meshes.argtypes = [vp, C.POINTER(Mesh), u32]
        L.grt_update_meshes.argtypes = [vp, C.POINTER(Mesh), u32]
        L.grt_get_bvh_info.argtypes = [vp, C.POINTER(BvhInfo)]
        L.grt_debug_bvh_depth.argtypes = [vp, C.POINTER(u32)]
        L.grt_debug_copy_tree.argtypes = [vp, C.c_int, C.POINTER(DebugTree)]
        L.grt_debug_order_units.argtypes = [vp, C.POINTER(DebugOrder)]
        L.grt_debug_order_scratch_bytes.argtypes = []
        L.grt_debug_order_scratch_bytes.restype = u32
        L.grt_debug_estimate_costs.argtypes = [vp, C.POINTER(Params), u32, u32, u32, u32, u32, u32, u32, vp, u32]
        L.grt_debug_copy_schedule.argtypes = [vp, C.POINTER(DebugSchedule)]
        L.grt_render.argtypes = [vp, C.POINTER(Params), vp, vp, u32, u32, u32, u32, vp]
        L.grt_render_tiles.argtypes = [vp, C.POINTER(Params), vp, vp, u32, u32, u32, u32, u32, vp]
        L.grt_assemble_tiles.argtypes = [vp, vp, u32, u32, u32, u32, u32, u32, vp, vp]
        L.grt_render_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp]
        L.grt_render_aux.argtypes = [vp, C.POINTER(Params), vp, vp, C.POINTER(AuxOut), u32, u32, u32, u32, vp]
        L.grt_render_rays_aux.argtypes = [vp, C.POINTER(Params), vp, u64, vp, C.POINTER(AuxOut), vp]
        L.grt_backward.argtypes = [vp, C.POINTER(Params), vp, vp, vp, vp, C.POINTER(GaussianGrads), u32, u32, u32, u32, vp]
        L.grt_backward_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, C.POINTER(GaussianGrads), vp]
        L.grt_backward_ex.argtypes = [vp, C.POINTER(Params), vp, vp, vp, vp, C.POINTER(BackwardOut), u32, u32, u32, u32, vp]
        L.grt_backward_rays_ex.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, C.POINTER(BackwardOut), vp]
        L.grt_backward_mesh.argtypes = [vp, C.POINTER(Params), vp, vp, C.POINTER(GaussianGrads), u32, u32, u32, u32, vp]
        L.grt_backward_rays_mesh.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, C.POINTER(GaussianGrads), vp]
        L.grt_particle_stats_frame.argtypes = [vp, C.POINTER(Params), vp, C.POINTER(ParticleStats), u32, u32, u32, u32, vp]
        L.grt_particle_stats_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, C.POINTER(ParticleStats), vp]
        L.grt_particle_stats_mesh_frame.argtypes = [vp, C.POINTER(Params), vp, C.POINTER(ParticleStatsMesh), u32, u32, u32, u32, vp]
        L.grt_particle_stats_mesh_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, C.POINTER(ParticleStatsMesh), vp]
        L.grt_ray_picks_frame.argtypes = [vp, C.POINTER(Params), C.POINTER(RayPicks), u32, u32, u32, u32, vp]
        L.grt_ray_picks_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.POINTER(RayPicks), vp]
        L.grt_ray_events_frame.argtypes = [vp, C.POINTER(Params), C.POINTER(RayEvents), u32, u32, u32, u32, vp]
        L.grt_ray_events_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.POINTER(RayEvents), vp]
        L.grt_backward_events_frame.argtypes = [vp, C.POINTER(Params), vp, u32, u32, C.POINTER(GaussianGrads), u32, u32, u32, u32, vp]
        L.grt_backward_events_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, u32, u32, C.POINTER(GaussianGrads), vp]
        L.grt_ray_picks_mesh_frame.argtypes = [vp, C.POINTER(Params), C.POINTER(RayPicksMesh), u32, u32, u32, u32, vp]
        L.grt_ray_picks_mesh_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.POINTER(RayPicksMesh), vp]
        L.grt_ray_events_mesh_frame.argtypes = [vp, C.POINTER(Params), C.POINTER(RayEventsMesh), u32, u32, u32, u32, vp]
        L.grt_ray_events_mesh_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.POINTER(RayEventsMesh), vp]
        L.grt_backward_events_mesh_frame.argtypes = [vp, C.POINTER(Params), vp, u32, u32, u32, u32, C.POINTER(GaussianGrads), u32, u32, u32, u32, vp]
        L.grt_backward_events_mesh_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, u32, u32, u32, u32, C.POINTER(GaussianGrads), vp]
        L.grt_trace_segments_frame.argtypes = [vp, C.POINTER(Params), C.POINTER(Segments), C.POINTER(SegmentOut), u32, u32, u32, u32, vp]
        L.grt_trace_segments_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.POINTER(Segments), C.POINTER(SegmentOut), vp]
        L.grt_backward_segments_frame.argtypes = [vp, C.POINTER(Params), C.POINTER(Segments), vp, vp, C.POINTER(GaussianGrads), u32, u32, u32, u32, vp]
        L.grt_backward_segments_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.POINTER(Segments), vp, vp, C.POINTER(GaussianGrads), vp]
        L.grt_ray_depth_frame.argtypes = [vp, C.POINTER(Params), C.c_int, C.POINTER(DepthOut), u32, u32, u32, u32, vp]
        L.grt_ray_depth_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.c_int, C.POINTER(DepthOut), vp]
        L.grt_backward_depth_frame.argtypes = [vp, C.POINTER(Params), C.c_int, C.POINTER(DepthUpstream), C.POINTER(BackwardOut), u32, u32, u32, u32, vp]
        L.grt_backward_depth_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.c_int, C.POINTER(DepthUpstream), C.POINTER(BackwardOut), vp]
        L.grt_ray_depth_mesh_frame.argtypes = [vp, C.POINTER(Params), C.c_int, u32, C.POINTER(DepthMeshOut), u32, u32, u32, u32, u32, u32, vp]
        L.grt_ray_depth_mesh_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.c_int, u32, C.POINTER(DepthMeshOut), u32, u32, vp]
        L.grt_backward_depth_mesh_frame.argtypes = [vp, C.POINTER(Params), C.c_int, u32, C.POINTER(DepthMeshUpstream), C.POINTER(FeatureGrads),
                                                    u32, u32, u32, u32, u32, u32, vp]
        L.grt_backward_depth_mesh_rays.argtypes = [vp, C.POINTER(Params), vp, u64, C.c_int, u32, C.POINTER(DepthMeshUpstream),
                                                   C.POINTER(FeatureGrads), u32, u32, vp]
        L.grt_render_features_frame.argtypes = [vp, C.POINTER(Params), vp, u32, vp, u32, u32, u32, u32, vp]
        L.grt_render_features_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, u32, vp, vp]
        L.grt_backward_features_frame.argtypes = [vp, C.POINTER(Params), vp, u32, vp, C.POINTER(FeatureGrads), u32, u32, u32, u32, vp]
        L.grt_backward_features_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, u32, vp, C.POINTER(FeatureGrads), vp]
        L.grt_render_features_mesh_frame.argtypes = [vp, C.POINTER(Params), vp, u32, vp, u32, u32, u32, u32, u32, u32, vp]
        L.grt_render_features_mesh_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, u32, vp, u32, u32, vp]
        L.grt_backward_features_mesh_frame.argtypes = [vp, C.POINTER(Params), vp, u32, vp, C.POINTER(FeatureGrads), u32, u32, u32, u32, u32, u32, vp]
        L.grt_backward_features_mesh_rays.argtypes = [vp, C.POINTER(Params), vp, u64, vp, u32, vp, C.POINTER(FeatureGrads), u32, u32, vp]
        L.grt_query_points.argtypes = [vp, vp, u64, fl, C.POINTER(PointOut), vp]
        L.grt_backward_points.argtypes = [vp, vp, u64, fl, C.POINTER(PointUpstream), C.POINTER(PointGrads), vp]
        L.grt_sync.argtypes = [vp]
        L.grt_sync.restype = C.c_int
        L.grt_get_counters.argtypes = [vp, C.POINTER(Counters)]
        L.grt_last_kernel_ms.argtypes = [vp, C.POINTER(fl)]
        L.grt_host_activate.argtypes = [u64] + [vp] * 11
        L.grt_host_uvw_frame.argtypes = [vp, vp, vp, fl, fl, vp, vp, vp]
        L.grt_host_uvw_frame.restype = None
        L.grt_host_synth_scene.argtypes = [u64, u64] + [vp] * 6
        L.grt_host_ply_count.argtypes = [C.c_char_p, C.POINTER(u64)]
        L.grt_host_ply_read.argtypes = [C.c_char_p, u64] + [vp] * 6
        L.grt_host_ply_write.argtypes = [C.c_char_p, u64] + [vp] * 6
        L.grt_host_last_error.restype = C.c_char_p
        L.grt_host_primitive_counts.argtypes = [C.c_int, C.POINTER(u32), C.POINTER(u32)]
        L.grt_host_primitive_fill.argtypes = [C.c_int, vp, vp, vp]
        L.grt_host_obj_count.argtypes = [C.c_char_p, C.POINTER(u32), C.POINTER(u32)]
        L.grt_host_obj_read.argtypes = [C.c_char_p, u32, vp, vp, vp]
        L.grt_host_obj_write.argtypes = [C.c_char_p, u32, vp, vp, u32, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_check(rc):
    if rc != 0:
        raise GrtError(f"grt host error {rc}: {lib().grt_host_last_error().decode()}")


# ---------------------------------------------------------------------------------------------
# host helpers (no GPU needed)
# ---------------------------------------------------------------------------------------------
def raw_columns(n):
    return dict(pos=np.zeros((n, 3), np.float32), f_dc=np.zeros((n, 3), np.float32),
                f_rest=np.zeros((n, 45), np.float32), opacity=np.zeros(n, np.float32),
                scale=np.zeros((n, 3), np.float32), rot=np.zeros((n, 4), np.float32))


def synth_scene(seed, n):
    """Deterministic synthetic 3DGS scene (raw PLY columns), SURVEY.md §8(d)."""
    r = raw_columns(n)
    _host_check(lib().grt_host_synth_scene(seed, n, _p(r["pos"]), _p(r["f_dc"]), _p(r["f_rest"]), _p(r["opacity"]),
                                           _p(r["scale"]), _p(r["rot"])))
    return r


def activate(raw):
    """Raw PLY columns -> activated attributes (src/GaussianData.cpp:97-131)."""
    n = len(raw["pos"])
    raw = {k: np.ascontiguousarray(v, np.float32) for k, v in raw.items()}
    out = dict(pos=np.zeros((n, 3), np.float32), scale=np.zeros((n, 3), np.float32), quat=np.zeros((n, 4), np.float32),
               opacity=np.zeros(n, np.float32), sh=np.zeros((n, 16, 3), np.float32))
    _host_check(lib().grt_host_activate(n, _p(raw["pos"]), _p(raw["f_dc"]), _p(raw["f_rest"]), _p(raw["opacity"]),
                                        _p(raw["scale"]), _p(raw["rot"]), _p(out["pos"]), _p(out["scale"]),
                                        _p(out["quat"]), _p(out["opacity"]), _p(out["sh"])))
    return out


def read_ply(path):
    n = C.c_uint64()
    _host_check(lib().grt_host_ply_count(path.encode(), C.byref(n)))
    r = raw_columns(n.value)
    _host_check(lib().grt_host_ply_read(path.encode(), n.value, _p(r["pos"]), _p(r["f_dc"]), _p(r["f_rest"]),
                                        _p(r["opacity"]), _p(r["scale"]), _p(r["rot"])))
    return r


def write_ply(path, raw):
    raw = {k: np.ascontiguousarray(v, np.float32) for k, v in raw.items()}
    _host_check(lib().grt_host_ply_write(path.encode(), len(raw["pos"]), _p(raw["pos"]), _p(raw["f_dc"]),
                                         _p(raw["f_rest"]), _p(raw["opacity"]), _p(raw["scale"]), _p(raw["rot"])))


def uvw_frame(eye, lookat, up, fovy_deg, aspect):
    e, l, u = (np.ascontiguousarray(x, np.float32) for x in (eye, lookat, up))
    U, V, W = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    lib().grt_host_uvw_frame(_p(e), _p(l), _p(u), fovy_deg, aspect, _p(U), _p(V), _p(W))
    return U, V, W


def default_params(width, height, acts_pos_mean, sh_degree=0, fisheye=False, mesh_type=MIRROR, max_bounces=32,
                   eye=(0.0, 0.0, 3.0), fovy=60.0):
    """Reference defaults: eye (0,0,3), lookat = mean Gaussian position, up (0,1,0), fovY 60
    (src/gui.cpp:52-55); t_min 1e-3, t_max 1e5, minTransmittance 1e-3, alpha_min 0.01
    (src/GaussianTracer.cpp:479-482)."""
    U, V, W = uvw_frame(eye, acts_pos_mean, (0.0, 1.0, 0.0), fovy, float(np.float32(width) / np.float32(height)))
    p = Params()
    p.width, p.height, p.sh_degree_max = width, height, sh_degree
    for name, v in (("eye", eye), ("U", U), ("V", V), ("W", W)):
        arr = getattr(p, name)
        for k in range(3):
            arr[k] = float(v[k])
    p.t_min, p.t_max, p.minTransmittance, p.alpha_min = 1e-3, 1e5, 1e-3, 0.01
    p.mode_fisheye, p.type, p.max_bounces = int(fisheye), mesh_type, max_bounces
    return p


def gaussian_center(pos):
    """GaussianData::getCenter (src/GaussianData.cpp:139-151): sequential fp32 sum / n."""
    c = np.zeros(3, np.float32)
    for k in range(3):
        c[k] = np.cumsum(pos[:, k], dtype=np.float32)[-1] / np.float32(len(pos))
    return c


PRIM_PLANE, PRIM_SPHERE = 0, 1


def primitive_mesh(kind, center=(0.0, 0.0, 0.0)):
    """The reference's procedural plane / sphere (src/geometry/Primitives.cpp:6-140) placed by translate(center),
    from the C ABI (the same arrays the C++ facade's createPlane/createSphere hold): (verts, normals, faces)."""
    nv, nf = C.c_uint32(), C.c_uint32()
    _host_check(lib().grt_host_primitive_counts(kind, C.byref(nv), C.byref(nf)))
    v = np.zeros((nv.value, 3), np.float32); n = np.zeros((nv.value, 3), np.float32); f = np.zeros((nf.value, 3), np.uint32)
    _host_check(lib().grt_host_primitive_fill(kind, _p(v), _p(n), _p(f)))
    c = np.asarray(center, np.float32)
    return (v if not c.any() else (v + c[None]).astype(np.float32)), n, f  # (-0.0 + 0.0 would lose the sign bit)


def load_obj(path, center=(0.0, 0.0, 0.0)):
    """Primitives::createLoadMesh (src/geometry/Primitives.cpp:142-202): un-indexed soup, Y flipped, translate(center)."""
    nv, nf = C.c_uint32(), C.c_uint32()
    _host_check(lib().grt_host_obj_count(path.encode(), C.byref(nv), C.byref(nf)))
    v = np.zeros((nv.value, 3), np.float32); n = np.zeros((nv.value, 3), np.float32); f = np.zeros(nv.value, np.uint32)
    _host_check(lib().grt_host_obj_read(path.encode(), nv.value, _p(v), _p(n), _p(f)))
    return (v + np.asarray(center, np.float32)[None]).astype(np.float32), n, f.reshape(-1, 3)


def write_obj(path, verts, normals, faces):
    v = np.ascontiguousarray(verts, np.float32); n = np.ascontiguousarray(normals, np.float32)
    f = np.ascontiguousarray(faces, np.uint32)
    _host_check(lib().grt_host_obj_write(path.encode(), len(v), _p(v), _p(n), len(f), _p(f)))


def sphere_mesh(center, radius=0.3, tess_u=180, tess_v=90):
    """UV sphere with the reference's construction (src/geometry/Primitives.cpp:63-140) at any tessellation, placed by
    translate(center) — numpy formulation for the small test meshes; primitive_mesh(PRIM_SPHERE) is the reference's
    180 x 90 sphere itself."""
    f32 = np.float32
    phi_step = f32(2.0) * f32(np.pi) / f32(tess_u)
    theta_step = f32(np.pi) / f32(tess_v - 1)
    lat = np.arange(tess_v, dtype=np.float32) * theta_step
    lon = np.arange(tess_u + 1, dtype=np.float32) * phi_step
    st, ct = np.sin(lat).astype(f32), np.cos(lat).astype(f32)
    sp, cp = np.sin(lon).astype(f32), np.cos(lon).astype(f32)
    n = np.stack([np.outer(st, cp), np.repeat(ct[:, None], tess_u + 1, 1), np.outer(st, sp)], -1).astype(f32)
    normals = n.reshape(-1, 3)
    verts = (normals * f32(radius)).astype(f32) + np.asarray(center, f32)[None]
    cols = tess_u + 1
    la, lo = np.meshgrid(np.arange(tess_v - 1), np.arange(tess_u), indexing="ij")
    ll, lr = la * cols + lo, la * cols + lo + 1
    ur, ul = (la + 1) * cols + lo + 1, (la + 1) * cols + lo
    faces = np.stack([np.stack([ll, lr, ur], -1), np.stack([ur, ul, ll], -1)], 2).reshape(-1, 3).astype(np.uint32)
    return verts.astype(f32), normals.copy(), faces


def plane_mesh(center, width=0.3, height=0.5):
    """Primitives::createPlane (src/geometry/Primitives.cpp:6-61)."""
    f32 = np.float32
    c = np.asarray(center, f32)
    v = np.array([[-width / 2, -height / 2, 0], [width / 2, -height / 2, 0], [-width / 2, height / 2, 0],
                  [width / 2, height / 2, 0]], f32) + c[None]
    n = np.tile(np.array([[0, 0, 1]], f32), (4, 1))
    f = np.array([[0, 1, 3], [3, 2, 0]], np.uint32)
    return v.astype(f32), n, f


# ---------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------
class Tracer:
    """One context per GPU (mirrors class GaussianTracer, src/GaussianTracer.h:27-111)."""

    def __init__(self, device=0, scene=None):
        """scene = another Tracer: this one is a VIEW of it (grt_create_view) — a frame slot of its own on that
        Tracer's Gaussians / BVHs / meshes."""
        import torch
        if not torch.cuda.is_available():
            raise GrtError("no GPU visible: libgrt_hip has no CPU fallback")
        self._torch = torch
        self.device = device if scene is None else scene.device
        self._h = C.c_void_p()
        self._scene = scene  # keeps the parent alive as long as the view
        self.n_particles = 0  # of the last upload
        self.n_uploads = 0    # uploads so far (grt_torch: a backward refuses a scene that is no longer its forward's)
        self._has_meshes = False  # set_meshes has set at least one face (a view reads its scene's: has_meshes)
        rc = lib().grt_create(C.byref(self._h), device) if scene is None else lib().grt_create_view(scene._h, C.byref(self._h))
        if rc != 0:
            raise GrtError(f"grt_create failed ({rc}): {lib().grt_last_error(None).decode()}")

    def view(self):
        return Tracer(scene=self)

    @property
    def has_meshes(self):
        """Whether meshes are set on the scene this tracer renders (a view: its scene's)."""
        return self._scene.has_meshes if self._scene is not None else self._has_meshes

    def _check(self, rc):
        if rc != 0:
            e = GrtError(f"grt error {rc}: {lib().grt_last_error(self._h).decode()}")
            e.code = rc
            raise e

    def memory_info(self):
        o = MemoryInfo()
        self._check(lib().grt_get_memory_info(self._h, C.byref(o)))
        return {n: int(getattr(o, n)) for n, _ in o._fields_}

    def check(self):
        """grt_sync: waits for the last frame and raises (code ERR_LIMIT) when a wave gave up on live rays."""
        self._check(lib().grt_sync(self._h))

    def set_option(self, opt, val):
        self._check(lib().grt_set_option(self._h, opt, val))

    def upload(self, acts, alpha_min=0.01):
        a = {k: np.ascontiguousarray(v, np.float32) for k, v in acts.items()}
        self.n_particles = len(a["pos"])
        self.n_uploads += 1
        g = Gaussians(*(a[k].ctypes.data for k in ("pos", "scale", "quat", "opacity", "sh")))
        self._check(lib().grt_upload_gaussians(self._h, C.byref(g), len(a["pos"])))
        self._check(lib().grt_build_bvh(self._h, alpha_min))

    def update_device(self, acts, alpha_min=0.01, mode="auto"):
        """grt_update_gaussians_device: the scene from a dict of CUDA tensors (pos [n][3], scale [n][3], quat [n][4], opacity [n],
        sh [n][16][3]; made float32 and contiguous on the tracer's GPU when they are not), never through the host.  mode "auto" refits
        the BVH in hand when that is possible and rebuilds it otherwise, "refit" raises when it is not, "rebuild" is upload() from
        device memory.  Returns {'mode_used', 'reason', 'device_ms', 'area_ratio'} (include/grt.h: grt_update_info)."""
        t = self._torch
        dev = t.device("cuda", self.device)
        a = {k: t.as_tensor(acts[k]).detach().to(dev, t.float32).contiguous() for k in ("pos", "scale", "quat", "opacity", "sh")}
        n = int(a["pos"].shape[0])
        shapes = {"pos": (n, 3), "scale": (n, 3), "quat": (n, 4), "opacity": (n,), "sh": (n, 16, 3)}
        for k, v in a.items():
            if tuple(v.shape) != shapes[k]:
                raise GrtError(f"update_device: '{k}' has shape {tuple(v.shape)}, expected {shapes[k]}")
        return self.update_device_ptrs(Gaussians(*(a[k].data_ptr() if n else None for k in ("pos", "scale", "quat", "opacity", "sh"))),
                                       n, alpha_min, mode)

    def update_device_ptrs(self, g, n, alpha_min=0.01, mode="auto"):
        """(testing) update_device from a Gaussians struct of raw pointers, as the C ABI takes them."""
        info = UpdateInfo()
        rc = lib().grt_update_gaussians_device(self._h, C.byref(g), n, alpha_min, UPDATE_MODES.get(mode, mode), self._stream(), C.byref(info))
        if rc == 0:  # (a refused update leaves the scene, and these, as they were)
            self.n_particles = n
            self.n_uploads += 1
        self._check(rc)
        return {n_: (int(getattr(info, n_)) if n_ in ("mode_used", "reason") else float(getattr(info, n_))) for n_, _ in info._fields_}

    def set_meshes(self, meshes):
        keep, arr = [], (Mesh * max(len(meshes), 1))()
        for i, (v, n, f) in enumerate(meshes):
            v = np.ascontiguousarray(v, np.float32); n = np.ascontiguousarray(n, np.float32)
            f = np.ascontiguousarray(f, np.uint32)
            keep += [v, n, f]
            arr[i] = Mesh(v.ctypes.data, n.ctypes.data, len(v), f.ctypes.data, len(f))
        self._has_meshes = False  # (a refused call leaves the context without meshes)
        self._check(lib().grt_set_meshes(self._h, arr, len(meshes)))
        self._has_meshes = any(len(f) for f in keep[2::3])

    def update_meshes(self, meshes):
        """Same topology, new positions / normals: the mesh LBVH is re-fitted, not rebuilt."""
        keep, arr = [], (Mesh * max(len(meshes), 1))()
        for i, (v, n, f) in enumerate(meshes):
            v = np.ascontiguousarray(v, np.float32); n = np.ascontiguousarray(n, np.float32)
            f = np.ascontiguousarray(f, np.uint32)
            keep += [v, n, f]
            arr[i] = Mesh(v.ctypes.data, n.ctypes.data, len(v), f.ctypes.data, len(f))
        self._check(lib().grt_update_meshes(self._h, arr, len(meshes)))

    def bvh_info(self):
        o = BvhInfo()
        self._check(lib().grt_get_bvh_info(self._h, C.byref(o)))
        return {n: (list(getattr(o, n)) if n.startswith("scene") else getattr(o, n)) for n, _ in o._fields_}

    def bvh_depth_walked(self):
        """(testing) depth of the Gaussian LBVH walked on the host; must be <= bvh_info()['height']."""
        d = C.c_uint32(0)
        self._check(lib().grt_debug_bvh_depth(self._h, C.byref(d)))
        return int(d.value)

    def debug_tree(self, which=0):
        """(testing) copy of the built Gaussian (which = 0) or mesh (1) tree as numpy arrays: nodes [n][16] float32, wnodes [n][32],
        qnodes [n][wide][8], pbox [m][8], order [m] uint32, rec [m][16] (Gaussian) / [m][12] (mesh) and the counts as ints.  Child refs and ids are the
        raw bits of floats: .view(np.uint32) reads them."""
        t = DebugTree()
        self._check(lib().grt_debug_copy_tree(self._h, which, C.byref(t)))
        w = t.wide
        out = {n: int(getattr(t, n)) for n in ("n_prims", "n_nodes", "height", "root_ref", "leaf_max", "has_pieces", "wide")}
        arr = {"nodes": np.zeros((t.n_nodes, 16), np.float32), "wnodes": np.zeros((t.n_nodes, 32), np.float32),
               "qnodes": np.zeros((t.n_qnodes, w, 8), np.float32), "pbox": np.zeros((t.n_pbox, 8), np.float32),
               "order": np.zeros(t.n_prims, np.uint32), "rec": np.zeros((t.n_prims, t.rec_floats), np.float32)}
        for n, a in arr.items():
            setattr(t, n, a.ctypes.data if a.size else None)
        self._check(lib().grt_debug_copy_tree(self._h, which, C.byref(t)))
        out.update(arr)
        return out

    def debug_order(self, op, **kw):
        """(testing) grt_debug_order_units: a launch-order kernel family on the caller's uint32 CUDA tensors (keywords = the fields of
        grt_debug_order, tensors for the pointers).  The work runs on the context's own stream: the device is synchronised in front of
        the call and behind it.  Returns the struct (extra_cap_used, pct4_used)."""
        o = DebugOrder()
        o.op = op
        for k, v in kw.items():
            setattr(o, k, (v.data_ptr() if v is not None else None) if k.startswith("d_") else v)
        self.sync()
        rc = lib().grt_debug_order_units(self._h, C.byref(o))
        self.sync()
        self._check(rc)
        return o

    def debug_estimate_costs(self, params, d_cost, stride=1, window=None, tiles=None):
        """(testing) grt_debug_estimate_costs into the zeroed uint32 CUDA tensor d_cost: window = (x0, y0, x1, y1) (default: the frame)
        or tiles = (tile_w, tile_h, first, stride, count)."""
        g = (tiles[0], tiles[1], tiles[2], tiles[3], tiles[4], 0) if tiles else (0, 0) + tuple(window or (0, 0, params.width, params.height))
        self.sync()
        rc = lib().grt_debug_estimate_costs(self._h, C.byref(params), *g, stride, d_cost.data_ptr() if d_cost is not None else None,
                                            d_cost.numel() if d_cost is not None else 0)
        self.sync()
        self._check(rc)

    def debug_schedule(self):
        """(testing) grt_debug_copy_schedule: the slot's scheduling state as a dict — the counts and flags as ints, 'order' (order_launch
        entries + 3 diagnostic words, or n_units bare entries; empty when no order is held), 'quad' (the quad list), 'cost' (d_cost)
        as uint32 numpy arrays."""
        t = DebugSchedule()
        self._check(lib().grt_debug_copy_schedule(self._h, C.byref(t)))
        arr = {"order": np.zeros(t.n_order, np.uint32), "quad": np.zeros(t.n_quad, np.uint32), "cost": np.zeros(t.n_units, np.uint32)}
        for n, a in arr.items():
            setattr(t, n, a.ctypes.data if a.size else None)
        self._check(lib().grt_debug_copy_schedule(self._h, C.byref(t)))
        out = {n: int(getattr(t, n)) for n in ("n_units", "order_launch", "order_valid", "order_classes", "quad_valid", "n_order", "n_quad")}
        out.update(arr)
        return out

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def render(self, params, window=None, want_u8=True, want_f32=False, out_u8=None, out_f32=None):
        t = self._torch
        w, h = params.width, params.height
        dev = f"cuda:{self.device}"
        if want_u8 and out_u8 is None:
            out_u8 = t.zeros((h, w, 3), dtype=t.uint8, device=dev)
        if want_f32 and out_f32 is None:
            out_f32 = t.zeros((h, w, 3), dtype=t.float32, device=dev)
        x0, y0, x1, y1 = window if window else (0, 0, w, h)
        self._check(lib().grt_render(self._h, C.byref(params), out_u8.data_ptr() if out_u8 is not None else None,
                                     out_f32.data_ptr() if out_f32 is not None else None, x0, y0, x1, y1,
                                     self._stream()))
        return out_u8, out_f32

    def render_tiles(self, params, tile_w, tile_h, first, stride, count, out_u8=None, out_f32=None):
        self._check(lib().grt_render_tiles(self._h, C.byref(params), out_u8.data_ptr() if out_u8 is not None else None,
                                           out_f32.data_ptr() if out_f32 is not None else None, tile_w, tile_h, first,
                                           stride, count, self._stream()))

    def assemble_tiles(self, gathered, world, max_cnt, tile, width, height, out_u8):
        """gathered: ONE uint8 tensor [world][max_cnt][tile][tile][3] (the ranks' compact buffers) -> out_u8 [height][width][3]."""
        self._check(lib().grt_assemble_tiles(self._h, gathered.data_ptr(), world, max_cnt, tile, tile, width, height,
                                             out_u8.data_ptr(), self._stream()))

    def render_rays(self, params, rays, out=None):
        t = self._torch
        if out is None:
            out = t.zeros((rays.shape[0], 3), dtype=t.float32, device=rays.device)
        self._check(lib().grt_render_rays(self._h, C.byref(params), rays.data_ptr(), rays.shape[0], out.data_ptr(),
                                          self._stream()))
        return out

    def _aux_buffers(self, shape, dev, alpha, depth, count):
        t = self._torch
        out = {}
        if alpha:
            out["alpha"] = t.zeros(shape, dtype=t.float32, device=dev)
        if depth:
            out["depth"] = t.zeros(shape, dtype=t.float32, device=dev)
        if count:
            out["count"] = t.zeros(shape, dtype=t.uint32, device=dev)
        ptrs = AuxOut(*(out[k].data_ptr() if k in out else None for k in ("alpha", "depth", "count")))
        return out, ptrs

    def render_aux(self, params, window=None, want_u8=True, want_f32=False, alpha=True, depth=True, count=True):
        """A frame with per-pixel opacity, expected depth and hit count beside colour (grt_render_aux; definitions in include/grt.h).
        Returns a dict of torch tensors: 'u8' [h][w][3] / 'f32' [h][w][3] (when wanted), 'alpha' / 'depth' float32 [h][w], 'count'
        uint32 [h][w] (when asked for).  Pixels outside the window stay 0.  depth / alpha is the mean distance of the first segment."""
        t = self._torch
        w, h = params.width, params.height
        dev = f"cuda:{self.device}"
        out, ptrs = self._aux_buffers((h, w), dev, alpha, depth, count)
        if want_u8:
            out["u8"] = t.zeros((h, w, 3), dtype=t.uint8, device=dev)
        if want_f32:
            out["f32"] = t.zeros((h, w, 3), dtype=t.float32, device=dev)
        x0, y0, x1, y1 = window if window else (0, 0, w, h)
        self._check(lib().grt_render_aux(self._h, C.byref(params), out["u8"].data_ptr() if want_u8 else None,
                                         out["f32"].data_ptr() if want_f32 else None, C.byref(ptrs), x0, y0, x1, y1,
                                         self._stream()))
        return out

    def render_rays_aux(self, params, rays, want_f32=True, alpha=True, depth=True, count=True):
        """grt_render_rays_aux: rays [n][6] (device, float32 o, d) -> dict of 'f32' [n][3] and 'alpha' / 'depth' / 'count' [n]
        (depth in units of |d|)."""
        t = self._torch
        n = rays.shape[0]
        out, ptrs = self._aux_buffers((n,), rays.device, alpha, depth, count)
        if want_f32:
            out["f32"] = t.zeros((n, 3), dtype=t.float32, device=rays.device)
        self._check(lib().grt_render_rays_aux(self._h, C.byref(params), rays.data_ptr(), n,
                                              out["f32"].data_ptr() if want_f32 else None, C.byref(ptrs), self._stream()))
        return out

    def _grad_buffers(self, into, groups, dev):
        """The gradient tensors of a backward call: `into` (accumulated into; its keys are the groups computed) or zeroed ones for
        `groups` (default: all five)."""
        t = self._torch
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        if into is None:
            into = {k: t.zeros((n,) + GRAD_SHAPES[k], dtype=t.float32, device=dev) for k in (groups or GRAD_SHAPES)}
        for k, v in into.items():
            if k not in GRAD_SHAPES or tuple(v.shape) != (n,) + GRAD_SHAPES[k] or v.dtype != t.float32 or not v.is_contiguous():
                raise GrtError(f"backward: gradient tensor '{k}' must be contiguous float32 of shape {(n,) + GRAD_SHAPES[k]}")
        return into, GaussianGrads(*(into[k].data_ptr() if k in into else None for k in ("pos", "scale", "quat", "opacity", "sh")))

    def backward(self, params, rgbf, alpha, grad_rgbf, grad_alpha=None, window=None, into=None, groups=None, ray_grads=False):
        """grt_backward: gradients of a loss on the frame (rgbf [h][w][3], alpha [h][w] as render_aux wrote them; grad_rgbf / grad_alpha
        the loss's gradients with respect to them) with respect to the uploaded Gaussians -> dict of torch tensors pos, scale, quat,
        opacity, sh (allocated zeroed, or accumulated into `into`).  Not bitwise reproducible (float atomics); include/grt.h.
        ray_grads: grt_backward_ex — the dict also holds "rays" [h][w][6] float32 (dloss/d eye, dloss/d unit direction per pixel; zero
        outside the window), which IS bitwise reproducible; groups=[] with ray_grads is the rays-only call (no atomics, no buffer)."""
        dev = f"cuda:{self.device}"
        x0, y0, x1, y1 = window if window else (0, 0, params.width, params.height)
        keep = [x.contiguous() if x is not None else None for x in (rgbf, alpha, grad_rgbf, grad_alpha)]
        if ray_grads:
            into, out, hold = self._ex_buffers(into, groups, dev, (params.height, params.width, 6))
            self._check(lib().grt_backward_ex(self._h, C.byref(params), *(x.data_ptr() if x is not None else None for x in keep), C.byref(out),
                                              x0, y0, x1, y1, self._stream()))
            return into
        into, ptrs = self._grad_buffers(into, groups, dev)
        self._check(lib().grt_backward(self._h, C.byref(params), *(x.data_ptr() if x is not None else None for x in keep), C.byref(ptrs),
                                       x0, y0, x1, y1, self._stream()))
        return into

    def backward_rays(self, params, rays, rgbf, alpha, grad_rgbf, grad_alpha=None, into=None, groups=None, ray_grads=False):
        """grt_backward_rays: as backward() for rays [n][6] (device, float32 o, d); rgbf [n][3], alpha [n] as render_rays_aux wrote them.
        ray_grads: grt_backward_rays_ex — "rays" [n][6] (dloss/do, dloss/dd) beside the groups."""
        keep = [x.contiguous() if x is not None else None for x in (rgbf, alpha, grad_rgbf, grad_alpha)]
        if ray_grads:
            into, out, hold = self._ex_buffers(into, groups, rays.device, (rays.shape[0], 6))
            self._check(lib().grt_backward_rays_ex(self._h, C.byref(params), rays.data_ptr(), rays.shape[0],
                                                   *(x.data_ptr() if x is not None else None for x in keep), C.byref(out), self._stream()))
            return into
        into, ptrs = self._grad_buffers(into, groups, rays.device)
        self._check(lib().grt_backward_rays(self._h, C.byref(params), rays.data_ptr(), rays.shape[0],
                                            *(x.data_ptr() if x is not None else None for x in keep), C.byref(ptrs), self._stream()))
        return into

    def backward_mesh(self, params, grad_rgbf, grad_alpha=None, window=None, into=None, groups=None):
        """grt_backward_mesh: backward() for a frame with meshes set (mirror, glass, normal; the meshes held fixed) — gradients of a
        loss on the frame render_aux renders, with respect to the uploaded Gaussians.  No forward outputs are passed.  Without meshes
        it differentiates the Gaussian-only frame, as backward() does."""
        dev = f"cuda:{self.device}"
        x0, y0, x1, y1 = window if window else (0, 0, params.width, params.height)
        keep = [x.contiguous() if x is not None else None for x in (grad_rgbf, grad_alpha)]
        into, ptrs = self._grad_buffers(into, groups, dev)
        self._check(lib().grt_backward_mesh(self._h, C.byref(params), *(x.data_ptr() if x is not None else None for x in keep), C.byref(ptrs),
                                            x0, y0, x1, y1, self._stream()))
        return into

    def backward_rays_mesh(self, params, rays, grad_rgbf, grad_alpha=None, into=None, groups=None):
        """grt_backward_rays_mesh: backward_mesh() for rays [n][6] (device, float32 o, d), as render_rays_aux renders them."""
        keep = [x.contiguous() if x is not None else None for x in (grad_rgbf, grad_alpha)]
        into, ptrs = self._grad_buffers(into, groups, rays.device)
        self._check(lib().grt_backward_rays_mesh(self._h, C.byref(params), rays.data_ptr(), rays.shape[0],
                                                 *(x.data_ptr() if x is not None else None for x in keep), C.byref(ptrs), self._stream()))
        return into

    def particle_stats(self, params, rays=None, ray_weight=None, window=None, into=None, outputs=STATS_OUTPUTS):
        """grt_particle_stats_frame / grt_particle_stats_rays (rays [n][6] given): which particles the rays of the frame (or of its
        window, or of the buffer) composited, and how strongly -> dict of torch tensors [n_particles] by original id on the tracer's
        GPU: 'weight_sum' float32 (sum of ray_weight * T_i * alpha_i over the composited events), 'weight_max' float32 (peak
        T_i * alpha_i, not scaled by the ray's weight), 'count' uint32 as render_aux's (number of composited events); include/grt.h.
        ray_weight: [h][w] or [n] float32 (None = 1); a ray of weight exactly 0 is not traced and enters none of the three.
        The tensors are allocated zeroed for `outputs`, or the call ACCUMULATES (add, max, add) into the tensors of `into` (its keys
        are the outputs computed; 'count' may be uint32 or int32): several views sum up into one dict.  count and weight_max are
        bitwise reproducible, weight_sum is not (float atomics)."""
        return self._particle_stats("particle_stats", STATS_OUTPUTS, None, params, rays, ray_weight, window, into, outputs)

    def particle_stats_mesh(self, params, rays=None, ray_weight=None, window=None, into=None, outputs=MESH_STATS_OUTPUTS, steps=None):
        """grt_particle_stats_mesh_frame / grt_particle_stats_mesh_rays: particle_stats() of a frame whose rays bounce off the meshes
        set on the tracer (include/grt.h) — the particles met behind a mirror or through glass are counted with the ones the camera
        rays meet.  Beside 'weight_sum', 'weight_max' and 'count' (on w_i = T_i * alpha_i, ONE transmittance running through all of
        a ray's segments) the dict holds 'colour_sum' and 'colour_max' on the colour weight c_s * w_i with which the particle's
        radiance enters the pixel.  steps = (first, last): only the events of these iterations of the bounce loop are counted
        (1-based, inclusive; last None = open; None = all): (1, 1) is what the camera rays meet directly, (2, None) what is met only
        through a bounce.  Everything else is particle_stats(): ray_weight, window, `into` accumulating (add, max, add, add, max),
        `outputs` choosing what is computed (without a colour output a ray is walked once, else twice).  On a tracer without meshes
        count, weight_max and weight_sum are particle_stats()'s."""
        if steps is None:
            first, last = 0, 0
        else:
            first, last = steps
            first, last = int(first), 0 if last is None else int(last)
            if first < 0 or last < 0 or (steps[1] is not None and last == 0):
                raise GrtError(f"particle_stats_mesh: steps must be (first, last) with 1 <= first <= last, or last None, not {tuple(steps)}")
        return self._particle_stats("particle_stats_mesh", MESH_STATS_OUTPUTS, (first, last), params, rays, ray_weight, window, into, outputs)

    def _particle_stats(self, who, names, steps, params, rays, ray_weight, window, into, outputs):
        """The checks, the allocation and the call of particle_stats (steps None) and particle_stats_mesh."""
        t = self._torch
        dev = t.device("cuda", self.device)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        if into is None:
            bad = [k for k in outputs if k not in names]
            if bad or not len(outputs):
                raise GrtError(f"{who}: outputs must be a non-empty subset of {names}, not {tuple(outputs)}")
            into = {k: t.zeros((n,), dtype=t.uint32 if k == "count" else t.float32, device=dev) for k in outputs}
        for k, v in into.items():
            ok_dt = (t.uint32, t.int32) if k == "count" else (t.float32,)
            if k not in names or tuple(v.shape) != (n,) or v.dtype not in ok_dt or not v.is_contiguous() or v.device != dev:
                raise GrtError(f"{who}: tensor '{k}' must be contiguous {'uint32 / int32' if k == 'count' else 'float32'} of shape "
                               f"({n},) on {dev}")
        fields = [into[k].data_ptr() if k in into and n else None for k in names]
        ptrs = ParticleStats(*fields) if steps is None else ParticleStatsMesh(*fields, *steps)
        if not n:  # (an empty scene: nothing to write, and no pointer to hand over)
            return into
        if rays is not None:
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise GrtError(f"{who}: rays must have shape [n][6], not {tuple(rays.shape)}")
            rays = rays.detach().to(dev, t.float32).contiguous()
            shape = (rays.shape[0],)
        else:
            shape = (params.height, params.width)
        if ray_weight is not None:
            ray_weight = t.as_tensor(ray_weight).detach().to(dev, t.float32).contiguous()
            if tuple(ray_weight.shape) != shape:
                raise GrtError(f"{who}: ray_weight must have shape {shape}, not {tuple(ray_weight.shape)}")
        wp = ray_weight.data_ptr() if ray_weight is not None else None
        L = lib()
        if rays is not None:
            if window is not None:
                raise GrtError(f"{who}: rays and window exclude each other")
            fn = L.grt_particle_stats_rays if steps is None else L.grt_particle_stats_mesh_rays
            self._check(fn(self._h, C.byref(params), rays.data_ptr() if shape[0] else None, shape[0], wp, C.byref(ptrs), self._stream()))
        else:
            x0, y0, x1, y1 = window if window else (0, 0, params.width, params.height)
            fn = L.grt_particle_stats_frame if steps is None else L.grt_particle_stats_mesh_frame
            self._check(fn(self._h, C.byref(params), wp, C.byref(ptrs), x0, y0, x1, y1, self._stream()))
        return into

    def ray_picks(self, params, rays=None, window=None, cross_T=0.5, picks=PICK_RULES, fields=PICK_FIELDS):
        """grt_ray_picks_frame / grt_ray_picks_rays (rays [n][6] given): per ray the first composited event, the event of largest
        weight T_i * alpha_i ('peak') and the first event behind which the transmittance is <= cross_T ('cross'; 0.5: the median
        depth) -> {pick: {field: tensor}} of shape [h][w] or [n] on the tracer's GPU; include/grt.h.  'id' is the particle's original
        id (uint32; PICK_NONE where the ray has no such event — .to(torch.int64) to index with it), 't' the event's distance and
        'weight' its T_i * alpha_i (float32; 0 where none).  The tensors are allocated pre-filled with PICK_NONE, 0, 0, so pixels
        outside a window and rays that are not traced read as "none".  Bitwise reproducible; nothing here is differentiable."""
        t = self._torch
        dev = t.device("cuda", self.device)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        picks, fields = tuple(picks), tuple(fields)
        if not picks or any(k not in PICK_RULES for k in picks):
            raise GrtError(f"ray_picks: picks must be a non-empty subset of {PICK_RULES}, not {picks}")
        if not fields or any(k not in PICK_FIELDS for k in fields):
            raise GrtError(f"ray_picks: fields must be a non-empty subset of {PICK_FIELDS}, not {fields}")
        if "cross" in picks and not 0.0 < float(cross_T) < 1.0:
            raise GrtError(f"ray_picks: cross_T must lie in (0, 1), not {cross_T}")
        if rays is not None:
            if window is not None:
                raise GrtError("ray_picks: rays and window exclude each other")
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise GrtError(f"ray_picks: rays must have shape [n][6], not {tuple(rays.shape)}")
            rays = rays.detach().to(dev, t.float32).contiguous()
            shape = (rays.shape[0],)
        else:
            shape = (params.height, params.width)
        # (PICK_NONE is int32 -1: filled as such, the kernels of the wider unsigned types are not everywhere)
        out = {k: {f: (t.full(shape, -1, dtype=t.int32, device=dev).view(t.uint32) if f == "id" else t.zeros(shape, dtype=t.float32, device=dev))
                   for f in PICK_FIELDS if f in fields} for k in PICK_RULES if k in picks}
        if not n or not shape[0] or not shape[-1]:  # (an empty scene or no ray: every element is "none" already)
            return out
        ptrs = RayPicks(*(PickOut(*(out[k][f].data_ptr() if k in out and f in out[k] else None for f in PICK_FIELDS)) for k in PICK_RULES),
                        float(cross_T))
        if rays is not None:
            self._check(lib().grt_ray_picks_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], C.byref(ptrs), self._stream()))
        else:
            x0, y0, x1, y1 = window if window else (0, 0, params.width, params.height)
            self._check(lib().grt_ray_picks_frame(self._h, C.byref(params), C.byref(ptrs), x0, y0, x1, y1, self._stream()))
        return out

    def _event_inputs(self, what, params, rays, window, max_events, first):
        """rays [n][6] (or None) as a contiguous float32 tensor on the tracer's GPU, the shape of one slot plane, the window, K and first."""
        t = self._torch
        dev = t.device("cuda", self.device)
        K, first = int(max_events), int(first)
        if K < 1 or first < 0 or first + K > 0xFFFFFFFF:
            raise GrtError(f"{what}: max_events must be >= 1 and first >= 0 with first + max_events below 2^32, not {max_events} and {first}")
        if rays is not None:
            if window is not None:
                raise GrtError(f"{what}: rays and window exclude each other")
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise GrtError(f"{what}: rays must have shape [n][6], not {tuple(rays.shape)}")
            rays = rays.detach().to(dev, t.float32).contiguous()
            shape = (rays.shape[0],)
        else:
            shape = (params.height, params.width)
        return rays, shape, (window if window else (0, 0, params.width, params.height)), dev, K, first

    def ray_events(self, params, rays=None, window=None, max_events=32, first=0, fields=EVENT_FIELDS):
        """grt_ray_events_frame / grt_ray_events_rays (rays [n][6] given): every ray's own list of composited events, the events
        first .. first + max_events - 1 in compositing order -> dict of torch tensors on the tracer's GPU; include/grt.h.  Slot-major:
        'id' (uint32, the particle's original id, PICK_NONE in an unused slot), 't' (float32, the event's key distance) and 'alpha'
        (float32, the alpha the forward composites) have shape [K][h][w] or [K][n]; 'count' (uint32, ALL events of the ray, not capped
        by K) and 'T_in' (float32, the transmittance in front of event `first`) [h][w] or [n].  T = T_in * cumprod(1 - alpha, 0) are the
        transmittances behind the listed events.  The tensors are allocated pre-filled with PICK_NONE, 0, 0, 0, 1, so pixels outside a
        window and rays that are not traced read as "no event".  Bitwise reproducible; backward_events takes dloss/dalpha back."""
        t = self._torch
        rays, shape, (x0, y0, x1, y1), dev, K, first = self._event_inputs("ray_events", params, rays, window, max_events, first)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        fields = tuple(fields)
        if not fields or any(k not in EVENT_FIELDS for k in fields):
            raise GrtError(f"ray_events: fields must be a non-empty subset of {EVENT_FIELDS}, not {fields}")
        # (PICK_NONE is int32 -1: filled as such, the kernels of the wider unsigned types are not everywhere)
        make = {"id": lambda: t.full((K,) + shape, -1, dtype=t.int32, device=dev).view(t.uint32),
                "t": lambda: t.zeros((K,) + shape, dtype=t.float32, device=dev),
                "alpha": lambda: t.zeros((K,) + shape, dtype=t.float32, device=dev),
                "count": lambda: t.zeros(shape, dtype=t.int32, device=dev).view(t.uint32),
                "T_in": lambda: t.ones(shape, dtype=t.float32, device=dev)}
        out = {k: make[k]() for k in EVENT_FIELDS if k in fields}
        if not n or not shape[0] or not shape[-1]:  # (an empty scene or no ray: every element is "no event" already)
            return out
        ptrs = RayEvents(*(out[k].data_ptr() if k in out else None for k in EVENT_FIELDS), first, K)
        if rays is not None:
            self._check(lib().grt_ray_events_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], C.byref(ptrs), self._stream()))
        else:
            self._check(lib().grt_ray_events_frame(self._h, C.byref(params), C.byref(ptrs), x0, y0, x1, y1, self._stream()))
        return out

    def backward_events(self, params, grad_alpha, rays=None, window=None, first=0, into=None, groups=None):
        """grt_backward_events_frame / grt_backward_events_rays: grad_alpha [K][h][w] or [K][n] holds dloss/dalpha of the events
        ray_events listed (same params, rays / window and first; K is its first dimension) -> dict of torch tensors pos, scale, quat,
        opacity: the gradients with respect to the uploaded Gaussians, allocated zeroed for `groups` (default: all four) or ACCUMULATED
        into the tensors of `into` (its keys are the groups computed).  Values in slots behind a ray's last event are ignored, a ray
        whose column is all zero is not traced, an event where the 0.99 clamp binds adds nothing.  One traversal.  'sh' is refused:
        colour does not depend on the listed quantities.  Not bitwise reproducible (float atomics); include/grt.h."""
        t = self._torch
        if not t.is_tensor(grad_alpha) or grad_alpha.dim() < 2:
            raise GrtError("backward_events: grad_alpha must be a tensor of shape [K][h][w] or [K][n]")
        rays, shape, (x0, y0, x1, y1), dev, K, first = self._event_inputs("backward_events", params, rays, window, grad_alpha.shape[0], first)
        if tuple(grad_alpha.shape) != (K,) + shape:
            raise GrtError(f"backward_events: grad_alpha must have shape [K]{list(shape)}, not {tuple(grad_alpha.shape)}")
        grad_alpha = grad_alpha.detach().to(dev, t.float32).contiguous()
        if "sh" in (into if into is not None else (groups if groups is not None else ())):
            raise GrtError("backward_events: 'sh' is not a group of this call (colour does not depend on the listed events' alpha)")
        if (into is not None and not into) or (into is None and groups is not None and not len(groups)):
            raise GrtError("backward_events: no gradient group asked for")
        into, ptrs = self._grad_buffers(into, groups if groups is not None else EVENT_GROUPS, dev)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        if not n or not grad_alpha.numel():
            return into
        if rays is not None:
            self._check(lib().grt_backward_events_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], grad_alpha.data_ptr(), first, K,
                                                       C.byref(ptrs), self._stream()))
        else:
            self._check(lib().grt_backward_events_frame(self._h, C.byref(params), grad_alpha.data_ptr(), first, K, C.byref(ptrs),
                                                        x0, y0, x1, y1, self._stream()))
        return into

    def ray_picks_mesh(self, params, rays=None, window=None, cross_T=0.5, picks=PICK_RULES, fields=MESH_PICK_FIELDS, steps=None):
        """grt_ray_picks_mesh_frame / grt_ray_picks_mesh_rays: ray_picks() of a frame whose rays bounce off the meshes set
        (mirror, glass, normal) -> {pick: {field: tensor}}; include/grt.h.  Beside 'id', 't' and 'weight' every pick has 'step' (uint32,
        the 1-based iteration of the bounce loop the event was met in; 0 where none) and 'point' (float32 [..][3], the world position
        o_s + t d_s on that iteration's ray); 't' is measured along that ray.  steps = (first, last): only the events of these
        iterations are candidates (1-based, inclusive; last None: open; None: all) — (2, None) picks what is seen only through a bounce;
        the cross rule tests the ray's own transmittance whatever the range.  Bitwise reproducible; nothing here is differentiable."""
        t = self._torch
        dev = t.device("cuda", self.device)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        picks, fields = tuple(picks), tuple(fields)
        if not picks or any(k not in PICK_RULES for k in picks):
            raise GrtError(f"ray_picks_mesh: picks must be a non-empty subset of {PICK_RULES}, not {picks}")
        if not fields or any(k not in MESH_PICK_FIELDS for k in fields):
            raise GrtError(f"ray_picks_mesh: fields must be a non-empty subset of {MESH_PICK_FIELDS}, not {fields}")
        if "cross" in picks and not 0.0 < float(cross_T) < 1.0:
            raise GrtError(f"ray_picks_mesh: cross_T must lie in (0, 1), not {cross_T}")
        s_first, s_last = self._mesh_steps("ray_picks_mesh", steps)
        if rays is not None:
            if window is not None:
                raise GrtError("ray_picks_mesh: rays and window exclude each other")
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise GrtError(f"ray_picks_mesh: rays must have shape [n][6], not {tuple(rays.shape)}")
            rays = rays.detach().to(dev, t.float32).contiguous()
            shape = (rays.shape[0],)
        else:
            shape = (params.height, params.width)
        # (PICK_NONE is int32 -1: filled as such, the kernels of the wider unsigned types are not everywhere)
        make = {"id": lambda: t.full(shape, -1, dtype=t.int32, device=dev).view(t.uint32),
                "t": lambda: t.zeros(shape, dtype=t.float32, device=dev),
                "weight": lambda: t.zeros(shape, dtype=t.float32, device=dev),
                "step": lambda: t.zeros(shape, dtype=t.int32, device=dev).view(t.uint32),
                "point": lambda: t.zeros(shape + (3,), dtype=t.float32, device=dev)}
        out = {k: {f: make[f]() for f in MESH_PICK_FIELDS if f in fields} for k in PICK_RULES if k in picks}
        if not n or not shape[0] or not shape[-1]:  # (an empty scene or no ray: every element is "none" already)
            return out
        ptrs = RayPicksMesh(*(PickMeshOut(*(out[k][f].data_ptr() if k in out and f in out[k] else None for f in MESH_PICK_FIELDS))
                              for k in PICK_RULES), float(cross_T), s_first, s_last)
        if rays is not None:
            self._check(lib().grt_ray_picks_mesh_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], C.byref(ptrs), self._stream()))
        else:
            x0, y0, x1, y1 = window if window else (0, 0, params.width, params.height)
            self._check(lib().grt_ray_picks_mesh_frame(self._h, C.byref(params), C.byref(ptrs), x0, y0, x1, y1, self._stream()))
        return out

    def ray_events_mesh(self, params, rays=None, window=None, max_events=32, first=0, fields=MESH_EVENT_FIELDS, steps=None, max_steps=0):
        """grt_ray_events_mesh_frame / grt_ray_events_mesh_rays: ray_events() of a frame whose rays bounce off the meshes set -> dict of
        torch tensors; include/grt.h.  The events of the iterations `steps` (as ray_picks_mesh; None: all) are numbered over the whole
        ray; beside 'id', 't', 'alpha' [K][..] there is 'step' (uint32 [K][..], the event's 1-based iteration; 0 unused), 't' measured on
        that iteration's ray.  max_steps = P > 0 adds the ray's path: 'path_rays' [P][..][6] (o_s, d_s of iteration slot + 1),
        'path_t_far' [P][..], 'path_state' (uint32 [P][..]: STEP_LAST, STEP_GAUSSIAN, STEP_TERMINATE; PICK_NONE unused) and 'n_steps'
        (uint32 [..], ALL iterations, not capped by P).  Bitwise reproducible; backward_events_mesh takes dloss/dalpha back."""
        t = self._torch
        rays, shape, (x0, y0, x1, y1), dev, K, first = self._event_inputs("ray_events_mesh", params, rays, window, max_events, first)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        fields, P = tuple(fields), int(max_steps)
        if not fields or any(k not in MESH_EVENT_FIELDS for k in fields):
            raise GrtError(f"ray_events_mesh: fields must be a non-empty subset of {MESH_EVENT_FIELDS}, not {fields}")
        if P < 0 or P > 0xFFFFFFFF:
            raise GrtError(f"ray_events_mesh: max_steps must be >= 0, not {max_steps}")
        s_first, s_last = self._mesh_steps("ray_events_mesh", steps)
        # (PICK_NONE is int32 -1: filled as such, the kernels of the wider unsigned types are not everywhere)
        make = {"id": lambda: t.full((K,) + shape, -1, dtype=t.int32, device=dev).view(t.uint32),
                "t": lambda: t.zeros((K,) + shape, dtype=t.float32, device=dev),
                "alpha": lambda: t.zeros((K,) + shape, dtype=t.float32, device=dev),
                "step": lambda: t.zeros((K,) + shape, dtype=t.int32, device=dev).view(t.uint32),
                "count": lambda: t.zeros(shape, dtype=t.int32, device=dev).view(t.uint32),
                "T_in": lambda: t.ones(shape, dtype=t.float32, device=dev)}
        out = {k: make[k]() for k in MESH_EVENT_FIELDS if k in fields}
        if P:
            out["path_rays"] = t.zeros((P,) + shape + (6,), dtype=t.float32, device=dev)
            out["path_t_far"] = t.zeros((P,) + shape, dtype=t.float32, device=dev)
            out["path_state"] = t.full((P,) + shape, -1, dtype=t.int32, device=dev).view(t.uint32)
            out["n_steps"] = t.zeros(shape, dtype=t.int32, device=dev).view(t.uint32)
        if not n or not shape[0] or not shape[-1]:  # (an empty scene or no ray: every element is "no event" already)
            return out
        ptr = lambda k: out[k].data_ptr() if k in out else None
        ptrs = RayEventsMesh(*(ptr(k) for k in MESH_EVENT_FIELDS), first, K, s_first, s_last, *(ptr(k) for k in MESH_PATH_FIELDS), P)
        if rays is not None:
            self._check(lib().grt_ray_events_mesh_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], C.byref(ptrs), self._stream()))
        else:
            self._check(lib().grt_ray_events_mesh_frame(self._h, C.byref(params), C.byref(ptrs), x0, y0, x1, y1, self._stream()))
        return out

    def backward_events_mesh(self, params, grad_alpha, rays=None, window=None, first=0, into=None, groups=None, steps=None):
        """grt_backward_events_mesh_frame / grt_backward_events_mesh_rays: backward_events() for the lists of ray_events_mesh (same
        params, rays / window, first and steps; K is grad_alpha's first dimension).  Every listed alpha is differentiated on its own
        iteration's ray, the mesh hits and the next rays held fixed.  One traversal; float atomics; include/grt.h."""
        t = self._torch
        if not t.is_tensor(grad_alpha) or grad_alpha.dim() < 2:
            raise GrtError("backward_events_mesh: grad_alpha must be a tensor of shape [K][h][w] or [K][n]")
        rays, shape, (x0, y0, x1, y1), dev, K, first = self._event_inputs("backward_events_mesh", params, rays, window, grad_alpha.shape[0], first)
        if tuple(grad_alpha.shape) != (K,) + shape:
            raise GrtError(f"backward_events_mesh: grad_alpha must have shape [K]{list(shape)}, not {tuple(grad_alpha.shape)}")
        grad_alpha = grad_alpha.detach().to(dev, t.float32).contiguous()
        if "sh" in (into if into is not None else (groups if groups is not None else ())):
            raise GrtError("backward_events_mesh: 'sh' is not a group of this call (colour does not depend on the listed events' alpha)")
        if (into is not None and not into) or (into is None and groups is not None and not len(groups)):
            raise GrtError("backward_events_mesh: no gradient group asked for")
        s_first, s_last = self._mesh_steps("backward_events_mesh", steps)
        into, ptrs = self._grad_buffers(into, groups if groups is not None else EVENT_GROUPS, dev)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        if not n or not grad_alpha.numel():
            return into
        if rays is not None:
            self._check(lib().grt_backward_events_mesh_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], grad_alpha.data_ptr(), first, K,
                                                            s_first, s_last, C.byref(ptrs), self._stream()))
        else:
            self._check(lib().grt_backward_events_mesh_frame(self._h, C.byref(params), grad_alpha.data_ptr(), first, K, s_first, s_last,
                                                             C.byref(ptrs), x0, y0, x1, y1, self._stream()))
        return into

    def _segment_inputs(self, what, params, rays, t_near, t_far, T_in, window):
        """rays [n][6] (or None) as a contiguous float32 tensor on the tracer's GPU, the shape of one output plane, the window, and
        the three per-ray inputs as contiguous float32 tensors of that shape (a scalar is expanded on the device; None stays None: the
        call's default) with their Segments structure."""
        t = self._torch
        dev = t.device("cuda", self.device)
        if rays is not None:
            if window is not None:
                raise GrtError(f"{what}: rays and window exclude each other")
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise GrtError(f"{what}: rays must have shape [n][6], not {tuple(rays.shape)}")
            rays = rays.detach().to(dev, t.float32).contiguous()
            shape = (rays.shape[0],)
        else:
            shape = (params.height, params.width)
        keep = []
        for name, v in (("t_near", t_near), ("t_far", t_far), ("T_in", T_in)):
            if v is None:
                keep.append(None)
            elif t.is_tensor(v) and v.dim() > 0:
                if tuple(v.shape) != shape:
                    raise GrtError(f"{what}: {name} must be a scalar or have shape {list(shape)}, not {tuple(v.shape)}")
                keep.append(v.detach().to(dev, t.float32).contiguous())
            else:
                keep.append(t.full(shape, float(v), dtype=t.float32, device=dev))
        seg = Segments(*(x.data_ptr() if x is not None else None for x in keep))
        return rays, shape, (window if window else (0, 0, params.width, params.height)), dev, keep, seg

    def trace_segments(self, params, rays=None, t_near=None, t_far=None, T_in=None, window=None, outputs=SEGMENT_OUTPUTS):
        """grt_trace_segments_frame / grt_trace_segments_rays (rays [n][6] given): the reference's trace() for one segment [t_near,
        t_far] of every ray, entered with the transmittance T_in -> dict of torch tensors on the tracer's GPU: 'radiance' [n][3] or
        [h][w][3] (R = sum T_i alpha_i L_i, NOT multiplied by the opacity), 'T_out' (T_in prod (1 - alpha_i)), 'depth' (sum T_i alpha_i
        t_i) and 'count' (uint32) [n] or [h][w]; include/grt.h.  t_near, t_far, T_in: tensors of that shape, scalars (expanded on the
        device) or None (params.t_min, params.t_max, 1).  A ray whose range is empty, reversed, not positive or not finite, or whose
        T_in is not above minTransmittance, is untraced: zeros, and T_out a bit copy of T_in.  Outside a window the tensors hold 0 and
        T_in's values.  Bitwise reproducible; backward_segments takes dloss/dradiance and dloss/dT_out back."""
        t = self._torch
        rays, shape, (x0, y0, x1, y1), dev, keep, seg = self._segment_inputs("trace_segments", params, rays, t_near, t_far, T_in, window)
        outputs = tuple(outputs)
        if not outputs or any(k not in SEGMENT_OUTPUTS for k in outputs):
            raise GrtError(f"trace_segments: outputs must be a non-empty subset of {SEGMENT_OUTPUTS}, not {outputs}")
        make = {"radiance": lambda: t.zeros(shape + (3,), dtype=t.float32, device=dev),
                "T_out": lambda: keep[2].clone() if keep[2] is not None else t.ones(shape, dtype=t.float32, device=dev),
                "depth": lambda: t.zeros(shape, dtype=t.float32, device=dev),
                "count": lambda: t.zeros(shape, dtype=t.int32, device=dev).view(t.uint32)}
        out = {k: make[k]() for k in SEGMENT_OUTPUTS if k in outputs}
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        if not n or not shape[0] or not shape[-1]:  # (an empty scene or no ray: every element is untraced already)
            return out
        ptrs = SegmentOut(*(out[k].data_ptr() if k in out else None for k in SEGMENT_OUTPUTS))
        if rays is not None:
            self._check(lib().grt_trace_segments_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], C.byref(seg), C.byref(ptrs),
                                                      self._stream()))
        else:
            self._check(lib().grt_trace_segments_frame(self._h, C.byref(params), C.byref(seg), C.byref(ptrs), x0, y0, x1, y1, self._stream()))
        return out

    def backward_segments(self, params, grad_radiance, grad_T_out=None, rays=None, t_near=None, t_far=None, T_in=None, window=None,
                          into=None, groups=None):
        """grt_backward_segments_frame / grt_backward_segments_rays: grad_radiance [n][3] or [h][w][3] and grad_T_out [n] or [h][w]
        (None: zero) hold dloss/dR and dloss/dT_out of the segments trace_segments traced (same params, rays / window, t_near, t_far,
        T_in) -> dict of torch tensors pos, scale, quat, opacity, sh: the gradients with respect to the uploaded Gaussians, allocated
        zeroed for `groups` (default: all five) or ACCUMULATED into the tensors of `into` (its keys are the groups computed).  No
        forward outputs are passed; a ray whose four upstream values are exactly 0 is not traced.  Not bitwise reproducible (float
        atomics); include/grt.h."""
        t = self._torch
        rays, shape, (x0, y0, x1, y1), dev, keep, seg = self._segment_inputs("backward_segments", params, rays, t_near, t_far, T_in, window)
        if not t.is_tensor(grad_radiance) or tuple(grad_radiance.shape) != shape + (3,):
            raise GrtError(f"backward_segments: grad_radiance must be a tensor of shape {list(shape + (3,))}")
        if grad_T_out is not None and tuple(grad_T_out.shape) != shape:
            raise GrtError(f"backward_segments: grad_T_out must have shape {list(shape)}, not {tuple(grad_T_out.shape)}")
        g_R = grad_radiance.detach().to(dev, t.float32).contiguous()
        g_T = grad_T_out.detach().to(dev, t.float32).contiguous() if grad_T_out is not None else None
        if (into is not None and not into) or (into is None and groups is not None and not len(groups)):
            raise GrtError("backward_segments: no gradient group asked for")
        into, ptrs = self._grad_buffers(into, groups, dev)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        if not n or not g_R.numel():
            return into
        if rays is not None:
            self._check(lib().grt_backward_segments_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], C.byref(seg), g_R.data_ptr(),
                                                         g_T.data_ptr() if g_T is not None else None, C.byref(ptrs), self._stream()))
        else:
            self._check(lib().grt_backward_segments_frame(self._h, C.byref(params), C.byref(seg), g_R.data_ptr(),
                                                          g_T.data_ptr() if g_T is not None else None, C.byref(ptrs), x0, y0, x1, y1,
                                                          self._stream()))
        return into

    def _depth_inputs(self, what, params, rays, window, kind):
        """rays [n][6] (or None) as a contiguous float32 tensor on the tracer's GPU, the shape of one output plane, the window, the
        device and the kind's number."""
        t = self._torch
        dev = t.device("cuda", self.device)
        if kind not in DEPTH_KINDS:
            raise GrtError(f"{what}: kind must be one of {tuple(DEPTH_KINDS)}, not {kind!r}")
        if rays is not None:
            if window is not None:
                raise GrtError(f"{what}: rays and window exclude each other")
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise GrtError(f"{what}: rays must have shape [n][6], not {tuple(rays.shape)}")
            rays = rays.detach().to(dev, t.float32).contiguous()
            shape = (rays.shape[0],)
        else:
            shape = (params.height, params.width)
        return rays, shape, (window if window else (0, 0, params.width, params.height)), dev, DEPTH_KINDS[kind]

    def ray_depth(self, params, rays=None, window=None, kind="peak", outputs=DEPTH_OUTPUTS):
        """grt_ray_depth_frame / grt_ray_depth_rays (rays [n][6] given): the distance moments of every whole ray -> dict of torch
        tensors [n] or [h][w] on the tracer's GPU: 'dist' (sum w_i tau_i), 'dist2' (sum w_i tau_i^2), 'T_out' (prod (1 - alpha_i)) and
        'count' (uint32); include/grt.h.  kind "key": tau_i is the event's key distance (the aux depth's); "peak": the distance of the
        particle's maximum response along the ray, which is differentiable (backward_depth).  tau is in units of |d|, not clamped to
        the range and may be negative; dist / (1 - T_out) is the mean.  An untraced ray and a pixel outside a window hold 0, 0, 1, 0.
        Bitwise reproducible."""
        t = self._torch
        rays, shape, (x0, y0, x1, y1), dev, kind = self._depth_inputs("ray_depth", params, rays, window, kind)
        outputs = tuple(outputs)
        if not outputs or any(k not in DEPTH_OUTPUTS for k in outputs):
            raise GrtError(f"ray_depth: outputs must be a non-empty subset of {DEPTH_OUTPUTS}, not {outputs}")
        make = {"dist": lambda: t.zeros(shape, dtype=t.float32, device=dev), "dist2": lambda: t.zeros(shape, dtype=t.float32, device=dev),
                "T_out": lambda: t.ones(shape, dtype=t.float32, device=dev),
                "count": lambda: t.zeros(shape, dtype=t.int32, device=dev).view(t.uint32)}
        out = {k: make[k]() for k in DEPTH_OUTPUTS if k in outputs}
        if not shape[0] or not shape[-1]:  # (no ray: nothing to write.  An empty scene goes to the library: its refusals hold)
            return out
        ptrs = DepthOut(*(out[k].data_ptr() if k in out else None for k in DEPTH_OUTPUTS))
        if rays is not None:
            self._check(lib().grt_ray_depth_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], kind, C.byref(ptrs), self._stream()))
        else:
            self._check(lib().grt_ray_depth_frame(self._h, C.byref(params), kind, C.byref(ptrs), x0, y0, x1, y1, self._stream()))
        return out

    def backward_depth(self, params, grad_dist=None, grad_dist2=None, grad_T_out=None, rays=None, window=None, kind="peak", into=None,
                       groups=None, ray_grads=False):
        """grt_backward_depth_frame / grt_backward_depth_rays: grad_dist, grad_dist2, grad_T_out [n] or [h][w] (each may be None, not
        all) hold dloss/ddist, dloss/ddist2 and dloss/dT_out of what ray_depth computed (same params, rays / window, kind) -> dict of
        torch tensors pos, scale, quat, opacity: the gradients with respect to the uploaded Gaussians, allocated zeroed for `groups`
        (default: all four) or ACCUMULATED into the tensors of `into`.  ray_grads: the dict also holds "rays" [n][6] or [h][w][6]
        (dloss/do, dloss/dd as the kernel holds d: no projection), WRITTEN and bitwise reproducible; groups=[] with ray_grads is the
        rays-only call (no atomics, no gradient buffer).  A ray whose three upstream values are exactly 0 is not traced; include/grt.h."""
        t = self._torch
        rays, shape, (x0, y0, x1, y1), dev, kind = self._depth_inputs("backward_depth", params, rays, window, kind)
        ups = []
        for name, g in (("grad_dist", grad_dist), ("grad_dist2", grad_dist2), ("grad_T_out", grad_T_out)):
            if g is not None and (not t.is_tensor(g) or tuple(g.shape) != shape):
                raise GrtError(f"backward_depth: {name} must be a tensor of shape {list(shape)}")
            ups.append(g.detach().to(dev, t.float32).contiguous() if g is not None else None)
        if all(g is None for g in ups):
            raise GrtError("backward_depth: no upstream (grad_dist, grad_dist2 and grad_T_out are all None)")
        if any(k not in DEPTH_GROUPS for k in (groups or ())):  # (an 'sh' tensor in `into` is handed on and left untouched)
            raise GrtError(f"backward_depth: the gradient groups are {DEPTH_GROUPS} (the depth has no colour)")
        if groups is None and into is None:
            groups = DEPTH_GROUPS
        if ray_grads:
            into, out, hold = self._ex_buffers(into, groups, dev, shape + (6,))
        else:
            if (into is not None and not into) or (into is None and not len(groups)):
                raise GrtError("backward_depth: no gradient group asked for")
            into, hold = self._grad_buffers(into, groups, dev)
            out = BackwardOut(C.pointer(hold), None)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        # (no ray: nothing to write.  An empty scene has no gradient array to point at — its tensors hold no element —, so only a call
        # with the rays' output goes to the library, which WRITES that output's zeros)
        if not shape[0] or not shape[-1] or (not n and not ray_grads):
            return into
        if not n:
            out = BackwardOut(None, into["rays"].data_ptr())
        up = DepthUpstream(*(g.data_ptr() if g is not None else None for g in ups))
        if rays is not None:
            self._check(lib().grt_backward_depth_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], kind, C.byref(up), C.byref(out),
                                                      self._stream()))
        else:
            self._check(lib().grt_backward_depth_frame(self._h, C.byref(params), kind, C.byref(up), C.byref(out), x0, y0, x1, y1,
                                                       self._stream()))
        return into

    def ray_depth_mesh(self, params, rays=None, window=None, kind="peak", outputs=DEPTH_MESH_OUTPUTS, steps=None, surface=False):
        """grt_ray_depth_mesh_frame / grt_ray_depth_mesh_rays (rays [n][6] given): ray_depth() of a frame whose rays bounce off the
        meshes set on the tracer (include/grt.h) -> dict of torch tensors [n] or [h][w] on the tracer's GPU: 'dist', 'dist2', 'weight'
        and 'count' (uint32).  An event of iteration s lies at the path prefix P_s (the sum of the earlier iterations' segment ends)
        plus its own distance on the step's ray (kind "key" or "peak"), and enters with the colour weight c_s * T_i * alpha_i;
        dist / weight is the mean path length of what the pixel shows.  steps = (first, last) as in render_features_mesh; surface:
        a terminating hit of a NORMAL mesh adds its own surface with 1 - D.  On a tracer without meshes dist is (1 - T_out) *
        ray_depth()'s.  An untraced ray and a pixel outside a window hold zeros.  Bitwise reproducible."""
        t = self._torch
        rays, shape, (x0, y0, x1, y1), dev, kind = self._depth_inputs("ray_depth_mesh", params, rays, window, kind)
        first, last = self._mesh_steps("ray_depth_mesh", steps)
        outputs = tuple(outputs)
        if not outputs or any(k not in DEPTH_MESH_OUTPUTS for k in outputs):
            raise GrtError(f"ray_depth_mesh: outputs must be a non-empty subset of {DEPTH_MESH_OUTPUTS}, not {outputs}")
        out = {k: (t.zeros(shape, dtype=t.int32, device=dev).view(t.uint32) if k == "count" else t.zeros(shape, dtype=t.float32, device=dev))
               for k in DEPTH_MESH_OUTPUTS if k in outputs}
        if not shape[0] or not shape[-1]:  # (no ray: nothing to write.  An empty scene goes to the library: its refusals hold)
            return out
        ptrs = DepthMeshOut(*(out[k].data_ptr() if k in out else None for k in DEPTH_MESH_OUTPUTS))
        flags = DEPTH_SURFACE if surface else 0
        if rays is not None:
            self._check(lib().grt_ray_depth_mesh_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], kind, flags, C.byref(ptrs), first, last,
                                                      self._stream()))
        else:
            self._check(lib().grt_ray_depth_mesh_frame(self._h, C.byref(params), kind, flags, C.byref(ptrs), first, last, x0, y0, x1, y1,
                                                       self._stream()))
        return out

    def backward_depth_mesh(self, params, grad_dist=None, grad_dist2=None, grad_weight=None, rays=None, window=None, kind="peak", into=None,
                            groups=None, steps=None, surface=False):
        """grt_backward_depth_mesh_frame / grt_backward_depth_mesh_rays: grad_dist, grad_dist2, grad_weight [n] or [h][w] (each may be
        None, not all) hold dloss/ddist, dloss/ddist2 and dloss/dweight of what ray_depth_mesh computed (same params, rays / window,
        kind, steps, surface) -> dict of torch tensors pos, scale, quat, opacity: the gradients with respect to the uploaded Gaussians,
        allocated zeroed for `groups` (default: all four) or ACCUMULATED into the tensors of `into`.  The meshes, the path and its
        prefix are held fixed; nothing is computed for rays or the camera.  A ray whose three upstream values are exactly 0 is not
        traced; include/grt.h."""
        t = self._torch
        rays, shape, (x0, y0, x1, y1), dev, kind = self._depth_inputs("backward_depth_mesh", params, rays, window, kind)
        first, last = self._mesh_steps("backward_depth_mesh", steps)
        ups = []
        for name, g in (("grad_dist", grad_dist), ("grad_dist2", grad_dist2), ("grad_weight", grad_weight)):
            if g is not None and (not t.is_tensor(g) or tuple(g.shape) != shape):
                raise GrtError(f"backward_depth_mesh: {name} must be a tensor of shape {list(shape)}")
            ups.append(g.detach().to(dev, t.float32).contiguous() if g is not None else None)
        if all(g is None for g in ups):
            raise GrtError("backward_depth_mesh: no upstream (grad_dist, grad_dist2 and grad_weight are all None)")
        if any(k not in DEPTH_GROUPS for k in (groups or ())) or any(k not in DEPTH_GROUPS for k in (into or ())):
            raise GrtError(f"backward_depth_mesh: the gradient groups are {DEPTH_GROUPS} (the depth has no colour)")
        if groups is None and into is None:
            groups = DEPTH_GROUPS
        if (into is not None and not into) or (into is None and not len(groups)):
            raise GrtError("backward_depth_mesh: no gradient group asked for")
        into, hold = self._grad_buffers(into, groups, dev)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        if not shape[0] or not shape[-1] or not n:  # (no ray or no particle: nothing to add)
            return into
        ptrs = FeatureGrads(hold.pos, hold.scale, hold.quat, hold.opacity, None)
        up = DepthMeshUpstream(*(g.data_ptr() if g is not None else None for g in ups))
        flags = DEPTH_SURFACE if surface else 0
        if rays is not None:
            self._check(lib().grt_backward_depth_mesh_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], kind, flags, C.byref(up),
                                                           C.byref(ptrs), first, last, self._stream()))
        else:
            self._check(lib().grt_backward_depth_mesh_frame(self._h, C.byref(params), kind, flags, C.byref(up), C.byref(ptrs), first, last,
                                                            x0, y0, x1, y1, self._stream()))
        return into

    def _feature_inputs(self, what, params, feat, rays, window):
        """feat [n_particles][C] and rays [n][6] (or None) as contiguous float32 tensors on the tracer's GPU, the shape of the rays'
        side of the output, and the window."""
        t = self._torch
        dev = t.device("cuda", self.device)
        n = self._scene.n_particles if self._scene is not None else self.n_particles
        feat = t.as_tensor(feat).detach().to(dev, t.float32).contiguous()
        if feat.dim() != 2 or feat.shape[0] != n or feat.shape[1] < 1:
            raise GrtError(f"{what}: feat must have shape [{n}][C] with C >= 1, not {tuple(feat.shape)}")
        if rays is not None:
            if window is not None:
                raise GrtError(f"{what}: rays and window exclude each other")
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise GrtError(f"{what}: rays must have shape [n][6], not {tuple(rays.shape)}")
            rays = rays.detach().to(dev, t.float32).contiguous()
            shape = (rays.shape[0],)
        else:
            shape = (params.height, params.width)
        return feat, rays, shape, (window if window else (0, 0, params.width, params.height)), dev, n

    def _mesh_steps(self, what, steps):
        """steps = None or (first, last | None) as the (step_first, step_last) of the mesh calls (include/grt.h)."""
        if steps is None:
            return 0, 0
        first, last = steps
        first, last = int(first), 0 if last is None else int(last)
        if first < 0 or last < 0 or (steps[1] is not None and last == 0):
            raise GrtError(f"{what}: steps must be (first, last) with 1 <= first <= last, or last None, not {tuple(steps)}")
        return first, last

    def render_features(self, params, feat, rays=None, window=None):
        """grt_render_features_frame / grt_render_features_rays (rays [n][6] given): the caller's per-particle channels feat
        [n_particles][C] (by original id) composited with the frame's weights, F[ray][c] = sum_i T_i alpha_i feat[id_i][c] over the
        composited events; include/grt.h.  Returns a float32 tensor [h][w][C] (zero outside the window) or [n][C] on the tracer's
        GPU.  F is not multiplied by alpha and not normalised.  Any C >= 1: more than 16 channels run in slices of 16."""
        return self._render_features("render_features", None, params, feat, rays, window)

    def render_features_mesh(self, params, feat, rays=None, window=None, steps=None):
        """grt_render_features_mesh_frame / grt_render_features_mesh_rays: render_features() of a frame whose rays bounce off the
        meshes set on the tracer (include/grt.h) — a particle's channels enter the pixel with the colour weight c_s * T_i * alpha_i its
        radiance enters the colour with, ONE transmittance running through all of a ray's segments; a mesh surface itself has no
        feature.  steps = (first, last): only the events of these iterations of the bounce loop carry their feature row (1-based,
        inclusive; last None = open; None = all): (2, None) is what is seen only through a bounce.  On a tracer without meshes the
        result is (1 - T_end) * render_features().  Any C >= 1: more than 16 channels run in slices of 16."""
        return self._render_features("render_features_mesh", self._mesh_steps("render_features_mesh", steps), params, feat, rays, window)

    def _render_features(self, what, steps, params, feat, rays, window):
        """The checks, the allocation and the calls of render_features (steps None) and render_features_mesh."""
        t = self._torch
        feat, rays, shape, (x0, y0, x1, y1), dev, n = self._feature_inputs(what, params, feat, rays, window)
        C_ = feat.shape[1]
        L = lib()
        parts = []
        for c0 in range(0, C_, MAX_FEATURE_CHANNELS):
            f = feat[:, c0:c0 + MAX_FEATURE_CHANNELS].contiguous()
            out = t.zeros(shape + (f.shape[1],), dtype=t.float32, device=dev)
            if n and out.numel():
                if rays is not None and steps is None:
                    self._check(L.grt_render_features_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], f.data_ptr(), f.shape[1],
                                                           out.data_ptr(), self._stream()))
                elif rays is not None:
                    self._check(L.grt_render_features_mesh_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], f.data_ptr(), f.shape[1],
                                                                out.data_ptr(), steps[0], steps[1], self._stream()))
                elif steps is None:
                    self._check(L.grt_render_features_frame(self._h, C.byref(params), f.data_ptr(), f.shape[1], out.data_ptr(), x0, y0, x1, y1,
                                                            self._stream()))
                else:
                    self._check(L.grt_render_features_mesh_frame(self._h, C.byref(params), f.data_ptr(), f.shape[1], out.data_ptr(), steps[0],
                                                                 steps[1], x0, y0, x1, y1, self._stream()))
            parts.append(out)
        return parts[0] if len(parts) == 1 else t.cat(parts, -1)

    def backward_features(self, params, feat, grad_out, rays=None, window=None, into=None, groups=None):
        """grt_backward_features_frame / grt_backward_features_rays: gradients of sum(grad_out * F) for the F of render_features (same
        params, feat, rays / window; grad_out shaped like F) -> dict of torch tensors over pos, scale, quat, opacity (with respect to
        the uploaded Gaussians) and feat [n_particles][C], allocated zeroed for `groups` (default: all five), or ACCUMULATED into the
        tensors of `into` (its keys are the groups computed).  'feat' alone is one traversal and uses no buffer of the tracer.  Any
        C >= 1: more than 16 channels run in slices of 16 whose gradients add up (the backward is linear in the upstream).  Not
        bitwise reproducible (float atomics); include/grt.h."""
        return self._backward_features("backward_features", None, params, feat, grad_out, rays, window, into, groups)

    def backward_features_mesh(self, params, feat, grad_out, rays=None, window=None, into=None, groups=None, steps=None):
        """grt_backward_features_mesh_frame / grt_backward_features_mesh_rays: backward_features() for the F of render_features_mesh
        (same params, feat, rays / window, steps) on a frame whose rays bounce off the tracer's meshes; the meshes and every discrete
        decision are held fixed (include/grt.h).  A ray is walked twice, also for 'feat' alone (which uses no buffer of the tracer)."""
        return self._backward_features("backward_features_mesh", self._mesh_steps("backward_features_mesh", steps), params, feat, grad_out,
                                       rays, window, into, groups)

    def _backward_features(self, what, steps, params, feat, grad_out, rays, window, into, groups):
        """The checks, the allocation and the calls of backward_features (steps None) and backward_features_mesh."""
        t = self._torch
        feat, rays, shape, (x0, y0, x1, y1), dev, n = self._feature_inputs(what, params, feat, rays, window)
        C_ = feat.shape[1]
        grad_out = t.as_tensor(grad_out).detach().to(dev, t.float32).contiguous()
        if tuple(grad_out.shape) != shape + (C_,):
            raise GrtError(f"{what}: grad_out must have shape {shape + (C_,)}, not {tuple(grad_out.shape)}")
        shapes = {k: ((C_,) if k == "feat" else GRAD_SHAPES[k]) for k in FEATURE_GROUPS}
        if into is None:
            bad = [k for k in (groups if groups is not None else ()) if k not in FEATURE_GROUPS]
            if bad or (groups is not None and not len(groups)):
                raise GrtError(f"{what}: groups must be a non-empty subset of {FEATURE_GROUPS}, not {tuple(groups)}")
            into = {k: t.zeros((n,) + shapes[k], dtype=t.float32, device=dev) for k in (groups if groups is not None else FEATURE_GROUPS)}
        for k, v in into.items():
            if k not in FEATURE_GROUPS or tuple(v.shape) != (n,) + shapes[k] or v.dtype != t.float32 or not v.is_contiguous() or v.device != dev:
                raise GrtError(f"{what}: gradient tensor '{k}' must be contiguous float32 of shape {(n,) + shapes[k]} on {dev}")
        if not into:
            raise GrtError(f"{what}: no gradient group asked for")
        if not n or not grad_out.numel():
            return into
        L = lib()
        sliced = C_ > MAX_FEATURE_CHANNELS
        for c0 in range(0, C_, MAX_FEATURE_CHANNELS):
            f = feat[:, c0:c0 + MAX_FEATURE_CHANNELS].contiguous()
            g = grad_out[..., c0:c0 + MAX_FEATURE_CHANNELS].contiguous()
            gf = None
            if "feat" in into:  # (a slice of the [n][C] tensor is not contiguous: its gradient goes through a tensor of its own)
                gf = t.zeros_like(f) if sliced else into["feat"]
            ptrs = FeatureGrads(*(into[k].data_ptr() if k in into else None for k in FEATURE_GROUPS[:4]), gf.data_ptr() if gf is not None else None)
            if rays is not None and steps is None:
                self._check(L.grt_backward_features_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], f.data_ptr(), f.shape[1],
                                                         g.data_ptr(), C.byref(ptrs), self._stream()))
            elif rays is not None:
                self._check(L.grt_backward_features_mesh_rays(self._h, C.byref(params), rays.data_ptr(), shape[0], f.data_ptr(), f.shape[1],
                                                              g.data_ptr(), C.byref(ptrs), steps[0], steps[1], self._stream()))
            elif steps is None:
                self._check(L.grt_backward_features_frame(self._h, C.byref(params), f.data_ptr(), f.shape[1], g.data_ptr(), C.byref(ptrs),
                                                          x0, y0, x1, y1, self._stream()))
            else:
                self._check(L.grt_backward_features_mesh_frame(self._h, C.byref(params), f.data_ptr(), f.shape[1], g.data_ptr(), C.byref(ptrs),
                                                               steps[0], steps[1], x0, y0, x1, y1, self._stream()))
            if gf is not None and sliced:
                into["feat"][:, c0:c0 + MAX_FEATURE_CHANNELS] += gf
        return into

    def _point_inputs(self, what, points, alpha_min):
        """points [n][3] as a contiguous float32 tensor on the tracer's GPU, the device, and alpha_min as the library takes it (0: the
        scene's own)."""
        t = self._torch
        dev = t.device("cuda", self.device)
        if not t.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
            raise GrtError(f"{what}: points must be a tensor of shape [n][3]")
        return points.detach().to(dev, t.float32).contiguous(), dev, (0.0 if alpha_min is None else float(alpha_min))

    def query_points(self, points, alpha_min=None, outputs=POINT_OUTPUTS):
        """grt_query_points: the Gaussian field at points [n][3] -> dict of torch tensors [n] on the tracer's GPU: 'density' (sum of the
        contributing particles' a_i = min(0.99, opacity response)), 'occupancy' (1 - prod (1 - a_i)), 'peak' (max a_i), 'peak_id'
        (uint32: the original id of the maximum, the lowest of equal ones, PICK_NONE where nothing contributes) and 'count' (uint32);
        include/grt.h.  A particle contributes where a_i > alpha_min (None: the scene's own; a larger value is allowed, a smaller one
        refused).  A non-finite point and one outside every leaf box hold 0, 0, 0, PICK_NONE, 0.  Meshes are ignored.  Bitwise
        reproducible.  Pass the points in a spatially coherent order (grid order is one): one point per lane."""
        t = self._torch
        points, dev, amin = self._point_inputs("query_points", points, alpha_min)
        outputs = tuple(outputs)
        if not outputs or any(k not in POINT_OUTPUTS for k in outputs):
            raise GrtError(f"query_points: outputs must be a non-empty subset of {POINT_OUTPUTS}, not {outputs}")
        n = int(points.shape[0])
        out = {k: (t.zeros((n,), dtype=t.int32, device=dev).view(t.uint32) if k in ("peak_id", "count")
                   else t.zeros((n,), dtype=t.float32, device=dev)) for k in POINT_OUTPUTS if k in outputs}
        if not n:  # (no point: nothing to write)
            return out
        ptrs = PointOut(*(out[k].data_ptr() if k in out else None for k in POINT_OUTPUTS))
        self._check(lib().grt_query_points(self._h, points.data_ptr(), n, amin, C.byref(ptrs), self._stream()))
        return out

    def backward_points(self, points, grad_density=None, grad_occupancy=None, alpha_min=None, into=None, groups=None, point_grads=False):
        """grt_backward_points: grad_density, grad_occupancy [n] (each may be None, not both) hold dloss/ddensity and dloss/doccupancy
        of what query_points computed (same points, alpha_min) -> dict of torch tensors pos, scale, quat, opacity: the gradients with
        respect to the uploaded Gaussians, allocated zeroed for `groups` (default: all four) or ACCUMULATED into the tensors of `into`.
        point_grads: the dict also holds "points" [n][3] (dloss/dx), WRITTEN and bitwise reproducible; groups=[] with point_grads is
        the points-only call (no atomics, no gradient buffer).  A point whose two upstream values are exactly 0 is not walked;
        include/grt.h."""
        t = self._torch
        points, dev, amin = self._point_inputs("backward_points", points, alpha_min)
        n = int(points.shape[0])
        ups = []
        for name, g in (("grad_density", grad_density), ("grad_occupancy", grad_occupancy)):
            if g is not None and (not t.is_tensor(g) or tuple(g.shape) != (n,)):
                raise GrtError(f"backward_points: {name} must be a tensor of shape [{n}]")
            ups.append(g.detach().to(dev, t.float32).contiguous() if g is not None else None)
        if all(g is None for g in ups):
            raise GrtError("backward_points: no upstream (grad_density and grad_occupancy are both None)")
        if any(k not in POINT_GROUPS for k in (groups or ())):  # (an 'sh' tensor in `into` is handed on and left untouched)
            raise GrtError(f"backward_points: the gradient groups are {POINT_GROUPS} (a density has no colour)")
        if groups is None and into is None:
            groups = POINT_GROUPS
        pts_t = None
        if into is not None:
            into = dict(into)
            pts_t = into.pop("points", None)
            point_grads = point_grads or pts_t is not None
        if into is None and not len(groups):
            into = {}
        if into is not None and not into and not point_grads:
            raise GrtError("backward_points: no gradient group asked for")
        into, hold = self._grad_buffers(into, groups, dev)
        into = dict(into)
        if point_grads:
            if pts_t is None:
                pts_t = t.zeros((n, 3), dtype=t.float32, device=dev)
            elif tuple(pts_t.shape) != (n, 3) or pts_t.dtype != t.float32 or not pts_t.is_contiguous() or pts_t.device != dev:
                raise GrtError(f"backward_points: gradient tensor 'points' must be contiguous float32 of shape {(n, 3)} on {dev}")
            into["points"] = pts_t
        n_part = self._scene.n_particles if self._scene is not None else self.n_particles
        # (no point: nothing to write.  An empty scene has no gradient array to point at, so only a call with the points' output goes
        # to the library, which WRITES that output's zeros)
        if not n or (not n_part and not point_grads):
            return into
        g = PointGrads(*((getattr(hold, k) if n_part else None) for k in POINT_GROUPS), pts_t.data_ptr() if point_grads else None)
        up = PointUpstream(*(u.data_ptr() if u is not None else None for u in ups))
        self._check(lib().grt_backward_points(self._h, points.data_ptr(), n, amin, C.byref(up), C.byref(g), self._stream()))
        return into

    def _ex_buffers(self, into, groups, dev, ray_shape):
        """The outputs of an extended backward call: the groups' tensors as _grad_buffers makes them (groups=[] or into={}: none, the
        rays-only call) and the "rays" tensor: into["rays"] when given (WRITTEN, not added to; pixels outside a window keep what
        they held), else a zeroed one."""
        t = self._torch
        rays_t = None
        if into is not None:
            into = dict(into)
            rays_t = into.pop("rays", None)
        if into is None and groups is not None and len(groups) == 0:
            into = {}
        into, ptrs = self._grad_buffers(into, groups, dev)
        into = dict(into)
        if rays_t is None:
            rays_t = t.zeros(ray_shape, dtype=t.float32, device=dev)
        elif tuple(rays_t.shape) != tuple(ray_shape) or rays_t.dtype != t.float32 or not rays_t.is_contiguous():
            raise GrtError(f"backward: gradient tensor 'rays' must be contiguous float32 of shape {tuple(ray_shape)}")
        into["rays"] = rays_t
        out = BackwardOut(C.pointer(ptrs) if len(into) > 1 else None, into["rays"].data_ptr())
        return into, out, ptrs

    def counters(self):
        c = Counters()
        self._check(lib().grt_get_counters(self._h, C.byref(c)))
        return c.as_dict()

    def last_kernel_ms(self):
        ms = C.c_float()
        self._check(lib().grt_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def sync(self):
        self._torch.cuda.synchronize(self.device)

    def close(self):
        if self._h:
            lib().grt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
