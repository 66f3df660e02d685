/*
 * grt.h — C ABI of libgrt_hip.so, the MI355X-native replacement for the OptiX pipeline behind
 * GaussianTracer::render() (reference: Ray-Studio2/gaussian-ray-tracing).
 *
 * Plain C: pointers, sizes, PODs.  No HIP, torch, OptiX or C++ types in any signature
 * (a hipStream_t crosses as void*; device pointers cross as void* / typed pointers).
 * Every entry point returns GRT_OK (0) or a negative grt_status; grt_last_error(ctx) holds the
 * text (the reference throws std::runtime_error with call text, src/Exception.h:19-80 — the C++
 * facade gaussian-ray-tracing_amd/host/GaussianTracer.cpp converts codes back to exceptions).
 *
 * What each entry point replaces in the reference:
 *   grt_create / grt_destroy      createContext..createSBT + dtor          src/GaussianTracer.cpp:85-295, 54-70
 *   grt_create_view               (new) a second frame slot on the same scene: what D frames in flight need, where the
 *                                 reference has one stream and one frame at a time (src/GaussianTracer.cpp:504,537)
 *   grt_upload_gaussians          particle upload in initializeParams      src/GaussianTracer.cpp:491-502
 *   grt_build_bvh                 createGaussianParticlesBVH/createGAS/    src/GaussianTracer.cpp:297-317,
 *                                 buildAccelationStructure (OptiX, closed)   319-399, 422-473
 *   grt_update_gaussians_device   (new) the scene of an optimisation step: attributes from DEVICE memory, the LBVH re-fitted
 *                                 instead of rebuilt while the particles move a little
 *   grt_set_meshes                createGAS+createIAS for primitives,      src/GaussianTracer.cpp:578-709
 *                                 sendGeometryAttributesToDevice
 *   grt_update_meshes             updateInstanceTransforms (refit, no rebuild) src/GaussianTracer.cpp:711-794
 *   grt_render                    render(): param upload + optixLaunch of  src/GaussianTracer.cpp:508-538,
 *                                 raygen/anyhit/closesthit/miss              shaders/tracer.cu:17-187
 *   grt_render_tiles              (new) screen-tile sharding for N GPUs    SURVEY.md §8(e)
 *   grt_assemble_tiles            (new) rank 0's un-permute of the gathered tiles   SURVEY.md §8(e)
 *   grt_render_rays               (new) ray-buffer input for parity tests  SURVEY.md §7 hard part 1
 *   grt_sync                      CUDA_SYNC_CHECK()                        src/GaussianTracer.cpp:537
 *   grt_host_*                    host-side pieces the facade shares with ctypes users:
 *                                 GaussianData::parse (src/GaussianData.cpp:25-132), Camera::UVWFrame
 *                                 (src/Camera.cpp:3-13), grt_host_primitive_* / grt_host_obj_* = Primitives
 *                                 (src/geometry/Primitives.cpp:6-216)
 *
 * Ownership: the library owns every device allocation it makes; the caller owns output buffers;
 * host input arrays are borrowed for the duration of the call only.  A context is bound to one
 * device and is not re-entrant; distinct contexts may be driven from distinct threads/processes.
 */
#ifndef GRT_H
#define GRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRT_API __attribute__((visibility("default")))

typedef struct grt_ctx grt_ctx;

typedef enum {
    GRT_OK = 0,
    GRT_ERR_INVALID = -1,   /* bad argument / call order */
    GRT_ERR_HIP = -2,       /* a HIP runtime call failed */
    GRT_ERR_NO_DEVICE = -3, /* no usable GPU: the product path has no CPU fallback */
    GRT_ERR_IO = -4,        /* file could not be read / parsed */
    GRT_ERR_LIMIT = -5      /* scene exceeds a built-in limit (e.g. BVH height) */
} grt_status;

/* enum MeshType — src/Parameters.h:78-83 */
enum { GRT_MIRROR = 0, GRT_NORMAL = 1, GRT_GLASS = 2 };

/* Activated Gaussians, one host array per attribute (reference AoS GaussianParticle,
 * src/GaussianData.h:12-20).  quat is (w,x,y,z), already normalised; scale and opacity are
 * already exp()/sigmoid()-activated exactly as src/GaussianData.cpp:97-131 does on the host. */
typedef struct {
    const float* pos;     /* [n][3]  */
    const float* scale;   /* [n][3]  */
    const float* quat;    /* [n][4]  */
    const float* opacity; /* [n]     */
    const float* sh;      /* [n][16][3] : sh[k] = (f_rest_{k-1}, f_rest_{14+k}, f_rest_{29+k}), sh[0] = f_dc */
} grt_gaussians;

/* Triangle mesh already placed in world space by the caller (the facade applies
 * Primitive::transform): verts[nv][3]; normals[nv][3] pre-multiplied by mat3(transform)
 * (src/GaussianTracer.cpp:659-662); faces[nf][3]. */
typedef struct {
    const float* verts;
    const float* normals;
    uint32_t nv;
    const uint32_t* faces;
    uint32_t nf;
} grt_mesh;

/* struct Params — src/Parameters.h:42-74, minus the OptiX handles / device pointers the library
 * now owns (handle, d_particles, mesh_handle, d_meshes, traceState, output_buffer). */
typedef struct {
    uint32_t width, height;
    uint32_t sh_degree_max;
    float eye[3], U[3], V[3], W[3];
    float t_min, t_max, minTransmittance, alpha_min;
    int32_t mode_fisheye;
    int32_t type;         /* GRT_MIRROR / GRT_NORMAL / GRT_GLASS */
    uint32_t max_bounces; /* reference constant MAX_BOUNCES = 32, shaders/tracer.cuh:13 */
} grt_params;

typedef struct {
    uint64_t rays;        /* rays spawned (pixels; fisheye: r <= 1 only) */
    uint64_t segments;    /* Gaussian trace() calls (primary + secondary segments) */
    uint64_t hit_evals;   /* k-buffer entries consumed with T > minT (entry and exit both count) */
    uint64_t rounds;      /* k-buffer traversal rounds (traceGPs equivalents) */
    uint64_t node_visits; /* BVH node box tests by live rays (Gaussian BVH + mesh BVH) */
    uint64_t proxy_tests; /* exact icosahedron-slab tests executed */
    uint64_t rec_fetches; /* BVH node / proxy record bytes fetched by the wave-cooperative kernels, in 16-B units, at
                             the granularity they are loaded (one scalar load per wave): streaming kernel — a 4-wide
                             node = 8, a proxy record + its eye record = 5; round-based wave kernel — a 64-B record = 4 */
    uint64_t stall_exits; /* rays a wave-per-tile kernel (tile or streaming) gave up on with transmittance left: two passes in
                             a row composited nothing, or the step watchdog / stack guard fired (must be 0: a non-zero value
                             means a pixel is missing hits).  Counted with GRT_OPT_COUNTERS; the same events set the sticky
                             error word in EVERY kernel variant: grt_sync / grt_get_counters then return GRT_ERR_LIMIT */
} grt_counters;

typedef struct {
    uint64_t n_particles;   /* uploaded */
    uint64_t n_proxies;     /* hittable particles (opacity > alpha_min) */
    uint32_t n_nodes;       /* internal nodes of the Gaussian LBVH */
    uint32_t height;        /* LBVH height (levels of internal nodes) */
    uint32_t mesh_faces;
    uint32_t mesh_height;
    float build_ms;         /* device time of the last grt_build_bvh */
    float mesh_update_ms;   /* device time of the last grt_set_meshes (build) / grt_update_meshes (refit) */
    float scene_lo[3], scene_hi[3];
    uint64_t n_primitives;  /* leaves of the Gaussian LBVH: the hittable particles, large anisotropic ones as several pieces
                               (GRT_OPT_SPLIT) */
} grt_bvh_info;

typedef struct {
    uint64_t scene_bytes;         /* device memory of the scene this context renders (shared by a context and its views) */
    uint64_t slot_bytes;          /* device memory of this frame slot: eye records, overflow pool, feedback, wavefront queues,
                                     the backward pass's gradient buffers */
    uint64_t overflow_pool_bytes; /* of which: the tile kernel's pool of window-overflow bags */
    uint32_t overflow_chunks;     /* chunks (32 KiB: 32 entries x 64 rays; a tile takes up to three) in that pool */
    uint32_t overflow_demand;     /* the demand the pool follows: median of what the last eight frames read back asked for */
    uint64_t alpha_cull_bytes;    /* device memory of the scene's alpha-radius box array (GRT_OPT_ALPHA_CULL), 32 B per primitive of the
                                     Gaussian BVH; NOT part of scene_bytes, which keeps counting what it has always counted */
} grt_memory_info;

enum { GRT_OPT_COUNTERS = 1 /* 1: use the instrumented kernel and fill grt_counters.  A counted frame runs the reference's full event
                               stream: hit_evals counts every consumed icosahedron event, those with alpha <= alpha_min included.
                               An uncounted camera-ray frame of the tile kernel skips the particles none of a tile's rays passes
                               inside the alpha sphere (response x opacity = alpha_min): events that change nothing.  The pixels
                               are the same bytes either way; counted frames are never the timed ones */,
       GRT_OPT_KERNEL = 2   /* 0 = auto: camera-ray frames on the tile kernel (csrc/grt_tile.h: BVH culling per child box
                               against the tile frustum; also stage 2 of the wavefront pipeline of mesh frames) — or on the
                               streaming kernel when the BVH was built with GRT_OPT_LEAF_MAX > 4; ray buffers on the per-lane kernel.
                               1 = per-lane kernel everywhere, 2 = round-based wave kernel for camera rays without meshes
                               (per-lane otherwise), 3 = streaming kernel, 4 = its 32-slot variant everywhere (testing),
                               5 = same as 0 */,
       GRT_OPT_LEAF_MAX = 3 /* max primitives per BVH leaf, 1..8 (default 4); applies to the next build */,
       GRT_OPT_SWIZZLE = 4  /* XCD-aware launch order: runs of value 16x16 screen blocks (4 x value 8x8 tiles of the
                               streaming kernel) go to one XCD, i.e. one L2 (0 = identity; default 2) */,
       GRT_OPT_FEEDBACK = 5 /* 1 (default): launch the scheduling units (8x8 tiles for the streaming kernel, 16x16 blocks
                               for the others) heaviest-first using the previous frame's per-unit cost; in launches of
                               <= 3072 blocks (a multi-GPU rank's share of a frame) additionally run the heaviest tiles on
                               the 32-slot big-window kernel on a second stream (shorter critical path).
                               3: heaviest-first only.  5: big-window split always.  0: off */,
       GRT_OPT_HEAVY_THRESHOLD_X2 = 6 /* a unit is heavy when its cost exceeds value/2 x the median cost (default 4) */,
       GRT_OPT_HEAVY_CAP_DIV = 7      /* at most 1/value of the units go to the big-window kernel (default 8) */,
       /* tile kernel (GRT_OPT_KERNEL = 5) tuning; pixels never depend on these */
       GRT_OPT_TILE_READY_MIN = 8     /* lanes that must hold a final event for a compositing sweep to start or go on (fewer when few lanes still want anything), 1..64 (24) */,
       GRT_OPT_TILE_BAND = 9          /* particles within value/1024 of the front distance are tested as one batch (64) */,
       GRT_OPT_TILE_LOOKAHEAD = 10    /* nodes within value/1024 of the nearest node's distance are expanded together (64) */,
       GRT_OPT_TILE_RESERVE = 11      /* with fewer than value free frontier slots the nearest leaf ranges are tested first (-1 = default: 16, trees with pieces 24) */,
       GRT_OPT_TILE_PRIO_DIV = 12     /* the heaviest 1/value of the tiles (by last frame's cost) run at raised wave priority; 0 = off */,
       GRT_OPT_COST_RADIUS = 13       /* scheduling feedback under a moving camera: a tile's cost is the largest of last frame's costs
                                         within value tiles of it (default 4; 0 = the tile's own cost) */,
       GRT_OPT_SIZE_CLASSES = 14      /* 1 (default): proxies much larger than average get subtrees of their own in the Gaussian LBVH
                                         (size class in the top Morton bits); 0: plain Morton order.  Per context; next build */,
       GRT_OPT_COLD_ESTIMATE = 15     /* 1: a frame with no previous-frame costs (first frame, new size) launches its tiles in the
                                         order of the number of particle centres projecting into them; 2 (default): and the tiles whose
                                         estimate exceeds GRT_OPT_COLD_PARTS_PCT % of the largest (and the load condition of the part
                                         waves) run as four part waves already in that frame; 0: screen order */,
       GRT_OPT_BUNDLE_ROUNDS = 16     /* mesh frames on the tile kernel: how many bounce iterations trace their Gaussian segment wave-
                                         cooperatively (the bounced rays of an 8x8 tile as one bundle) before the per-lane kernel
                                         finishes whatever still bounces; 0..4, default 2.  Same image for every value */,
       GRT_OPT_BUNDLE_BUDGET = 17     /* work (steps + particles fetched + 2 x exact tests) a bundle may take before it is given up and its
                                         rays are traced one per wave (a bundle whose rays have spread too far to share work); default
                                         896, doubled for GRT_GLASS.  Same image for every value */,
       GRT_OPT_SINGLE_LOOKAHEAD = 18  /* one-ray-per-wave mode: as GRT_OPT_TILE_LOOKAHEAD (default 256 = 25 %) */,
       GRT_OPT_SINGLE_BAND = 19       /* one-ray-per-wave mode: as GRT_OPT_TILE_BAND (default 256 = 25 %) */,
       GRT_OPT_SPLIT = 24             /* spatial splits: a proxy much longer than the typical one whose world box is mostly empty (a needle or
                                         sheet that is not axis-aligned) enters the LBVH as up to 512 pieces, each with the box of its cell;
                                         value = piece length in quarters of the geometric-mean proxy diagonal (8 = 2 x; 0 = off).  Default -1:
                                         the length follows the scene, by the primitives per proxy that cutting at 8 would give: under 1.02 no
                                         pieces at all (the benchmark scenes), under 1.25 -> 6 (mildly anisotropic proxies, a few times longer
                                         than thick: a trained scene), under 1.5 -> 8, under 1.7 -> 10, under 2.2 -> 12, else 16 (scene-sized
                                         needles and sheets, where every piece re-tests its particle).  Pure acceleration structure: same hits,
                                         same pixels.  Per context; next build */,
       GRT_OPT_TILE_BAND_ABS = 25     /* trees with pieces: absolute floor of the tile kernel's leaf band and node look-ahead, in 1/64 of the
                                         geometric-mean proxy diagonal (default 512 = 8 x; 0 = relative bands only).  Scheduling only */,
       /* testing knobs (frames never change; speed and the failure signal do) */
       GRT_OPT_OVF_CHUNKS = 21        /* tile kernel's pool of window-overflow bags: 0 (default) = sized from the demand of the
                                         frames before (1.25 x the median of eight); n > 0: exactly n chunks of 32 KiB; < 0: no pool (every overflow costs another pass) */,
       GRT_OPT_OVF_ENTRIES = 22       /* per-lane capacity of a bag actually used, 1..96 (0 = default 96) */,
       GRT_OPT_MAX_ITERS = 23         /* step watchdog of the tile kernel (0 = default 2^21): a tile over it gives up on its rays
                                         and sets the sticky error word */,
       GRT_OPT_LANE_BUDGET = 20       /* whatever still bounces after the bundle rounds finishes on the per-lane traversal; a Gaussian
                                         segment over this many iterations there sends its ray to the one-ray-per-wave mode, which
                                         finishes it (default 128).  Same image for every value */,
       GRT_OPT_TILE_PARTS4_PCT = 27   /* tile kernel, camera rays (mesh frames: their primary stage, GRT_OPT_MESH_PARTS): an 8x8 tile whose cost in the previous frame exceeded
                                         value % of the heaviest tile's — and GRT_OPT_TILE_PARTS_LOAD_PCT % of the launch's total cost per
                                         resident wave — is launched as FOUR waves of 4x4 pixels (a quarter of the rays each, a narrower
                                         frustum).  A frame takes at least its longest tile; a frame bound by its total work (1080p on
                                         one GPU) splits nothing.  Default 60; 0 = never.  Pixels never depend on it */,
       GRT_OPT_TILE_PARTS2_PCT = 26   /* ... above value % of the heaviest (and below the four-way threshold): TWO waves of 4x8 pixels.
                                         Default 0 = never (half a heavy tile takes as long as the whole) */,
       GRT_OPT_TILE_PARTS_LOAD_PCT = 28, /* see GRT_OPT_TILE_PARTS4_PCT (default 75; 0 = no such condition) */
       GRT_OPT_MESH_PARTS = 29          /* 1 (default): the part waves also split the heavy tiles of a MESH frame's primary stage
                                           (each part queues its own chunk of continuation rays); 0: camera-ray frames without
                                           meshes only, as before round 4's last change */,
       GRT_OPT_ORDER_MULTI_MIN = 30     /* (testing) launches of value tiles and more have their launch order made by several workgroups in
                                           four short kernels instead of one workgroup (default 16384: from 1080p on; behind every frame of
                                           a moving camera: 54 -> ~25 us at 1080p, 249 -> ~30 us at 4K).  Same order either way */,
       GRT_OPT_STATIC_SHARP = 31        /* 1 (default): once a view has stood still for two frames its launch order is made from the tiles' own
                                           costs instead of the map dilated by GRT_OPT_COST_RADIUS (which is for a camera that moves); 0: always
                                           dilated, as before */,
       GRT_OPT_COLD_PARTS_PCT = 32,     /* see GRT_OPT_COLD_ESTIMATE (default 40) */
       GRT_OPT_QUAD_PARTS = 33          /* 1 (default): the four-way parts of camera-ray frames without meshes or pieces run on the QUAD kernel
                                           (one 4x4 quadrant per wave, lanes = rays x slots: four survivors of a leaf step are slab-tested
                                           at once, one per slot, a ray's pending events are the pool of its four windows), launched beside
                                           the camera-ray kernel — in launches that their parts bound (up to 12 288 tiles: a small frame, a
                                           rank's share of a frame), with a four-way threshold scaled down to half for launches of one tile per resident
                                           wave and fewer; 2: whatever the size (testing); > 2: and at most that many parts (testing); 0: part
                                           waves of the camera-ray kernel with 16 of 64 lanes in use (round 4).  Same pixels either way */,
       GRT_OPT_OVF_CLASSES = 34         /* 1 (default): a tile STARTS in one, two or three 32-entry chunks of the overflow pool by how deep
                                           its bags got in the frame before (one when nothing is known of it) and moves to three fresh
                                           ones when it outgrows them (the frame slot's memory: 1.30 -> 0.63 GB on the 1080p benchmark
                                           frame under a standing camera); 0: three for every tile that overflows (round 4).  Same
                                           pixels either way */,
       GRT_OPT_BVH_ROTATIONS = 35       /* applies to the next build of the Gaussian BVH (refused on a view): bottom-up sweeps of tree rotations
                                           behind the LBVH build — what the reference asks OptiX for with PREFER_FAST_TRACE,
                                           src/GaussianTracer.cpp:360.  -1 (default): one sweep for trees that hold pieces of split proxies,
                                           none otherwise; 0: none; n (<= 8): n sweeps on any tree.  Levels and the reported height
                                           (grt_bvh_info) are re-derived behind every sweep.  Culling structure only: same pixels */,
       GRT_OPT_BUNDLE_PREDICT = 36      /* mesh frames on the tile kernel.  1 (default): an 8x8 tile whose bounced rays gave up as a bundle
                                           (GRT_OPT_BUNDLE_BUDGET) is remembered FOR THE VIEW it happened under; while that view stands, its
                                           continuation rays go one per wave at once, on a list that the one-ray-per-wave kernel works off
                                           BESIDE the bundle kernel (second stream) instead of behind it, and the bundle that would be thrown
                                           away is not run.  A frame with other parameters (a camera that moves), another scene, frame
                                           geometry or budget uses no verdicts: every tile is tried as a bundle, as in round 5.  0: always
                                           so.  Same rays through the same two kernels: same pixels */,
       GRT_OPT_MESH_PRIMARY_WAVE = 37   /* mesh frames, stage 1 (camera ray -> closest mesh hit -> closest-hit shading: traceMesh of
                                           shaders/tracer.cuh:266-287, shaders/tracer.cu:112-122,155-187).  0: every lane walks the mesh
                                           tree alone, in a kernel of its own in front of the Gaussian stage (rounds 1-5); 1: the 64 rays
                                           of an 8x8 tile walk it TOGETHER (nodes and triangles by scalar loads, a child is entered when
                                           any lane wants it, one stack per wave), still a kernel of its own; 2 (default): that walk runs
                                           at the head of the tile kernel's primary stage — no launch, no 48-B record per pixel (other
                                           pipelines, and mesh trees too deep for the tile kernel's stack: as 1).  The same hit records bit for
                                           bit */,
       GRT_OPT_SPLIT_VOL_PCT = 38       /* spatial splits: a proxy longer than the piece length is cut when the boxes of its cells together hold
                                           less than value % of its own box's volume (default 400: practically always; rounds 3-5: 50).  Per context;
                                           next build.  Same pixels */,
       GRT_OPT_BWD_PLAIN_ATOMICS = 39   /* (testing) backward pass: 1 = every lane adds its own 14 values per event to its particle's row of the
                                           gradient buffer; 0 (default): lanes of a wave that composite the same particle in the same slot
                                           of their k-buffers reduce over the wave first.  Same gradients within the float32 tolerance */,
       GRT_OPT_REFIT_MAX_AREA_PCT = 40  /* grt_update_gaussians_device with GRT_UPDATE_AUTO: a refit that leaves grt_update_info::area_ratio above
                                           value / 100 is followed by a rebuild in the same call (default 200: DESIGN.md 5.9; 0 = never).  A forced
                                           GRT_UPDATE_REFIT never rebuilds.  Refused on a view.  Culling structure only: same pixels */,
       GRT_OPT_ALPHA_CULL = 41          /* 1 (default): the tile kernel's leaf step of an uncounted camera-ray frame (aux frames and the quad
                                           kernel's parts included) culls a particle with the bounding sphere of its ALPHA ellipsoid
                                           (response x opacity = alpha_min) instead of its proxy's circumsphere: the particles it no longer
                                           fetches are those whose trip ended at the pre-test.  A second box array of 32 B per primitive
                                           (grt_memory_info::alpha_cull_bytes).  Counted frames, bundles, single rays and frames whose
                                           alpha_min lies below the scene's keep the circumsphere; 0: so does every frame.  Refused on
                                           nothing; pixels never depend on it */ };

/* ---- context ---- */
GRT_API int grt_create(grt_ctx** out, int device);
/* A view: a frame slot of its own (stream, eye records, scheduling feedback, overflow pool, queues, counters, error
 * word) that renders `scene`'s Gaussians, BVHs and meshes.  Scene calls (grt_upload_gaussians, grt_build_bvh,
 * grt_update_gaussians_device, grt_set_meshes, grt_update_meshes, GRT_OPT_LEAF_MAX / GRT_OPT_SIZE_CLASSES) are refused on a view.  Destroying a
 * scene with live views is deferred until the last view is destroyed. */
GRT_API int grt_create_view(grt_ctx* scene, grt_ctx** out);
GRT_API void grt_destroy(grt_ctx* ctx);
GRT_API const char* grt_last_error(const grt_ctx* ctx); /* ctx may be NULL: last error of grt_create */
GRT_API int grt_set_option(grt_ctx* ctx, int option, int value);

/* ---- scene ---- */
GRT_API int grt_upload_gaussians(grt_ctx* ctx, const grt_gaussians* host, uint64_t n);
GRT_API int grt_build_bvh(grt_ctx* ctx, float alpha_min);
/* The scene of a training step: the five attribute arrays from DEVICE memory (the layout and meaning of grt_gaussians: activated
 * values, quat normalised; contiguous float32), and the Gaussian BVH brought up to date.  The call synchronises the device, so its
 * reads are ordered after everything queued before it — on `stream` (a hipStream_t, NULL = the context's own; the convention of
 * grt_render's stream argument) as on any other — and the caller may overwrite its arrays as soon as it returns: the library keeps
 * copies of its own (the backward pass reads them by original id).  n has the limit of grt_upload_gaussians.  A pointer that is not
 * device memory of the context's GPU, a NULL pointer with n > 0, and a view are refused with GRT_ERR_INVALID.
 *   GRT_UPDATE_REBUILD  grt_upload_gaussians + grt_build_bvh from device memory: the same tree, array for array (the build is
 *                       deterministic).
 *   GRT_UPDATE_REFIT    keeps the sorted order, the hierarchy and the leaf ranges of the tree in hand and recomputes, in this
 *                       sequence: the primitive boxes; the binary nodes' boxes, level by level (the levels are derived on the
 *                       first refit of a tree); the per-primitive boxes, the 4-wide and per-child views and the proxy records.
 *                       A piece of a split proxy keeps its particle and its cell (any grid partitions the proxy-local box: a
 *                       stale piece length costs speed, never hits); the cell's box follows the particle's new values.
 *                       Possible when a tree is built, n is unchanged, the build options (GRT_OPT_LEAF_MAX, _SIZE_CLASSES,
 *                       _SPLIT, _SPLIT_VOL_PCT, _BVH_ROTATIONS) are those of the last build, and the set of particles in the
 *                       tree — hittable (opacity > alpha_min) and finite — is unchanged (decided on the device).  Otherwise:
 *                       GRT_ERR_INVALID, the reason in grt_last_error, the scene left as it was before the call.
 *   GRT_UPDATE_AUTO     refits when possible, rebuilds otherwise — and rebuilds behind a refit that left area_ratio above
 *                       GRT_OPT_REFIT_MAX_AREA_PCT (an unrelated scene that happens to have the same n).
 * The proxy half-width s = sqrtf(2 logf(opacity / alpha_min)) stays the HOST libm's, as in grt_build_bvh: the opacities are read
 * back (4 B per particle), s is computed on at most 16 threads and sent up.  An update with the n of the last one allocates and
 * frees no scene memory on the refit path.  Pixels never depend on the mode: the tree only culls. */
enum { GRT_UPDATE_AUTO = 0, GRT_UPDATE_REFIT = 1, GRT_UPDATE_REBUILD = 2 };
enum { GRT_UPDATE_REASON_NONE = 0, GRT_UPDATE_REASON_FIRST_BUILD = 1, GRT_UPDATE_REASON_N_CHANGED = 2,
       GRT_UPDATE_REASON_SET_CHANGED = 3 /* the hittable, finite particles are not those in the tree */,
       GRT_UPDATE_REASON_OPTION_CHANGED = 4, GRT_UPDATE_REASON_AREA = 5 };
typedef struct {
    uint32_t mode_used;   /* GRT_UPDATE_REFIT or GRT_UPDATE_REBUILD: what was done */
    uint32_t reason;      /* GRT_UPDATE_REASON_*: why GRT_UPDATE_AUTO rebuilt (0 after a refit and after a rebuild that was asked for) */
    float    device_ms;   /* device time of the update on the context's stream, from behind the upload of s to its last kernel (the
                             one-word readback of the set test included; a rebuild: the copies + grt_bvh_info::build_ms) */
    float    area_ratio;  /* sum over the binary nodes of their two child boxes' half-areas, now / at the last BUILD (1.0 after a
                             build and for a tree without internal nodes) */
} grt_update_info;
GRT_API int grt_update_gaussians_device(grt_ctx* ctx, const grt_gaussians* dev, uint64_t n, float alpha_min, int mode,
                                        void* stream, grt_update_info* out);
GRT_API int grt_set_meshes(grt_ctx* ctx, const grt_mesh* meshes, uint32_t n_meshes);
/* The same meshes, moved: new positions / normals for the topology of the last grt_set_meshes (same nv, nf per
 * mesh).  The mesh LBVH keeps its hierarchy and re-fits its boxes (reference: updateInstanceTransforms rebuilds GAS +
 * IAS on every gizmo frame and leaks the old ones, src/GaussianTracer.cpp:711-794).  GRT_ERR_INVALID when counts differ. */
GRT_API int grt_update_meshes(grt_ctx* ctx, const grt_mesh* meshes, uint32_t n_meshes);
GRT_API int grt_get_bvh_info(const grt_ctx* ctx, grt_bvh_info* out);
GRT_API int grt_get_memory_info(const grt_ctx* ctx, grt_memory_info* out);
/* (testing) depth of the Gaussian LBVH walked on the host over a copy of its node records, in levels of internal nodes: must not
 * exceed grt_bvh_info::height, which sizes the kernels' traversal stacks (synchronises the device; ~0.1 s per million nodes). */
GRT_API int grt_debug_bvh_depth(grt_ctx* ctx, uint32_t* out_depth);
/* (testing) A copy of a built tree, for checkers that restate its invariants (tests/bvh_check.py).  Two calls: with every buffer
 * NULL the counts are filled in; then every non-NULL buffer receives its array (sized by those counts).  Synchronises the device.
 * which = 0: the Gaussian LBVH, rec = the proxy records [n_prims][16]; which = 1: the mesh LBVH, rec = the triangles [n_prims][12].
 * n_nodes = 0 when the root is a leaf range; qnodes and pbox exist for the Gaussian tree only (n_qnodes = n_pbox = 0 otherwise). */
typedef struct {
    uint32_t n_prims, n_nodes, height, root_ref, leaf_max, has_pieces;
    uint32_t n_qnodes, n_pbox, wide, rec_floats; /* wide = children per qnodes record; rec_floats = floats per record (16 or 12) */
    float* nodes;     /* [n_nodes][16]: the binary records, child refs as raw bits in floats 12, 13 */
    float* wnodes;    /* [n_nodes][32]: the 4-wide records */
    float* qnodes;    /* [n_qnodes][wide][8]: the per-child records of the tile kernel */
    float* pbox;      /* [n_pbox][8]: (lo.xyz, 0)(hi.xyz, radius) of every sorted primitive */
    uint32_t* order;  /* [n_prims]: sorted position -> input primitive (piece, particle or face) */
    float* rec;       /* [n_prims][rec_floats] */
} grt_debug_tree;
GRT_API int grt_debug_copy_tree(grt_ctx* ctx, int which, grt_debug_tree* out);
/* (testing) The launch-order kernels on arrays the CALLER owns (device pointers), through the very host functions a frame calls them
 * by, for checkers that restate their contract (tests/order_check.py).  Asynchronous on the context's own stream; nothing of the frame
 * slot's state is read or written.  op selects the function:
 *   GRT_DEBUG_ORDER_PARTS      order_units_with_parts: d_cost (orders the units), d_cost_raw (their own cost words; may be d_cost itself),
 *                              n, extra_cap (0xFFFFFFFF: the library's own room for n units), pct2 / pct4 / pct_load, resident_waves,
 *                              multi_min, bag_classes, d_zero (NULL, or the array to zero: d_cost_raw, which may be d_cost too), d_scratch
 *                              (NULL, or grt_debug_order_scratch_bytes() of zeroed device memory) -> d_order [n + extra_cap + 3].
 *                              quad_pct4 != 0: pct4 is taken as GRT_OPT_TILE_PARTS4_PCT and scaled as a quad-parts launch of n units scales it.
 *                              out: extra_cap_used, pct4_used
 *   GRT_DEBUG_ORDER_PLAIN      order_units_by_cost: d_cost, n, heavy_cap, thr_x2, d_out (NULL, or one word: the heavy units), d_zero
 *                              (NULL, or the array to zero) -> d_order [n]
 *   GRT_DEBUG_ORDER_QUAD_LIST  quad_part_list: d_order [n] (entries, padding included; re-coded in place), cap -> d_out [min(cap, 4096)],
 *                              d_count [1]
 *   GRT_DEBUG_ORDER_DILATE     dilate_unit_costs: d_cost [nbx nby 4], nbx, nby, radius -> d_out [nbx nby 4] */
enum { GRT_DEBUG_ORDER_PARTS = 0, GRT_DEBUG_ORDER_PLAIN = 1, GRT_DEBUG_ORDER_QUAD_LIST = 2, GRT_DEBUG_ORDER_DILATE = 3 };
typedef struct {
    uint32_t op, n;
    const uint32_t* d_cost;
    const uint32_t* d_cost_raw;
    uint32_t* d_order;
    uint32_t* d_zero;
    uint32_t* d_scratch;
    uint32_t* d_out;
    uint32_t* d_count;
    uint32_t extra_cap, pct2, pct4, pct_load, resident_waves, multi_min, bag_classes, quad_pct4;
    uint32_t heavy_cap, thr_x2;
    uint32_t cap;
    uint32_t nbx, nby;
    int32_t  radius;
    uint32_t extra_cap_used, pct4_used; /* out (GRT_DEBUG_ORDER_PARTS) */
} grt_debug_order;
GRT_API int grt_debug_order_units(grt_ctx* ctx, grt_debug_order* io);
GRT_API uint32_t grt_debug_order_scratch_bytes(void);
/* (testing) The cold frame's estimate (particle centres per 8x8 tile) of the uploaded scene into the caller's zeroed d_cost [n_units],
 * with the launch geometry of grt_render (tile_w = 0: the window x0, y0, x1, y1) or of grt_render_tiles (tile_w, tile_h, x0 = first
 * tile, y0 = tile stride, x1 = number of tiles), every stride-th particle.  n_units must be the geometry's: 4 per 16x16 block.
 * Asynchronous on the context's own stream; the frame slot is not touched. */
GRT_API int grt_debug_estimate_costs(grt_ctx* ctx, const grt_params* p, uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0,
                                     uint32_t x1, uint32_t y1, uint32_t stride, uint32_t* d_cost, uint32_t n_units);
/* (testing) What the frame slot's scheduling state holds right now, copied to host buffers behind a synchronisation of the device.  Two
 * calls, as grt_debug_copy_tree: with every buffer NULL the counts are filled in; then every non-NULL buffer receives its array.
 * n_order = order_launch + 3 (the entries and the three diagnostic words) or n_units (bare entries, order_launch = 0), 0 when
 * order_valid = 0; n_quad = the quad list's count word (0 when quad_valid = 0); cost = the n_units cost words. */
typedef struct {
    uint32_t n_units, order_launch, order_valid, order_classes, quad_valid, n_order, n_quad;
    uint32_t* order; /* [n_order] */
    uint32_t* quad;  /* [n_quad] */
    uint32_t* cost;  /* [n_units] */
} grt_debug_schedule;
GRT_API int grt_debug_copy_schedule(grt_ctx* ctx, grt_debug_schedule* out);

/* ---- render (all asynchronous on `stream`, a hipStream_t; NULL = the context's own stream) ----
 * d_rgb8 : device uchar3 frame, row-major y*width+x (shaders/tracer.cuh:484-496), may be NULL
 * d_rgbf : device float3 frame holding accumColor before clamp/quantise, may be NULL
 * Window [x0,x1) x [y0,y1) restricts which pixels are traced and written (0,0,width,height = all). */
GRT_API int grt_render(grt_ctx* ctx, const grt_params* p, uint8_t* d_rgb8, float* d_rgbf, uint32_t x0, uint32_t y0,
                       uint32_t x1, uint32_t y1, void* stream);
/* Tiles are numbered row-major over the ceil(width/tile_w) x ceil(height/tile_h) grid.  Renders
 * tiles first_tile + j*tile_stride (j = 0..n_tiles-1) into COMPACT buffers [j][tile_h][tile_w][3];
 * pixels of a border tile that fall outside the frame are written as 0. */
GRT_API int grt_render_tiles(grt_ctx* ctx, const grt_params* p, uint8_t* d_rgb8, float* d_rgbf, uint32_t tile_w,
                             uint32_t tile_h, uint32_t first_tile, uint32_t tile_stride, uint32_t n_tiles,
                             void* stream);
/* Rank 0 of an N-rank frame ("rank 0 un-permutes tiles with a trivial copy kernel"): d_gathered holds the
 * ranks' compact buffers back to back, [world][max_cnt][tile_h][tile_w][3] (tile t of the grid = tile t / world of rank
 * t % world, as grt_render_tiles with first_tile = rank, tile_stride = world writes them); d_rgb8 receives the frame. */
GRT_API int grt_assemble_tiles(grt_ctx* ctx, const uint8_t* d_gathered, uint32_t world, uint32_t max_cnt, uint32_t tile_w,
                               uint32_t tile_h, uint32_t width, uint32_t height, uint8_t* d_rgb8, void* stream);
/* d_rays[n][6] = origin, direction (device); d_rgbf[n][3] */
GRT_API int grt_render_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, float* d_rgbf,
                            void* stream);
/* ---- aux outputs: per-pixel (per-ray) opacity, expected depth and hit count beside colour ----
 * What 3DGRT-style renderers return as pred_opacity / pred_dist / hits_count.  Each array holds one value per pixel, row-major
 * y*width+x like d_rgbf (grt_render_rays_aux: one per ray).  Device pointers; each may be NULL.
 *   alpha  (float32) the reference's accumAlpha at the end of the raygen loop (shaders/tracer.cu:58-106; kept at :81 and :97,
 *          its input is the density trace() returns, shaders/tracer.cuh:372).  Without meshes: clamp(0 + (1 - T_final), 0, 1).
 *          Mesh frames: summed over the segments with the reference's own clamps (renderNormal's terminate adds alpha and 1 - alpha
 *          unclamped, shaders/tracer.cuh:417-428).
 *   depth  (float32) sum over the events composited in the ray's FIRST Gaussian segment — t_min to the first mesh hit, or to t_max
 *          when there is none — of (T_i alpha_i) t_i: t_i the event's distance as the k-buffer orders it (the entry or the exit
 *          face of the proxy: the hit.distance trace() folds into rayLastHitDistance, shaders/tracer.cuh:354; both events of a
 *          particle count), T_i the transmittance before the event, alpha_i its alpha.  Only events with alpha_min < alpha_i count
 *          (tracer.cuh:361), repeats of a split particle's pieces are dropped as for colour.  Evaluated as (T * alpha) * t in
 *          float32, before T is updated, and added in compositing order: the same bits on every kernel.  NOT normalised:
 *          depth / alpha is the mean distance, in world units for camera rays (unit directions) and in units of |d| for
 *          caller-supplied rays.  (Not the distance of the peak response: DESIGN.md 5.7.)
 *   count  (uint32) the number of terms of that sum.
 *   Fisheye pixels with r > 1 receive 0, 0, 0; pixels outside the window are not written (as for colour).
 * aux == NULL, or all three pointers NULL: exactly grt_render / grt_render_rays.  Either colour buffer may be NULL on an aux frame.
 * GRT_OPT_COUNTERS = 1 together with an aux output: GRT_ERR_INVALID.  Camera-ray frames without meshes run the tile kernel's aux
 * instantiation (four-way parts as part waves, no quad kernel); mesh frames, ray buffers, GRT_OPT_KERNEL 1-4 and trees the tile
 * kernel refuses run the per-lane aux kernel (mesh frames: the whole bounce loop per lane).  Colour is bit-identical to the plain
 * call's.  grt_render_tiles / multi-GPU frames have no aux outputs. */
typedef struct {
    float* alpha;
    float* depth;
    uint32_t* count;
} grt_aux_out;
GRT_API int grt_render_aux(grt_ctx* ctx, const grt_params* p, uint8_t* d_rgb8, float* d_rgbf, const grt_aux_out* aux,
                           uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_render_rays_aux(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, float* d_rgbf,
                                const grt_aux_out* aux, void* stream);
/* ---- backward pass: gradients of a loss on the frame with respect to the Gaussians (Gaussian-only frames) ----
 * The function that is differentiated is what a ray without meshes renders (shaders/tracer.cu:68-82, 101; trace(),
 * shaders/tracer.cuh:328-373):
 *     rad   = sum_i T_i alpha_i L_i        T_1 = 1, T_{i+1} = T_i (1 - alpha_i)
 *     A     = clamp(1 - T_end, 0, 1)       (grt_aux_out::alpha)
 *     rgbf  = rad * A                      (the frame's colour is radiance TIMES density: directLight = rad * alpha)
 * over the k-buffer's events i in key order (t, id, entry < exit): BOTH the entry and the exit event of a proxy are composited, with
 * the same alpha; repeats of a split particle's pieces are dropped; an event counts when alpha_min < alpha_i, where
 *     alpha_i = min(0.99, opacity r),  r = exp(-1/2 |p_g|^2),  p_g = A (mu - o - d_val d),  d_val = -(o_g.d_g) / max(1e-6, d_g.d_g),
 *     o_g = A (o - mu),  d_g = A d,  A = diag(1/s) R^T,  R = glm::mat3_cast(q) of the quaternion AS UPLOADED (no normalisation inside),
 *     L_i = max(0, 0.5 + sum_k Y_k(d/|d|) sh_k)  over the k < (sh_degree_max + 1)^2.
 * It is differentiated WITH ITS DISCRETE DECISIONS HELD FIXED: which events exist and their order, alpha_min < alpha, the 0.99 clamp
 * (zero gradient into opacity and geometry where it binds), max(L, 0) per channel (zero gradient into SH where it binds),
 * max(1e-6, .) (the denominator a constant where it binds; d_val minimises |p_g|^2, so p_g is differentiated at fixed d_val), where
 * the ray stops (T > minTransmittance).  With g_C = dloss/drgbf, g_A = dloss/dalpha (NULL = 0), g_rad = A g_C,
 * g_A' = g_A + g_C.rad, S_i = sum_{j>i} T_j alpha_j L_j:
 *     dloss/dalpha_i = g_rad.(T_i L_i - S_i / (1 - alpha_i)) + g_A' T_end / (1 - alpha_i)
 *     dloss/dL_i     = T_i alpha_i g_rad  (per channel, where L_i > 0)                      -> sh_k += Y_k * that
 *     dalpha_i/dopacity = r,  dalpha_i/dr = opacity  (when opacity r < 0.99);  dr/dp_g = -r p_g;  with v = mu - (o + d_val d), p_g = A v:
 *     d/dmu = A^T g_p,   d/ds_k = -g_p,k (R^T v)_k / s_k^2,   d/dR_jk = v_j g_p,k / s_k -> q through mat3_cast.
 * Gradients are with respect to the ACTIVATED attributes of grt_gaussians; the chain through exp / sigmoid / normalise is the
 * caller's.  Gradients with respect to rays / camera come from grt_backward_ex below; upstream gradients of depth / count are
 * not computed (a distance with gradients: grt_ray_depth_* / grt_backward_depth_* below).
 *   d_rgbf, d_alpha          what the forward call wrote for the same parameters and window (grt_render_aux: d_rgbf and aux.alpha);
 *                            required.  (The kernel re-derives rad and T_end with a sweep of its own: DESIGN.md 5.8.)
 *   d_grad_rgbf, d_grad_alpha  upstream gradients, laid out like d_rgbf / alpha; d_grad_alpha may be NULL (= 0).
 *   grads                    device arrays by ORIGINAL particle id like grt_gaussians: [n][3] [n][3] [n][4] [n] [n][16][3]; each may be
 *                            NULL (that group is not computed).  The gradients are ADDED to what the arrays hold: the caller zeroes them.
 * Fisheye pixels with r > 1 and pixels outside the window contribute nothing; so do rays the raygen loop does not trace
 * (|d| <= 0.1, max_bounces = 0).  Asynchronous on `stream` like grt_render; grt_last_kernel_ms reports the backward's device time.
 * Refused with GRT_ERR_INVALID (text in grt_last_error; the context stays usable): meshes set (mesh frames are differentiated by
 * grt_backward_mesh / grt_backward_rays_mesh below), GRT_OPT_COUNTERS = 1, no BVH, a NULL required pointer.  The sums are float atomics whose order of arrival differs from call
 * to call: gradients are NOT bitwise reproducible between calls (tests compare within a tolerance measured for float32 evaluation).
 * A frame rendered after a backward is bit-identical to one rendered before it.  Backward calls of one context share its gradient
 * buffer: a call on another stream than the last one's waits for that one.  The buffer — 64 B per particle, and 180 B more per
 * particle once a backward at SH degree >= 1 has run (244 MB at a million particles) — is allocated by the first backward and kept
 * until the context is destroyed; grt_memory_info::slot_bytes counts it. */
typedef struct {
    float* pos;
    float* scale;
    float* quat;
    float* opacity;
    float* sh;
} grt_gaussian_grads;
GRT_API int grt_backward(grt_ctx* ctx, const grt_params* p, const float* d_rgbf, const float* d_alpha, const float* d_grad_rgbf,
                         const float* d_grad_alpha, const grt_gaussian_grads* grads, uint32_t x0, uint32_t y0, uint32_t x1,
                         uint32_t y1, void* stream);
GRT_API int grt_backward_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const float* d_rgbf,
                              const float* d_alpha, const float* d_grad_rgbf, const float* d_grad_alpha,
                              const grt_gaussian_grads* grads, void* stream);
/* ---- backward pass, extended: gradients with respect to the rays as well (pose refinement, learned ray generators) ----
 * Same function, same rule: rgbf = rad * A, every discrete decision held fixed, p_g differentiated at fixed d_val (exact: d_val
 * minimises |p_g|^2; where max(1e-6, .) binds, the stated convention).  The reference has no backward pass; the function is its
 * raygen loop and trace() (shaders/tracer.cu:58-106, shaders/tracer.cuh:328-373), the response is computeResponse
 * (shaders/tracer.cuh:187-214: p_g depends on the ray through o and d only), the colour's direction is SHToRadiance's
 * (shaders/tracer.cuh:216-264).  With g_p, T_i, alpha_i, g_rad as above, for a ray (o, d), summed over its composited events i:
 *     m_i        = A_i^T g_p,i                       (the vector added to pos of particle i; zero where the 0.99 clamp binds)
 *     dloss/do   = - sum_i m_i
 *     dloss/dd   = - sum_i d_val,i m_i  +  (I - dn dn^T) g_dn / |d|
 *     g_dn       = sum_i sum_k (dY_k/dn)(dn) (sh_i,k . gL_i)
 *     dn         = d/|d|
 *     gL_i       = T_i alpha_i g_rad on the channels with L_i > 0
 *     Y_k        = the polynomials of SHToRadiance, differentiated as polynomials in x, y, z (degree 0: no colour term)
 * The hit geometry is a discrete decision and contributes nothing: which proxies are met, their key distances, t_min / t_max and
 * the raygen guard.  A ray that is not traced (fisheye r > 1, |d| <= 0.1, a NaN direction, max_bounces = 0) or whose upstream is
 * zero has gradient zero — exact zeros, never NaN.
 *   out->gaussians   as `grads` of grt_backward (ADDED to), or NULL; a structure of five NULLs counts as NULL.
 *   out->rays        [n][6] (grt_backward_rays_ex) or [h][w][6] (grt_backward_ex): (dloss/do, dloss/dd), WRITTEN, not added: every
 *                    ray of the buffer and every pixel of the window receives its six floats; pixels outside the window are not
 *                    written.  Camera frames: the gradient with respect to the eye and to the UNIT direction the raygen produced
 *                    (shaders/tracer.cuh:115-165), through the (I - dn dn^T) / |d| above; the chain to U, V, W is the caller's.
 *   out->rays NULL   exactly grt_backward / grt_backward_rays (which keep their own kernels).  Both NULL: GRT_ERR_INVALID.
 * Every refusal of grt_backward holds (meshes set among them: grt_backward_mesh / grt_backward_rays_mesh differentiate mesh frames,
 * with respect to the Gaussians only).  The rays' gradients have no atomic in their path — a ray belongs to one lane, its events
 * are summed in its own order and the six floats are stored once: two calls give them BIT FOR BIT, with and without the Gaussian
 * output, merged or plain atomics.  A call without Gaussian output touches no gradient buffer and allocates none
 * (grt_memory_info::slot_bytes is unchanged by it). */
typedef struct {
    const grt_gaussian_grads* gaussians; /* may be NULL */
    float* rays;                         /* [n][6] or [h][w][6]; may be NULL */
} grt_backward_out;
GRT_API int grt_backward_ex(grt_ctx* ctx, const grt_params* p, const float* d_rgbf, const float* d_alpha, const float* d_grad_rgbf,
                            const float* d_grad_alpha, const grt_backward_out* out, uint32_t x0, uint32_t y0, uint32_t x1,
                            uint32_t y1, void* stream);
GRT_API int grt_backward_rays_ex(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const float* d_rgbf,
                                 const float* d_alpha, const float* d_grad_rgbf, const float* d_grad_alpha,
                                 const grt_backward_out* out, void* stream);
/* ---- backward pass of mesh frames: mirror, glass and normal-shaded meshes in the scene, gradients with respect to the Gaussians ----
 * The function that is differentiated is the raygen loop (shaders/tracer.cu:58-106) with the meshes held fixed.  A ray runs
 * iterations s = 1..S.  Each has its own ray (o_s, d_s) — the camera's, or the one reflected / refracted at the last mesh hit —, its
 * segment [t_min, tmax_s] (to the next mesh hit, or t_max) and a state from the mesh hit: Gaussian pass (a hit that bounces), last
 * pass (a miss), terminate (GRT_NORMAL's hit).  THE TRANSMITTANCE RUNS ON ACROSS SEGMENTS (trace() starts at T = 1 - density, and the
 * loop carries density): a ray has ONE event list with one running T, T_1 = 1, T_{i+1} = T_i (1 - alpha_i), cut into segments.  With
 * alpha_i and L_i as above, on the ray of the event's own segment:
 *     R_s = sum_{i in s} T_i alpha_i L_i,   T_end,s = T behind segment s,   D_s = 1 - T_end,s  (cumulative),   A_0 = B_0 = 0
 *     Gaussian pass   C += R_s (1 - A_{s-1});          A_s = clamp(A_{s-1} + D_s, 0, 1);   B_s = clamp(B_{s-1} + D_s, 0, 1)
 *     last pass       C += R_s D_s (1 - B_{s-1});      A_s = clamp(A_{s-1} + D_s, 0, 1)
 *     terminate       C += R_s + ncol (1 - D_s);       A_s = A_{s-1} + D_s + (1 - D_s)        (ncol = (normal + 1) / 2)
 *     rgbf = C,  alpha = A_S.
 * Held fixed: everything grt_backward holds fixed, and the mesh hit, its normal and the next ray; the number of iterations
 * (max_bounces, the 1000-iteration timeout, |d| > 0.1); whether each clamp binds at each step (derivative 0 through a binding
 * clamp); T > minTransmittance at a segment's start.  With c_s = dC/dR_s — 1 - A_{s-1}, D_s (1 - B_{s-1}), 1 by state — and
 * gD_s = dloss/dD_s at fixed R, for event i of segment s:
 *     dloss/dalpha_i = c_s g_C.(T_i L_i)
 *                      - 1/(1 - alpha_i) sum_{k behind i, in any segment} c_s(k) g_C.(T_k alpha_k L_k)
 *                      + 1/(1 - alpha_i) sum_{j >= s} gD_j T_end,j
 *     dloss/dL_i     = c_s T_i alpha_i g_C   (per channel, where L_i > 0; Y_k at d_s / |d_s|)
 * and below alpha_i the chain of grt_backward with (o_s, d_s).  gD_s comes from the loop run backwards: a = g_A, b = 0, u^A_s / u^B_s
 * = 1 where the clamp of step s does not bind, then from s = S down
 *     last pass       gD_s = (g_C.R_s)(1 - B_{s-1}) + u^A_s a;   b -= (g_C.R_s) D_s;   a = u^A_s a
 *     Gaussian pass   gD_s = u^A_s a + u^B_s b;                  a = u^A_s a - g_C.R_s;   b = u^B_s b
 *     terminate       gD_s = -g_C.ncol.
 * In closed form (what the kernel evaluates, with nothing stored per iteration: DESIGN.md 5.11): every iteration but the last is a
 * Gaussian pass, and there B_s = A_s.  With e the last Gaussian pass before the clamp binds (all of them when it never does), sig =
 * -(g_C.R_s*) when it binds at Gaussian pass s*, else g_A (no last pass), u^A_S g_A - (g_C.R_S) D_S (last pass), and Q_s = sum_{k <= s}
 * g_C.R_k:  gD_s = sig - (Q_e - Q_s) for a Gaussian pass s <= e, 0 for one behind it.  Without meshes there is one last pass and
 * this is grt_backward's function and derivative.
 *   d_grad_rgbf, d_grad_alpha, grads, the window, the rays, stream    as for grt_backward / grt_backward_rays; gradients are ADDED, by
 *                            original particle id.  No forward outputs are passed: the kernel re-derives what it needs.
 * Refused as grt_backward refuses — GRT_OPT_COUNTERS = 1, no BVH, a NULL required pointer, a window outside the frame,
 * sh_degree_max > 3, t_min <= 0 — but for meshes; a view differentiates its scene's meshes.  Gradients with respect to rays or camera
 * through a bounce, to mesh vertices or normals, and upstream gradients of depth / count are not computed.  Float atomics, the
 * context's gradient buffer and its flush are grt_backward's (GRT_OPT_BWD_PLAIN_ATOMICS applies); grt_last_kernel_ms reports kernel
 * plus flush; a frame rendered after the call is bit-identical to one rendered before it. */
GRT_API int grt_backward_mesh(grt_ctx* ctx, const grt_params* p, const float* d_grad_rgbf, const float* d_grad_alpha /* may be NULL */,
                              const grt_gaussian_grads* grads, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_backward_rays_mesh(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const float* d_grad_rgbf,
                                   const float* d_grad_alpha, const grt_gaussian_grads* grads, void* stream);
/* ---- per-particle contribution statistics: which particles a set of rays touched, and how strongly (Gaussian-only frames) ----
 * What visibility masks, densification gates ("was seen") and pruning ("never seen", "never significant") read beside the gradients.
 * The compositing weights exist only inside the traversal, so the answer comes from a traversal of its own.  A COMPOSITED EVENT is
 * exactly the backward pass's (above): the k-buffer's events i in key order (t, id, entry < exit), BOTH the entry and the exit event
 * of a proxy, repeats of a split particle's pieces dropped, an event counted when alpha_min < alpha_i, the walk going on while
 * T > minTransmittance and the last distance <= t_max.  Its weight is
 *     w_i = T_i alpha_i,     T_1 = 1, T_{i+1} = T_i (1 - alpha_i)       (T_i: the transmittance BEFORE the event)
 * both factors float32 and formed with the forward's own arithmetic, the product one float32 multiplication.  Over the rays r of the
 * window (grt_particle_stats_frame) or of the buffer (grt_particle_stats_rays), for every particle j by ORIGINAL id:
 *     weight_sum[j] += sum over the composited events of j on r of  w_ray(r) * w_i
 *     weight_max[j]  = max(weight_max[j], max over those events of  w_i)                (NOT scaled by w_ray)
 *     count[j]      += the number of those events
 * (with unit ray weights the sum of weight_sum over all particles is the sum over the rays of 1 - T_end: grt_aux_out::alpha before
 * its clamp; the sum of count is the sum of grt_aux_out::count.)
 *   d_ray_weight   [h][w] (laid out like the frame, read inside the window) or [n]; NULL = 1 for every ray.  A ray whose weight is
 *                  EXACTLY 0 is not traced and contributes to none of the three outputs (a mask: weight_max and count see the
 *                  rays of nonzero weight).  Weights may be negative; weight_sum is then a signed sum.
 *   out            device arrays [n] by original particle id; each may be NULL (that output is not computed), all three NULL:
 *                  GRT_ERR_INVALID.  The outputs are ACCUMULATED into what the arrays hold — add, max, add — so several views sum up
 *                  without a pass in between; the caller zeroes them.  weight_max must hold non-negative floats (it is updated by
 *                  an unsigned-integer atomic max on their bit patterns).
 * Skipped like in the backward: fisheye pixels with r > 1, pixels outside the window, rays the raygen loop does not trace
 * (|d| <= 0.1, a NaN direction, max_bounces = 0).  With n = 0 rays, an empty window or an empty scene the call returns GRT_OK and
 * writes nothing.  count and weight_max are BITWISE reproducible between calls (integer add, max); weight_sum is not (float atomics
 * arrive in varying order; tests compare within a tolerance measured for float32 evaluation).  GRT_OPT_BWD_PLAIN_ATOMICS = 1 makes
 * every lane issue its own atomics here too (testing).  The context owns no buffer for this: grt_memory_info::slot_bytes is
 * unchanged by a call, and a frame rendered after a call is bit-identical to one rendered before it.  Asynchronous on `stream` like
 * grt_render; grt_last_kernel_ms reports the call's device time.  A view computes the statistics of its scene.
 * Refused with GRT_ERR_INVALID (text in grt_last_error with the entry point's name in front; the context stays usable): meshes set
 * (statistics of mesh frames: grt_particle_stats_mesh_frame / grt_particle_stats_mesh_rays, below), GRT_OPT_COUNTERS = 1, no BVH, NULL p / out / rays, a window outside the frame,
 * sh_degree_max > 3, t_min <= 0.  GRT_ERR_LIMIT: a BVH so high that its per-lane LDS stacks exceed 160 KiB, as in the backward. */
typedef struct {
    float* weight_sum;
    float* weight_max;
    uint32_t* count;
} grt_particle_stats;
GRT_API int grt_particle_stats_frame(grt_ctx* ctx, const grt_params* p, const float* d_ray_weight /* may be NULL */,
                                     const grt_particle_stats* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_particle_stats_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n,
                                    const float* d_ray_weight /* may be NULL */, const grt_particle_stats* out, void* stream);
/* ---- per-particle contribution statistics of MESH frames: what a view sees through mirrors and glass ----
 * The statistics above for a scene with meshes set (grt_set_meshes): rays bounce as grt_render / grt_render_aux trace them, and the
 * particles met behind a bounce are counted with the ones met in front of it.  A ray runs iterations s = 1..S, as documented at
 * grt_backward_mesh.  It has ONE event list with ONE running transmittance, T_1 = 1 and T_{i+1} = T_i (1 - alpha_i), cut into the
 * segments of its iterations; the loop carries it across segments as the forward does, through `density`.  A COMPOSITED EVENT is
 * exactly the mesh backward's.  For event i in segment s:
 *     w_i  = T_i alpha_i        the plain statistics' weight, one float32 multiplication
 *     cw_i = c_s w_i            the COLOUR WEIGHT, with which the particle's radiance L_i enters the pixel (dC/dL_i), where
 *     c_s  = 1 - A_{s-1}            for a Gaussian pass (A: the accumulated alpha in front of the iteration),
 *            D_S (1 - B_{S-1})      for the last pass (D_S: the density 1 - T behind the ray's last segment, B: the blocking),
 *            1                      for a terminating GRT_NORMAL hit,
 * c_s formed in float32 as the forward forms it and multiplied ONCE with w_i.  The two weights diverge behind a bounce: A sums
 * cumulative densities and saturates long before T is spent, so a reflected particle can have a large w_i and a colour weight of 0.
 * "Was met" reads count / weight_*; "matters to the image" reads colour_*.  Per particle j by ORIGINAL id, over the rays r:
 *     weight_sum[j] += sum w_ray(r) * w_i      weight_max[j] = max(weight_max[j], max w_i)      count[j] += number of events
 *     colour_sum[j] += sum w_ray(r) * cw_i     colour_max[j] = max(colour_max[j], max cw_i)
 *   step_first, step_last   the iterations whose events are counted, 1-based, inclusive; 0, 0 = all; step_last = 0 leaves the range
 *                  open.  Events outside the range are still composited (T and A run through them); they only enter no output.
 *                  (1, 1): what the camera rays meet directly; (2, 0): what is met only through a bounce.
 * Everything else is the plain call's contract: the outputs are ACCUMULATED (add, max, add, add, max) into the caller's arrays; each
 * pointer may be NULL, all five NULL: GRT_ERR_INVALID; a ray of weight exactly 0 is not traced; weight_max and colour_max are updated
 * by an unsigned-integer atomic max on the bit patterns of non-negative floats; count, weight_max and colour_max are BITWISE
 * reproducible between calls, the two sums are not; GRT_OPT_BWD_PLAIN_ATOMICS applies; the context owns no buffer for this and a
 * frame rendered after a call is bit-identical to one rendered before it; a view computes the statistics of its scene.  With neither
 * colour output asked for a ray is walked once, else twice (D_S is known only at the end of the last segment).
 * On a scene WITHOUT meshes a ray has one last pass: count, weight_max and weight_sum are the plain call's, cw_i = (1 - T_end) w_i.
 * Refused with GRT_ERR_INVALID like the plain call, without its meshes row: GRT_OPT_COUNTERS = 1, no BVH, NULL p / out / rays, a
 * window outside the frame, sh_degree_max > 3, t_min <= 0; and p->type outside MIRROR/NORMAL/GLASS, step_first > step_last with
 * step_last != 0.  GRT_ERR_LIMIT as in the backward.  (Feature channels of mesh frames: grt_render_features_mesh_frame; picks and
 * event lists: grt_ray_picks_mesh_frame, grt_ray_events_mesh_frame, below.) */
typedef struct {
    float* weight_sum;
    float* weight_max;
    uint32_t* count;
    float* colour_sum;
    float* colour_max;
    uint32_t step_first, step_last;
} grt_particle_stats_mesh;
GRT_API int grt_particle_stats_mesh_frame(grt_ctx* ctx, const grt_params* p, const float* d_ray_weight /* may be NULL */,
                                          const grt_particle_stats_mesh* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_particle_stats_mesh_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n,
                                         const float* d_ray_weight /* may be NULL */, const grt_particle_stats_mesh* out, void* stream);
/* ---- per-particle feature channels rendered through the Gaussians, with gradients (Gaussian-only frames) ----
 * The caller's own per-particle quantity — semantic or language embeddings, labels, an error or an age for a heat map, any learned
 * channel — composited with the renderer's weights, and the gradient back to it and to the Gaussians: feature-field distillation on
 * frozen geometry, or joint training of colour and features on one scene.  A COMPOSITED EVENT is exactly the backward pass's and the
 * statistics' (above): the k-buffer's events i in key order, BOTH the entry and the exit event of a proxy, repeats of a split
 * particle's pieces dropped, an event counted when alpha_min < alpha_i, the walk going on while T > minTransmittance and the last
 * distance <= t_max; the same rays are skipped (fisheye r > 1, |d| <= 0.1, a NaN direction, max_bounces = 0, an empty tree).
 *   feat       [n][C] float32 on the device, by ORIGINAL particle id, owned by the caller and passed per call like a ray buffer: the
 *              context keeps nothing of it.
 *   channels   C, 1 .. GRT_MAX_FEATURE_CHANNELS (more channels: several calls over slices of 16).
 * FORWARD, over the composited events i of a ray in compositing order:
 *     F[ray][c] = sum_i w_i feat[id_i][c],     w_i = T_i alpha_i,     T_1 = 1, T_{i+1} = T_i (1 - alpha_i)
 * T_i the transmittance BEFORE the event, w_i ONE float32 product of the forward's own two factors (as for the statistics), each term
 * added as F_c = F_c + w_i * f_c in float32 without contraction.  F is NOT multiplied by the frame's alpha and is not normalised: with
 * feat = 1 it is sum w_i = 1 - T_end up to rounding (grt_aux_out::alpha before its clamp).  Every element of the window
 * ([h][w][C], laid out like the frame) or of the buffer ([n][C]) is WRITTEN once — zeros for a ray that is not traced; pixels outside
 * the window are untouched.  No atomic is in its path: the forward is bitwise reproducible, and windows tile a frame bit for bit.
 * BACKWARD of loss = sum_ray sum_c g[ray][c] F[ray][c], every discrete decision held fixed as in grt_backward.  Per ray, with
 *     phi_i = sum_c g_c feat[id_i][c],     Phi = sum_i w_i phi_i,     P_i = sum_{j<=i} w_j phi_j      (formed in compositing order)
 *     dloss/dalpha_i        = T_i phi_i - (Phi - P_i) / (1 - alpha_i)
 *     dloss/dfeat[j][c]    += sum over the composited events i of particle j of  w_i g[ray][c]
 * dloss/dalpha_i is grt_backward's with the one-channel radiance L = (phi_i, 0, 0), g_rad = (1, 0, 0), S = (Phi - P_i, 0, 0) and
 * g_A' = 0; below alpha_i the chain to pos, scale, quat and opacity is grt_backward's own — nothing where the 0.99 clamp binds, the
 * quaternion AS UPLOADED.  A ray whose C upstream values are all exactly 0 is not traced.  All gradients are ADDED into the caller's
 * arrays ([n][3] [n][3] [n][4] [n] and [n][C], by original id; the caller zeroes them); any subset of the five may be NULL, all five
 * NULL: GRT_ERR_INVALID.  With pos, scale, quat and opacity all NULL the call is ONE traversal and touches no buffer of the context;
 * otherwise two (Phi comes from a first sweep: the forward's F is not an argument), through the context's 64-B-per-particle gradient
 * buffer and its flush exactly as grt_backward (created by the first such call; the higher-SH buffer never is).  Float atomics: not
 * bitwise reproducible between calls; GRT_OPT_BWD_PLAIN_ATOMICS = 1 makes every lane issue its own (testing).
 * The forward uses no buffer of the context (grt_memory_info::slot_bytes is unchanged by it); a frame rendered after either call is
 * bit-identical to one rendered before it; a view computes its scene's result.  Asynchronous on `stream` like grt_render;
 * grt_last_kernel_ms reports the call's device time.  With no rays, no particles or an empty tree the calls return GRT_OK: the
 * forward writes zeros, the backward nothing.
 * Refused with GRT_ERR_INVALID (text in grt_last_error with the entry point's name in front; the context stays usable): everything
 * grt_backward refuses (NULL p, no BVH, GRT_OPT_COUNTERS = 1, sh_degree_max > 3, t_min <= 0, a window outside the frame, a NULL ray
 * buffer), meshes set (feature channels are rendered for Gaussian-only frames), channels 0 or above GRT_MAX_FEATURE_CHANNELS, a NULL
 * feat, output or upstream.  GRT_ERR_LIMIT: a BVH so high that its per-lane LDS stacks exceed 160 KiB, as in the backward.
 * Not computed: gradients with respect to rays or the camera through features, an alpha / depth / normalised output (grt_render_aux
 * has alpha); mesh frames have calls of their own (grt_render_features_mesh_frame, below). */
#define GRT_MAX_FEATURE_CHANNELS 16
typedef struct {
    float* pos;
    float* scale;
    float* quat;
    float* opacity;
    float* feat; /* [n][channels] */
} grt_feature_grads;
GRT_API int grt_render_features_frame(grt_ctx* ctx, const grt_params* p, const float* d_feat, uint32_t channels, float* d_out, uint32_t x0,
                                      uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_render_features_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const float* d_feat,
                                     uint32_t channels, float* d_out, void* stream);
GRT_API int grt_backward_features_frame(grt_ctx* ctx, const grt_params* p, const float* d_feat, uint32_t channels, const float* d_grad_out,
                                        const grt_feature_grads* grads, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_backward_features_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const float* d_feat,
                                       uint32_t channels, const float* d_grad_out, const grt_feature_grads* grads, void* stream);
/* ---- feature channels of MESH frames: what a view shows through mirrors and glass, with gradients ----
 * The feature calls above for a scene with meshes set (grt_set_meshes): rays bounce as grt_render / grt_render_aux trace them, and
 * the particles met behind a bounce enter the pixel's features with the weight their radiance enters its colour with.  A ray runs
 * iterations s = 1..S exactly as documented at grt_backward_mesh: ONE event list with ONE running transmittance carried through
 * `density`, the same composited events.  feat[n][C], channels (1 .. GRT_MAX_FEATURE_CHANNELS), the output layout and the untraced
 * rays (zeros) are the plain calls'.
 * FORWARD.  Per segment, in compositing order and in float32 without contraction (Phi = Phi + w_i * f_c, as the plain call forms F),
 *     Phi_s[c] = sum_{i in s} w_i feat[id_i][c],     w_i = T_i alpha_i,
 * and at the iteration's step of the loop F[c] = F[c] + Phi_s[c] * c_s with the segment's colour weight of
 * grt_particle_stats_mesh, formed in float32 as the forward forms it:
 *     c_s = 1 - A_{s-1}   Gaussian pass;     D_S (1 - B_{S-1})   last pass;     1   a terminating GRT_NORMAL hit.
 * A mesh surface itself contributes NO feature (the ncol (1 - D_s) term of the colour has no counterpart), and nothing is clamped.
 * On a scene WITHOUT meshes a ray has one last pass, so F = (1 - T_end) F_plain: the mesh calls weight with the frame's own alpha,
 * the plain calls do not.  With feat[j] = particle j's radiance F is the frame's rgbf on every frame that neither clamps a radiance
 * channel nor ends on a GRT_NORMAL hit.  Plain stores, no atomic: bitwise reproducible, and windows tile a frame bit for bit.
 *   step_first, step_last   as for grt_particle_stats_mesh: the iterations whose events carry their feature row, 1-based, inclusive;
 *                  0, 0 = all; step_last = 0 leaves the range open.  Events outside the range are still composited — T, A and B run
 *                  through them — with a feature row of ZERO.  (2, 0) renders what is seen only through a bounce.
 * BACKWARD of loss = sum_ray sum_c g[ray][c] F[ray][c], every discrete decision of grt_backward_mesh held fixed.  Per event
 * phi_i = sum_c g_c feat[id_i][c], and 0 for an event outside the step range; dloss/dalpha_i is grt_backward_mesh's formula with the
 * one-channel radiance L_i = (phi_i, 0, 0), g_C = (1, 0, 0), g_A = 0, no ncol term and no radiance clamp; below alpha_i the chain to
 * pos, scale, quat and opacity is unchanged (with the segment's own ray); and
 *     dloss/dfeat[j][c] += sum over the composited events i of particle j inside the step range of  c_s w_i g[ray][c].
 * All gradients are ADDED into the caller's arrays; any subset of the five may be NULL, all five NULL: GRT_ERR_INVALID.  A ray whose C
 * upstream values are all exactly 0 is not traced.  A ray is walked twice (D_S is known only at the end of the last segment), also
 * for the feature gradient alone; that call touches no buffer of the context, the others go through its gradient buffer and flush
 * as grt_backward_mesh.  Float atomics (GRT_OPT_BWD_PLAIN_ATOMICS applies).  The forward uses no buffer of the context; a frame rendered
 * after either call is bit-identical to one rendered before it; a view computes its scene's result.  With no rays, no particles or
 * an empty tree the calls return GRT_OK: the forward writes zeros, the backward nothing.
 * Refused with GRT_ERR_INVALID (the entry point's name in front; the context stays usable) like the plain calls, without their
 * meshes row: NULL p, no BVH, GRT_OPT_COUNTERS = 1, sh_degree_max > 3, t_min <= 0, a window outside the frame, a NULL ray buffer,
 * channels 0 or above GRT_MAX_FEATURE_CHANNELS, a NULL feat, output or upstream; and p->type outside MIRROR/NORMAL/GLASS,
 * step_first > step_last with step_last != 0.  GRT_ERR_LIMIT as in the mesh backward (the LDS stack of the higher of the two trees).
 * Not computed: gradients with respect to rays, camera or meshes, a feature of the surface.  (Picks and event lists of mesh frames:
 * grt_ray_picks_mesh_frame, grt_ray_events_mesh_frame, below.) */
GRT_API int grt_render_features_mesh_frame(grt_ctx* ctx, const grt_params* p, const float* d_feat, uint32_t channels, float* d_out,
                                           uint32_t step_first, uint32_t step_last, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                                           void* stream);
GRT_API int grt_render_features_mesh_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const float* d_feat,
                                          uint32_t channels, float* d_out, uint32_t step_first, uint32_t step_last, void* stream);
GRT_API int grt_backward_features_mesh_frame(grt_ctx* ctx, const grt_params* p, const float* d_feat, uint32_t channels,
                                             const float* d_grad_out, const grt_feature_grads* grads, uint32_t step_first,
                                             uint32_t step_last, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_backward_features_mesh_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const float* d_feat,
                                            uint32_t channels, const float* d_grad_out, const grt_feature_grads* grads,
                                            uint32_t step_first, uint32_t step_last, void* stream);
/* ---- per-ray picks: which particle a ray sees first, strongest and at its median, and where (Gaussian-only frames) ----
 * What picking and lasso selection in a viewer, per-pixel id and label maps, and a surface depth (TSDF fusion, mesh extraction, depth
 * regularisers) read: grt_aux_out::depth is the expected distance sum w_i t_i and smears across silhouettes; the particle statistics
 * are per particle, not per pixel.  A COMPOSITED EVENT is exactly the backward pass's, the statistics' and the features' (above): the
 * k-buffer's events i in key order (t, id, entry < exit), BOTH the entry and the exit event of a proxy, repeats of a split particle's
 * pieces dropped, an event counted when alpha_min < alpha_i, the walk going on while T > minTransmittance and the last distance
 * <= t_max.  Its weight is w_i = T_i alpha_i, T_i the transmittance BEFORE the event: ONE float32 product of the forward's own two
 * factors, as for the statistics.  Per ray, three rules select one event each:
 *     first    the first composited event
 *     peak     the event of largest w_i; a later event replaces the pick only when its weight is STRICTLY greater (the earliest wins a tie)
 *     cross    the first event i with T_i (1 - alpha_i) <= cross_T: the float32 transmittance BEHIND the event, as the compositing loop
 *              forms it.  cross_T = 0.5 gives the median depth.
 * and for each rule the call writes
 *     id       the particle's ORIGINAL id (it indexes the arrays of grt_gaussians), GRT_PICK_NONE where there is no such event
 *     t        the event's key distance — the t_i of grt_aux_out::depth, in units of |d| for caller-supplied rays — else 0.0f
 *     weight   w_i, else 0.0f
 * Every element of the window ([h][w], laid out like the frame) or of the buffer ([n]) is WRITTEN exactly once per requested array:
 * GRT_PICK_NONE, 0.0f, 0.0f for a ray with no such event and for a ray that is not traced (fisheye r > 1, |d| <= 0.1, a NaN direction,
 * max_bounces = 0, an empty tree or an empty scene); pixels outside the window are untouched.  Each of the nine arrays may be NULL (it
 * is not written).  No atomic is in the path: the call is BITWISE reproducible, and windows tile a frame bit for bit.
 * The call uses no buffer of the context (grt_memory_info::slot_bytes is unchanged by it); a frame rendered after it is bit-identical
 * to one rendered before it; a view computes its scene's result.  Asynchronous on `stream` like grt_render; grt_last_kernel_ms
 * reports the call's device time.  With n = 0 rays or an empty window the call returns GRT_OK and writes nothing.
 * Refused with GRT_ERR_INVALID (text in grt_last_error with the entry point's name in front; the context stays usable): everything
 * grt_particle_stats_* refuses (GRT_OPT_COUNTERS = 1, no BVH, NULL p / out / rays, a window outside the frame, sh_degree_max > 3,
 * t_min <= 0), meshes set (ray picks are computed for Gaussian-only frames), all nine pointers NULL, cross_T outside (0, 1) (NaN
 * included) while any array of `cross` is requested.  GRT_ERR_LIMIT: a BVH so high that its per-lane LDS stacks exceed 160 KiB, as
 * in the statistics.  Not computed: more than one pick per rule, gradients of any kind.  Mesh frames have calls of their own
 * (grt_ray_picks_mesh_frame, below). */
#define GRT_PICK_NONE 0xFFFFFFFFu
typedef struct {
    uint32_t* id;
    float* t;
    float* weight;
} grt_pick_out; /* each may be NULL */
typedef struct {
    grt_pick_out first, peak, cross;
    float cross_T;
} grt_ray_picks;
GRT_API int grt_ray_picks_frame(grt_ctx* ctx, const grt_params* p, const grt_ray_picks* out, uint32_t x0, uint32_t y0, uint32_t x1,
                                uint32_t y1, void* stream);
GRT_API int grt_ray_picks_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const grt_ray_picks* out, void* stream);
/* ---- per-ray event lists with gradients: the composited events themselves, for any per-ray loss (Gaussian-only frames) ----
 * Everything the renderer reports per pixel, per particle and per pick is computed from one thing: the ray's list of composited events
 * (id_i, t_i, alpha_i) in compositing order.  These calls hand that list out, and take dloss/dalpha_i back: with T_i = prod_{j<i}
 * (1 - alpha_j) and w_i = T_i alpha_i formed by the CALLER from the returned alpha, any loss on a ray's events — a depth-distortion
 * regulariser sum_ij w_i w_j |t_i - t_j|, quantile depths, a transmittance profile, a loss on sum w_i t_i, an entropy term — is
 * differentiable with respect to pos, scale, quat and opacity without a kernel of its own.  A COMPOSITED EVENT is exactly the picks',
 * the features', the statistics' and the backward pass's (above): key order (t, id, entry < exit), BOTH events of a proxy, repeats of a
 * split particle's pieces dropped, alpha_min < alpha_i, the walk going on while T > minTransmittance and the last distance <= t_max.
 * FORWARD.  The events `first` .. `first + K - 1` of every ray (K = max_events; first = 0: the first K) go to slot s = i - first:
 *     id     [K][N]  the particle's ORIGINAL id, GRT_PICK_NONE in an unused slot
 *     t      [K][N]  the event's key distance — the t_i of grt_aux_out::depth and of the picks, in units of |d| for caller-supplied
 *                    rays —, 0.0f in an unused slot.  t_i is the proxy-hit distance, a piecewise function of the proxy's faces: it is
 *                    DATA and carries no gradient.
 *     alpha  [K][N]  the alpha the forward composites (after the 0.99 clamp), 0.0f in an unused slot
 *     count  [N]     ALL composited events of the ray, not capped by K (grt_aux_out::count)
 *     T_in   [N]     the float32 transmittance in front of event `first` as the compositing loop forms it (T *= 1 - alpha, one
 *                    multiplication per event): 1 for first = 0, the ray's final T when count <= first, 1 for a ray that is not traced
 * N = width * height for a frame (element py * width + px, as in every per-pixel array), n for a ray buffer.  The layout is SLOT-MAJOR:
 * element [s][r] is at s * N + r, so a slot plane is contiguous and cumprod(1 - alpha) along the first axis gives the transmittances.
 * Every element [s][r], s < K, of the window or of the buffer is WRITTEN exactly once per requested array — GRT_PICK_NONE, 0.0f, 0.0f
 * behind the ray's last listed event and for a ray that is not traced (fisheye r > 1, |d| <= 0.1, a NaN direction, max_bounces = 0, an
 * empty tree or an empty scene) — and so are count and T_in; pixels outside the window are untouched.  Each of the five arrays may be
 * NULL (it is not written).  No atomic, no wave operation and no buffer of the context (grt_memory_info::slot_bytes is unchanged): the
 * call is BITWISE reproducible, windows tile a frame bit for bit, and pages (first = 0, K, 2K, ...) concatenate to the one long call.
 * BACKWARD.  d_grad_alpha [K][N], laid out like alpha for the same first and max_events: g[s][r] = dloss/dalpha of the event in slot s
 * of ray r, every discrete decision held fixed as in grt_backward.  The call ADDS
 *     sum over the listed events of  g[s][r] * d alpha_i / d (pos, scale, quat, opacity)
 * into the caller's arrays ([n][3] [n][3] [n][4] [n] by original id; the caller zeroes them) — grt_backward's own chain below alpha_i,
 * the quaternion AS UPLOADED, nothing where the 0.99 clamp binds (alpha_i = 0.99 does not move).  Values of g in slots behind a ray's
 * last listed event are NOT read as gradients of anything; a ray whose K upstream values are all exactly 0 is not traced.  ONE
 * traversal (dloss/dalpha is the caller's), through the context's 64-B-per-particle gradient buffer and its flush exactly as
 * grt_backward.  Float atomics: not bitwise reproducible; GRT_OPT_BWD_PLAIN_ATOMICS = 1 makes every lane issue its own (testing).
 * A loss over more than K events of a ray takes a larger K: the pages of the forward are values, not a graph.
 * Both: asynchronous on `stream` like grt_render; grt_last_kernel_ms reports the call's device time; a frame rendered after either
 * call is bit-identical to one rendered before it; a view computes its scene's result.  With n = 0 rays or an empty window the calls
 * return GRT_OK and write nothing; with no particles or an empty tree the forward writes "none", the backward nothing.
 * Refused with GRT_ERR_INVALID (text in grt_last_error with the entry point's name in front; the context stays usable): everything
 * grt_backward refuses (NULL p, no BVH, GRT_OPT_COUNTERS = 1, sh_degree_max > 3, t_min <= 0, a window outside the frame, a NULL ray
 * buffer), meshes set (ray events are listed for Gaussian-only frames), max_events = 0, first + max_events overflowing 32 bits, no
 * output (forward: out NULL or all five arrays NULL; backward: out NULL or pos, scale, quat and opacity all NULL), a NULL upstream,
 * out->sh != NULL (colour does not depend on the listed quantities).  GRT_ERR_LIMIT: a BVH so high that its per-lane LDS stacks
 * exceed 160 KiB, as in the backward.  Not computed: gradients through t_i, gradients with respect to rays or the camera.  Mesh frames
 * have calls of their own (grt_ray_events_mesh_frame, below). */
typedef struct grt_ray_events {
    uint32_t* id;    /* [K][N] */
    float* t;        /* [K][N] */
    float* alpha;    /* [K][N] */
    uint32_t* count; /* [N] */
    float* T_in;     /* [N] */
    uint32_t first, max_events; /* K = max_events >= 1; first + K must not overflow */
} grt_ray_events;
GRT_API int grt_ray_events_frame(grt_ctx* ctx, const grt_params* p, const grt_ray_events* out, uint32_t x0, uint32_t y0, uint32_t x1,
                                 uint32_t y1, void* stream);
GRT_API int grt_ray_events_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const grt_ray_events* out, void* stream);
GRT_API int grt_backward_events_frame(grt_ctx* ctx, const grt_params* p, const float* d_grad_alpha, uint32_t first, uint32_t max_events,
                                      const grt_gaussian_grads* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_backward_events_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const float* d_grad_alpha,
                                     uint32_t first, uint32_t max_events, const grt_gaussian_grads* out, void* stream);
/* ---- per-ray picks and event lists of MESH frames: what a ray sees through mirrors and glass ----
 * The two per-ray queries above for a scene with meshes set (grt_set_meshes): rays bounce as grt_render / grt_render_aux trace them.
 * A ray runs iterations s = 1..S exactly as documented at grt_backward_mesh, each on its own ray (o_s, d_s): ONE event list with ONE
 * running transmittance carried across segments through `density` (the start of a step is T = 1 - density, two float32 roundings).
 * A COMPOSITED EVENT is exactly the mesh backward's; its weight is w_i = T_i alpha_i, T_i the running transmittance BEFORE the event,
 * one float32 product — the w_i of grt_particle_stats_mesh.
 *   step_first, step_last   as for grt_particle_stats_mesh: the iterations whose events are candidates (picks) or are numbered and
 *                  listed (event lists), 1-based, inclusive; 0, 0 = all; step_last = 0 leaves the range open.  Events outside the
 *                  range are still composited: T, A and B run through them.  (2, 0): what is seen only through a bounce.
 * The colour weight c_s w_i is NOT used by either query: it needs a second walk (D_S is known only behind the last segment), and
 * grt_particle_stats_mesh already reports it; alpha, step and path_state of the event list let a caller rebuild A, B and c_s.
 * PICKS.  The rules of grt_ray_picks among the events inside the step range: first — the first such event; peak — the largest w_i,
 * replaced only by a STRICTLY greater weight; cross — the first such event with T_i (1 - alpha_i) <= cross_T, T the ray's OWN running
 * transmittance, not one restarted at the range.  Per rule:
 *     id       the particle's ORIGINAL id                          weight   w_i
 *     t        the key distance along the iteration's own ray,     step     the 1-based iteration s
 *              in units of |d_s|                                   point    [N][3]: o_s[k] + t * d_s[k], one float32 multiplication
 *                                                                           and one addition per component, no contraction
 * "None" — a ray with no such event, a ray that is not traced — is GRT_PICK_NONE, 0.0f, 0.0f, 0, (0, 0, 0).  Every element of the
 * window or of the buffer is WRITTEN exactly once per requested array; each of the fifteen arrays may be NULL.  No atomic and no
 * buffer of the context: BITWISE reproducible, windows tile a frame bit for bit, a frame rendered after the call is bit-identical to
 * one rendered before it, a view computes its scene's result.  On a scene WITHOUT meshes, with steps 0, 0, id, t and weight are
 * grt_ray_picks' bytes and step is 1.
 * Refused with GRT_ERR_INVALID as grt_particle_stats_mesh_* (GRT_OPT_COUNTERS = 1, no BVH, NULL p / out / rays, a window outside the
 * frame, sh_degree_max > 3, t_min <= 0, p->type outside MIRROR/NORMAL/GLASS, step_first > step_last with step_last != 0), and: all
 * fifteen pointers NULL, cross_T outside (0, 1) (NaN included) while any array of `cross` is requested.  GRT_ERR_LIMIT as in the mesh
 * backward (the LDS stack of the higher of the two trees). */
typedef struct {
    uint32_t* id;
    float* t;
    float* weight;
    uint32_t* step;
    float* point; /* [N][3] */
} grt_pick_mesh_out; /* each may be NULL */
typedef struct {
    grt_pick_mesh_out first, peak, cross;
    float cross_T;
    uint32_t step_first, step_last;
} grt_ray_picks_mesh;
GRT_API int grt_ray_picks_mesh_frame(grt_ctx* ctx, const grt_params* p, const grt_ray_picks_mesh* out, uint32_t x0, uint32_t y0,
                                     uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_ray_picks_mesh_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const grt_ray_picks_mesh* out,
                                    void* stream);
/* EVENT LISTS.  FORWARD: the events inside the step range are numbered 0, 1, ... in compositing order over the WHOLE ray; events
 * first .. first + K - 1 go to slot n - first of id, t, alpha (as grt_ray_events) and step (the 1-based iteration; t is measured on
 * that iteration's ray).  count is ALL events inside the range; T_in the running float32 T in front of event `first` — the T behind
 * the ray's last segment when count <= first, 1 for a ray that is not traced.  Unused slots hold GRT_PICK_NONE, 0, 0, 0.
 * The PATH: slot s - 1 of path_rays / path_t_far / path_state holds iteration s — its ray, the end of its segment (the mesh hit
 * distance, or t_max) and its state —, whatever the step range; with them (step, t) becomes a world position and A, B and c_s can be
 * rebuilt from alpha.  Iterations beyond max_steps are not stored; n_steps counts them all.  Unused path slots hold zeros and
 * GRT_PICK_NONE.  All stores are plain: BITWISE reproducible, windows tile, pages (first = 0, K, 2K, ...) concatenate.  On a scene
 * WITHOUT meshes, with steps 0, 0, id, t, alpha, count and T_in are grt_ray_events' bytes.
 * BACKWARD.  d_grad_alpha [K][N] for the same first, max_events and step range: dloss/dalpha of the listed event.  The call ADDS
 * sum g * d alpha_i / d (pos, scale, quat, opacity) into the caller's arrays, alpha_i differentiated on THE ITERATION'S OWN RAY
 * (o_s, d_s), the mesh hits, normals and next rays held fixed; nothing where the 0.99 clamp binds; a ray whose K upstream values are
 * all exactly 0 is not traced.  ONE traversal, through the gradient buffer and its flush as grt_backward; float atomics
 * (GRT_OPT_BWD_PLAIN_ATOMICS applies).
 * Refused with GRT_ERR_INVALID as grt_ray_events_* / grt_backward_events_* with the meshes row replaced by the mesh calls' own
 * (p->type outside MIRROR/NORMAL/GLASS), and: step_first > step_last with step_last != 0, max_steps = 0 while a path array is given,
 * (backward) out->sh != NULL, no geometry group, a NULL upstream.  GRT_ERR_LIMIT as in the mesh backward.  Not computed: picks by
 * colour weight, gradients through t_i, through the path, or with respect to rays, camera or meshes. */
#define GRT_STEP_LAST 0u      /* the last Gaussian pass: the ray met no mesh, or max_bounces is spent */
#define GRT_STEP_GAUSSIAN 1u  /* a Gaussian pass: the segment ends at a mesh hit that bounces */
#define GRT_STEP_TERMINATE 3u /* the segment ends at a GRT_NORMAL hit */
typedef struct grt_ray_events_mesh {
    uint32_t* id;    /* [K][N], slot-major as grt_ray_events */
    float* t;        /* [K][N] */
    float* alpha;    /* [K][N] */
    uint32_t* step;  /* [K][N] */
    uint32_t* count; /* [N] */
    float* T_in;     /* [N] */
    uint32_t first, max_events, step_first, step_last;
    float* path_rays;     /* [P][N][6]: (o_s, d_s) of iteration s = slot + 1 */
    float* path_t_far;    /* [P][N]: the segment's end (mesh hit distance, or t_max) */
    uint32_t* path_state; /* [P][N]: GRT_STEP_LAST, GRT_STEP_GAUSSIAN, GRT_STEP_TERMINATE; GRT_PICK_NONE unused */
    uint32_t* n_steps;    /* [N]: ALL iterations the ray ran, not capped by P */
    uint32_t max_steps;   /* P; may be 0 when no path array is given */
} grt_ray_events_mesh;
GRT_API int grt_ray_events_mesh_frame(grt_ctx* ctx, const grt_params* p, const grt_ray_events_mesh* out, uint32_t x0, uint32_t y0,
                                      uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_ray_events_mesh_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const grt_ray_events_mesh* out,
                                     void* stream);
GRT_API int grt_backward_events_mesh_frame(grt_ctx* ctx, const grt_params* p, const float* d_grad_alpha, uint32_t first, uint32_t max_events,
                                           uint32_t step_first, uint32_t step_last, const grt_gaussian_grads* out, uint32_t x0, uint32_t y0,
                                           uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_backward_events_mesh_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const float* d_grad_alpha,
                                          uint32_t first, uint32_t max_events, uint32_t step_first, uint32_t step_last,
                                          const grt_gaussian_grads* out, void* stream);
/* ---- ray segments: per-ray range and carried transmittance, with gradients ----
 * Every call above renders a WHOLE ray: one t_min / t_max for all rays, transmittance 1 at the start, the reference's pixel rad * A.
 * These calls are the reference's trace() itself (shaders/tracer.cuh:328-373): ONE segment [t_near, t_far] of every ray, entered with
 * the transmittance T_in the ray's earlier segments left, returning the plain radiance and the transmittance behind it.  With them a
 * caller composites the Gaussians against a depth buffer of other geometry (the ray clipped to [t_min, z], the surface entering with
 * T_out), writes a bounce loop of its own (an analytic mirror, another BRDF, a portal, a shadow ray: the reflected ray starts at
 * T_in = T_out of the segment before), or takes the plain volumetric colour sum_i w_i L_i that rgbf = rad * A cannot be divided into.
 * INPUT.  grt_segments: three device arrays [N] float32, each may be NULL (the default for every ray: p->t_min, p->t_max, 1); seg itself
 * may be NULL (all three defaults).  When an array is given, p->t_min / p->t_max are not read for it.  p->max_bounces is not looked at:
 * trace() has no bounce.  N = width * height for a frame (element py * width + px), n for a ray buffer.
 * FORWARD.  For ray r with a = t_near[r], b = t_far[r], T0 = T_in[r] the events are exactly those trace() composites on [a, b] when it
 * is entered with transmittance T0: key order, entry and exit hits, alpha_min < alpha_i, the 0.99 clamp, T_i = T0 prod_{j<i} (1 -
 * alpha_j), the walk going on while T > minTransmittance (compared with the running T, so T0 counts) and the last distance <= b.
 * An event whose distance equals t_near or t_far exactly is in NEITHER segment, so a chain cut at an event's own reported distance
 * (grt_ray_picks, grt_ray_events) loses it: trace() takes a + 1e-9f < t_i < b + 1e-9f in float32, and from 2^-5 on the 1e-9f is
 * rounded away (below 2^-5 the sum is the next float or the one after, and an event at t_far itself is kept).
 *     radiance [N][3]  R = sum_i T_i alpha_i L_i, accumulated as the frame does: R = R + (L T) alpha
 *     T_out    [N]     T0 prod_i (1 - alpha_i)
 *     depth    [N]     sum_i T_i alpha_i t_i (t_i: the event's key distance, in units of |d|), (T alpha) t added before T is updated
 *     count    [N]     composited events
 * With the defaults count, depth and 1 - T_out equal grt_render_rays_aux's bit for bit, and R (1 - T_out) its rgbf.
 * A ray is UNTRACED when |d| > 0.1 fails, a > 0 fails (keys need positive distances), a <= b fails or b is not finite, T0 >
 * minTransmittance fails — a NaN in any of the three fails these tests —, the tree is empty, or a fisheye pixel has no ray.  It writes
 * R = 0, depth = 0, count = 0 and T_out as a BIT COPY of T_in (a NaN's payload included).  Every element of the buffer or of the window
 * is WRITTEN exactly once per requested array; pixels outside the window are untouched.  Each output may be NULL, not all.  No atomic, no
 * wave operation and no buffer of the context: the call is BITWISE reproducible and windows tile a frame bit for bit.
 * BACKWARD.  d_grad_radiance [N][3] = dloss/dR and d_grad_T_out [N] = dloss/dT_out (NULL: zero).  The call ADDS
 *     g_R . dR/dtheta + g_T dT_out/dtheta        theta in pos, scale, quat, opacity, sh
 * into the caller's arrays (grt_gaussian_grads; the caller zeroes them), every discrete decision held fixed as in grt_backward.  It takes
 * no forward outputs: its first sweep recomputes R and T_out.  A ray whose four upstream values are exactly 0 is not traced; nothing goes
 * into opacity or geometry where the 0.99 clamp binds.  Through the context's gradient buffer and its flush exactly as grt_backward.
 * Float atomics: not bitwise reproducible; GRT_OPT_BWD_PLAIN_ATOMICS = 1 makes every lane issue its own (testing).  The distances
 * (t_near, t_far, t_i in depth) and the event set are DATA: no gradients through them, through the rays, or through depth / count
 * (whole rays: grt_ray_depth_* below).  With
 * the event set fixed R and T_out are linear in T_in, so dloss/dT_in = (g_R . R + g_T T_out) / T_in is the caller's to form.
 * Both: asynchronous on `stream` like grt_render; grt_last_kernel_ms reports the call's device time; a view computes its scene's
 * result.  With n = 0 rays or an empty window the calls return GRT_OK and write nothing; with no particles or an empty tree the forward
 * writes untraced values, the backward nothing.
 * Refused with GRT_ERR_INVALID (text in grt_last_error with the entry point's name in front; the context stays usable): everything
 * grt_backward refuses (NULL p, no BVH, GRT_OPT_COUNTERS = 1, sh_degree_max > 3, p->t_min <= 0, a window outside the frame, a NULL ray
 * buffer), meshes set (trace() is the Gaussian-only call), no output (forward: out NULL or all four arrays NULL; backward: out NULL or
 * all five groups NULL), a NULL d_grad_radiance.  GRT_ERR_LIMIT: a BVH so high that its per-lane LDS stacks exceed 160 KiB. */
typedef struct grt_segments {     /* device pointers, [N] float32 each; NULL = the default for every ray */
    const float* t_near;          /* NULL: p->t_min */
    const float* t_far;           /* NULL: p->t_max */
    const float* T_in;            /* NULL: 1 */
} grt_segments;
typedef struct grt_segment_out {  /* device pointers, each may be NULL, not all */
    float* radiance;              /* [N][3]  R = sum_i T_i alpha_i L_i */
    float* T_out;                 /* [N]     T_in * prod_i (1 - alpha_i) */
    float* depth;                 /* [N]     sum_i T_i alpha_i t_i (t_i: the event's key distance, in units of |d|) */
    uint32_t* count;              /* [N]     composited events */
} grt_segment_out;
GRT_API int grt_trace_segments_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const grt_segments* seg,
                                    const grt_segment_out* out, void* stream);
GRT_API int grt_trace_segments_frame(grt_ctx* ctx, const grt_params* p, const grt_segments* seg, const grt_segment_out* out, uint32_t x0,
                                     uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_backward_segments_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, const grt_segments* seg,
                                       const float* d_grad_radiance, const float* d_grad_T_out /* may be NULL */,
                                       const grt_gaussian_grads* out, void* stream);
GRT_API int grt_backward_segments_frame(grt_ctx* ctx, const grt_params* p, const grt_segments* seg, const float* d_grad_radiance,
                                        const float* d_grad_T_out /* may be NULL */, const grt_gaussian_grads* out, uint32_t x0, uint32_t y0,
                                        uint32_t x1, uint32_t y1, void* stream);
/* ---- differentiable ray depth: key or peak distance, two moments, gradients ----
 * grt_aux_out::depth and grt_segment_out::depth are sums over the proxies' entry / exit face distances and carry no gradient.  These
 * calls give a WHOLE ray's distance moments with gradients to the Gaussians and to the ray, for Gaussian-only scenes (depth-supervised
 * fitting, depth-variance regularisers, pose refinement from a depth map).
 * FORWARD.  For a ray (o, d) the events i are exactly those grt_trace_segments_* composites with its defaults (p->t_min, p->t_max,
 * T = 1; p->max_bounces is not looked at).  With w_i = T_i alpha_i and T_out = prod_i (1 - alpha_i):
 *     dist  [N]  sum_i w_i tau_i         accumulated as the aux depth is: (T alpha) tau added before T is updated
 *     dist2 [N]  sum_i w_i tau_i^2       ((T alpha) tau) tau, likewise
 *     T_out [N]  the transmittance behind the ray,   count [N]  composited events
 *     GRT_DEPTH_KEY  (0): tau_i = the event's key distance (the t_i of grt_aux_out::depth)
 *     GRT_DEPTH_PEAK (1): tau_i = d_val,i = -(o_g.d_g) / max(1e-6, d_g.d_g),  o_g = A (o - mu),  d_g = A d,  A = diag(1/s) R^T: the
 *                         distance of the particle's maximum response along the ray (computeResponse, shaders/tracer.cuh:187-214)
 * tau is in units of |d| and is NOT normalised: dist / (1 - T_out) is the mean distance, dist2 / (1 - T_out) - mean^2 its variance.
 * Under PEAK the entry and the exit event of a particle carry the same tau.  tau is NOT clamped to the ray's range and MAY BE NEGATIVE
 * (a particle whose centre lies behind the origin but whose proxy the ray still meets).  With KEY, dist, count and 1 - T_out equal
 * grt_render_rays_aux's depth, count and alpha bit for bit (at max_bounces > 0).  An untraced ray (fisheye r > 1, |d| <= 0.1, a NaN
 * direction, an empty tree) writes 0, 0, T_out = 1, 0.  Every element of the buffer or of the window is WRITTEN once per requested
 * array; pixels outside the window are untouched.  No atomic, no wave operation, no buffer of the context: the call is BITWISE
 * reproducible and windows tile a frame bit for bit.
 * BACKWARD.  Upstreams g_D = dloss/ddist, g_D2 = dloss/ddist2, g_T = dloss/dT_out, [N] each, each may be NULL (zero), not all.  Every
 * discrete decision is held fixed as in grt_backward.  With f_i = g_D tau_i + g_D2 tau_i^2 and S_i = sum_{j>i} w_j f_j:
 *     dloss/dalpha_i = T_i f_i - (S_i + g_T T_out) / (1 - alpha_i)     down to pos, scale, quat, opacity as in grt_backward (zero
 *                                                                      where the 0.99 clamp binds)
 *     dloss/dtau_i   = w_i (g_D + 2 g_D2 tau_i)                        PEAK only; NOT gated by the 0.99 clamp (tau does not pass
 *                                                                      through it).  Under KEY the distances are data.
 * Below tau, with q = max(1e-6, d_g.d_g), a = -d_g / q, p_g = -(o_g + tau d_g) and b = (p_g - tau d_g) / q:
 *     dtau/dmu = A^T d_g / q,   dtau/do = -A^T d_g / q,   dtau/dd = A^T b,   dtau/ds_k = -(a_k o_g,k + b_k d_g,k) / s_k,
 *     dtau/dR_jk = (a_k (o - mu)_j + b_k d_j) / s_k -> q through mat3_cast.
 * Where max(1e-6, .) binds the denominator is a constant (grt_backward_ex's convention): b = -o_g / q.
 *   out->gaussians   ADDED to, by original id: pos, scale, quat, opacity.  A non-NULL sh is left untouched and is not a request.
 *   out->rays        [N][6], WRITTEN: dloss/do = -sum_i m_i + sum_i gtau_i dtau_i/do,  dloss/dd = -sum_i d_val,i m_i + sum_i gtau_i
 *                    dtau_i/dd  (m_i as in grt_backward_ex).  RAW partials with respect to d as the kernel holds it: there is no SH
 *                    term and so no projection; for camera frames the chain to U, V, W is the caller's.  Exact zeros for an untraced
 *                    ray and for a ray whose three upstream values are exactly 0 (such a ray is not traced).  No atomic in its path:
 *                    BITWISE reproducible, with and without the Gaussian output, merged or plain atomics.
 * The Gaussians' gradients go through the context's gradient buffer and its flush exactly as grt_backward's (float atomics, not
 * bitwise reproducible; GRT_OPT_BWD_PLAIN_ATOMICS = 1 as there); a call with out->gaussians NULL allocates no gradient buffer.
 * Both: asynchronous on `stream`; grt_last_kernel_ms reports the call's device time; a view computes its scene's result.  With n = 0
 * rays or an empty window the calls return GRT_OK and write nothing.
 * Refused with GRT_ERR_INVALID (text in grt_last_error with the entry point's name in front; the context stays usable): everything
 * grt_backward refuses, meshes set, an unknown kind, no output (forward: out NULL or all four arrays NULL; backward: out NULL, or rays
 * NULL and no pos / scale / quat / opacity array), no upstream (up NULL or all three NULL). */
enum { GRT_DEPTH_KEY = 0, GRT_DEPTH_PEAK = 1 };
typedef struct grt_depth_out {      /* device pointers, each may be NULL, not all */
    float* dist;                    /* [N]  sum_i w_i tau_i */
    float* dist2;                   /* [N]  sum_i w_i tau_i^2 */
    float* T_out;                   /* [N]  prod_i (1 - alpha_i) */
    uint32_t* count;                /* [N]  composited events */
} grt_depth_out;
typedef struct grt_depth_upstream { /* device pointers, [N] float32 each; each may be NULL (zero), not all */
    const float* dist;
    const float* dist2;
    const float* T_out;
} grt_depth_upstream;
GRT_API int grt_ray_depth_frame(grt_ctx* ctx, const grt_params* p, int kind, const grt_depth_out* out, uint32_t x0, uint32_t y0,
                                uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_ray_depth_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, int kind, const grt_depth_out* out,
                               void* stream);
GRT_API int grt_backward_depth_frame(grt_ctx* ctx, const grt_params* p, int kind, const grt_depth_upstream* up,
                                     const grt_backward_out* out, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_backward_depth_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, int kind,
                                    const grt_depth_upstream* up, const grt_backward_out* out, void* stream);
/* ---- differentiable ray depth of MESH frames: path length through mirrors and glass, with gradients ----
 * The depth calls above for a scene with meshes set (a LiDAR or monocular-depth loss on what a reflection shows, a depth-variance
 * regulariser behind glass, a depth map that includes an opaque mesh's own surface).  A ray runs iterations s = 1..S exactly as
 * documented at grt_backward_mesh and grt_render_features_mesh_frame: its own ray (o_s, d_s) per iteration, its segment
 * [t_min, tmax_s] (tmax_s: the mesh hit distance, for glass with the refraction shift, or t_max), ONE event list with ONE running
 * transmittance carried through `density`, and the segment's colour weight
 *     c_s = 1 - A_{s-1}   Gaussian pass;     D_S (1 - B_{S-1})   last pass;     1   a terminating GRT_NORMAL hit.
 * PATH PREFIX.  P_1 = 0, P_{s+1} = P_s + tmax_s, a float32 running sum per ray.  It is DATA: the mesh hit, its normal and the next
 * ray are held fixed, as in grt_backward_mesh.  Distances are in units of each step's own |d_s|, as the picks' t is.
 * An event i of segment s lies at x_i = P_s + tau_i, with tau_i the event's key distance (GRT_DEPTH_KEY) or the peak distance d_val on
 * the step's ray (o_s, d_s) (GRT_DEPTH_PEAK), and w_i = T_i alpha_i.
 *   step_first, step_last   as for grt_render_features_mesh_frame: 1-based, inclusive; 0, 0 = all; step_last = 0 leaves the range
 *                  open.  An event outside the range is composited — T, A and B run through it — but contributes to no output and
 *                  is not counted.  (2, 0) measures what is seen only through a bounce.
 * FORWARD.  Per segment, in compositing order, float32 without contraction, before T is updated:
 *     m0 += w;   wt = w * x;   m1 += wt;   m2 += wt * x
 * and at the iteration's step   weight += m0 * c_s;   dist += m1 * c_s;   dist2 += m2 * c_s.
 *   flags   GRT_DEPTH_SURFACE: a terminating (GRT_NORMAL) hit whose step is in range adds the surface itself, as the colour adds
 *           ncol (1 - D_S): with u = 1 - D_S and x_S = P_S + tmax_S,  weight += u;  dist += u * x_S;  dist2 += (u * x_S) * x_S.
 *   out     dist, dist2, weight (float32 [N]) and count (uint32 [N], the counted events); each may be NULL, not all.  dist / weight
 *           is the mean path length of what the pixel shows.  An untraced ray writes 0, 0, 0, 0; every element of the window or of
 *           the buffer is WRITTEN once per requested array.  No atomic, no wave operation: BITWISE reproducible, and windows tile
 *           a frame bit for bit.  With surface off, weight is grt_render_features_mesh_frame's output for feat = 1, bit for bit.
 * A context WITHOUT meshes is served: every ray then has one last pass, so dist = (1 - T_out) dist_plain and weight = (1 - T_out)^2.
 * BACKWARD of loss = sum_ray g_D dist + g_D2 dist2 + g_W weight; each upstream may be NULL (zero), not all; every discrete decision
 * held fixed.  A ray whose three upstream values are exactly 0 is not traced.  For a counted event phi_i = g_D x_i + (g_D2 x_i) x_i +
 * g_W, and 0 otherwise; dloss/dalpha_i is grt_backward_features_mesh_frame's with phi_i as its one-channel radiance.  Under
 * GRT_DEPTH_SURFACE a counted terminating step has phi_surf = g_D x_S + g_D2 x_S^2 + g_W, which enters as grt_backward_mesh's ncol
 * term does (gD_S = -phi_surf); the surface has no alpha of its own.  Under PEAK a counted event additionally has
 *     dloss/dtau_i = c_s w_i (g_D + 2 g_D2 x_i),
 * NOT gated by the 0.99 clamp, down to pos, scale and quat on (o_s, d_s) as in grt_backward_depth_frame.  Under KEY the distances are
 * data.  Gradients are ADDED by original id into grads->pos, scale, quat, opacity through the context's gradient buffer and its flush
 * (float atomics; GRT_OPT_BWD_PLAIN_ATOMICS applies); grads->feat is left untouched and is no request, and no sh is touched.
 * Both: asynchronous on `stream`; grt_last_kernel_ms reports the call's device time; a view computes its scene's result; the
 * forward uses no buffer of the context.  With no rays, no particles or an empty tree the calls return GRT_OK: the forward writes
 * zeros, the backward nothing.
 * Refused with GRT_ERR_INVALID (the entry point's name in front; the context stays usable): what the feature calls of mesh frames
 * refuse (NULL p, no BVH, GRT_OPT_COUNTERS = 1, sh_degree_max > 3, t_min <= 0, p->type outside MIRROR/NORMAL/GLASS, step_first >
 * step_last with step_last != 0, a window outside the frame, a NULL ray buffer), an unknown kind, unknown flag bits, no output
 * (forward: out NULL or all four arrays NULL; backward: grads NULL or pos, scale, quat and opacity all NULL), no upstream (up NULL or
 * all three NULL).  GRT_ERR_LIMIT as in the mesh backward.
 * NOT computed: gradients with respect to rays or the camera, gradients through the path (the mesh hit, its normal, the next ray),
 * gradients through P_s. */
#define GRT_DEPTH_SURFACE 1u
typedef struct grt_depth_mesh_out {      /* device pointers, each may be NULL, not all */
    float* dist;                         /* [N]  sum_s c_s sum_{i in s} w_i x_i (+ the surface) */
    float* dist2;                        /* [N]  sum_s c_s sum_{i in s} w_i x_i^2 (+ the surface) */
    float* weight;                       /* [N]  sum_s c_s sum_{i in s} w_i (+ the surface) */
    uint32_t* count;                     /* [N]  counted events */
} grt_depth_mesh_out;
typedef struct grt_depth_mesh_upstream { /* device pointers, [N] float32 each; each may be NULL (zero), not all */
    const float* g_dist;
    const float* g_dist2;
    const float* g_weight;
} grt_depth_mesh_upstream;
GRT_API int grt_ray_depth_mesh_frame(grt_ctx* ctx, const grt_params* p, int kind, uint32_t flags, const grt_depth_mesh_out* out,
                                     uint32_t step_first, uint32_t step_last, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                                     void* stream);
GRT_API int grt_ray_depth_mesh_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, int kind, uint32_t flags,
                                    const grt_depth_mesh_out* out, uint32_t step_first, uint32_t step_last, void* stream);
GRT_API int grt_backward_depth_mesh_frame(grt_ctx* ctx, const grt_params* p, int kind, uint32_t flags,
                                          const grt_depth_mesh_upstream* up, const grt_feature_grads* grads, uint32_t step_first,
                                          uint32_t step_last, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* stream);
GRT_API int grt_backward_depth_mesh_rays(grt_ctx* ctx, const grt_params* p, const float* d_rays, uint64_t n, int kind, uint32_t flags,
                                         const grt_depth_mesh_upstream* up, const grt_feature_grads* grads, uint32_t step_first,
                                         uint32_t step_last, void* stream);
/* ---- point queries: density, occupancy and owner at 3-D points, with gradients ----
 * Every call above answers a question about a ray.  These two answer one about a POINT x of space: how much Gaussian mass lies
 * here, is the point occupied, which particle owns it (marching cubes over an opacity field, occupancy grids and collision
 * queries, placing a mesh outside dense matter, cropping, floater pruning by local density, 3-D regularisers on the field).
 * For particle i with the uploaded (activated) pos mu, scale, quat, opacity o and A = diag(1/scale) R^T as the proxy records hold
 * it (the A of grt_ray_depth_frame above):
 *     y = A (x - mu),   r = exp(-|y|^2 / 2)  (the arithmetic of computeResponse, shaders/tracer.cuh:187-214, at d = 0),
 *     a_i(x) = min(0.99, o r)                (the hit alpha of grt_render, shaders/tracer.cuh:354-357)
 * and particle i CONTRIBUTES at x iff a_i(x) > alpha_min.  A particle with o <= alpha_min never contributes.
 *   alpha_min   0 = the scene's own (grt_build_bvh's).  A value ABOVE the scene's is allowed; one below it is refused: the proxies
 *               (inradius sqrt(2 log(o / alpha_min)) in Gaussian space) do not cover that set, and the call promises the exact set.
 * FORWARD.  Per point, over its contributing particles, [n] each, device pointers, each may be NULL, not all:
 *     density    sum_i a_i
 *     occupancy  1 - prod_i (1 - a_i)        in [0, 1]; independent of the order in exact arithmetic
 *     peak       max_i a_i
 *     peak_id    the ORIGINAL id of that maximum; of equal maxima the lowest id; GRT_PICK_NONE where nothing contributes
 *     count      contributing particles (uint32)
 * A point with a non-finite coordinate, or one that lies in no leaf box of the tree, writes 0, 0, 0, GRT_PICK_NONE, 0.  Every element
 * of every requested array is WRITTEN exactly once.  A split particle counts once (exactly one of its pieces owns a point).  No
 * atomic, no buffer of the context: the same bits from call to call on one tree.  Meshes set on the context are IGNORED (a density
 * does not bounce).  One point per lane: pass points in a SPATIALLY COHERENT order (grid order is one) — the lanes of a wave walk
 * the tree independently and diverge otherwise; the result does not depend on the order.
 * BACKWARD of loss = sum_x g_D density + g_O occupancy, the contributing set held fixed as grt_backward holds every discrete decision:
 *     dloss/da_i = g_D + g_O V / (1 - a_i),   V = prod_j (1 - a_j)   re-derived by a first walk (the forward's outputs are no arguments)
 * and below a_i the chain of grt_backward with v = mu - x; where the 0.99 clamp binds nothing goes into opacity, geometry or the point.
 *   up      g_density, g_occupancy: [n] float32, each may be NULL (zero), not both.  A point whose two values are exactly 0 is not
 *           walked.
 *   grads   pos, scale, quat, opacity: ADDED to, by original id, through the context's gradient buffer and its flush as in
 *           grt_backward (float atomics, not bitwise reproducible).
 *           points [n][3]: WRITTEN once per point with plain stores, dloss/dx = -sum_i m_i with m_i = A^T g_p,i, the value that goes
 *           to pos; exact zeros for a point that is not walked.  BITWISE reproducible, with and without the Gaussians' arrays; a
 *           call with points alone allocates no gradient buffer.
 * peak, peak_id and count carry no gradient.
 * Both: asynchronous on `stream`; grt_last_kernel_ms reports the call's device time; a view queries its parent's scene.  With n = 0
 * or an empty tree the calls return GRT_OK: the forward writes the zeros row, the backward zeros into points only.
 * Refused with GRT_ERR_INVALID (the entry point's name in front; the context stays usable, nothing is written): NULL points with
 * n > 0, no BVH, no output (forward: out NULL or all five arrays NULL; backward: grads NULL or all five arrays NULL), no upstream
 * (up NULL or both NULL), alpha_min below the scene's or not finite.  GRT_ERR_LIMIT: a tree too tall for the per-lane stack, as in
 * grt_backward. */
typedef struct grt_point_out {      /* device pointers, [n] each, each may be NULL, not all */
    float* density;
    float* occupancy;
    float* peak;
    uint32_t* peak_id;
    uint32_t* count;
} grt_point_out;
typedef struct grt_point_upstream { /* device pointers, [n] float32 each; each may be NULL (zero), not both */
    const float* g_density;
    const float* g_occupancy;
} grt_point_upstream;
typedef struct grt_point_grads {    /* device pointers, each may be NULL, not all */
    float* pos;                     /* [N][3] added to */
    float* scale;                   /* [N][3] added to */
    float* quat;                    /* [N][4] added to */
    float* opacity;                 /* [N]    added to */
    float* points;                  /* [n][3] written */
} grt_point_grads;
GRT_API int grt_query_points(grt_ctx* ctx, const float* d_points, uint64_t n, float alpha_min, const grt_point_out* out, void* stream);
GRT_API int grt_backward_points(grt_ctx* ctx, const float* d_points, uint64_t n, float alpha_min, const grt_point_upstream* up,
                                const grt_point_grads* grads, void* stream);
/* Waits for the context's stream and the last frame launched through this context (whatever stream it went to), then
 * reads the sticky device error word: GRT_ERR_LIMIT (text in grt_last_error, word cleared) when a wave had to give up on
 * live rays since the last check — the reference throws on traversal trouble (src/Exception.h:31-80). */
GRT_API int grt_sync(grt_ctx* ctx);
GRT_API int grt_get_counters(grt_ctx* ctx, grt_counters* out); /* syncs; counters of the last render; error word as grt_sync */
/* device time (ms, HIP events on the launch stream) of the last render's kernel; syncs */
GRT_API int grt_last_kernel_ms(grt_ctx* ctx, float* ms);

/* ---- host helpers (no GPU needed) ---- */
/* Raw 3DGS PLY columns -> activated attributes (src/GaussianData.cpp:97-131).  f_rest is [n][45]. */
GRT_API int grt_host_activate(uint64_t n, const float* pos, const float* f_dc, const float* f_rest,
                              const float* opacity_logit, const float* log_scale, const float* rot, float* out_pos,
                              float* out_scale, float* out_quat, float* out_opacity, float* out_sh);
/* Camera::UVWFrame (src/Camera.cpp:3-13) */
GRT_API void grt_host_uvw_frame(const float eye[3], const float lookat[3], const float up[3], float fovy_deg,
                                float aspect, float U[3], float V[3], float W[3]);
/* Deterministic synthetic 3DGS scene: fills raw PLY columns. */
GRT_API int grt_host_synth_scene(uint64_t seed, uint64_t n, float* pos, float* f_dc, float* f_rest,
                                 float* opacity_logit, float* log_scale, float* rot);
/* 3DGS PLY (binary little-endian or ascii; float properties looked up by name as
 * src/GaussianData.cpp:27-92 does).  Two-call pattern: n_out only, then fill. */
GRT_API int grt_host_ply_count(const char* path, uint64_t* n_out);
GRT_API int grt_host_ply_read(const char* path, uint64_t n, float* pos, float* f_dc, float* f_rest,
                              float* opacity_logit, float* log_scale, float* rot);
GRT_API int grt_host_ply_write(const char* path, uint64_t n, const float* pos, const float* f_dc, const float* f_rest,
                               const float* opacity_logit, const float* log_scale, const float* rot);
/* Procedural primitives of the reference (src/geometry/Primitives.cpp:6-140) at the origin: verts[nv][3],
 * normals[nv][3], faces[nf][3].  Two-call pattern: counts, then fill. */
enum { GRT_PRIM_PLANE = 0, GRT_PRIM_SPHERE = 1 };
GRT_API int grt_host_primitive_counts(int kind, uint32_t* nv, uint32_t* nf);
GRT_API int grt_host_primitive_fill(int kind, float* verts, float* normals, uint32_t* faces);
/* OBJ -> un-indexed triangle soup (one vertex per face corner, nf = nv / 3) with the reference's Y flip of positions
 * and normals (src/geometry/Primitives.cpp:142-202).  faces is [nv] = 0..nv-1.  grt_host_obj_write writes
 * "f a//a b//b c//c" with %.9g coordinates (fp32 round-trips). */
GRT_API int grt_host_obj_count(const char* path, uint32_t* nv, uint32_t* nf);
GRT_API int grt_host_obj_read(const char* path, uint32_t nv, float* verts, float* normals, uint32_t* faces);
GRT_API int grt_host_obj_write(const char* path, uint32_t nv, const float* verts, const float* normals, uint32_t nf,
                               const uint32_t* faces);
GRT_API const char* grt_host_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GRT_H */
