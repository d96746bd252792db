/*
 * rtu_render.h — the C-ABI of librtu_hip.so: the MI355X (gfx950) render path.
 *
 * This is the drop-in boundary behind the reference's BeginRender()
 * (main.cpp:66-68 -> SpawnRenderThreads main.cpp:29-64 -> Render
 * RenderFunctions.cpp:55-176). The host keeps the reference's scene graph /
 * RenderImage surface (see rtu_host.h) and calls, per frame:
 *
 *   rtu_create_context      once per GPU                    [no reference counterpart]
 *   rtu_upload_scene        <- the globals LoadScene fills  xmlload.cpp:64-131, main.cpp:17-27
 *   rtu_frame_setup         <- CalculateImageOrigin /       RenderFunctions.cpp:243-269
 *                              CalculateCurrentPoint (hoisted: origin,u,v)
 *   rtu_render_frame[_device] <- the per-pixel loop         RenderFunctions.cpp:62-174 with
 *                              PixelIterator::GetPixelLocation (PixelIterator.h:25-38),
 *                              Trace/ShadowTrace (RenderFunctions.cpp:181-240),
 *                              Object::IntersectRay (objFunctions.cpp:15-522),
 *                              MtlBlinn::Shade (mtlFunctions.cpp:120-298),
 *                              Light::Illuminate (lightFunctions.cpp:27-84, lights.h:32,48)
 *   rtu_destroy_context
 *
 * Output is linear float4 {r,g,b,z} per pixel (z = hInfo.z of the primary hit,
 * RTU_BIGFLOAT on a miss); gamma / Color24 / z-image stay on the host
 * (rtu_host.h) as in RenderFunctions.cpp:155-159 and scene.h:590-612.
 *
 * Plain pointers and sizes only; never throws; returns 0 or a negative RTU_ERR_*.
 * A context is single-caller. The caller owns host buffers; the library owns
 * its device buffers (scene, counters, recursion arena, default framebuffer).
 */
#ifndef RTU_RENDER_H_INCLUDED
#define RTU_RENDER_H_INCLUDED

#include "rtu_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTU_OK               0
#define RTU_ERR_ARG         (-1)  /* NULL / out-of-range argument */
#define RTU_ERR_HIP         (-2)  /* a HIP runtime call failed (see rtu_last_error) */
#define RTU_ERR_UNSUPPORTED (-3)  /* scene exceeds a device-path limit */
#define RTU_ERR_STOCHASTIC  (-4)  /* soft shadows / glossy bounces / depth of field in a frame with samples == 0 */
#define RTU_ERR_NO_SCENE    (-5)  /* render before rtu_upload_scene */
#define RTU_ERR_NO_DEVICE   (-6)  /* no such GPU */
#define RTU_ERR_CAPACITY    (-7)  /* more Shade() frames than provisioned (see rtu_frame_status) */
#define RTU_ERR_CANCELLED   (-8)  /* the caller's cancel flag was raised (rtu_set_cancel_flag, RtuProgress): StopRender(), main.cpp:70-72 */
#define RTU_ERR_SCENE_SHAPE (-9)  /* rtu_update_scene: not the shape of the uploaded scene (rtu_last_error names the first difference) */
#define RTU_ERR_STALE       (-10) /* a progressive session's context got a new scene (rtu_upload_scene / rtu_update_scene) */

#define RTU_BAND_ROWS 8  /* image rows per band; one wavefront renders an 8x8 pixel tile */

typedef struct RtuContext RtuContext;

/* One frame. Bands of RTU_BAND_ROWS rows are dealt round-robin to shards:
 * band b belongs to shard (b % shard_count); a context renders only its shard
 * and writes it COMPACTLY (local row lr -> global row rtu_shard_global_row). */
typedef struct RtuFrameDesc {
    int32_t width, height;
    int32_t shard_rank, shard_count;  /* 0,1 for a single GPU */
    int32_t max_bounce;               /* the bounceCount every root Shade() call of the frame receives (the reference passes 5,
                                         RenderFunctions.cpp:134-135; rtu_frame_setup sets 5): Shade() recurses through that many
                                         reflections / refractions and is its light loop alone at 0. Recipe P: both calls of the pixel
                                         and both of every gather bounce (:569-570) receive it. 0 .. RTU_MAX_BOUNCE, else RTU_ERR_ARG;
                                         the frames of one rtu_render_frames_device call must agree in it. A scene without a
                                         reflective or refractive material renders at 0 whatever is asked (the image is the same) */
    int32_t collect_stats;            /* 1: fill the ray / traversal counters RtuStats (the counting variant: the reference's own
                                         tree, no culling — slower); 2: the FAST variant as it is timed, counting per kernel what it
                                         touches (RtuTouched) */
    int32_t coop_threshold;           /* tuning: a deferred-ray list shorter than this is traced by the
                                         cooperative (8 lanes per ray) kernels; 0 = default */
    int32_t samples;                  /* 0: recipe W, one ray through every pixel centre (scenes with stochastic
                                         features are refused, RTU_ERR_STOCHASTIC). S >= 1: recipe S, the sample loop
                                         of Render() (RenderFunctions.cpp:73-152) with S samples per pixel: Halton
                                         pixel offsets, depth of field, soft shadows, glossy bounces, on the sample
                                         streams described below; rgb = mean of the samples, z = mean hInfo.z of the
                                         samples that hit */
    float   cam_pos[3];               /* camera.pos */
    float   origin[3];                /* CalculateImageOrigin(camera.focaldist) */
    float   u[3], v[3];               /* per-pixel steps of CalculateCurrentPoint */
    float   lens_up[3];               /* camera.up (as given) and normalize(dir x up): the lens disk of */
    float   lens_right[3];            /* RenderFunctions.cpp:93 */
    float   dof;                      /* camera.dof */
    int32_t gather_bounces;           /* 0, or 4 with samples >= 1: recipe P (config 5) — recipe S plus the Monte-Carlo gather
                                         of Render() (RenderFunctions.cpp:129-135: MonteCarlo with monteCarloBounces = 4 and one
                                         cosine-weighted hemisphere sample per bounce, :549-590, :320-337). Keys: the hit of the
                                         gather ray has child_key(key, 3), the Shade() tree lit by MonteCarlo()'s AmbientLight
                                         child_key(key, 4); purposes 0x40000, 0x40001: sampleX, samplePhi */
} RtuFrameDesc;

/* Sample streams of recipe S. The reference draws from rand() (shared by its threads, seeded with the
 * time: RenderFunctions.cpp:60), which nothing can reproduce. Here every rand() call becomes
 *     rand31(key, purpose) = mix32(key ^ mix32(purpose * 0x9e3779b9 + 0x85ebca6b)) >> 1     in [0, RAND_MAX]
 *     mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 * inside the reference's own float expressions. key belongs to one Shade() call: the primary hit of sample
 * i of pixel p (p = x + width * y in the whole image, whatever the sharding) has
 *     sample_key(p, i) = mix32(mix32(p + 0x68bc21eb) ^ (i * 0x9e3779b9 + 1)),
 * the Shade() of the hit of its secondary ray `slot` (0 refracted or totally reflected, 1 Fresnel
 * reflection, 2 mirror reflection) has child_key(key, slot) = mix32(key + (slot + 1) * 0x632be5ab).
 * purpose: 0, 1 lens sample (sampleX, sampleTheta); 16 + 2 l, 17 + 2 l light l's disk sample (sampleR,
 * sampleTheta); 0x10000 / 0x20000 / 0x30000 + 3 a + {0,1,2}: attempt a of SampleSphere for the first /
 * second refraction normal and for the reflection normal. sin, cos (and, recipe P, acos) of the sampled
 * angles are evaluated in binary64 with IEEE operations only and rounded to float (portable_sincos /
 * portable_acos in raytracer-utah_amd/csrc/rtu_intersect.h state the sequences), within one ulp of libm's. */

/* Ray and traversal counters of one frame (all shards of one context). Same
 * fields as RtuOracleStats so CPU and GPU can be compared exactly. */
typedef struct RtuStats {
    uint64_t primary_rays, primary_hits;
    uint64_t secondary_rays;  /* root-level Trace calls issued by Shade */
    uint64_t shadow_rays;     /* root-level ShadowTrace calls issued by Shadow */
    uint64_t node_tests;      /* ray x object-node intersection calls */
    uint64_t mesh_entries;    /* rays that passed a mesh's bounding box */
    uint64_t inner_visits, leaf_visits, leaf_elems;
    uint64_t tri_tests, tri_accepts;
} RtuStats;

int         rtu_device_count(void);
const char* rtu_error_string(int err);

/* What the machine says about GPU `device_id` (hipGetDeviceProperties): bench.py derives the HBM peak of its roofline from the
 * memory clock and bus width reported here ("confirm on the machine, do not hard-code") and falls back to the
 * constant of the microarchitecture guide when the figures are implausible. Needs no context. */
typedef struct RtuDeviceInfo {
    int32_t  compute_units, clock_khz, memory_clock_khz, memory_bus_bits;
    uint64_t l2_bytes, hbm_bytes;
    char     name[64], arch[64];
} RtuDeviceInfo;
int         rtu_device_info(int device_id, RtuDeviceInfo* out);

RtuContext* rtu_create_context(int device_id, int* err_out);
void        rtu_destroy_context(RtuContext* ctx);
const char* rtu_last_error(const RtuContext* ctx);

/* Validate, flatten into the device layout and copy to HBM. May be called again
 * to replace the scene. */
int  rtu_upload_scene(RtuContext* ctx, const RtuSceneDesc* scene);

/* The validation rtu_upload_scene runs first, on its own: every index the kernels follow (node parents, mesh,
 * material and texture ids, vertex / normal / texture-vertex indices, BVH children, leaf ranges, element ids) is
 * range-checked so that a malformed scene is an error code, never an out-of-bounds access on the GPU. Pure host
 * code, needs no GPU and no context; the message goes to err_buf (may be NULL). */
int  rtu_validate_scene(const RtuSceneDesc* scene, char* err_buf, size_t err_len);

/* Change the uploaded scene in place: node transformations (tm / itm / pos) and materials, every field of every light (type and
 * count too, within the limits of rtu_upload_scene), material values and material_maps, background / environment, camera. The
 * SHAPE must be the uploaded scene's: the same n_nodes and, per node, parent, obj_type, mesh_id, depth and subtree_end; the same
 * n_meshes and, per mesh, nv, nf, nvn, nvt and n_bvh_nodes; the same n_textures and, per texture, type, width and height; the
 * same n_materials; material_maps present in both or in neither. Otherwise RTU_ERR_SCENE_SHAPE. The mesh and texture arrays
 * of `scene` are not read beyond those headers: the copies uploaded before are used (vertex edits: rtu_update_meshes; new images need
 * rtu_upload_scene). The acceleration structures of the meshes and the textures stay; node records, node-level bounds, cover
 * meshes and occluder lists of shadow rays (built on the GPU, equal to what rtu_upload_scene builds for the same scene),
 * materials, lights and launch hints are rebuilt. RTU_ERR_NO_SCENE before any upload; a scene rtu_upload_scene would refuse
 * gets the same code. A refused update leaves the context as it was. Synchronous: waits for every launch in flight on the
 * context's streams first, so a batch enqueued before the call renders the old scene. */
int  rtu_update_scene(RtuContext* ctx, const RtuSceneDesc* scene);

/* Deform uploaded meshes in place. It is rtu_update_scene(ctx, scene) and, before the placement is rebuilt, for every mesh i of
 * mesh_ids[n_meshes] the arrays v, vn, bvh, elements and the header fields n_bvh_nodes, bvh_depth, bound_min, bound_max of
 * scene->meshes[i] are read and replace the uploaded ones (a host scene edited with rtu_scene_set_mesh_vertices, rtu_host.h, has
 * them ready). nv, nf, nvn, nvt and n_elements must be the uploaded mesh's (RTU_ERR_SCENE_SHAPE); n_bvh_nodes of a LISTED mesh may
 * differ, of an unlisted one not. f, fn, ft, vt are not read: the uploaded connectivity is used. n_meshes == 0 is rtu_update_scene.
 * Everything is validated before anything is written, and a refused call leaves the context as it was: ids in range and not
 * repeated (RTU_ERR_ARG); for each listed mesh what rtu_upload_scene checks of bvh / elements (child indices, leaf ranges, element
 * ids, bvh_depth not understated: RTU_ERR_ARG) and bvh_depth <= RTU_MAX_BVH_STACK (RTU_ERR_UNSUPPORTED).
 * Replaced per listed mesh: v, vn (copied); the `ref` tree (renumbered as at upload), its element order and triangle records,
 * any_empty_box, the mesh box and cull scale, n_bvh_nodes; the triangle records of the fast tree; the boxes of its collapsed
 * forms bvh4 / bvh8 — REFITTED on the GPU: each child box is the exact min / max (comparisons only) of the vertex coordinates of
 * the triangles in that child's range of element slots, the float VALUES a build of that topology would store (-0 and +0 are one
 * value; a NaN coordinate drops out as it does in the builder); triangle records are the upload's arithmetic bit for bit. KEPT: the
 * fast tree's topology — its element order, every ref word of bvh4 / bvh8, the LDS staging, rtu_mesh_info, the stack need of the
 * 4-wide walk. The topology stays that of the last UPLOAD however many updates follow: images never depend on it (exact ties,
 * stack overflows and the counting variant go through the `ref` tree), frame times may — after a large deformation a fresh
 * rtu_upload_scene can render faster. The shape the context remembers takes the new n_bvh_nodes and bounds (a later
 * rtu_update_scene / rtu_scene_shape_diff compares against the mesh as it is now); progressive sessions turn RTU_ERR_STALE; launch
 * hints are cleared. The `ref` tree's device buffer only grows: a sequence of updates that needs no growth allocates nothing.
 * Synchronous; waits for both of the context's streams first. RTU_ERR_NO_SCENE before any upload. */
int  rtu_update_meshes(RtuContext* ctx, const RtuSceneDesc* scene, const uint32_t* mesh_ids, int n_meshes);

/* Deform uploaded meshes from DEVICE memory: rtu_update_meshes for a caller whose vertices are made on the GPU (skinning, cloth, a
 * torch module). Only the vertices (and, if it has new ones, the normals) are handed over; the reference tree, which the host path
 * takes from rtu_scene_set_mesh_vertices, is REBUILT ON THE GPU (csrc/rtu_ref_build.h), bit for bit. Afterwards the context holds,
 * for each listed mesh, what rtu_scene_set_mesh_vertices + rtu_update_meshes would have left there for the same vertices: v, vn,
 * the `ref` tree (breadth-first), its element order and triangle records, the fast tree's records, any_empty_box, the mesh box,
 * scale, n_bvh_nodes, bvh_depth and the walks' stack need by bits; the refitted boxes of bvh4 / bvh8 by value.
 *   edits[i].mesh   the mesh; ids in range and not repeated (RTU_ERR_ARG).
 *   edits[i].d_v    float [3 nv] in device memory (NULL: RTU_ERR_ARG).
 *   edits[i].d_vn   float [3 nvn] in device memory, or NULL: the normals the context holds stay — or, with
 *                   RTU_MESH_EDIT_RECOMPUTE_NORMALS, are recomputed from d_v as rtu_scene_recompute_normals does (ComputeNormals,
 *                   bit for bit), which is allowed under that function's condition only: one normal per vertex and fn == f as
 *                   uploaded, else RTU_ERR_ARG. d_vn together with the flag, or an unknown flag: RTU_ERR_ARG.
 * `scene` is read as rtu_update_scene reads it; of scene->meshes[i] for a LISTED mesh only nv, nf, nvn, nvt and n_elements are
 * compared (RTU_ERR_SCENE_SHAPE) — its arrays, n_bvh_nodes, bvh_depth and bounds are not read: the host scene is stale by design.
 * hip_stream is the stream the vertices were produced on: the call orders its reads after that stream's work with an event (no
 * device-wide synchronisation) and is itself synchronous, like rtu_update_meshes. n_edits == 0 is rtu_update_scene.
 * Everything that can be checked first is; the one thing that cannot — a tree deeper than RTU_MAX_BVH_STACK, RTU_ERR_UNSUPPORTED as
 * in the host path — is known after the build, so the build goes into scratch, its header is read back and validated, and only
 * then is anything the kernels read replaced. A refused call leaves the context as it was. The shape the context remembers takes
 * the new n_bvh_nodes, bvh_depth and bounds: rtu_context_mesh_shape gives the header to put into the descriptor of a later
 * rtu_update_scene / rtu_update_meshes. Progressive sessions turn RTU_ERR_STALE, launch hints are cleared, rtu_keep_previous_vertices
 * works as for rtu_update_meshes. All scratch is grow-only: the first update of a mesh allocates, later ones nothing. */
#define RTU_MESH_EDIT_RECOMPUTE_NORMALS 1u
typedef struct RtuMeshDeviceEdit {
    uint32_t    mesh, flags;
    const void* d_v;    /* float[3 nv], device memory */
    const void* d_vn;   /* float[3 nvn], device memory; NULL keeps the uploaded normals,
                           or, with RECOMPUTE_NORMALS, has them recomputed from d_v */
} RtuMeshDeviceEdit;
int  rtu_update_meshes_device(RtuContext* ctx, const RtuSceneDesc* scene, const RtuMeshDeviceEdit* edits, int n_edits, void* hip_stream);
/* The header of mesh `mesh` as the context remembers it (nv, nf, nvn, nvt, n_bvh_nodes, n_elements, bvh_depth, bounds); arrays NULL. */
int  rtu_context_mesh_shape(RtuContext* ctx, uint32_t mesh, RtuMesh* header_out);

/* The shape check of rtu_update_scene on its own: RTU_OK when `b` has the shape of `a`, else RTU_ERR_SCENE_SHAPE with the first
 * difference in err_buf (may be NULL); RTU_ERR_ARG for a missing array. Pure host code. */
int  rtu_scene_shape_diff(const RtuSceneDesc* a, const RtuSceneDesc* b, char* err_buf, size_t err_len);

/* Fill width/height, cam_pos/origin/u/v from the camera (fp64 tan chain of
 * RenderFunctions.cpp:247 evaluated on the host, once per frame), single shard,
 * max_bounce 5, no stats. Pure host arithmetic; needs no GPU. */
int  rtu_frame_setup(const RtuCamera* camera, int width, int height, RtuFrameDesc* frame_out);

/* Shard geometry helpers (pure arithmetic). */
int  rtu_shard_rows(const RtuFrameDesc* frame);                    /* rows this shard renders */
int  rtu_shard_max_rows(int height, int shard_count);             /* max over ranks (gather padding) */
int  rtu_shard_global_row(const RtuFrameDesc* frame, int local_row);

/* Render this context's shard into DEVICE memory d_rgbz (rtu_shard_rows * width
 * float4, 16-byte aligned), asynchronously on hip_stream (a hipStream_t passed
 * as void*; NULL = the device's default stream, as in HIP itself). Inputs are already resident in
 * HBM; nothing is copied.
 * ONE STREAM PER CONTEXT between two rtu_frame_status calls: the context's frame records, append counters, camera table,
 * coverage masks and tile-occupancy words are shared by every launch sequence queued on it, and only stream order keeps
 * one sequence's kernels from another's. A caller that wants two sequences in flight on two streams uses two contexts
 * (bench.py and rtu_multi_render_frame do); switching streams after rtu_frame_status (which waits for the device) is fine. */
int  rtu_render_frame_device(RtuContext* ctx, const RtuFrameDesc* frame, void* d_rgbz, void* hip_stream);

/* Frames in flight: n_frames (<= RTU_MAX_FRAMES_IN_FLIGHT, and at most 2^26 pixels together) frames of recipe W of the uploaded scene — the same resolution, shard and
 * options, each with its own camera (cam_pos / origin / u / v) — rendered by ONE launch sequence into
 * d_rgbz = n_frames consecutive shard images (frame i at float4 offset i * rtu_shard_rows * width).
 * One 1080p frame at one sample per pixel is too little work to fill 256 CUs: sixteen in
 * flight render at 2.4 times the rays per second. Every frame is the image rtu_render_frame_device
 * gives for it, bit for bit. Asynchronous; rtu_frame_status afterwards as for a single frame. */
#define RTU_MAX_FRAMES_IN_FLIGHT 128
int  rtu_render_frames_device(RtuContext* ctx, const RtuFrameDesc* frames, int n_frames, void* d_rgbz, void* hip_stream);

/* The content of the reference's RenderImage from a rendered float4 image, on the device: d_z[i] = z,
 * d_rgb8[3 i ..] = Color24(pow(c, 1/2.2)) (RenderFunctions.cpp:152-160; binary64 pow, cyColor.h:226 clamp) —
 * 7 bytes per pixel instead of 16, which is what a multi-GPU gather should move. Asynchronous on hip_stream.
 * (The host path, rtu_image_from_rgbz, does the same with glibc's pow; the two agree except where the device
 * library's pow rounds a value sitting on a byte boundary the other way: within the +-1 level bar.) */
int  rtu_pack_image_device(RtuContext* ctx, const void* d_rgbz, size_t n_pixels, void* d_z, void* d_rgb8, void* hip_stream);

/* The two OUTPUT images of a batch of rendered frames, 4 bytes per pixel {r, g, b of Color24, z-image byte}: what Result.png and
 * ZBuffer.png are written from (main.cpp:59-61), and what a multi-GPU gather has to move when the frame rate makes the link to
 * the root the bottleneck (10 000 frames per second x 14.5 MB of float z + Color24 exceed one xGMI link). The z-image needs the
 * FRAME-wide zmin / zmax (ComputeZBufferImage, scene.h:590-612):
 *   rtu_minmax_z_device   d_minmax[2 i], [2 i + 1] (int64 each) = order-preserving keys of zmin and of zmax of frame i over this
 *                         shard's pixels (frame i at float4 offset i * pixels_per_frame), encoded so that the element-wise MINIMUM of
 *                         the arrays of all shards is the frame's (one all-reduce MIN of 2 n_frames int64; a single GPU skips it);
 *   rtu_pack_output_device quantises with those: byte = int((zmax - z) / (zmax - zmin) * 255) clamped, 0 for a miss, in binary32 with
 *                         a correctly rounded division, exactly as the reference; colours as rtu_pack_image_device.
 * Both asynchronous on hip_stream. */
int  rtu_minmax_z_device(RtuContext* ctx, const void* d_rgbz, size_t pixels_per_frame, int n_frames, void* d_minmax, void* hip_stream);
int  rtu_pack_output_device(RtuContext* ctx, const void* d_rgbz, size_t pixels_per_frame, int n_frames, const void* d_minmax, void* d_out4,
                            void* hip_stream);

/* Render into the context's own framebuffer and copy the shard to host memory
 * h_rgbz (rtu_shard_rows * width * 4 floats). Synchronous. stats may be NULL. */
int  rtu_render_frame(RtuContext* ctx, const RtuFrameDesc* frame, float* h_rgbz, RtuStats* stats);

/* After rtu_render_frame_device: wait for the device and report whether the frame is
 * complete. The Shade() recursion is evaluated level by level in pre-sized frame
 * arrays (one frame per pixel per level to begin with); RTU_ERR_CAPACITY means a level
 * overflowed: the arrays are re-provisioned from the counts the frame reported — render the
 * frame again (at most one round per recursion level). rtu_render_frame does the check and
 * the re-render itself. The report is STICKY: it covers every launch sequence queued on this context since the
 * previous rtu_frame_status (or synchronous render), not only the last one — a caller that pipelines several
 * rtu_render_frame(s)_device calls with different cameras and checks once learns that SOME frame of them is
 * incomplete and renders them again. */
int  rtu_frame_status(RtuContext* ctx);

/* ---- Adaptive sampling: recipes S / P that stop sampling a pixel once its samples agree ------------------------------------------
 * What the reference's sample loop declares next to maxSampleSize (RenderFunctions.cpp:26-29: minSampleSize = 8, targetVariance = 0.005,
 * sampleIncrement = 1) and what RenderImage::sampleCount / ComputeSampleCountImage keep (scene.h:545-546, 614-635).
 * An adaptive frame is a recipe S or P frame (samples >= 1, gather_bounces 0 or 4); frame.samples is the MAXIMUM per pixel, in [1, 255]
 * (the reference stores counts as uchar). Sample i of a pixel is the sample i of the fixed render with frame.samples samples: the same
 * key, the same pixel offset. Per pixel and channel, in binary32 with every operation rounded, in sample order:
 *     s += x (the sum of the fixed render), q += x * x;
 * at each checkpoint n = min_samples + k * increment < frame.samples: m = s / n, var = (q - s * m) / (n - 1) (n as float; n == 1:
 * var = +inf). The pixel STOPS at n when var <= target_variance for r, g and b, otherwise at frame.samples. Its rgb is s / n, its z the
 * mean z over the samples among its first n that hit, its count n. The decision depends on the pixel's own samples only — never on how
 * the samples are grouped into batches — so a pixel that stops at n is, bit for bit, the mean of the first n samples of the fixed render.
 * A pixel that has stopped is not traced any more: its rays are never spawned. */
#define RTU_MAX_BATCH 16  /* samples rendered by one launch sequence of recipes S / P, at most */
typedef struct RtuAdaptiveDesc {
    int32_t min_samples;      /* first checkpoint, in [1, samples] (minSampleSize) */
    int32_t increment;        /* >= 1 (sampleIncrement) */
    float   target_variance;  /* >= 0, +inf allowed (every pixel stops at min_samples); NaN refused (targetVariance) */
    int32_t max_batch;        /* samples per launch sequence, at most: 0 = the library's choice, else 1 .. RTU_MAX_BATCH (no effect on results) */
} RtuAdaptiveDesc;
/* The reference's constants: 8, 1, 0.005f, 0. */
int  rtu_adaptive_defaults(RtuAdaptiveDesc* out);
/* Render this shard adaptively and copy it to the host: h_rgbz as rtu_render_frame (rtu_shard_rows * width float4), h_counts
 * (may be NULL) the samples each pixel took (rtu_shard_rows * width bytes). Synchronous; stats (may be NULL) selects the counting
 * variant as for rtu_render_frame. shard_rank / shard_count are honoured (keys are global: the shards assemble to the single-GPU
 * image). The cancel flag is polled between batches. RTU_ERR_ARG: samples outside [1, 255], gather_bounces not 0 / 4, min_samples
 * outside [1, samples], increment < 1, a NaN or negative target, max_batch outside [0, RTU_MAX_BATCH]. */
int  rtu_render_frame_adaptive(RtuContext* ctx, const RtuFrameDesc* frame, const RtuAdaptiveDesc* adaptive, float* h_rgbz, uint8_t* h_counts,
                               RtuStats* stats);
/* The same into DEVICE memory (d_rgbz as rtu_render_frame_device, d_counts rtu_shard_rows * width bytes, may be NULL), queued on
 * hip_stream; like a sampled rtu_render_frame_device it synchronises per batch (the host sizes the next batch's launch from the
 * number of tiles still sampling). rtu_frame_status afterwards as for a single frame. */
int  rtu_render_frame_adaptive_device(RtuContext* ctx, const RtuFrameDesc* frame, const RtuAdaptiveDesc* adaptive, void* d_rgbz, void* d_counts,
                                      void* hip_stream);
/* Diagnostic: render samples [first, first + n) of the FIXED recipe S / P frame `frame` and copy their images — what the accumulator
 * adds, n x rtu_shard_rows x width float4 {r, g, b, z}, z = RTU_BIGFLOAT for a miss — to h_out. Synchronous. */
int  rtu_debug_sample_images(RtuContext* ctx, const RtuFrameDesc* frame, int first, int n, float* h_out);

/* ---- Progressive rendering: a recipe S / P frame refined call by call, shown at any time -------------------------------------------
 * What the reference's viewport shows while Render() runs (viewport.cpp:390-449): the image fills in and can be stopped. A SESSION keeps
 * the running sums of one frame between calls. frame is a recipe S or P frame (samples >= 1, gather_bounces 0 or 4, collect_stats 0);
 * frame.samples is the TARGET count S — it fixes the pixel offsets index / S + Halton(index, 4|5) (RenderFunctions.cpp:80-85), so it is
 * known from the start. Shards are honoured. adaptive (may be NULL: every pixel takes every sample) is checked as for
 * rtu_render_frame_adaptive (then S <= 255). RTU_ERR_ARG for anything else; *err_out (may be NULL) gets the code.
 *   rtu_progressive_advance   traces samples [done, done + n) in the batches of the one-shot render (RTU_MAX_BATCH, 2^25 pixels,
 *                             max_batch), each checked for capacity and rendered again if need be before it is added; the cancel flag
 *                             (rtu_set_cancel_flag) is polled before every batch: RTU_ERR_CANCELLED with done at the last batch added, the
 *                             session still usable. n < 1 or done + n > S: RTU_ERR_ARG. An adaptive session whose pixels have all stopped
 *                             traces nothing (done still advances). Synchronous: on return the sums are complete on `hip_stream`.
 *                             RTU_ERR_STALE once the context got a new scene (rtu_upload_scene / rtu_update_scene).
 *   rtu_progressive_status    samples done, and the 8x8 tiles that still sample: the length of an adaptive session's active-tile list
 *                             (all tiles before the first batch), all tiles of a fixed one until done == S, then 0. Either pointer may be NULL.
 *   rtu_progressive_snapshot  the image now, the session left as it is: pixel p with n samples so far (done; adaptive: its own count,
 *                             min(done, its stop)) is rgb = s / n, z = (sum of z) / hits (RTU_BIGFLOAT without a hit) — the binary32
 *                             operations of the one-shot resolve, so a session driven to S is the one-shot image bit for bit, and after
 *                             any pass the mean of each pixel's first n samples. counts (may be NULL; only when S <= 255) receives n.
 *                             done == 0: RTU_ERR_ARG. Still answers after RTU_ERR_STALE. The _device form writes d_rgbz (rtu_shard_rows
 *                             * width float4) and d_counts asynchronously on hip_stream; the host form is synchronous.
 * The session owns its sums (none of the context's own): a render on the same context between two calls neither disturbs it nor is
 * disturbed by it, and several sessions may be open on one context. rtu_destroy_context frees the device memory of its open sessions;
 * every call on such a handle but rtu_progressive_free then returns RTU_ERR_ARG. Messages: rtu_last_error of the context. */
typedef struct RtuProgressive RtuProgressive;
RtuProgressive* rtu_progressive_begin(RtuContext* ctx, const RtuFrameDesc* frame, const RtuAdaptiveDesc* adaptive, int* err_out);
int  rtu_progressive_advance(RtuProgressive* p, int n_samples, void* hip_stream);
int  rtu_progressive_status(const RtuProgressive* p, int32_t* samples_done, uint32_t* live_tiles);
int  rtu_progressive_snapshot_device(RtuProgressive* p, void* d_rgbz, void* d_counts, void* hip_stream);
int  rtu_progressive_snapshot(RtuProgressive* p, float* h_rgbz, uint8_t* h_counts);
void rtu_progressive_free(RtuProgressive* p);

/* ---- Ray queries: the scene along caller-supplied rays (raytracer-utah_amd/csrc/rtu_query.hip) ---------------------------------------
 * What the reference's viewport does for the pixel under the mouse (PrintPixelData), for any ray: picking, line of sight, depth for
 * a sensor that is no pinhole, baking. A ray is answered from the uploaded scene AS IT IS NOW (rtu_update_scene / rtu_update_meshes
 * included) by the walk the renders use.
 *   closest hit  Trace(ray) with HitInfo::Init's z replaced by tmax (RenderFunctions.cpp:181-212): t = hInfo.z, node = the hit node,
 *                material = its material_id (-1: none), p / N = hInfo.p / hInfo.N in world space (after FromNodeCoords),
 *                RTU_RAY_FRONT = hInfo.front. A miss: flags 0, t = tmax, node = material = -1, p = N = 0. The only bias is the
 *                reference's own acceptance thresholds (t > 0.001 on spheres and planes, t > 0.00001 on triangles): there is no tmin.
 *                As in the reference, a ray that starts inside a sphere whose far side lies beyond tmax reports that sphere with
 *                t = tmax (the stale-z branch of Sphere::IntersectRay, objFunctions.cpp:60-99).
 *   occlusion    ShadowTrace(ray) on the same start value, then GenLight::Shadow's conclusion `hit && hInfo.z > 0`
 *                (RenderFunctions.cpp:214-240, lightFunctions.cpp:27-37): 1 or 0 per ray. The occluder lists of the lights do not apply.
 * dir is used exactly as given — never renormalised, so the rays of rtu_camera_rays reproduce a render bit for bit — and must be of
 * unit length: the conservative bounds of the fast walk were argued, and are tested, for the renderer's own rays. A ray is INVALID
 * and is not traced when a component of org, dir or tmax is NaN or infinite, when tmax <= 0, or when |dot(dir, dir) - 1| > 2e-3
 * (binary32, (x x + y y) + z z): it gets RTU_RAY_INVALID with the values of a miss, or 0 from the occlusion form.
 * Textures are not evaluated; uvw, face index and barycentrics are not reported (rtu_ray_features adds the textured albedo of the hit,
 * rtu_ray_surface those three).
 * flags: 0, or RTU_QUERY_REFERENCE_WALK for the walk of the counting variant (the reference's own tree, no culling, no node-level
 * bounds): every field of every answer is the same, bit for bit; it is slower. rtu_debug_walk_stack_limit and rtu_debug_node_bounds
 * apply as to a render; rtu_debug_flags does not.
 * Errors: RTU_ERR_ARG for an unknown flag bit, for a NULL pointer with n > 0 and for a device pointer that is not 16-byte aligned
 * (d_occluded: any alignment); RTU_ERR_NO_SCENE before rtu_upload_scene. n == 0 is RTU_OK and launches nothing.
 * The _device forms read n RtuRay from and write n RtuRayHit (n bytes) to DEVICE memory, allocate nothing and are asynchronous on
 * hip_stream (NULL: the default stream). They read the scene's buffers only and touch none of the context's frame state — frame
 * records, counters, launch hints, the sticky report of rtu_frame_status. rtu_upload_scene and rtu_update_* wait for the context's OWN streams only: the caller synchronises hip_stream
 * before calling them. The host forms copy through buffers of the context (grow-only, at most 2^20 rays at a time) on the
 * context's stream and are synchronous. */
typedef struct RtuRay    { float org[3]; float tmax; float dir[3]; uint32_t reserved; } RtuRay;      /* 32 B */
typedef struct RtuRayHit { float t; int32_t node; uint32_t flags; int32_t material;
                           float p[3]; float pad0; float N[3]; float pad1; } RtuRayHit;               /* 48 B */
#define RTU_RAY_HIT      1u   /* something was hit in front of tmax */
#define RTU_RAY_FRONT    2u   /* HitInfo::front */
#define RTU_RAY_INVALID  4u   /* not traced: see above */
#define RTU_QUERY_REFERENCE_WALK 1u  /* flags argument: the counting variant's walk (the reference's tree, no culling) */
int  rtu_trace_rays_device(RtuContext* ctx, const void* d_rays, size_t n, uint32_t flags, void* d_hits, void* hip_stream);
int  rtu_occluded_rays_device(RtuContext* ctx, const void* d_rays, size_t n, uint32_t flags, void* d_occluded, void* hip_stream);
int  rtu_trace_rays(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t flags, RtuRayHit* h_hits);
int  rtu_occluded_rays(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t flags, uint8_t* h_occluded);
/* The primary rays of a render: the pixel-centre rays of image rows [row0, row0 + nrows) of `frame` (its camera, width and height;
 * shards and samples are ignored), width * nrows of them in image order, tmax = RTU_BIGFLOAT. The binary32 expressions are the
 * kernels' own (RenderFunctions.cpp:258-268, :97: cp = (origin + u * (x + 0.5f)) + v * (y + 0.5f), dir = normalize(cp - cam_pos)),
 * so rtu_trace_rays of them gives the z of rtu_render_frame bit for bit. Pure host code, needs no GPU and no context. RTU_ERR_ARG:
 * NULL frame, width or height < 1, rows outside the image, NULL rays_out with nrows > 0. */
int  rtu_camera_rays(const RtuFrameDesc* frame, int row0, int nrows, RtuRay* rays_out);

/* ---- Ray batches: radiance along caller-supplied rays (raytracer-utah_amd/csrc/render_rays_impl.h) -----------------------------------
 * What a render gives a pinhole camera's pixels, for any ray: a panoramic, fisheye or orthographic sensor, an environment probe, a
 * light-map bake, a re-shade of chosen pixels. Per ray one float4 {r, g, b, t}, linear, like a render's pixel:
 *   hit      the ray is traced as by rtu_trace_rays — Trace(ray) with HitInfo::Init's z replaced by tmax, dir used exactly as given —;
 *            rgb = Shade(ray, hInfo, lights, max_bounce) of the hit node's material (MtlBlinn::Shade, mtlFunctions.cpp:115-291: shadow
 *            rays, refraction / Fresnel / mirror recursion, textures: the hit carries uvw), t = hInfo.z. A node without a material gives
 *            white, as in a render. The stale-z sphere of rtu_trace_rays (t = tmax) is a hit and is shaded as the reference would.
 *   miss     rgb = environment.SampleEnvironment(dir), t = tmax: what the reference does for every ray that is not a pixel (a reflected
 *            or refracted ray that leaves the scene, mtlFunctions.cpp:250, :267, :289). The background is a function of the pixel, and
 *            a ray has none.
 *   invalid  (the rule of the ray queries above) {0, 0, 0, 0}, not traced. t == 0 means nothing else: a valid ray has tmax > 0.
 * eye is the `camera.pos` of Shade()'s view vector (mtlFunctions.cpp:137) for the root call AND every bounce, as the reference's single
 * camera is: the rays of rtu_camera_rays shaded with eye = cam_pos give rtu_render_frame's rgb at every hit pixel and its z at every
 * pixel, bit for bit (a miss pixel of a render shows the background instead). One eye per call.
 * flags: 0, or RTU_QUERY_REFERENCE_WALK for the counting variant (collect_stats = 1 of a frame: the reference's tree, every Shade() call
 * a frame); the output is the same, bit for bit. max_bounce as RtuFrameDesc.max_bounce (0 where no material recurses).
 * A scene with stochastic features is refused (RTU_ERR_STOCHASTIC) as a samples == 0 frame is: these two calls are recipe W.
 * rtu_shade_rays_sampled / rtu_shade_rays_sampled_device below shade rays by recipe S, each ray on the sample stream of its own key.
 * Errors: RTU_ERR_ARG for a NULL pointer with n > 0 (or a NULL descriptor), a device pointer that is not 16-byte aligned, an unknown flag
 * bit, non-zero reserved, max_bounce outside 0 .. RTU_MAX_BOUNCE, a non-finite eye, n > 2^26 in the device form; RTU_ERR_NO_SCENE before
 * rtu_upload_scene. n == 0 is RTU_OK and launches nothing.
 * THIS CALL IS A RENDER, unlike the ray queries: it uses the context's frame records, append counters and launch hints (under a key of
 * its own), and the ONE STREAM PER CONTEXT rule of rtu_render_frame_device applies. The _device form reads n RtuRay from and writes n
 * float4 to DEVICE memory and is asynchronous on hip_stream; rtu_frame_status afterwards as for a frame — RTU_ERR_CAPACITY: call it
 * again —, rtu_get_stats after a RTU_QUERY_REFERENCE_WALK call as after a counting render. The host form copies through grow-only
 * buffers of the context in chunks of at most 2^20 rays, checks capacity and repeats a chunk itself, and is synchronous; stats non-NULL
 * selects the counting variant, the counters summed over the chunks (of camera rays: the RtuStats of the frame).
 * rtu_debug_flags 64 and 2048, rtu_debug_node_bounds, rtu_debug_walk_stack_limit and rtu_debug_tail_from apply as to a render and change
 * no bit. The touched-bytes mode (collect_stats == 2) does not exist for ray batches. */
typedef struct RtuShadeDesc {      /* 32 B */
    float    eye[3];      /* the `camera.pos` of MtlBlinn::Shade's view vector (mtlFunctions.cpp:137), for the root call and every bounce */
    int32_t  max_bounce;  /* bounceCount of the root Shade() calls, 0 .. RTU_MAX_BOUNCE; as RtuFrameDesc.max_bounce */
    uint32_t flags;       /* 0, or RTU_QUERY_REFERENCE_WALK: the counting variant (the reference's tree, every call a frame) */
    uint32_t reserved[3]; /* must be 0 */
} RtuShadeDesc;
int  rtu_shade_defaults(RtuShadeDesc* out);   /* eye 0, max_bounce 5, flags 0; pure host code */
int  rtu_shade_rays_device(RtuContext* ctx, const void* d_rays, size_t n, const RtuShadeDesc* desc, void* d_rgbt, void* hip_stream);
int  rtu_shade_rays(RtuContext* ctx, const RtuRay* h_rays, size_t n, const RtuShadeDesc* desc, float* h_rgbt, RtuStats* stats);

/* ---- Sampled ray batches: recipe S along caller-supplied rays (render_rays2.hip / render_rays3.hip) ---------------------------------
 * rtu_shade_rays with ONE Shade() call of RECIPE S per ray (direct lighting only: gather_bounces 0; rtu_shade_rays_paths / _device below
 * add the Monte-Carlo gather of recipe P per ray): soft shadows and glossy bounces on
 * the sample streams stated above ("Sample streams of recipe S"). keys[i] is the `key` of ray i's root Shade() call — what
 * sample_key(p, i) is to a sample of a pixel: the disk sample of light l draws from rand31(key, 16 + 2 l ...), the glossy normals of the
 * root call from 0x10000 / 0x20000 / 0x30000 ..., and the Shade() of the hit of secondary ray `slot` continues with
 * child_key(key, slot), exactly as behind a render's primary hit. The answer to a ray depends on the scene, the eye, max_bounce, that
 * ray and that key — not on its index, the batch size or the order. Whatever the caller needs for the ray itself (a lens point, an
 * offset inside a pixel) it draws itself; purposes 0 and 1 are free for that, and rtu_camera_sample_rays uses them as the renders
 * do. One sample per ray: averaging is the caller's (several keys per direction, e.g. rtu_sample_key(direction index, k)).
 * hit / miss / invalid / a node without material, eye, max_bounce, flags (RTU_QUERY_REFERENCE_WALK), stats, RtuRay.reserved (ignored)
 * and every error are as for rtu_shade_rays; RtuShadeDesc is the same structure under the same rules. A scene WITHOUT stochastic
 * features is accepted: its arithmetic is recipe S's on that scene, which draws nothing. d_keys / h_keys: n uint32, 4-byte aligned
 * (RTU_ERR_ARG otherwise, and for NULL with n > 0).
 * The calls are renders, as rtu_shade_rays: frame records, append counters, launch hints (under a key of their own — neither a sampled
 * frame's nor an unsampled batch's), the ONE STREAM PER CONTEXT rule, rtu_frame_status after the _device form (RTU_ERR_CAPACITY: call
 * it again), n <= 2^26 in the _device form; the host form copies rays and keys through grow-only buffers of the context in chunks of at
 * most 2^20 rays, repeats a chunk that ran out of capacity itself, and is synchronous. rtu_debug_flags 64 and 2048,
 * rtu_debug_node_bounds, rtu_debug_walk_stack_limit and rtu_debug_tail_from apply and change no bit.
 * Against a render: the rays and keys of rtu_camera_sample_rays(frame, k) shaded with eye = cam_pos are sample k of the recipe S frame
 * — rtu_debug_sample_images(frame, k, 1) — bit for bit in t at every ray and in rgb at every hit ray (a miss shows the environment
 * where a render shows the background). */
int  rtu_shade_rays_sampled_device(RtuContext* ctx, const void* d_rays, const void* d_keys, size_t n, const RtuShadeDesc* desc, void* d_rgbt,
                                   void* hip_stream);
int  rtu_shade_rays_sampled(RtuContext* ctx, const RtuRay* h_rays, const uint32_t* h_keys, size_t n, const RtuShadeDesc* desc, float* h_rgbt,
                            RtuStats* stats);
/* ---- Path-traced ray batches: recipe P along caller-supplied rays (render_rays4.hip / render_rays5.hip, render_paths_impl.h) ---------
 * rtu_shade_rays_sampled with the 4-bounce Monte-Carlo gather of recipe P behind every hit (RenderFunctions.cpp:129-135, :549-590,
 * :320-337): indirect light for a light-map bake, an environment probe, a fisheye or panoramic sensor. Per ray one float4 {r, g, b, t}
 * under the rules of rtu_shade_rays_sampled, except:
 *   hit      rgb = Shade(h0, lights + MonteCarlo's AmbientLight) + Shade(h0, lights), exactly what a recipe-P sample of a pixel gets
 *            (:134-135); t = hInfo.z. A node without material gives white, t = hInfo.z, and gathers nothing.
 *   miss     environment.SampleEnvironment(dir), t = tmax. An invalid ray: sixteen zero bytes, not traced, no chain.
 *   keys     keys[i] is the key of ray i's root call. The hemisphere sample at a chain hit draws from that hit's key with purposes
 *            0x40000 / 0x40001, the gather ray's hit continues with child_key(key, 3), the AmbientLight tree with child_key(key, 4):
 *            all as stated for RtuFrameDesc.gather_bounces. The gather depth is the reference's 4 (monteCarloBounces); it is not a
 *            parameter. eye and max_bounce apply to every Shade() tree of the chain, as cam_pos and max_bounce of a recipe-P frame do.
 * Against a render: the rays and keys of rtu_camera_sample_rays(frame, k) shaded with eye = cam_pos equal
 * rtu_debug_sample_images(frame with gather_bounces = 4, k, 1) bit for bit — t at every ray, rgb at every hit ray.
 * flags, stats, RtuRay.reserved and every error are as for the sampled pair (NULL and misaligned pointers, unknown flag bits, reserved,
 * max_bounce, a non-finite eye, RTU_ERR_NO_SCENE; n == 0 is RTU_OK and launches nothing); a scene without stochastic features is
 * accepted. LIMIT: a chain costs 352 bytes of chain records and results (5 depths x 4 float4 + 2 float4), so the _device form takes
 * the recipe-P frame path's own cap on chains per launch sequence: n <= 2^25 (the 2^25 pixels a batch of samples of a recipe S / P
 * frame may have by default; the frame path's tuning knob RTU_GI_BATCH_LOG2 does not move this limit), RTU_ERR_ARG beyond. The host form works in chunks of at most 2^20 rays.
 * THE CALL IS A RENDER: it uses the context's frame records, append counters, chain records and results (grow-only, shared with
 * recipe-P frames) and launch hints under a key of its own; the ONE STREAM PER CONTEXT rule applies. The _device form queues the whole
 * sequence asynchronously on hip_stream — the roots, four chain steps, five shading steps from the deepest depth up, the final sum —;
 * rtu_frame_status afterwards reports completeness, and on RTU_ERR_CAPACITY the caller calls the _device form again. The host form
 * repeats the shading steps of a chunk itself with the grown capacities (chain records do not depend on them) and is synchronous.
 * The counting variant (RTU_QUERY_REFERENCE_WALK, or stats non-NULL in the host form) gives the same bytes; its counters are summed
 * over the chunks; gather rays are in no ray counter, as in a recipe-P frame (their traversal counters are). As a recipe-P frame with
 * counters, the host form does not repeat a counting chunk that ran out of frame records: it returns RTU_ERR_CAPACITY — shade the
 * batch once without counters first. rtu_debug_flags 64 and 2048, rtu_debug_node_bounds, rtu_debug_walk_stack_limit and
 * rtu_debug_tail_from apply and change no bit; a cut level forced by rtu_debug_tail_from skips the chain steps, which have no recursion
 * levels, and applies to all five shading steps of the next call (in the host form: of its first chunk's first attempt). */
int  rtu_shade_rays_paths_device(RtuContext* ctx, const void* d_rays, const void* d_keys, size_t n, const RtuShadeDesc* desc, void* d_rgbt,
                                 void* hip_stream);
int  rtu_shade_rays_paths(RtuContext* ctx, const RtuRay* h_rays, const uint32_t* h_keys, size_t n, const RtuShadeDesc* desc, float* h_rgbt,
                          RtuStats* stats);
/* ---- The two halves of a recipe-P sample (render_rays6.hip / render_rays7.hip, render_gather_impl.h) ----------------------------------
 * rtu_shade_rays_paths is Shade(h0, lights + AmbientLight(c)) + Shade(h0, lights) with c = what MonteCarlo(h0, 4) gathered behind the
 * ray's hit (RenderFunctions.cpp:549-590, :134-135). These two pairs hand out c alone and take one from outside, so that the indirect
 * term can be computed where it is needed and reused where it is not (the irradiance map below; a light-map bake; a probe):
 *   rtu_gather_rays          per ray one float4 {c.r, c.g, c.b, t}: c the intensity of the AmbientLight that MonteCarlo(hInfo, 4) appends
 *                            for the ray's root hit and key — the roots, the four chain steps and the shading steps of depth 4 .. 1 of
 *                            rtu_shade_rays_paths, then the sum of depth 0 written out instead of consumed. A miss, an invalid ray and a
 *                            node without material give c = 0 (nothing is gathered for them); t as rtu_shade_rays_paths: hInfo.z, tmax on
 *                            a miss, 0 for an invalid ray.
 *   rtu_shade_rays_ambient   per ray {r, g, b, t} of a recipe-S ray batch whose root call is lit by lights + AmbientLight(amb[i]): the two
 *                            trees of :134-135, the ambient one on child_key(keys[i], 4). amb: n float4 {r, g, b, ignored}, 16-byte
 *                            aligned in the _device form. No gather ray is traced. amb enters as (0 + amb) + 0, the sum MonteCarlo()
 *                            itself forms (:568-570): amb bit for bit, but for a negative zero, which becomes +0. Miss / invalid /
 *                            no material as rtu_shade_rays_paths.
 * rtu_shade_rays_ambient(rays, keys, rtu_gather_rays(rays, keys)) is rtu_shade_rays_paths(rays, keys) byte for byte; with amb = 0 it is
 * rtu_shade_rays_sampled plus what the ambient tree sees of the environment through reflection and refraction (nothing on a scene
 * whose environment is black or whose materials are childless: the same bytes there).
 * keys, eye, max_bounce, flags (RTU_QUERY_REFERENCE_WALK), stats, every error, n <= 2^25 in the _device forms, the chunks of the host
 * forms and THE CALL IS A RENDER are as stated for rtu_shade_rays_paths; so is the capacity rule: rtu_frame_status after a _device
 * form, RTU_ERR_CAPACITY: call it again. Both share the context's chain records with recipe-P frames and path-traced batches. */
int  rtu_gather_rays_device(RtuContext* ctx, const void* d_rays, const void* d_keys, size_t n, const RtuShadeDesc* desc, void* d_ct, void* hip_stream);
int  rtu_gather_rays(RtuContext* ctx, const RtuRay* h_rays, const uint32_t* h_keys, size_t n, const RtuShadeDesc* desc, float* h_ct, RtuStats* stats);
int  rtu_shade_rays_ambient_device(RtuContext* ctx, const void* d_rays, const void* d_keys, const void* d_amb, size_t n, const RtuShadeDesc* desc,
                                   void* d_rgbt, void* hip_stream);
int  rtu_shade_rays_ambient(RtuContext* ctx, const RtuRay* h_rays, const uint32_t* h_keys, const float* h_amb, size_t n, const RtuShadeDesc* desc,
                            float* h_rgbt, RtuStats* stats);
/* The primary rays and keys of sample `sample` (0 <= sample < frame->samples) of the recipe S frame `frame`, image rows
 * [row0, row0 + nrows), width * nrows of each in image order; shards are ignored. key = sample_key(x + width * y, sample); the pixel
 * offset is sample / S + Halton(sample, 4 | 5) in x | y (RenderFunctions.cpp:80-85, :96); the origin is the lens point
 * (cam_pos + lens_up * (rad * sin)) + lens_right * (rad * cos) with rad = sqrt((sampleX * dof) * dof), sampleX = rand31(key, 0) / 2^31,
 * the angle rand31(key, 1) / float(RAND_MAX / 2 pi) through portable_sincos (:88-93); dir = normalize(cp - origin), tmax = RTU_BIGFLOAT.
 * The binary32 expressions are the kernels' own in the same order. Pure host code, needs no GPU and no context. RTU_ERR_ARG: NULL
 * frame, width or height < 1, samples < 1, sample outside [0, samples), rows outside the image, a NULL output with nrows > 0. */
int  rtu_camera_sample_rays(const RtuFrameDesc* frame, int sample, int row0, int nrows, RtuRay* rays_out, uint32_t* keys_out);
/* The same on the device (k_camera_sample_rays, raytracer-utah_amd/csrc/rtu_camrays.hip, one lane per pixel): width * height RtuRay to
 * d_rays and as many keys to d_keys, image order, the bits of rtu_camera_sample_rays(frame, sample, 0, height, ...) — a new sample of a
 * frame costs no upload. Needs no scene, allocates nothing, asynchronous on hip_stream. RTU_ERR_ARG as the host form, and for a NULL
 * context, a NULL d_rays or d_keys, d_rays not 16-byte or d_keys not 4-byte aligned, more than 2^26 pixels. */
int  rtu_camera_sample_rays_device(RtuContext* ctx, const RtuFrameDesc* frame, int sample, void* d_rays, void* d_keys, void* hip_stream);
uint32_t rtu_sample_key(uint32_t pixel, uint32_t sample);   /* sample_key(p, i) as stated above; pure host code */
uint32_t rtu_child_key(uint32_t key, uint32_t slot);        /* child_key(key, slot) as stated above; pure host code */

/* ---- Ray sorting: a coherent order for caller-supplied rays (raytracer-utah_amd/csrc/rtu_raysort.hip, rtu_raysort.h) ----------------------
 * The five ray entries above answer rays in whatever order they come, and pay for an incoherent one: neighbouring lanes walk different
 * parts of the scene (a shuffled batch costs 1.2 to 2.3 times the same rays in image order). These calls bring a batch into
 * a coherent order on the GPU, so that a caller can sort, call any entry UNCHANGED on the sorted buffers, and put the answers back:
 *     rtu_ray_order_device(ctx, d_rays, n, d_order, s);
 *     rtu_permute_device(ctx, d_rays, d_sorted, d_order, n, 32, 0, s);      (and the keys of a sampled batch: elem_bytes 4)
 *     rtu_trace_rays_device(ctx, d_sorted, n, 0, d_hits_sorted, s);
 *     rtu_permute_device(ctx, d_hits_sorted, d_hits, d_order, n, 48, 1, s);
 * Every entry answers a ray whatever its index (a sampled ray: whatever its index, given its key), so d_hits holds the bytes the
 * unsorted call writes.
 *   THE BOX  rtu_ray_sort_box: lo[3], hi[3] — the union of the finite node-level bounds of the uploaded scene as it is now (kept at
 *            rtu_upload_scene, refreshed by rtu_update_scene / rtu_update_meshes); [-w, w]^3 with w the largest |coordinate| of the scene
 *            when no node has a finite bound. RTU_ERR_NO_SCENE before an upload. A box is DEGENERATE when a bound is not finite, when
 *            hi < lo on an axis or when hi - lo is not finite: every spatial cell is then 0, and no ray misses.
 *   THE KEY  rtu_ray_sort_keys (pure host code, needs no GPU and no context; RTU_ERR_ARG: NULL box, a NULL array with n > 0) and the
 *            kernel evaluate, in binary32 with one rounding per operation, in this order (min / max are comparisons):
 *              an INVALID ray (the rule of the ray queries above)                                           0xFFFFFFFF
 *              inside = lo <= org <= hi on every axis; if not inside (and the box is not degenerate):
 *                t0 = 0, t1 = tmax; per axis k = x, y, z: dir[k] == 0: a miss if org[k] < lo[k] or org[k] > hi[k], else nothing;
 *                otherwise ta = (lo[k] - org[k]) / dir[k], tb = (hi[k] - org[k]) / dir[k], t0 = max(t0, min(ta, tb)),
 *                t1 = min(t1, max(ta, tb)); t0 > t1: a miss. A valid ray that MISSES the box has key 0x40000000 | directional (below):
 *                behind every ray that enters the box, and still ordered by direction — such rays are shaded too (the environment)
 *              p = org if inside, else org + t0 * dir, clamped to [lo, hi] per axis
 *              cell[k] = min(15, (int)floorf((p[k] - lo[k]) / (hi[k] - lo[k]) * 16.0f)), 0 where hi[k] - lo[k] is 0;
 *              spatial = the 12-bit Morton code of the cells: bit i of cell x, y, z at bit 3 i, 3 i + 1, 3 i + 2
 *              s = (|dx| + |dy|) + |dz|, px = dx / s, py = dy / s; dz < 0: (px, py) = ((1 - |py|) * sgn(px), (1 - |px|) * sgn(py)) with
 *              sgn(a) = a >= 0 ? 1 : -1 (the octahedral map); u = px * 0.5f + 0.5f, v = py * 0.5f + 0.5f,
 *              qu = clamp((int)floorf(u * 512.0f), 0, 511), qv likewise; directional = the 18-bit Morton code: bit i of qu, qv at bit
 *              2 i, 2 i + 1
 *              key = spatial << 18 | directional                                                             (30 bits; a miss: bit 30)
 *            No libm function is involved, so host and device agree bit for bit.
 *   THE ORDER rtu_ray_order_device writes order[0 .. n) (uint32, DEVICE memory), the permutation that sorts the keys of the n rays at
 *            d_rays in the context's box STABLY — equal keys keep their index order: order = argsort(keys, stable), a pure function of
 *            the rays and the scene. Ray order[i] of the batch is ray i of the sorted batch. Asynchronous on hip_stream. The scratch
 *            (keys and indices double-buffered, digit histograms: 16 bytes per ray) is grow-only storage of the context, so the ONE STREAM
 *            PER CONTEXT rule of rtu_render_frame_device applies to this call: two orderings, or an ordering and a render, in flight
 *            on two streams need two contexts. It is no render: it touches no frame record, counter, launch hint or rtu_frame_status
 *            report. rtu_ray_order is the synchronous host form (rays and order copied through grow-only buffers of the context).
 *            RTU_ERR_ARG: n > 2^26, a NULL pointer with n > 0, d_rays not 16-byte or d_order not 4-byte aligned, a NULL context;
 *            RTU_ERR_NO_SCENE before rtu_upload_scene; n == 0 is RTU_OK and launches nothing. An order stays a valid permutation
 *            after the scene changes; it is then the order of the scene it was computed for.
 *   PERMUTE  rtu_permute_device: scatter == 0: dst[i] = src[order[i]] (rays and keys going in); scatter == 1: dst[order[i]] = src[i]
 *            (answers coming out), for n elements of elem_bytes = 1 (occlusion bytes), 4 (keys), 16 (float4), 32 (RtuRay) or 48
 *            (RtuRayHit). Stateless: any stream, no scene needed. RTU_ERR_ARG: another elem_bytes, scatter not 0 / 1, n > 2^26, a NULL
 *            pointer with n > 0, src == dst, src or dst not aligned to min(elem_bytes, 16) or order not to 4 bytes. The kernel does NOT
 *            validate order: an index >= n is the caller's error (an out-of-bounds access), and the buffers must not overlap. */
int  rtu_ray_sort_box(const RtuContext* ctx, float box_out[6]);
int  rtu_scene_sort_box(const RtuSceneDesc* scene, float box_out[6]);   /* the box rtu_upload_scene(scene) would keep: pure host code (validates the scene first) */
int  rtu_ray_sort_keys(const float box[6], const RtuRay* rays, size_t n, uint32_t* keys_out);
int  rtu_ray_order_device(RtuContext* ctx, const void* d_rays, size_t n, void* d_order, void* hip_stream);
int  rtu_ray_order(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t* h_order);
int  rtu_permute_device(RtuContext* ctx, const void* d_src, void* d_dst, const void* d_order, size_t n, uint32_t elem_bytes, int scatter,
                        void* hip_stream);

/* ---- Sensors: images for cameras that are no pinhole (raytracer-utah_amd/csrc/rtu_sensor.hip, rtu_sensor.h) ---------------------------
 * The ray entries above answer rays; a SENSOR is what fires them and averages the answers: the renderer's outer loop — rays and keys
 * written on the GPU where the shading kernels read them, the batch loop with its capacity check, the sums in sample order, the exact
 * mean — for a panoramic (equirectangular), a fisheye (equidistant) and an orthographic sensor. The shading behind the rays is
 * rtu_shade_rays_device / _sampled_device / _paths_device unchanged, so an image is tied to them bit for bit.
 *   samples == 0, gather_bounces 0   recipe W: one ray per pixel at offset (0.5, 0.5); a stochastic scene: RTU_ERR_STOCHASTIC
 *   samples S >= 1, gather_bounces 0 recipe S: sample k at ox = (float)k * (float)(1.0 / S) + halton(k, 4), oy likewise with base 5 —
 *                                    the offsets of rtu_camera_sample_rays —, key = rtu_sample_key(x + width * y, k). Purposes 0 and
 *                                    1 of the key stay undrawn: a sensor has no lens.
 *   samples S >= 1, gather_bounces 4 recipe P, offsets and keys as recipe S
 * THE RAY of pixel (x, y) with offsets (ox, oy): binary32, one rounding per operation, in the order written; sincos is the
 * portable_sincos of the sample streams; tmax = RTU_BIGFLOAT. u = ((float)x + ox) / (float)width, v = ((float)y + oy) / (float)height.
 *   RTU_SENSOR_EQUIRECT  u >= 1: u -= 1; v > 1: v = 1 (the offsets reach into [0, 2)). lon = u * 6.2831855f, pol = v * 3.1415927f,
 *                        (sl, cl) = sincos(lon), (sp, cp) = sincos(pol), h = forward * (-cl) + right * (-sl),
 *                        dir = norm3(up * cp + h * sp), org = pos: the centre column looks along forward, the top row along up.
 *   RTU_SENSOR_FISHEYE   (equidistant) R = 0.5f * (float)min(width, height), dx = (((float)x + ox) - 0.5f * (float)width) / R, dy likewise
 *                        with y and height, r = sqrtf(dx * dx + dy * dy). r > 1: outside the image circle: org = pos, dir = 0 — an
 *                        INVALID ray by the rule of the ray queries: never traced, sixteen zero bytes. r == 0: dir = forward. Otherwise
 *                        a = r * (fov_deg * 0.008726646f) (within [0, pi] for fov_deg <= 360), (sa, ca) = sincos(a),
 *                        dir = norm3(forward * ca + (right * (dx / r) + up * (-(dy / r))) * sa), org = pos.
 *   RTU_SENSOR_ORTHO     org = (pos + right * ((u - 0.5f) * extent[0])) + up * ((0.5f - v) * extent[1]), dir = forward.
 * rtu_sensor_rays (pure host code, needs no GPU and no context) is the specification of these expressions: the rays and keys of
 * sample `sample` for image rows [row0, row0 + nrows), width * nrows of each in image order, under the row and argument rules of
 * rtu_camera_sample_rays. samples == 0: sample must be 0, keys are rtu_sample_key(pixel, 0) (no entry reads them for recipe W).
 * rtu_sensor_rays_device writes the same bits for samples [sample0, sample0 + nsamples) into DEVICE memory, sample-major: ray
 * (k - sample0) * pixels + pixel (pixels = width * height), d_rays 16-byte aligned (32 bytes per ray), d_keys 4-byte aligned or NULL.
 * Asynchronous on hip_stream, allocates nothing, needs no scene and touches nothing of the context but its device id: any stream.
 * The buffers go as they are to rtu_trace_rays_device / rtu_occluded_rays_device (depth, visibility) or to the shading entries.
 * THE IMAGE  rtu_render_sensor / rtu_render_sensor_device: per pixel one float4 {r, g, b, z}; with n = max(samples, 1):
 *   rgb = (the sum of the samples' rgb in sample order, binary32) / n; z = (the sum of t over the samples that hit) / their number, or
 *   RTU_BIGFLOAT when none hit — the resolve of a recipe S frame. A miss adds the environment colour (as for every ray batch) and is
 *   no hit; a sample outside the fisheye circle adds zeros and is no hit (t == 0 identifies it); a hit adds its colour, and t to z.
 * pos is the eye of every Shade() call (one eye per call, as RtuShadeDesc.eye), flags (0 or RTU_QUERY_REFERENCE_WALK) and max_bounce go
 * to the shading entry; the image is the same with and without the flag, byte for byte. Both calls are RENDERS as the ray batches
 * are (frame records, counters, launch hints; ONE STREAM PER CONTEXT) but leave the frame accumulators and every progressive session
 * alone: rays, keys, samples and sums live in grow-only buffers of their own, so a second call of the same shape allocates nothing.
 * They run batches of at most min(RTU_MAX_BATCH, 2^25 / pixels) samples; a batch that ran out of frame records is shaded again with
 * the grown capacities (the counting variant of recipe P returns RTU_ERR_CAPACITY, as rtu_shade_rays_paths does); the cancel flag is
 * polled before every batch (RTU_ERR_CANCELLED). Both forms return when the image is complete — the _device form has then waited
 * for hip_stream —, and rtu_frame_status is clean afterwards.
 * RTU_ERR_ARG: a NULL descriptor or output, an unknown model, width or height < 1, width * height > 2^25, a non-finite pos, frame
 * vector, fov_deg or extent, a frame vector with |dot(a, a) - 1| > 2e-3 or a pair with |dot(a, b)| > 2e-3 (the band of the ray rule;
 * the vectors are used as given), fov_deg outside (0, 360] (fisheye), an extent <= 0 (orthographic), samples < 0 or > 65536,
 * gather_bounces not 0 / 4 or 4 with samples == 0, max_bounce outside 0 .. RTU_MAX_BOUNCE, an unknown flag bit, non-zero reserved, a
 * misaligned device pointer; rtu_sensor_rays_device: sample0 / nsamples outside the samples, more than 2^26 rays. RTU_ERR_NO_SCENE
 * (the render entries) before rtu_upload_scene. */
#define RTU_SENSOR_EQUIRECT 0
#define RTU_SENSOR_FISHEYE  1
#define RTU_SENSOR_ORTHO    2
typedef struct RtuSensorDesc {     /* 128 B */
    int32_t  model;                /* RTU_SENSOR_* */
    int32_t  width, height;
    int32_t  samples;              /* as RtuFrameDesc.samples: 0 recipe W, S >= 1 recipes S / P */
    int32_t  gather_bounces;       /* as RtuFrameDesc.gather_bounces: 0, or 4 for recipe P */
    int32_t  max_bounce;           /* as RtuFrameDesc.max_bounce */
    uint32_t flags;                /* 0, or RTU_QUERY_REFERENCE_WALK */
    float    pos[3];               /* ray origin (equirectangular, fisheye), window centre (orthographic); the eye of every Shade() call */
    float    right[3], up[3], forward[3];  /* an orthonormal frame, used as given */
    float    fov_deg;              /* fisheye: the full angle, in (0, 360] */
    float    extent[2];            /* orthographic: width and height of the window in world units, > 0 */
    uint32_t reserved[10];         /* must be 0 */
} RtuSensorDesc;
/* Writes exactly sizeof(RtuSensorDesc) bytes: an equirectangular 1 x 1 sensor at the origin, right +x, up +y, forward -z, samples 0,
 * gather_bounces 0, max_bounce 5, flags 0, fov_deg 180, extent 1 x 1. Pure host code. */
int  rtu_sensor_defaults(RtuSensorDesc* out);
int  rtu_sensor_rays(const RtuSensorDesc* sensor, int sample, int row0, int nrows, RtuRay* rays_out, uint32_t* keys_out);
int  rtu_sensor_rays_device(RtuContext* ctx, const RtuSensorDesc* sensor, int sample0, int nsamples, void* d_rays, void* d_keys, void* hip_stream);
int  rtu_render_sensor(RtuContext* ctx, const RtuSensorDesc* sensor, float* h_rgbz);
int  rtu_render_sensor_device(RtuContext* ctx, const RtuSensorDesc* sensor, void* d_rgbz, void* hip_stream);
/* Diagnostic: on != 0 brackets the two kernels of later sensor renders (k_sensor_rays, k_sensor_accumulate) and each whole render with
 * HIP events on the render's stream (it then waits for every batch's accumulation); ms_out3 (may be NULL) gets the milliseconds summed
 * since the previous call: {k_sensor_rays, k_sensor_accumulate, the renders}; they are reset. The images do not change. */
int  rtu_debug_sensor_timing(RtuContext* ctx, int on, float* ms_out3);

/* ---- Adaptive sensors: a sensor that stops sampling a pixel once its samples agree (raytracer-utah_amd/csrc/rtu_sensor_adaptive.hip,
 * rtu_sensor_adaptive.h) ----
 * "Adaptive sampling" above, for sensors. The sensor is a recipe S or P sensor; sensor.samples is the MAXIMUM per pixel, in [1, 255]
 * (counts are bytes, as for frames); samples == 0 (recipe W) is RTU_ERR_ARG. adaptive is the RtuAdaptiveDesc of the frame entries under
 * their checks: min_samples in [1, samples], increment >= 1, a target that is neither NaN nor negative (+inf allowed), max_batch in
 * [0, RTU_MAX_BATCH], which has no effect on results.
 * SAMPLE IDENTITY  Sample i of a pixel is sample i of the fixed sensor with sensor.samples samples: the offsets of
 * rtu_sensor_rays(sensor, i) and the key rtu_sample_key(x + width * y, i).
 * THE RULE is the frame rule word for word, applied to the {r, g, b, t} the sensor accumulator adds (a fisheye sample outside the image
 * circle adds zeros and is no hit). Per pixel and channel, in binary32 with every operation rounded, in sample order:
 *     s += x, q += x * x;
 * at each checkpoint n = min_samples + k * increment < samples: var = (q - s * (s / n)) / (n - 1) (n as float; n == 1: var = +inf). The
 * pixel STOPS at n when var <= target_variance for r, g and b — a NaN variance never stops —, otherwise at samples. Its rgb is s / n,
 * its z the mean t of the hits among its first n samples, or RTU_BIGFLOAT when none hit; its count is n. So a pixel that stops at n is,
 * bit for bit, the mean of the first n samples rtu_render_sensor would sum, and min_samples == samples gives rtu_render_sensor's bytes.
 * The decision never depends on how the samples are grouped into batches: a pixel that passes a checkpoint inside a batch ignores
 * the rest of that batch.
 * A stopped pixel's rays are never generated: after the first batch the rays are those of a list of live pixels, kept on the device
 * in ascending pixel order; the next batch has min(max_batch or RTU_MAX_BATCH, 2^25 / live pixels, samples - done) samples, and the
 * loop ends when the list is empty. Both calls are RENDERS as rtu_render_sensor is (ONE STREAM PER CONTEXT); they touch the sensor
 * buffers and buffers of their own — never the frame accumulators, a progressive or a temporal session —, and a second call of one
 * shape allocates nothing. A batch that ran out of frame records is shaded again before it is added (the counting variant of recipe P
 * returns RTU_ERR_CAPACITY, as rtu_render_sensor does); the cancel flag is polled before every batch (RTU_ERR_CANCELLED);
 * rtu_frame_status is clean on return. rtu_render_sensor_adaptive is synchronous: h_rgbz width * height float4, h_counts (may be NULL)
 * width * height bytes. rtu_render_sensor_adaptive_device writes DEVICE memory (d_rgbz 16-byte aligned, d_counts may be NULL), queues
 * on hip_stream and synchronises once per batch, as rtu_render_frame_adaptive_device does: it returns when the image is complete.
 * RTU_ERR_ARG, RTU_ERR_NO_SCENE: as rtu_render_sensor, and the rules above. */
int  rtu_render_sensor_adaptive(RtuContext* ctx, const RtuSensorDesc* sensor, const RtuAdaptiveDesc* adaptive, float* h_rgbz, uint8_t* h_counts);
int  rtu_render_sensor_adaptive_device(RtuContext* ctx, const RtuSensorDesc* sensor, const RtuAdaptiveDesc* adaptive, void* d_rgbz, void* d_counts,
                                       void* hip_stream);
/* Diagnostic: the number of batches of the last adaptive sensor render of this context (0: none yet); for batch b < capacity
 * live_out[b] (may be NULL) gets the live pixels it traced and batch_out[b] (may be NULL) its samples: it traced live * samples rays.
 * RTU_ERR_ARG for a NULL context or a negative capacity. */
int  rtu_debug_sensor_adaptive_trace(RtuContext* ctx, uint32_t* live_out, uint32_t* batch_out, int capacity);

/* ---- First-hit features: the guides of a feature-guided filter (raytracer-utah_amd/csrc/rtu_features.hip) ---------------------------
 * Per ray one RtuRayHit — every byte as rtu_trace_rays_device writes it, the invalid-ray rule and RTU_QUERY_REFERENCE_WALK included —
 * and one float4 ALBEDO {r, g, b, 0}: what MtlBlinn::Shade returns for that hit under one AmbientLight of intensity (1, 1, 1) with
 * bounceCount 0 (mtlFunctions.cpp:125-133). On a front face that is diffuse.Sample(hInfo.uvw) — texture maps evaluated at the hit's
 * texture coordinates, the sub-material a MultiMtl node was given, white for a node without a material, as in a render; on a back
 * face {0, 0, 0}. A miss or an invalid ray: {0, 0, 0, 0}. These are the bits rtu_shade_rays gives with max_bounce 0 for the scene with
 * that one light.
 *   rtu_ray_features     n caller-supplied rays, as rtu_trace_rays takes them.
 *   rtu_frame_features   the pixel-centre ray of every pixel of `frame` (the rays of rtu_camera_rays, generated in the kernel: no ray
 *                        buffer, no upload), width * height answers in image order. frame.shard_count must be 1 (RTU_ERR_ARG);
 *                        samples, gather_bounces, dof and max_bounce are ignored: the guide of a depth-of-field or multi-sample frame
 *                        is its pixel-centre pinhole ray.
 * Errors as for rtu_trace_rays_device: RTU_ERR_ARG for an unknown flag bit, a NULL pointer with n > 0, a device pointer that is not
 * 16-byte aligned, a NULL frame or a resolution outside 1 .. 65536; RTU_ERR_NO_SCENE. n == 0 is RTU_OK and launches nothing.
 * The _device forms allocate nothing, read the scene's buffers only, touch no frame state and are asynchronous on hip_stream. The host
 * forms copy through grow-only buffers of the context (at most 2^20 rays / pixels at a time) on its stream and are synchronous. */
int  rtu_ray_features_device(RtuContext* ctx, const void* d_rays, size_t n, uint32_t flags, void* d_hits, void* d_albedo, void* hip_stream);
int  rtu_ray_features(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t flags, RtuRayHit* h_hits, float* h_albedo);
int  rtu_frame_features_device(RtuContext* ctx, const RtuFrameDesc* frame, void* d_hits, void* d_albedo, void* hip_stream);
int  rtu_frame_features(RtuContext* ctx, const RtuFrameDesc* frame, RtuRayHit* h_hits, float* h_albedo);

/* ---- Surface records: which triangle a ray hit, and where on it (k_features_surface, raytracer-utah_amd/csrc/rtu_features.hip) -----
 * The features above with one more output per ray: an RtuRaySurface, what the mesh walk interpolated hInfo.p, hInfo.N and hInfo.uvw
 * from. For baking, for picking a triangle, and for following a point of a deforming surface (the same weights over other vertices).
 *   triangle-mesh hit   mesh = the node's mesh_id; face = the index of the triangle in the mesh's f / fn / ft (cyTriMesh's face index,
 *                       never a slot of a tree); bc = the weights of the face's vertices 0, 1, 2 — {BC3, BC1, BC2} of
 *                       TriObj::IntersectTriangle (objFunctions.cpp:302-304), each in (0, 1) — so that in binary32, one rounding per
 *                       operation, (v[f[face][0]] bc[0] + v[f[face][1]] bc[1]) + v[f[face][2]] bc[2] is hInfo.p in the node's space
 *                       (cyTriMesh::Interpolate), and FromNodeCoords up the node's chain gives RtuRayHit.p bit for bit; likewise vn over
 *                       fn (normalised) for N and vt over ft for uvw. On an exact tie the triangle is the reference's winner.
 *   sphere, plane hit   mesh = face = -1, bc = 0; uvw = hInfo.uvw as a textured render carries it.
 *   miss, invalid ray   mesh = face = -1, bc = 0, uvw = 0.
 * uvw of a mesh hit is 0 where a render has none either: a mesh without texture coordinates, and every mesh of a scene without
 * textures (n_textures == 0: texture coordinates travel to the device with textured scenes only). hits and albedo are, byte for byte, what rtu_ray_features / rtu_frame_features write:
 * the walks are the same, one ray per lane, and hand the winner out at their end. RTU_QUERY_REFERENCE_WALK, the invalid-ray rule,
 * the errors and what the _device and host forms touch are those of the features; the surface pointer of a _device form must be
 * 16-byte aligned too (RTU_ERR_ARG). */
typedef struct RtuRaySurface { int32_t mesh; int32_t face; float bc[3]; float uvw[3]; } RtuRaySurface;   /* 32 B */
int  rtu_ray_surface_device(RtuContext* ctx, const void* d_rays, size_t n, uint32_t flags, void* d_hits, void* d_albedo, void* d_surface,
                            void* hip_stream);
int  rtu_ray_surface(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t flags, RtuRayHit* h_hits, float* h_albedo, RtuRaySurface* h_surface);
int  rtu_frame_surface_device(RtuContext* ctx, const RtuFrameDesc* frame, void* d_hits, void* d_albedo, void* d_surface, void* hip_stream);
int  rtu_frame_surface(RtuContext* ctx, const RtuFrameDesc* frame, RtuRayHit* h_hits, float* h_albedo, RtuRaySurface* h_surface);

/* ---- Denoising: an edge-avoiding filter for sampled previews (raytracer-utah_amd/csrc/rtu_denoise.h, rtu_denoise.hip) ---------------
 * A five-pass (n_passes) 5 x 5 a-trous wavelet filter on albedo-demodulated colour, guided by the features above. It has no
 * transcendental function; all arithmetic is binary32, one rounding per operation, no contraction, in this order — the host form and
 * the device form give the same bits:
 *   per pixel p   c = rgb of the float4 {r, g, b, z} image, H = its RtuRayHit, a = its albedo; p is VALID iff H.flags & RTU_RAY_HIT.
 *   demodulate    per channel d = a > 0.01f ? a : 1.0f, e = c / d.
 *   pass i        (i = 0 .. n_passes - 1) step s = 1 << i, sc = sigma_color * 2^-i (exact), sc2 = sc * sc. For a valid p, the taps
 *                 q = p + s * (dx, dy), dy outer, dx inner, both -2 .. 2, skipping q outside the image and q not valid:
 *                   h = k[dy + 2] * k[dx + 2], k = {1/16, 1/4, 3/8, 1/4, 1/16} (exact products)
 *                   dot = (Np.x Nq.x + Np.y Nq.y) + Np.z Nq.z;  t = dot > 0 ? dot : 0 (a NaN gives 0), then t = t * t repeated
 *                   normal_log2_power times
 *                   D = Pq - Pp;  dd = (Np.x D.x + Np.y D.y) + Np.z D.z;  x = dd / (sigma_plane * Hp.t);  wp = 1 / (1 + x * x)
 *                   delta = e_q - e_p;  dc = (dr dr + dg dg) + db db;  wc = 1 / (1 + dc / sc2)
 *                   w = ((h * t) * wp) * wc;  per channel acc = acc + e_q * w;  wsum = wsum + w
 *                 then e_p = wsum > 0 ? acc / wsum : e_p. Every tap reads the PREVIOUS pass's e.
 *   output        rgb = e * d for a valid pixel, the input rgb bit for bit for any other; z is always the input z bit for bit.
 * RTU_ERR_ARG: a NULL pointer, width or height outside 1 .. 65536, n_passes outside 1 .. 8, normal_log2_power outside 0 .. 7, a sigma
 * that is not > 0, a non-zero reserved word, a device pointer that is not 16-byte aligned.
 *   rtu_denoise          pure host code, no GPU and no context: the executable statement of the rules above. h_rgbz_out may be h_rgbz_in.
 *   rtu_denoise_device   the same bits from device memory, asynchronous on hip_stream. d_out == d_in is allowed. Its four planes
 *                        (64 B per pixel) are grow-only buffers of the context: one stream per context at a time, and no allocation
 *                        once a frame of that size has been filtered. Needs no scene.
 * The filter is for previews of recipes S and P at low sample counts; measured error ratios are in DESIGN.md section 22. */
typedef struct RtuDenoiseDesc {    /* 32 B */
    int32_t  width, height;
    int32_t  n_passes;             /* 1 .. 8 */
    float    sigma_color;          /* > 0 */
    float    sigma_plane;          /* > 0 */
    int32_t  normal_log2_power;    /* 0 .. 7: the cosine of the normals is raised to 2^this */
    uint32_t reserved[2];          /* must be 0 */
} RtuDenoiseDesc;
int  rtu_denoise_defaults(RtuDenoiseDesc* out);   /* width, height 0; n_passes 5, sigma_color 1, sigma_plane 0.05, normal_log2_power 5 */
int  rtu_denoise(const RtuDenoiseDesc* desc, const float* h_rgbz_in, const RtuRayHit* h_hits, const float* h_albedo, float* h_rgbz_out);
int  rtu_denoise_device(RtuContext* ctx, const RtuDenoiseDesc* desc, const void* d_in, const void* d_hits, const void* d_albedo, void* d_out,
                        void* hip_stream);
/* The snapshot of rtu_progressive_snapshot, filtered: rtu_denoise of it with rtu_frame_features of the session's frame. desc_or_NULL:
 * NULL selects rtu_denoise_defaults; width and height are the session's frame's, those of desc are ignored. The session computes its
 * frame's features once, at the first such call, and keeps them (its camera and scene are fixed): from the second call on nothing is
 * allocated. The session's sums are not touched. RTU_ERR_ARG: a sharded session (shard_count != 1), done == 0, a desc outside its
 * rules. After RTU_ERR_STALE it still answers from the features it holds, as rtu_progressive_snapshot does; a session that holds none
 * returns RTU_ERR_STALE. The _device form writes width * height float4 asynchronously on hip_stream; the host form is synchronous. */
int  rtu_progressive_snapshot_denoised_device(RtuProgressive* p, const RtuDenoiseDesc* desc_or_NULL, void* d_rgbz, void* hip_stream);
int  rtu_progressive_snapshot_denoised(RtuProgressive* p, const RtuDenoiseDesc* desc_or_NULL, float* h_rgbz);

/* ---- Temporal accumulation: sampled previews that follow a moving camera (raytracer-utah_amd/csrc/rtu_temporal.h, rtu_temporal.hip) ----
 * One new sample per pixel is blended into what earlier frames accumulated for the same surface point, found by projecting the
 * pixel's first-hit point into the PREVIOUS camera. The guides are the features above (pinhole pixel-centre rays). A HISTORY is three
 * planes of width * height float4 each, E then P then N, 48 B per pixel, owned by the caller:
 *   E = {e.r, e.g, e.b, n}   accumulated albedo-demodulated colour and the history length n
 *   P = {p.x, p.y, p.z, t}   first-hit point and its distance
 *   N = {N.x, N.y, N.z, node as bits}
 * It has no transcendental function; all arithmetic is binary32, one rounding per operation, no contraction, IEEE divisions, in this
 * order — the host form and the device form give the same bits. dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;
 * a x b = {a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x}; vector operations are per component.
 *   per pixel     c = rgb of the float4 {r, g, b, z} image, H = its RtuRayHit, a = its albedo; the pixel is VALID iff
 *                 H.flags & RTU_RAY_HIT. d = a > 0.01f ? a : 1.0f per channel and e_cur = c / d, as in "Denoising".
 *   not valid     rgbz_out is the input bit for bit; history out E = 0, P = 0, N = {0, 0, 0, node -1}.
 *   lookup        hist_prev == NULL: none. The fields cam_pos, origin, u, v, width, height of prev_cam and cur_cam equal bit for bit
 *                 (the STATIC path): the one tap is the pixel itself with weight 1. Otherwise, with prev = prev_cam:
 *                   D = H.p - prev.cam_pos;  nrm = prev.u x prev.v;  s = dot(prev.origin - prev.cam_pos, nrm) / dot(D, nrm)
 *                   none unless s is finite and s > 0
 *                   Q = (prev.cam_pos + D * s) - prev.origin
 *                   fx = dot(Q, prev.u) / dot(prev.u, prev.u) - 0.5f;  fy = dot(Q, prev.v) / dot(prev.v, prev.v) - 0.5f
 *                   none unless -1 <= fx < width and -1 <= fy < height (a NaN fails; tested before any conversion to an integer)
 *                   x0 = floor(fx), wx = fx - x0, ux = 1 - wx; y0, wy, uy likewise
 *                   four taps in the order (x0, y0) weight ux * uy, (x0 + 1, y0) wx * uy, (x0, y0 + 1) ux * wy, (x0 + 1, y0 + 1) wx * wy
 *   a tap q       is ACCEPTED iff it lies inside the image, E_q.n > 0, the bits of its node equal those of H.node,
 *                 dot(H.N, N_q) >= normal_min and |dot(H.N, P_q.xyz - H.p)| <= sigma_plane * H.t (a NaN fails either).
 *                 For the accepted taps in their order: acc = acc + E_q.rgb * w;  nacc = nacc + E_q.n * w;  wsum = wsum + w.
 *                 wsum > 0.01f: e_prev = acc / wsum, n_prev = nacc / wsum; otherwise n_prev = 0.
 *   blend         c has a channel that is not finite (the sample is not accumulated): with n_prev == 0 rgbz_out is the input bit for
 *                 bit and E = 0; otherwise e = e_prev, n = n_prev.
 *                 else n_prev == 0: e = e_cur, n = 1.
 *                 else n = min(n_prev + 1, max_history), A = 1 / n, e = e_prev + (e_cur - e_prev) * A.
 *   output        rgb = e * d; z is the input z bit for bit. History out E = {e, n}, P = {H.p, H.t}, N = {H.N, H.node}.
 * Only cam_pos, origin, u, v, width and height of the two cameras are read; both sizes must be the desc's. With hist_prev == NULL
 * prev_cam may be NULL. hist_out must not overlap hist_prev (taps read anywhere in it); rgbz_out may be rgbz.
 * RTU_ERR_ARG: a NULL pointer, width or height outside 1 .. 65536 or more than 2^26 pixels, max_history outside 1 .. 65535, sigma_plane
 * not > 0, normal_min outside -1 .. 1, an unknown flag bit, a non-zero reserved word, a camera of another size, overlapping histories,
 * a device pointer that is not 16-byte aligned. flags are read by sessions only.
 *   rtu_temporal_accumulate          pure host code, no GPU and no context: the executable statement of the rules above.
 *   rtu_temporal_accumulate_device   the same bits from device memory (k_temporal, one lane per pixel), asynchronous on hip_stream.
 *                                    Allocates nothing, needs no scene, touches no state of the context. */
#define RTU_TEMPORAL_DENOISE 1u     /* a session filters the accumulated image with rtu_denoise_device and its defaults */
typedef struct RtuTemporalDesc {   /* 32 B */
    int32_t  width, height;
    int32_t  max_history;          /* 1 .. 65535: the blend weight never falls below 1 / max_history */
    float    sigma_plane;          /* > 0: a tap further than sigma_plane * t from the pixel's tangent plane is another surface */
    float    normal_min;           /* -1 .. 1: smallest Ncur . Ntap of an accepted tap */
    uint32_t flags;                /* session only: RTU_TEMPORAL_DENOISE */
    uint32_t reserved[2];          /* must be 0 */
} RtuTemporalDesc;
int  rtu_temporal_defaults(RtuTemporalDesc* out);   /* width, height 0; max_history 32, sigma_plane 0.05, normal_min 0.9, flags 0 */
int  rtu_temporal_accumulate(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                             const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out);
int  rtu_temporal_accumulate_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                    const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                    void* d_rgbz_out, void* hip_stream);
/* A session that drives it. Frame k of the session, counted from 0 since rtu_temporal_begin or the last rtu_temporal_reset, of the
 * recipe S / P frame `frame` (samples = S >= 1, gather_bounces 0 or 4, shard_count 1, collect_stats 0, the desc's size; its camera may
 * differ from call to call):
 *   1. the rays and keys of sample k mod S (rtu_camera_sample_rays_device),
 *   2. shaded by rtu_shade_rays_sampled_device (gather_bounces 0) or rtu_shade_rays_paths_device (4) with eye = cam_pos and the frame's
 *      max_bounce; the capacity of the frame records is checked and the batch shaded again until it is complete, as
 *      rtu_progressive_advance does — THIS PART IS SYNCHRONOUS on hip_stream,
 *   3. rtu_frame_features_device of the frame, and rtu_temporal_accumulate_device against the previous frame's camera and history
 *      (frame 0: none) into d_rgbz,
 *   4. with RTU_TEMPORAL_DENOISE: rtu_denoise_device with rtu_denoise_defaults on d_rgbz, in place. The history stays unfiltered.
 * Steps 3 and 4 are asynchronous on hip_stream. The image is that of a ray batch: a pixel whose ray misses shows the environment, not
 * the background image, and z = RTU_BIGFLOAT. All buffers — rays, keys, the current sample, guides, two histories (212 B per pixel) —
 * belong to the session and are allocated by rtu_temporal_begin (which needs no scene); a frame allocates nothing once the context's
 * frame records have grown to what the scene needs. ONE STREAM PER CONTEXT as for every launch. A session does not go stale: once the
 * context got a new scene (rtu_upload_scene, rtu_update_scene, rtu_update_meshes) the next frame starts over with no history and k = 0.
 * WHAT MAY DIFFER FROM CALL TO CALL, in every kind of session below as well: the camera, and samples, gather_bounces and max_bounce.
 * Every rule that names S takes the S of the frame given in THAT call — sample k mod S here, a steered session's extra samples
 * S + (k mod S) * E + j, a gradient session's (k - 1) mod S, a sparse session's (k div m) mod S — and k goes on counting; the history
 * is kept, it does not know what recipe filled it. After such a change a gradient session's re-shaded sample is no longer the previous
 * frame's sample (another S: another ray; another gather_bounces or max_bounce: another estimate along the same ray), so the frame
 * that follows the change may show lambda > 0 with the camera and the scene at rest; the frame after it is exact again.
 * A REFUSED CALL LEAVES THE SESSION AS IT WAS: the frame counter, the history, the scene generation the session has seen and everything
 * a session shows of itself are those of the last frame that returned RTU_OK, also when a scene update is pending.
 * RTU_ERR_ARG: a desc outside its rules, a frame of another size, sharded, with counters or of recipe W, with max_bounce or samples
 * outside what rtu_render_frame takes, with a cam_pos that is not finite, of recipe P with more than 2^25 pixels, a NULL or misaligned
 * d_rgbz; RTU_ERR_NO_SCENE before an upload. rtu_temporal_frame is the host
 * form, synchronous on the context's stream.
 * rtu_temporal_history_device writes width * height floats: the history length n of every pixel after the last frame (0 before the
 * first). Ownership as for progressive sessions: rtu_destroy_context releases the device memory of open sessions, the handle stays
 * valid for rtu_temporal_free alone. */
typedef struct RtuTemporal RtuTemporal;
RtuTemporal* rtu_temporal_begin(RtuContext* ctx, const RtuTemporalDesc* desc, int* err_out);
int  rtu_temporal_frame_device(RtuTemporal* t, const RtuFrameDesc* frame, void* d_rgbz, void* hip_stream);
int  rtu_temporal_frame(RtuTemporal* t, const RtuFrameDesc* frame, float* h_rgbz);
int  rtu_temporal_history_device(RtuTemporal* t, void* d_n, void* hip_stream);
int  rtu_temporal_reset(RtuTemporal* t);
void rtu_temporal_free(RtuTemporal* t);

/* ---- Temporal accumulation across scene updates: moving nodes (rtu_temporal.h tp_pixel with MOVING, rtu_temporal.hip k_temporal<true, false>) ----
 * rtu_temporal_frame starts over once the scene changed. The entries below keep the history instead: a pixel's hit point is first
 * carried to where that point of its NODE was in the previous frame's scene, by an affine map per node, and the lookup of "Temporal
 * accumulation" is made from there.
 *
 * THE TABLE  rtu_scene_motion (pure host code, no GPU and no context) makes one RtuNodeMotion per node of `cur` (the pre-order index
 *   of RtuSceneDesc.nodes, which is RtuRayHit.node). With W(x) = FromNodeCoords from the node up to the root (tm x + pos per level)
 *   and W^-1(p) = ToNodeCoords from the root down (itm (p - pos) per level, the scene's own itm):
 *     m = W_prev o W_cur^-1 as three rows {a, b, c, d}: p_prev.k = dot(row_k.abc, p) + row_k.d
 *     g = the transpose of the linear part of W_cur o W_prev^-1 (the inverse-transpose of m's linear part): N_prev = g N, normalised
 *   both composed in binary64 and rounded to binary32 once at the end. A node whose whole chain (tm and pos of itself and of every
 *   ancestor) is bit-identical in both scenes gets RTU_MOTION_STATIC and the identity in m and g; a node whose mesh_id is one of
 *   reset_mesh_ids — the list given to rtu_update_meshes: a deformed surface has no rigid map — gets RTU_MOTION_RESET (besides).
 *   RTU_ERR_SCENE_SHAPE: `cur` has not the shape of `prev` (rtu_scene_shape_diff; n_bvh_nodes of a mesh in reset_mesh_ids may
 *   differ, as rtu_update_meshes allows). RTU_ERR_ARG: a NULL pointer (reset_mesh_ids may be
 *   NULL with n_reset == 0), n_reset < 0, a mesh id >= n_meshes.
 *
 * THE RULE  rtu_temporal_accumulate_motion is rtu_temporal_accumulate with, for a VALID pixel, k = H.node and T = motion[k]:
 *   no lookup     k < 0, k >= n_nodes, or T.flags & RTU_MOTION_RESET.
 *   T is STATIC   Pm = H.p, Nm = H.N bit for bit. If hist_prev is given and the two cameras are equal bit for bit, the one tap is the
 *                 pixel itself with weight 1 (the STATIC path of "Temporal accumulation").
 *   otherwise     Pm.k = dot(row_k.abc, H.p) + row_k.d;  q = {dot(g_0, H.N), dot(g_1, H.N), dot(g_2, H.N)};  l = dot(q, q);
 *                 Nm = q / sqrtf(l) per component (correctly rounded); no lookup if a component of Pm or of Nm is not finite.
 *   Every pixel that does not take the one-tap path is reprojected into the previous camera by the expressions of "Temporal
 *   accumulation" with Pm in place of H.p — also when the cameras are equal. A tap is ACCEPTED iff it lies inside the image,
 *   E_q.n > 0, the bits of its node equal those of H.node, dot(Nm, N_q) >= normal_min and |dot(Nm, P_q.xyz - Pm)| <= sigma_plane * H.t.
 *   history_cap   0: none. 1 .. 65535: where n_prev > 0, n_prev = min(n_prev, (float)history_cap) before the blend, for EVERY pixel —
 *                 a moving object changes shadows and bounce light on surfaces that did not move; the caller's control over lag.
 *   The history written is that of "Temporal accumulation": the current H.p, H.t, H.N, H.node.
 * So an all-STATIC table with history_cap 0 gives the bits of rtu_temporal_accumulate. RTU_ERR_ARG: what rtu_temporal_accumulate
 * refuses; a NULL table; history_cap outside 0 .. 65535; in the host form a table entry with a non-zero reserved word or an unknown
 * flag bit. THE DEVICE FORM TRUSTS THE TABLE (it is device memory, 16-byte aligned, n_nodes entries, never written): it allocates
 * nothing, needs no scene and is asynchronous on hip_stream.
 *
 * MOTION VECTORS  rtu_motion_vectors / _device write one float4 {fx, fy, 1, 0} per pixel: the continuous coordinates in the previous
 *   image the four taps are taken around (an integer is a pixel centre), for a VALID pixel whose node is inside the table and not
 *   RESET, with Pm and s finite and s > 0; {0, 0, 0, 0} otherwise. It always projects: no one-tap path, no bounds test. Only
 *   width and height of `desc` are read (the other fields must still be valid). Host and device form give the same bits.
 *
 * THE SESSION  rtu_temporal_frame_moved[_device] is rtu_temporal_frame[_device] except that (a) another scene generation does not
 *   clear the history nor the sample counter — the session adopts it — and (b) step 3 uses the motion form with h_motion, a HOST
 *   table of n_nodes entries (== the uploaded scene's node count, else RTU_ERR_ARG; checked as the host form checks it) that
 *   describes the scene of the PREVIOUS FRAME of this session against the scene now: after two updates between frames, call
 *   rtu_scene_motion on the two scenes that were rendered. The table is copied through staging memory of the session into a grow-only
 *   device buffer of the session before the call returns; after the first frame that needs them a frame allocates nothing. On frame 0
 *   the table is not used. Plain and moved frames may be mixed; a plain frame after an update starts over as before. */
#define RTU_MOTION_STATIC 1u   /* the node's whole chain (tm, pos of itself and every ancestor) is bit-identical in both scenes */
#define RTU_MOTION_RESET  2u   /* no lookup for pixels that show this node */
typedef struct RtuNodeMotion {   /* 96 B */
    float    m[12];      /* prev_from_cur, three rows {a, b, c, d}: p_prev.k = dot(row_k.abc, p) + row_k.d */
    float    g[9];       /* three rows: N_prev is g N, normalised */
    uint32_t flags;
    uint32_t reserved[2];  /* 0 */
} RtuNodeMotion;
int  rtu_scene_motion(const RtuSceneDesc* prev, const RtuSceneDesc* cur, const uint32_t* reset_mesh_ids, int n_reset,
                      RtuNodeMotion* out /* cur->n_nodes */);
int  rtu_temporal_accumulate_motion(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                    const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out,
                                    const RtuNodeMotion* motion, uint32_t n_nodes, int32_t history_cap);
int  rtu_temporal_accumulate_motion_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                           const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                           void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap, void* hip_stream);
int  rtu_motion_vectors(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuRayHit* h_hits, const RtuNodeMotion* motion,
                        uint32_t n_nodes, float* h_mv);
int  rtu_motion_vectors_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const void* d_hits,
                               const RtuNodeMotion* d_motion, uint32_t n_nodes, void* d_mv, void* hip_stream);
int  rtu_temporal_frame_moved_device(RtuTemporal* t, const RtuFrameDesc* frame, const RtuNodeMotion* h_motion, uint32_t n_nodes, int32_t history_cap,
                                     void* d_rgbz, void* hip_stream);
int  rtu_temporal_frame_moved(RtuTemporal* t, const RtuFrameDesc* frame, const RtuNodeMotion* h_motion, uint32_t n_nodes, int32_t history_cap,
                              float* h_rgbz);

/* ---- Temporal accumulation on deforming meshes (rtu_temporal.h tp_deform_source, rtu_temporal.hip k_temporal_deform<MOMENTS>) ----
 * rtu_scene_motion marks a deformed mesh RTU_MOTION_RESET: its pixels start over. But a point given as (face, barycentrics) — an
 * RtuRaySurface of "Surface records" — has an exact previous position: the same weights over the PREVIOUS vertices, through the node's
 * previous transformation. The entries below look the history up from there.
 *
 * PREVIOUS VERTICES  rtu_keep_previous_vertices(ctx, on), default off: nothing changes. With it on, rtu_update_meshes keeps the v and vn
 *   it replaces as the previous generation of every LISTED mesh (the two grow-only buffers change places: the first such update of a
 *   mesh allocates the second pair, later ones nothing). "Previous" means before the LAST rtu_update_meshes only: for a mesh that
 *   update did not list, before any update, after rtu_upload_scene and after the switch changed, previous is current. A caller who
 *   updates a mesh twice between two frames marks it RESET.
 *
 * THE TABLE  rtu_scene_motion_deform is rtu_scene_motion with a second list: a node whose mesh_id is in deform_mesh_ids and not in
 *   reset_mesh_ids gets flags = RTU_MOTION_DEFORM and
 *     m = W_prev, node coordinates to world of the PREVIOUS scene over the whole ancestor chain, as three rows {a, b, c, d}
 *     g = the transpose of the linear part of W_prev^-1
 *   composed in binary64 and rounded once; reserved stays 0. A mesh in both lists is RESET. n_bvh_nodes of a listed mesh may differ.
 *   With n_deform == 0 the table is rtu_scene_motion's, byte for byte. RTU_ERR_ARG besides rtu_scene_motion's: n_deform < 0, a NULL
 *   list with n_deform > 0, a mesh id >= n_meshes.
 *
 * THE RULE  rtu_temporal_accumulate_deform (three planes) and _deform_moments (four) are rtu_temporal_accumulate_motion and
 *   rtu_temporal_accumulate_moments with one more input, the frame's surface records. For a VALID pixel with k = H.node inside the
 *   table, T = motion[k] with RTU_MOTION_DEFORM (and not RESET), S its record, f / fn the faces and v_prev / vn_prev the previous
 *   positions / normals of mesh nodes[k].mesh_id:
 *     x = (v_prev[f[S.face][0]] S.bc[0] + v_prev[f[S.face][1]] S.bc[1]) + v_prev[f[S.face][2]] S.bc[2]     (binary32, no contraction)
 *     n likewise of vn_prev over fn;  Pm.k = dot(row_k.abc, x) + row_k.d;  q = g n;  Nm = q / sqrtf(dot(q, q))
 *     no lookup if S.mesh is not nodes[k].mesh_id, S.face is outside 0 .. nf - 1, or a component of Pm or Nm is not finite.
 *   A DEFORM pixel always reprojects (no one-tap path; RTU_MOTION_STATIC beside DEFORM is ignored); the tap test and the history written
 *   are the motion form's. Every other pixel follows the motion form bit for bit: a table without DEFORM entries gives its bytes.
 *   The host forms read v_prev, vn_prev, f, fn and mesh_id from prev_scene (n_nodes must be its node count), which must be a scene
 *   rtu_validate_scene accepts: the indices in f / fn are used as they are. A mesh of prev_scene without one of the four arrays has
 *   no face: records on it give no lookup. The _device forms read
 *   the context's own f, fn and the previous v, vn it kept: they need the switch above (else RTU_ERR_ARG), a scene (RTU_ERR_NO_SCENE),
 *   n_nodes == the uploaded scene's node count and 16-byte aligned surface records; the first call after an upload, an update or a
 *   change of the switch rewrites a small table of the context (grow-only; it waits for the context's own stream and copies
 *   synchronously), other calls allocate nothing. As for rtu_update_meshes itself, the caller synchronises any OTHER stream it gave a
 *   deform entry before the call that rewrites the table: the rewrite is not ordered against kernels in flight there.
 *   rtu_motion_vectors_deform[_device] is rtu_motion_vectors with Pm as above for DEFORM pixels ({0, 0, 0, 0} where there is no lookup).
 *
 * THE SESSION  rtu_temporal_frame_deformed[_device] is rtu_temporal_frame_moved[_device] except that step 3 takes the guides from
 *   rtu_frame_surface_device and uses the deform accumulator (the table may carry RTU_MOTION_DEFORM). The session grows a buffer of
 *   32 B per pixel for the records on the first such frame and allocates nothing afterwards. It needs the context's
 *   rtu_keep_previous_vertices (else RTU_ERR_ARG) and a plain, RTU_TEMPORAL_DENOISE or variance session: a steered, gradient or sparse
 *   session (hole rays included) is refused with RTU_ERR_UNSUPPORTED. A refused call leaves the session as it was. Plain, moved and
 *   deformed frames may be mixed in one session. The table describes the scene of the previous frame of the session against the scene
 *   now, and "previous vertices" are those before the last rtu_update_meshes: ONE rtu_update_meshes per deformed frame, or RESET. */
#define RTU_MOTION_DEFORM 4u   /* m = W_prev, g from W_prev^-1: the deform forms carry (face, barycentrics) over the previous vertices */
int  rtu_keep_previous_vertices(RtuContext* ctx, int on);
int  rtu_scene_motion_deform(const RtuSceneDesc* prev, const RtuSceneDesc* cur, const uint32_t* deform_mesh_ids, int n_deform,
                             const uint32_t* reset_mesh_ids, int n_reset, RtuNodeMotion* out /* cur->n_nodes */);
int  rtu_temporal_accumulate_deform(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                    const RtuRayHit* h_hits, const float* h_albedo, const RtuRaySurface* h_surface, const RtuSceneDesc* prev_scene,
                                    const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out, const RtuNodeMotion* motion, uint32_t n_nodes,
                                    int32_t history_cap);
int  rtu_temporal_accumulate_deform_moments(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                            const RtuRayHit* h_hits, const float* h_albedo, const RtuRaySurface* h_surface, const RtuSceneDesc* prev_scene,
                                            const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out, const RtuNodeMotion* motion, uint32_t n_nodes,
                                            int32_t history_cap);
int  rtu_temporal_accumulate_deform_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                           const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_surface, const void* d_hist_prev,
                                           void* d_hist_out, void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap,
                                           void* hip_stream);
int  rtu_temporal_accumulate_deform_moments_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                                   const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_surface,
                                                   const void* d_hist_prev, void* d_hist_out, void* d_rgbz_out, const RtuNodeMotion* d_motion,
                                                   uint32_t n_nodes, int32_t history_cap, void* hip_stream);
int  rtu_motion_vectors_deform(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuRayHit* h_hits, const RtuRaySurface* h_surface,
                               const RtuSceneDesc* prev_scene, const RtuNodeMotion* motion, uint32_t n_nodes, float* h_mv);
int  rtu_motion_vectors_deform_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const void* d_hits, const void* d_surface,
                                      const RtuNodeMotion* d_motion, uint32_t n_nodes, void* d_mv, void* hip_stream);

int  rtu_temporal_frame_deformed_device(RtuTemporal* t, const RtuFrameDesc* frame, const RtuNodeMotion* h_motion, uint32_t n_nodes, int32_t history_cap,
                                        void* d_rgbz, void* hip_stream);
int  rtu_temporal_frame_deformed(RtuTemporal* t, const RtuFrameDesc* frame, const RtuNodeMotion* h_motion, uint32_t n_nodes, int32_t history_cap,
                                 float* h_rgbz);

/* ---- Variance-guided filtering: the filter steered by per-pixel variance from temporal moments (rtu_variance.h, rtu_variance.hip) ----
 * The history gets a fourth plane with the first and second moment of the sample's luminance; out of it comes the variance of the
 * accumulated mean per pixel, and that variance sets the colour edge-stop of every a-trous pass: a pixel with a long history is left
 * nearly alone, a disoccluded one is filtered hard. Binary32, one rounding per operation, no contraction, IEEE divisions, in this
 * order — host and device forms give the same bits. dot, d, e, VALID, k as in "Denoising" and "Temporal accumulation";
 * l(e) = (0.2126f e.r + 0.7152f e.g) + 0.0722f e.b.
 *
 * 1. MOMENTS  rtu_temporal_accumulate_moments is rtu_temporal_accumulate_motion on a MOMENTS HISTORY: four planes E, P, N, M of
 *   width * height float4 each, 64 B per pixel, M = {m1, m2, 0, 0}. rgbz_out and the planes E, P, N are the motion form's bit for
 *   bit. With l = l(e_cur) and l2 = l * l:
 *     an ACCEPTED tap adds M_q.x * w to m1acc and M_q.y * w to m2acc, in the taps' order; wsum > 0.01f: m1_prev = m1acc / wsum,
 *     m2_prev = m2acc / wsum; otherwise both 0.
 *     the sample is not accumulated (c not finite), or l2 is not finite (l or l * l overflowed: THE MOMENTS SKIP THIS SAMPLE, while E
 *     and n take it): m = m_prev — zeros for a fresh pixel.
 *     else n_prev == 0: m1 = l, m2 = l2.
 *     else m1 = m1_prev + (l - m1_prev) * A, m2 = m2_prev + (l2 - m2_prev) * A with the A of the blend.
 *     M = {m1, m2, 0, 0} where E is written (the pixel is valid and has an accumulated colour), zeros elsewhere.
 *   So M.xy are the bits that E.xy of rtu_temporal_accumulate_motion has when it is fed the image {l, l2, 0, z} with albedo {1, 1, 1, 0},
 *   wherever both images are finite in the same pixels. hist_out (64 B per pixel) must not overlap hist_prev. Errors as for the
 *   motion form.
 *
 * 2. VARIANCE  rtu_variance: one float per pixel out of a moments history and the RtuRayHit of its frame. With n = E_p.n:
 *     v = 0 unless p is valid and n > 0.
 *     x = m2 - m1 * m1;  vt = x > 0 ? x : 0 (a NaN gives 0).
 *     n >= min_history: var = vt.
 *     n <  min_history: rp = 1 / (sigma_plane * H_p.t). Over the taps q = p + (dx, dy), dy outer, dx inner, both -3 .. 3, that lie in
 *       the image, are valid and have E_q.n > 0 (p is one of them):
 *         dot = dot(Np, Nq);  t = dot > 0 ? dot : 0, then t = t * t repeated normal_log2_power times
 *         x = dot(Np, Pq - Pp) * rp;  wp = 1 / (1 + x * x);  w = t * wp
 *         s1 = s1 + M_q.x * w;  s2 = s2 + M_q.y * w;  ws = ws + w
 *       ws > 0: a1 = s1 / ws, a2 = s2 / ws, x = a2 - a1 * a1, vs = x > 0 ? x : 0; otherwise vs = 0 (no usable tap: a zero or NaN
 *       normal). var = (vs > vt ? vs : vt) * ((float)min_history / n).
 *     v = var / n.
 *
 * 3. THE FILTER  rtu_denoise_variance: n_passes passes at steps 1, 2, 4, ... on e = c / d as in "Denoising", each pixel carrying its
 *   variance v (the caller's, for every pixel) with it. Per valid pixel p and pass, sl2 = sigma_lum * sigma_lum:
 *     g = sum of v_q * k3 / sum of k3 over q = p + (dx, dy), dy outer, dx inner, both -1 .. 1 (distance 1 whatever the step), q in
 *       the image and valid; k3 = {1/4, 1/2, 1/4}[dy + 1] * {1/4, 1/2, 1/4}[dx + 1]; both sums in that order, then one division.
 *     r = 1 / (sl2 * g + 1e-8f);  lp = l(e_p);  rp = 1 / (sigma_plane * H_p.t) (made once, before the first pass)
 *     the 25 taps of "Denoising", in its order and with its skips:
 *       t as above;  x = dot(Np, Pq - Pp) * rp;  wp = 1 / (1 + x * x);  dl = l(e_q) - lp;  wc = 1 / (1 + (dl * dl) * r)
 *       w = (h * (t * wp)) * wc;  per channel acc = acc + e_q * w;  vacc = vacc + v_q * (w * w);  wsum = wsum + w
 *     wsum > 0: e_p = acc / wsum and, with ws2 = wsum * wsum, v_p = ws2 > 0 ? vacc / ws2 : v_p; otherwise both stay.
 *   Every tap reads the PREVIOUS pass's e and v. There is no halving of a sigma: the variance that shrinks from pass to pass tightens
 *   the later passes. Two divisions per tap. Output as in "Denoising": rgb = e * d for a valid pixel, the input rgb bit for bit for
 *   any other, z always the input z bit for bit.
 *
 * RTU_ERR_ARG: a NULL pointer, width or height outside 1 .. 65536 or more than 2^26 pixels, n_passes outside 1 .. 8, normal_log2_power
 * outside 0 .. 7, a sigma that is not > 0, min_history outside 1 .. 65535, a non-zero reserved word, a device pointer that is not
 * 16-byte aligned (d_v: 4-byte). The host forms are pure host code, no GPU and no context: the executable statement of the rules. The
 * _device forms give the same bits from device memory, asynchronous on hip_stream: rtu_temporal_accumulate_moments_device
 * (k_temporal<true, true>) and rtu_variance_device (k_variance) allocate nothing, need no scene and touch no state of the context;
 * rtu_denoise_variance_device uses the four grow-only planes of rtu_denoise_device (64 B per pixel, one stream per context, no
 * allocation once a frame of that size has been filtered by either), d_out == d_in is allowed.
 *
 * THE SESSION  rtu_temporal_begin_variance opens an RtuTemporal whose frames, plain and moved, are those of "Temporal accumulation"
 * except that step 3 uses the moments form — a plain frame with an all-STATIC table of the uploaded scene's nodes and history_cap 0,
 * which gives the plain form's E, P, N — and step 4 is rtu_variance_device of the new history, then rtu_denoise_variance_device on
 * d_rgbz, in place. The history stays unfiltered. variance_desc: its width and height are ignored, the session's are used.
 * RTU_TEMPORAL_DENOISE in temporal_desc is RTU_ERR_ARG here. Two moments histories, the variance and the table belong to the session
 * (248 B per pixel in all); everything else — rtu_temporal_history_device, rtu_temporal_reset, rtu_temporal_free, ownership, one
 * stream per context, no allocation after the first frame (the first moved frame, for the staging memory) — as for any session.
 * Not done here: filtered colour is not fed back into the history, fireflies are not clamped, progressive sessions hold no second
 * moment, sharded frames are refused. Measured error ratios are in DESIGN.md section 25. */
typedef struct RtuVarianceDesc {   /* 40 B */
    int32_t  width, height;
    int32_t  n_passes;             /* 1 .. 8 */
    float    sigma_lum;            /* > 0: the colour edge-stop in standard deviations of the pixel's luminance */
    float    sigma_plane;          /* > 0 */
    int32_t  normal_log2_power;    /* 0 .. 7 */
    int32_t  min_history;          /* 1 .. 65535: below it the variance is estimated over the 7 x 7 neighbourhood */
    uint32_t reserved[3];          /* must be 0 */
} RtuVarianceDesc;
int  rtu_variance_defaults(RtuVarianceDesc* out);   /* width, height 0; n_passes 3, sigma_lum 2, sigma_plane 0.05, normal_log2_power 5, min_history 4 */
int  rtu_temporal_accumulate_moments(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                     const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out,
                                     const RtuNodeMotion* motion, uint32_t n_nodes, int32_t history_cap);
int  rtu_temporal_accumulate_moments_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                            const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                            void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap, void* hip_stream);
int  rtu_variance(const RtuVarianceDesc* desc, const float* h_hist, const RtuRayHit* h_hits, float* h_v);
int  rtu_variance_device(RtuContext* ctx, const RtuVarianceDesc* desc, const void* d_hist, const void* d_hits, void* d_v, void* hip_stream);
int  rtu_denoise_variance(const RtuVarianceDesc* desc, const float* h_rgbz_in, const RtuRayHit* h_hits, const float* h_albedo, const float* h_v,
                          float* h_rgbz_out);
int  rtu_denoise_variance_device(RtuContext* ctx, const RtuVarianceDesc* desc, const void* d_in, const void* d_hits, const void* d_albedo,
                                 const void* d_v, void* d_out, void* hip_stream);
RtuTemporal* rtu_temporal_begin_variance(RtuContext* ctx, const RtuTemporalDesc* temporal_desc, const RtuVarianceDesc* variance_desc, int* err_out);

/* ---- Steered sampling: a budget of extra rays per frame, spent where the variance is highest (rtu_steer.h, rtu_steer.hip) ----
 * A variance session fires one new sample per pixel whatever the pixel's history. The entries below spend `budget` further rays of a
 * frame on the pixels whose accumulated mean is least certain, and fold what they bring into the history before it is filtered. All
 * weights are integers and their sum is exact: the allocation does not depend on the order in which anything is added, and host and
 * device forms give the same words. The floating-point expressions are binary32, one rounding per operation, no contraction, IEEE
 * divisions, in this order. VALID, d, e, l(e) as in "Temporal accumulation" and "Variance-guided filtering"; p is the pixel's index
 * x + width * y; mix32 is that of "Sample streams of recipe S".
 *
 * 1. ALLOCATION  rtu_sample_allocation: out of a moments history, the RtuRayHit of its frame and the variance v of rtu_variance,
 *   uint32 counts[pixels], uint32 offsets[pixels] and the total.
 *     w = 0 unless p is VALID and E_p.n > 0.
 *     x = (v_p / (M_p.x * M_p.x + 1.0f)) * 16777216.0f: the variance of the mean — absolute where the mean luminance is small
 *       against 1, relative to its square where it is large.
 *     w = 0 if x is a NaN or not > 0; otherwise w = x >= 1048576.0f ? 1048576 : (uint32_t)x.
 *     Wsum = the sum of w over all pixels, in 64 bits. Wsum == 0: every count is 0.
 *     h = mix32(p + 0x9e3779b9u * (frame_index + 1u)) >> 16                          (a dither of 16 bits per pixel and frame)
 *     c = (budget * w + ((h * Wsum) >> 16)) / Wsum in 64-bit unsigned arithmetic, then c = min(c, max_extra).
 *     o = the exclusive scan of c in pixel order; THE CUT: offsets_p = min(o_p, budget), counts_p = min(c_p, budget - offsets_p),
 *     total = min(sum of c, budget). So offsets is the exclusive scan of counts, and total <= budget.
 *   Without the dither a budget below one ray per pixel would floor to nothing; with it the expected count of a pixel is its share.
 *
 * 2. THE EXTRA RAYS  rtu_extra_sample_rays: with S = frame->samples >= 1, E = max_extra, k = frame_index and F = `frame` with
 *   samples = S * (1 + E): ray offsets_p + j (j < counts_p) and its key are those of pixel p in
 *   rtu_camera_sample_rays(F, S + (k mod S) * E + j), bit for bit, and owner[offsets_p + j] = p. The sample indices are disjoint
 *   from 0 .. S - 1 and distinct over (k mod S, j): every extra sample is a sample image of a recipe S / P frame of S * (1 + E)
 *   samples. `capacity` is the number of rays, keys and owners the output arrays hold.
 *
 * 3. THE FOLD  rtu_temporal_refine: the shaded {r, g, b, t} of the extra rays folded into the planes E and M of a moments history and
 *   into rgbz, all in place. For a VALID pixel with E.n > 0 and counts_p > 0, for j = 0 .. counts_p - 1 in order, with c the rgb of
 *   rgbt[offsets_p + j]:
 *     a channel of c is not finite: the sample is skipped.
 *     otherwise e_cur = c / d;  n = min(n + 1, max_history);  A = 1 / n;  e = e + (e_cur - e) * A;
 *     l = l(e_cur), l2 = l * l; if l2 is finite m1 = m1 + (l - m1) * A and m2 = m2 + (l2 - m2) * A (the skip rule of the moments).
 *   Then E = {e, n}, M.xy = {m1, m2}, rgb = e * d. The planes P and N, z and every other pixel pass bit for bit. So a pixel with one
 *   extra sample gets the bits a second rtu_temporal_accumulate_moments on the STATIC one-tap path would give it (where no component
 *   of E is a negative zero). Of desc only width, height and max_history are used (the others must still be valid).
 *
 * RTU_ERR_ARG: a NULL pointer; width or height outside 1 .. 65536 or more than 2^26 pixels; budget above 2^26; max_extra outside
 * 1 .. 15; a non-zero reserved word; a frame of another size than the desc, with samples < 1 or S * (1 + E) > 65536; capacity or
 * n_rays above 2^26; a device pointer that is not 16-byte aligned (counts, offsets, keys, owner, total: 4-byte). The host forms — pure
 * host code, no GPU and no context — also refuse a count above max_extra (rays) and a pixel whose offsets_p + counts_p exceeds
 * capacity / n_rays. THE DEVICE FORMS TRUST counts AND offsets but never leave the arrays: a count is taken as min(count, max_extra),
 * a ray or sample at or beyond capacity / n_rays is not written / not read. They are asynchronous on hip_stream and need no scene.
 * rtu_sample_allocation_device (k_steer_weight: a reduction per workgroup and one 64-bit atomic add each; k_steer_counts,
 * k_steer_sums, k_steer_finish: a three-step scan) keeps 4 B per pixel and per 1024 pixels in a grow-only buffer of the context: one
 * stream per context, nothing allocated from the second call at a size. rtu_extra_sample_rays_device (k_steer_rays) and
 * rtu_temporal_refine_device (k_refine), one lane per pixel, allocate nothing and touch no state of the context.
 *
 * THE SESSION  rtu_temporal_begin_steered opens a variance session whose frames, plain and moved, continue after step 3 and
 * rtu_variance_device with: the allocation, frame_index = the session's frame counter k of this frame; the extra rays; their shading
 * by the unchanged rtu_shade_rays_sampled_device / rtu_shade_rays_paths_device path of step 2 with n = the total, which is read back
 * (4 bytes; this part of a frame is synchronous already); the fold into the new history and d_rgbz; rtu_variance_device again on the
 * folded history; then the filter. steer_desc: width, height and frame_index are ignored. budget == 0 gives a variance session's
 * bits and launches nothing more. A frame needs S * (1 + max_extra) <= 65536 (with budget > 0; RTU_ERR_ARG otherwise, whatever the
 * allocation of that frame would have been). rtu_temporal_extra_counts_device writes width * height
 * uint32: the counts of the last frame (zeros before the first, after a reset and with budget 0); rtu_temporal_steer_total returns
 * their sum. Counts, offsets, and min(budget, pixels * max_extra) rays, keys, owners and results (68 B each) belong to the session; a
 * frame allocates nothing after the first. Everything else as for a variance session. Measured error ratios and times are in
 * DESIGN.md section 26. */
typedef struct RtuSteerDesc {      /* 32 B */
    int32_t  width, height;
    uint32_t budget;               /* 0 .. 2^26: extra rays per frame, at most */
    int32_t  max_extra;            /* 1 .. 15: extra rays per pixel, at most */
    uint32_t frame_index;          /* varies the dither from frame to frame, and selects the extra samples */
    uint32_t reserved[3];          /* must be 0 */
} RtuSteerDesc;
int  rtu_steer_defaults(RtuSteerDesc* out);   /* width, height 0; budget 0, max_extra 3, frame_index 0 */
int  rtu_sample_allocation(const RtuSteerDesc* desc, const float* h_hist, const RtuRayHit* h_hits, const float* h_v, uint32_t* counts,
                           uint32_t* offsets, uint32_t* total);
int  rtu_sample_allocation_device(RtuContext* ctx, const RtuSteerDesc* desc, const void* d_hist, const void* d_hits, const void* d_v,
                                  void* d_counts, void* d_offsets, void* d_total, void* hip_stream);
int  rtu_extra_sample_rays(const RtuSteerDesc* desc, const RtuFrameDesc* frame, const uint32_t* counts, const uint32_t* offsets, size_t capacity,
                           RtuRay* rays_out, uint32_t* keys_out, uint32_t* owner_out);
int  rtu_extra_sample_rays_device(RtuContext* ctx, const RtuSteerDesc* desc, const RtuFrameDesc* frame, const void* d_counts, const void* d_offsets,
                                  size_t capacity, void* d_rays, void* d_keys, void* d_owner, void* hip_stream);
int  rtu_temporal_refine(const RtuTemporalDesc* desc, float* h_hist, const RtuRayHit* h_hits, const float* h_albedo, const uint32_t* counts,
                         const uint32_t* offsets, const float* h_rgbt, size_t n_rays, float* h_rgbz);
int  rtu_temporal_refine_device(RtuContext* ctx, const RtuTemporalDesc* desc, void* d_hist, const void* d_hits, const void* d_albedo,
                                const void* d_counts, const void* d_offsets, const void* d_rgbt, size_t n_rays, void* d_rgbz, void* hip_stream);
RtuTemporal* rtu_temporal_begin_steered(RtuContext* ctx, const RtuTemporalDesc* temporal_desc, const RtuVarianceDesc* variance_desc,
                                        const RtuSteerDesc* steer_desc, int* err_out);
int  rtu_temporal_extra_counts_device(RtuTemporal* t, void* d_counts, void* hip_stream);
int  rtu_temporal_steer_total(RtuTemporal* t, uint32_t* total_out);

/* ---- Temporal gradients: a pixel's history is shortened where its shading changed (rtu_gradient.h, rtu_gradient.hip) ----
 * Neither a variance nor a steered session notices that the LIGHT arriving at a surface point changed: after rtu_update_scene moved or
 * dimmed a light every node is RTU_MOTION_STATIC, the whole history is kept and the old lighting fades over max_history frames. The
 * entries below re-shade one pixel of every 3 x 3 STRATUM with the random numbers of the previous frame, compare it with what the
 * previous frame saw there, and cap the history where the two differ. With the camera at rest and the node static the re-shaded
 * sample is the previous frame's ray with the previous frame's key: the difference is exactly zero unless the scene changed.
 * Binary32, one rounding per operation, no contraction, IEEE divisions and square roots, in this order; host and device forms give the
 * same bits. VALID, d, l(e), mix32, the table, Pm, Nm, the projection {s, fx, fy} and a tap's ACCEPTED are those of the sections above.
 *
 * 1. STRATA AND GRADIENT RAYS  SW = ceil(width / 3), SH = ceil(height / 3); stratum (sx, sy) has index s = sx + SW * sy and OWNS one
 *   pixel per frame: h = mix32(s + 0x9e3779b9u * (frame_index + 1u)), x = 3 sx + (h >> 16) % min(3, width - 3 sx),
 *   y = 3 sy + (h >> 24) % min(3, height - 3 sy), owner_s = x + width * y. rtu_gradient_rays writes, per stratum, owner_s and the ray
 *   and key of that pixel in rtu_camera_sample_rays(frame, sample), bit for bit: `sample` is the caller's — a session passes
 *   (k - 1) mod S, the sample the previous frame used. The frame must have the desc's size and samples > sample >= 0.
 *
 * 2. THE SAMPLE'S LUMINANCE  rtu_sample_luminance: one float per pixel of a frame's raw sample image, L_p = l(c / d); 0 for a pixel
 *   that is not VALID or whose c has a channel that is not finite.
 *
 * 3. GRADIENTS AND LAMBDA  rtu_temporal_gradient: out of the two cameras, the current frame's RtuRayHit and albedo, the table, the
 *   previous moments history and luminance plane, the owners and the shaded {r, g, b, t} of the gradient rays (one per stratum),
 *   one float4 diff_s and one float lambda_s per stratum. With p = owner_s and c the rgb of rgbt_s:
 *     no gradient, diff_s = {0, 0, 0, 0}: p is not VALID; a channel of c is not finite; rtu_temporal_accumulate_moments would make no
 *       lookup for p (hist_prev == NULL, node outside the table, RESET, a component of Pm or Nm of a node that is not STATIC not
 *       finite, s not finite or not > 0); q (below) outside the image; the tap q is not ACCEPTED for p.
 *     q = p on the one-tap path (the cameras equal bit for bit and p's node STATIC); otherwise q = (floor(fx + 0.5f), floor(fy + 0.5f))
 *       from the accumulator's fx, fy (compared with 0 and the size as floats: a NaN fails, before any conversion to an integer).
 *     lc = l(c / d_p);  lp = L_prev[q];  num = lc - lp;  den = lc > lp ? lc : lp
 *     noise = 0 on the one-tap path (the comparand is the same ray with the same key); otherwise x = M_q.y - M_q.x * M_q.x and
 *       noise = 2 * (x > 0 ? x : 0): the comparand is another ray, this is its per-sample variance, twice.
 *     diff_s = {num, den, noise, 0}
 *   Then per stratum, over the strata (sx + dx, sy + dy), dy outer, dx inner, both -radius .. radius, that lie in the strata grid:
 *     Nsum, Dsum, Zsum = the sums of diff.x, diff.y, diff.z in that order
 *     x = |Nsum| - kappa * sqrtf(Zsum);  a = x > 0 ? x : 0 (a NaN gives 0);  r = a / Dsum
 *     lambda_s = 0 unless Dsum > 0 and r is not a NaN; otherwise r < 1 ? r : 1.
 *
 * 4. THE CAPPED ACCUMULATOR  rtu_temporal_accumulate_gradient is rtu_temporal_accumulate_moments with one more input, `lambda`: one
 *   float per stratum (SW * SH floats), or NULL. For pixel (x, y), L = lambda[(x / 3) + SW * (y / 3)]. Where L > 0 and n_prev > 0 —
 *   after history_cap, which keeps its meaning, and before the blend —: n_prev = min(n_prev, L < 1 ? 1 / L - 1 : 0). So the weight of
 *   the new sample is not below L (roughly), and L >= 1 starts the pixel over: n_prev = 0, e_prev, m1_prev and m2_prev zeros, as for
 *   a pixel that found no history — so n = 1, e = e_cur and the moments are those of a fresh pixel.
 *   A NaN caps nothing. The moments are blended with the same A: where history was dropped the variance rises, the filter smooths
 *   harder and a steered session sends its extra rays there. With lambda NULL or all zero the output is the moments form's bit for bit.
 *
 * RTU_ERR_ARG: what the moments form refuses; a NULL pointer (hist_prev, and with it prev_cam and L_prev, may be NULL: no gradient
 * anywhere); a gradient desc of another size than the temporal desc or outside its rules: width, height 1 .. 65536 and 2^26 pixels,
 * radius 0 .. 3, kappa >= 0 and finite, enabled 0 or 1, reserved words 0; a device pointer that is not 16-byte aligned (keys, owners,
 * luminance planes, lambda: 4-byte). The host forms — pure host code, no GPU and no context — also refuse an owner outside the image.
 * THE DEVICE FORMS TRUST THE TABLE AND THE OWNERS but never leave the arrays: an owner outside the image gives no gradient. They
 * allocate nothing, need no scene, touch no state of the context and are asynchronous on hip_stream: rtu_gradient_rays_device
 * (k_gradient_rays, a lane per stratum), rtu_sample_luminance_device (k_sample_luminance), rtu_temporal_gradient_device
 * (k_gradient_diff, then k_gradient_lambda: one 16-byte load per tap) and rtu_temporal_accumulate_gradient_device
 * (k_temporal<true, true, true>). rgbz_out == rgbz is allowed as for every accumulator; no other output may overlap an input.
 *
 * THE SESSION  rtu_temporal_begin_gradient opens a variance session, or with steer_desc a steered session, whose frames, plain and
 * moved, change in four ways when the session has a previous frame (not frame 0, not the frame after rtu_temporal_reset, not a plain
 * frame after a scene change: those start over as before and take no gradient): (a) behind the rays and keys of sample k mod S the
 * gradient rays of sample (k - 1) mod S with frame_index = k are written into the same buffers; (b) the unchanged shading path of step
 * 2 shades width * height + SW * SH rays in its one launch sequence; (c) after the guides come rtu_temporal_gradient_device and
 * rtu_temporal_accumulate_gradient_device in place of the moments form; (d) rtu_sample_luminance_device of the new sample is kept for
 * the next frame (this on every frame). gradient_desc: width and height are ignored, the session's are used; enabled == 0 gives the
 * parent session's bits and launches nothing more. rtu_temporal_lambda_device writes width * height floats, the lambda of every
 * pixel's stratum in the last frame; zeros where no gradient was taken (before the first frame, after a frame that started over, with
 * enabled == 0). Two luminance planes (8 B per pixel) and 76 B per stratum — ray, key, result, owner, diff, lambda — belong to the
 * session besides the parent's, about 16.5 B per pixel in all, allocated at begin; a frame allocates nothing after the first: a
 * frame that starts over also shades SW * SH gradient rays (those of sample (k + S - 1) mod S) and uses none of their results, so
 * that every frame's batch has one size and the context's frame records grow once.
 * Everything else as for the parent session. Not done here: the previous pixel's key is not forwarded under reprojection (the noise
 * floor stands in for the cancellation that would bring), the gradient samples are not folded into the history, lambda is one value
 * per stratum, progressive sessions take no gradients. Measured error ratios and times are in DESIGN.md section 27. */
typedef struct RtuGradientDesc {   /* 32 B */
    int32_t  width, height;
    int32_t  radius;               /* 0 .. 3: strata on each side that lambda is summed over */
    float    kappa;                /* >= 0: the noise floor in standard deviations of the summed difference */
    uint32_t enabled;              /* session only: 0 gives the parent session */
    uint32_t frame_index;          /* selects the owners (rtu_gradient_rays); a session sets it */
    uint32_t reserved[2];          /* must be 0 */
} RtuGradientDesc;
int  rtu_gradient_defaults(RtuGradientDesc* out);   /* width, height 0; radius 1, kappa 2, enabled 1, frame_index 0 */
int  rtu_gradient_rays(const RtuGradientDesc* desc, const RtuFrameDesc* frame, int sample, RtuRay* rays_out, uint32_t* keys_out,
                       uint32_t* owner_out);
int  rtu_gradient_rays_device(RtuContext* ctx, const RtuGradientDesc* desc, const RtuFrameDesc* frame, int sample, void* d_rays, void* d_keys,
                              void* d_owner, void* hip_stream);
int  rtu_sample_luminance(const RtuGradientDesc* desc, const float* h_rgbz, const RtuRayHit* h_hits, const float* h_albedo, float* h_lum);
int  rtu_sample_luminance_device(RtuContext* ctx, const RtuGradientDesc* desc, const void* d_rgbz, const void* d_hits, const void* d_albedo,
                                 void* d_lum, void* hip_stream);
int  rtu_temporal_gradient(const RtuTemporalDesc* desc, const RtuGradientDesc* gradient_desc, const RtuFrameDesc* prev_cam,
                           const RtuFrameDesc* cur_cam, const RtuRayHit* h_hits, const float* h_albedo, const RtuNodeMotion* motion,
                           uint32_t n_nodes, const float* h_hist_prev, const float* h_lum_prev, const uint32_t* owner, const float* h_rgbt,
                           float* h_diff_out, float* h_lambda_out);
int  rtu_temporal_gradient_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuGradientDesc* gradient_desc, const RtuFrameDesc* prev_cam,
                                  const RtuFrameDesc* cur_cam, const void* d_hits, const void* d_albedo, const RtuNodeMotion* d_motion,
                                  uint32_t n_nodes, const void* d_hist_prev, const void* d_lum_prev, const void* d_owner, const void* d_rgbt,
                                  void* d_diff_out, void* d_lambda_out, void* hip_stream);
int  rtu_temporal_accumulate_gradient(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                      const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out,
                                      const RtuNodeMotion* motion, uint32_t n_nodes, int32_t history_cap, const float* h_lambda);
int  rtu_temporal_accumulate_gradient_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                             const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                             void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap,
                                             const void* d_lambda, void* hip_stream);
RtuTemporal* rtu_temporal_begin_gradient(RtuContext* ctx, const RtuTemporalDesc* temporal_desc, const RtuVarianceDesc* variance_desc,
                                         const RtuSteerDesc* steer_desc_or_null, const RtuGradientDesc* gradient_desc, int* err_out);
int  rtu_temporal_lambda_device(RtuTemporal* t, void* d_lambda, void* hip_stream);

/* ---- Sparse sessions: one pixel of every block is shaded per frame, the history carries the rest (rtu_sparse.h, rtu_sparse.hip) ----
 * Every session above fires at least one new ray per pixel per frame, and shading that ray is most of a frame. A sparse session shades
 * ONE pixel of every B x B BLOCK per frame — the block's OWNER, which rotates from frame to frame — and lets the full-resolution
 * history carry the other pixels. The guides (RtuRayHit, albedo) stay at full resolution: reprojection and the surface test are what
 * they were, geometry edges stay sharp, and shading is amortised over B * B frames. Binary32, one rounding per operation, no
 * contraction, IEEE divisions, in this order; host and device forms give the same bits. VALID, d, the table, a tap's ACCEPTED and the
 * moments form's e, n, m, E, M, keep ("has an accumulated colour") are those of the sections above.
 *
 * 1. BLOCKS, OWNERS AND RAYS  SW = ceil(width / B), SH = ceil(height / B); block (bx, by) has index b = bx + SW * by and covers
 *   bw x bh pixels, bw = min(B, width - B bx), bh = min(B, height - B by), m = bw * bh. In frame frame_index = k (unsigned 32-bit):
 *     j = k mod m;  t = (j * M_B) mod m in a full block (m == B * B), M_1 = 1, M_2 = 3, M_3 = 5, M_4 = 7 (= 2 B - 1, coprime to B * B:
 *     consecutive frames land far apart and every pixel is the owner exactly once in B * B consecutive frames); t = j in a partial block;
 *     owner_b = (B bx + t mod bw) + width * (B by + t div bw);  s_b = (k div m) mod S, S = frame->samples.
 *   rtu_sparse_rays writes, per block in index order, owner_b and the ray and key of that pixel in rtu_camera_sample_rays(frame, s_b),
 *   bit for bit. A pixel thus walks through all S samples of the frame, not a residue class of them. The frame must have the desc's
 *   size and samples >= 1.
 *
 * 2. THE SPARSE ACCUMULATOR  rtu_temporal_accumulate_sparse is rtu_temporal_accumulate_moments with one changed input: in place of
 *   an image of samples it takes rgbt — SW * SH float4 {r, g, b, t}, what the ray-batch entries return for the rays of step 1 — and
 *   owner, SW * SH pixel indices. Pixel p = x + width * y belongs to block b = (x div B) + SW * (y div B).
 *     owner[b] == p: c = rgbt[b].rgb, z_out = rgbt[b].w, and everything is the moments form's rule for a pixel with that sample —
 *       also where it passes its input through (an invalid pixel; a valid one that found no history and whose c is not finite).
 *     otherwise: the pixel is treated as the moments form treats a pixel whose sample has a channel that is not finite — e = e_prev,
 *       n = n_prev, m = m_prev; with n_prev == 0, E = M = 0 —, z_out = H.t where the pixel is VALID and RTU_BIGFLOAT where not, and
 *       rgb = e * d where the pixel has an accumulated colour (VALID and n_prev > 0), zeros where not.
 *   The planes P and N are written as always, from the guides. hole_out — width * height bytes — is 1 for a pixel that is not its
 *   block's owner and has no accumulated colour, 0 for every other pixel (an owner that passed its sample through is 0).
 *   With B == 1 every pixel is an owner: the outputs are the moments form's bit for bit and hole_out is zeros. An owner entry that
 *   names no pixel of its block leaves the block without a sample; nothing else happens.
 *
 * 3. THE FILL  rtu_sparse_fill, for display only (the history is not touched): for every pixel p with hole[p] == 1 — no other pixel of
 *   rgbz is written —, over the blocks (bx + dx, by + dy), dy outer, dx inner, both -1 .. 1, that lie in the block grid, with q the
 *   block's owner and c the rgb of its rgbt: the block is skipped unless every channel of c is finite and q has p's validity. Then
 *     fdx = (float)(q.x - p.x), fdy likewise;  w = 1 / (1 + (fdx * fdx + fdy * fdy))
 *     e = c / d_q per channel where p is VALID, e = c where not;  A2 += e * w;  W2 += w
 *     and where p is VALID and the tap q would be ACCEPTED for p — node bits equal, dot(N_p, N_q) >= normal_min,
 *     |dot(N_p, P_q - P_p)| <= sigma_plane * H_p.t —: A1 += e * w;  W1 += w.
 *   Tier 1 (A1, W1) is used where W1 > 0, else tier 2 (A2, W2); rgb = (A / W) * d_p where p is VALID, A / W where not; zeros where
 *   both found nothing. z stays what step 2 wrote.
 *
 * RTU_ERR_ARG: what the moments form refuses; a NULL pointer (hist_prev, and with it prev_cam, may be NULL); a sparse desc of another
 * size than the temporal desc or the frame, or outside its rules: width, height 1 .. 65536 and 2^26 pixels, block 1 .. 4, reserved
 * words 0; a device pointer that is not 16-byte aligned (keys, owners: 4-byte; the hole plane: any). The host forms — pure host code,
 * no GPU and no context — also refuse, in rtu_sparse_fill, an owner outside the image. THE DEVICE FORMS TRUST THE TABLE AND THE OWNERS
 * but never leave the arrays: an owner outside the image is skipped by the fill. They allocate nothing, need no scene, touch no state
 * of the context and are asynchronous on hip_stream: rtu_sparse_rays_device (k_sparse_rays, a lane per block),
 * rtu_temporal_accumulate_sparse_device (k_temporal<true, true, false, true>) and rtu_sparse_fill_device (k_sparse_fill, a lane per
 * pixel). No output may overlap an input, but for rgbz of the fill, which is updated in place.
 *
 * THE SESSION  rtu_temporal_begin_sparse opens a variance session whose frames, plain and moved, change as follows: (1) in place of
 * rtu_camera_sample_rays_device, rtu_sparse_rays_device with frame_index = the session's k (frames since begin / reset / start-over);
 * (2) the unchanged shading path shades SW * SH rays, the capacity retry as before; (3) after the full-resolution guides come
 * rtu_temporal_accumulate_sparse_device in place of the moments form and rtu_sparse_fill_device; (4) rtu_variance_device and
 * rtu_denoise_variance_device, unchanged. sparse_desc: width and height are both 0 (the session's are used) or the session's, any other
 * size is refused; frame_index is ignored; block == 1
 * gives a variance session's bits and launches nothing more. rtu_temporal_holes counts the pixels of the last frame's hole plane (0
 * before the first frame and with block == 1; it waits for that frame through an event of the session's, on the context's own
 * stream: the stream the frame was given need not exist any more). The buffers — those of a variance session, whose ray, key and
 * result buffers keep the size of the image though a frame uses their first SW * SH entries, and besides 4 B per block (the owners),
 * one byte per pixel on the device and one of pinned host memory — belong to the session and are allocated at begin; a frame
 * allocates nothing after the first. Frame 0 shades one pixel per block like every other: the first B * B frames show mostly filled
 * pixels. Everything else — reset, free, the handle after rtu_destroy_context, the start-over after a scene change on a plain frame —
 * as for a variance session. RTU_ERR_ARG besides: RTU_TEMPORAL_DENOISE. Not done here: sparse sessions combined with steering or
 * gradients (there is no entry that opens one), a dense first frame, feeding the fill into the history, sharded frames. Measured
 * times, hole counts and error ratios are in DESIGN.md section 28. */
typedef struct RtuSparseDesc {     /* 32 B */
    int32_t  width, height;
    int32_t  block;                /* B, 1 .. 4 */
    uint32_t frame_index;          /* selects the owners and their samples (rtu_sparse_rays); a session sets it */
    uint32_t reserved[4];          /* must be 0 */
} RtuSparseDesc;
int  rtu_sparse_defaults(RtuSparseDesc* out);   /* width, height 0; block 2, frame_index 0 */
int  rtu_sparse_rays(const RtuSparseDesc* desc, const RtuFrameDesc* frame, RtuRay* rays_out, uint32_t* keys_out, uint32_t* owner_out);
int  rtu_sparse_rays_device(RtuContext* ctx, const RtuSparseDesc* desc, const RtuFrameDesc* frame, void* d_rays, void* d_keys, void* d_owner,
                            void* hip_stream);
int  rtu_temporal_accumulate_sparse(const RtuTemporalDesc* desc, const RtuSparseDesc* sparse_desc, const RtuFrameDesc* prev_cam,
                                    const RtuFrameDesc* cur_cam, const float* h_rgbt, const uint32_t* owner, const RtuRayHit* h_hits,
                                    const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out, uint8_t* h_hole_out,
                                    const RtuNodeMotion* motion, uint32_t n_nodes, int32_t history_cap);
int  rtu_temporal_accumulate_sparse_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuSparseDesc* sparse_desc, const RtuFrameDesc* prev_cam,
                                           const RtuFrameDesc* cur_cam, const void* d_rgbt, const void* d_owner, const void* d_hits,
                                           const void* d_albedo, const void* d_hist_prev, void* d_hist_out, void* d_rgbz_out, void* d_hole_out,
                                           const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap, void* hip_stream);
int  rtu_sparse_fill(const RtuTemporalDesc* desc, const RtuSparseDesc* sparse_desc, const RtuRayHit* h_hits, const float* h_albedo,
                     const uint32_t* owner, const float* h_rgbt, const uint8_t* h_hole, float* h_rgbz);
int  rtu_sparse_fill_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuSparseDesc* sparse_desc, const void* d_hits, const void* d_albedo,
                            const void* d_owner, const void* d_rgbt, const void* d_hole, void* d_rgbz, void* hip_stream);
RtuTemporal* rtu_temporal_begin_sparse(RtuContext* ctx, const RtuTemporalDesc* temporal_desc, const RtuVarianceDesc* variance_desc,
                                       const RtuSparseDesc* sparse_desc, int* err_out);
int  rtu_temporal_holes(RtuTemporal* t, uint32_t* count_out);

/* ---- Hole rays: a sparse session shades the pixels that have no colour at all, within a budget (rtu_holes.h, rtu_holes.hip) ----
 * A sparse session has nothing to show where there is neither a sample nor a history: all of frame 0 but the owners, most of the
 * image after a camera cut, the disocclusions of every moving frame. rtu_sparse_fill guesses those pixels from neighbouring blocks and
 * they stay guesses until their turn as owner comes, up to B * B - 1 frames later. The entries below spend real rays on them, at most
 * `budget` per frame, and make the result the pixel's history. Binary32, one rounding per operation, no contraction, IEEE divisions,
 * in this order; host and device forms give the same bits. VALID, d, l(e), mix32, E, M and the moments history are those of the
 * sections above.
 *
 * 1. THE ALLOCATION  rtu_hole_allocation: out of the hole plane of rtu_temporal_accumulate_sparse (width * height bytes) and the
 *   frame's RtuRayHit, uint32 counts[pixels], offsets[pixels] and the total. The weight is w_p = 1 iff hole[p] == 1 and p is VALID,
 *   otherwise 0: an invalid pixel (a miss) is never accumulated by any form, it would eat the budget in every frame, so it stays with
 *   the fill. Wsum, the dither h, the count c, the exclusive scan and THE CUT are rtu_sample_allocation's, word for word, with this w
 *   and max_extra = 1. So with budget >= Wsum every VALID hole gets exactly one ray and total = Wsum; with less, a hole is taken with
 *   probability budget / Wsum by the 16-bit dither of (p, frame_index), and the scan cuts at the budget: total <= budget always.
 *
 * 2. THE RAYS  No new rule: rtu_extra_sample_rays with an RtuSteerDesc of {the size, budget, max_extra = 1, frame_index = k}. With
 *   S = frame->samples and F = `frame` with samples = 2 S: ray offsets_p and its key are those of pixel p in
 *   rtu_camera_sample_rays(F, S + (k mod S)), bit for bit, and owner[offsets_p] = p. The sample indices are disjoint from the
 *   0 .. S - 1 the owners walk through: a hole-shaded pixel never receives the same sample again when its turn as owner comes. A frame
 *   needs 2 S <= 65536.
 *
 * 3. THE FOLD  rtu_hole_fold: the shaded {r, g, b, t} of the hole rays made the history of their pixels — in the moments history
 *   rtu_temporal_accumulate_sparse just wrote, its rgbz and its hole plane, all in place. For a pixel with counts_p >= 1,
 *   hole[p] == 1, VALID and offsets_p < n_rays, with c the rgb of rgbt[offsets_p]:
 *     a channel of c is not finite: nothing changes; the pixel stays a hole and the fill takes it.
 *     otherwise e = c / d, E = {e, 1};  l = l(e), l2 = l * l, M = {l, l2, 0, 0} if l2 is finite, else zeros (the skip rule of the
 *     moments);  rgb = e * d;  hole[p] = 0. z and the planes P and N are untouched.
 *   These are the bits rtu_temporal_accumulate_moments gives a VALID pixel that found no history and took the sample c. Every other
 *   pixel, and every other word, passes bit for bit. Of desc only width and height are used (the others must still be valid).
 *
 * RTU_ERR_ARG: a NULL pointer; width or height outside 1 .. 65536 or more than 2^26 pixels; budget above 2^26; a non-zero reserved
 * word; n_rays above 2^26; a device pointer that is not 16-byte aligned (counts, offsets, total: 4-byte; the hole plane: any). The
 * host forms — pure host code, no GPU and no context — also refuse, in rtu_hole_fold, a count above 1 and a pixel whose
 * offsets_p + counts_p exceeds n_rays. THE DEVICE FORMS TRUST counts AND offsets but never leave the arrays: any count >= 1 is one
 * sample, a sample at or beyond n_rays is not read and its pixel not written. They are asynchronous on hip_stream and need no scene.
 * rtu_hole_allocation_device (k_hole_weight: a lane per four pixels, the hit record read only where the hole byte is 1, a reduction
 * per workgroup and one 64-bit atomic add each; then k_steer_counts, k_steer_sums, k_steer_finish of "Steered sampling", unchanged)
 * works in the grow-only scratch of the context that rtu_sample_allocation_device uses: one stream per context, nothing allocated
 * from the second call at a size. rtu_hole_fold_device (k_hole_fold, a lane per pixel that ends after one 4-byte load wherever
 * counts_p == 0) allocates nothing and touches no state of the context.
 *
 * THE SESSION  rtu_temporal_begin_sparse_holes opens a sparse session. With block > 1 and budget > 0 its frames, plain and moved,
 * continue after the sparse accumulator (step 3 of "Sparse sessions") with: (1) the allocation, frame_index = the session's k;
 * (2) the total read back (4 bytes into pinned memory of the session, synchronous, as a steered session does); (3) if the total is
 * above 0: the hole rays written into the session's ray, key and result buffers BEHIND their first SW * SH entries (the holes never
 * exceed width * height - SW * SH: the batch always fits), shaded by the unchanged rtu_shade_rays_sampled_device /
 * rtu_shade_rays_paths_device path with n = the total, the capacity retry as before, and folded; (4) rtu_sparse_fill_device on what
 * is still a hole, rtu_variance_device and the filter, unchanged. hole_desc: width and height are both 0 or the session's;
 * frame_index is ignored. budget == 0 or block == 1 gives the sparse session's bits and launches nothing more.
 * rtu_temporal_holes counts the plane after the fold: what the fill had to fill. rtu_temporal_hole_rays returns the last frame's
 * total (0 before the first frame, after a reset and with budget 0). Beside the sparse session's buffers, allocated at begin: counts,
 * offsets and owners (4 B per pixel each), the total on the device and one pinned word. The context's frame records grow only when a
 * hole batch exceeds every earlier batch of the session (typically in frame 0 and after the first cut) — not "nothing after the
 * first frame". A refused call leaves the session as it was. Reset, free, the start-over after a scene change on a plain frame and
 * the handle after rtu_destroy_context: as for a sparse session. RTU_ERR_ARG: what a sparse session refuses; a hole desc outside its
 * rules or of another size; with budget > 0 and block > 1, a frame with 2 S > 65536. Not done here: hole rays for invalid pixels;
 * combining with steering or gradients; a cheaper k_variance start-up (a hole-shaded pixel has n = 1 and takes the neighbourhood
 * branch until min_history, the next step DESIGN.md section 28 names); avoiding the read-back. Measured error ratios and times are
 * in DESIGN.md section 29. */
typedef struct RtuHoleDesc {       /* 32 B */
    int32_t  width, height;
    uint32_t budget;               /* 0 .. 2^26: hole rays per frame, at most; 0 = none */
    uint32_t frame_index;          /* the dither and the sample index; a session sets it */
    uint32_t reserved[4];          /* must be 0 */
} RtuHoleDesc;
int  rtu_hole_defaults(RtuHoleDesc* out);   /* width, height 0; budget 0; frame_index 0 */
int  rtu_hole_allocation(const RtuHoleDesc* desc, const uint8_t* h_hole, const RtuRayHit* h_hits, uint32_t* counts, uint32_t* offsets,
                         uint32_t* total);
int  rtu_hole_allocation_device(RtuContext* ctx, const RtuHoleDesc* desc, const void* d_hole, const void* d_hits, void* d_counts, void* d_offsets,
                                void* d_total, void* hip_stream);
int  rtu_hole_fold(const RtuHoleDesc* desc, float* h_hist, float* h_rgbz, uint8_t* h_hole, const RtuRayHit* h_hits, const float* h_albedo,
                   const uint32_t* counts, const uint32_t* offsets, const float* h_rgbt, size_t n_rays);
int  rtu_hole_fold_device(RtuContext* ctx, const RtuHoleDesc* desc, void* d_hist, void* d_rgbz, void* d_hole, const void* d_hits,
                          const void* d_albedo, const void* d_counts, const void* d_offsets, const void* d_rgbt, size_t n_rays, void* hip_stream);
RtuTemporal* rtu_temporal_begin_sparse_holes(RtuContext* ctx, const RtuTemporalDesc* temporal_desc, const RtuVarianceDesc* variance_desc,
                                             const RtuSparseDesc* sparse_desc, const RtuHoleDesc* hole_desc, int* err_out);
int  rtu_temporal_hole_rays(RtuTemporal* t, uint32_t* count_out);

/* ---- Temporal accumulation for sensors: previews that follow a moving panoramic, fisheye or orthographic sensor (rtu_sensor.h
 * sensor_project, rtu_temporal.h TpSensorProj, rtu_temporal.hip k_temporal_sensor<MODEL, MOMENTS>) ----
 * "Temporal accumulation" with an RtuSensorDesc in place of each camera. Everything it states holds unchanged — the history planes, the
 * range test, the four taps and their order, the tap acceptance test, the blend, the moments of "Variance-guided filtering" — but the
 * lookup, which goes through THE PROJECTION of the previous sensor S: the counterpart of THE RAY of "Sensors", world point Pm to image
 * coordinates (fx, fy) in which pixel (x, y) has its centre at (x, y). binary32, one rounding per operation, in the order written, no
 * contraction, IEEE divide and sqrt, dot as in "Temporal accumulation". The only transcendental is acos(x): the portable_acos of the
 * sample streams — binary64 IEEE operations in fdlibm's sequence, rounded to float (sensor_acos in rtu_sensor.h states it for host
 * and device). W = (float)S.width, H = (float)S.height.
 *   Q = Pm - S.pos;  a = dot(Q, S.forward);  b = dot(Q, S.right);  c = dot(Q, S.up)
 *   angle(s, k), s >= 0:  L = sqrtf(s * s + k * k); none unless L is finite and L > 0
 *                         |k| <= s  : acos(k / L)
 *                         otherwise q = acos(s / L);  k > 0 ? 1.5707964f - q : 1.5707964f + q
 *                         (acos never gets an argument above about 0.71 in magnitude: well conditioned in binary32)
 *   RTU_SENSOR_EQUIRECT  h = sqrtf(a * a + b * b); none if h == 0 (a pole). pol = angle(h, c); th = angle(|b|, -a);
 *                        lon = b <= 0 ? th : 6.2831855f - th;  fx = lon / 6.2831855f * W - 0.5f;  fy = pol / 3.1415927f * H - 0.5f.
 *                        COLUMNS WRAP: a tap at column qx is taken at qx + width when qx < 0 and at qx - width when qx >= width.
 *                        Rows do not wrap.
 *   RTU_SENSOR_FISHEYE   p = sqrtf(b * b + c * c). p == 0: the image centre (0.5f * W - 0.5f, 0.5f * H - 0.5f) when a > 0, otherwise
 *                        none. Otherwise r = angle(p, a) / (fov_deg * 0.008726646f); none unless r <= 1;
 *                        R = 0.5f * (float)min(width, height);  fx = ((r * (b / p)) * R + 0.5f * W) - 0.5f;
 *                        fy = ((-(r * (c / p))) * R + 0.5f * H) - 0.5f. A history pixel outside the image circle has n = 0: no
 *                        tap accepts it.
 *   RTU_SENSOR_ORTHO     none unless a > 0;  fx = (b / extent[0] + 0.5f) * W - 0.5f;  fy = (0.5f - c / extent[1]) * H - 0.5f.
 * rtu_sensor_project (pure host code, no GPU and no context) is the executable statement of these expressions for n points {x, y, z}:
 * fxfy_out[2 i ..] = (fx, fy) and ok_out[i] = 1, or (0, 0) and 0 where the point has none. The range test is not part of it.
 *   lookup   NONE without a previous history, or when prev and cur differ in model, width or height (hist_prev is then not read).
 *            STATIC (the one tap is the pixel itself) when model, width, height, pos, right, up, forward are equal bit for bit, and
 *            fov_deg for a fisheye, extent for an orthographic sensor. REPROJECT through the projection of prev otherwise.
 * The scene is at rest: there is no motion table and no history_cap; the moments form is that of "Variance-guided filtering" with an
 * all-STATIC table, and for equal sensors both forms give the bits the camera forms give for equal cameras on the same arrays.
 * RTU_ERR_ARG: as for rtu_temporal_accumulate[_moments][_device]; a sensor outside the rules of "Sensors"; cur of another size than the
 * desc. With hist_prev == NULL prev may be NULL.
 *   rtu_temporal_accumulate_sensor, _sensor_moments                 pure host code: the executable statement.
 *   rtu_temporal_accumulate_sensor_device, _sensor_moments_device   the same bits from device memory (one lane per pixel),
 *                                                                   asynchronous on hip_stream; allocate nothing, need no scene.
 * SENSOR FRAMES of a session from rtu_temporal_begin (with or without RTU_TEMPORAL_DENOISE) or rtu_temporal_begin_variance. Frame k of
 * a recipe S / P sensor (samples = S >= 1, gather_bounces 0 or 4, the desc's size):
 *   1. the rays and keys of sample k mod S (rtu_sensor_rays_device),
 *   2. shaded by rtu_shade_rays_sampled_device / _paths_device with eye = pos and the sensor's max_bounce and flags, under the capacity
 *      repair of rtu_temporal_frame_device (SYNCHRONOUS on hip_stream),
 *   3. the guides: rtu_ray_features_device (flags 0) of the pixel-centre rays — the rays of the same sensor with samples = 0,
 *   4. the accumulator above, plain or moments, against the previous frame's sensor and history, into d_rgbz,
 *   5. the filter of the session, unchanged: rtu_denoise_device, or rtu_variance_device and rtu_denoise_variance_device. THE FILTER DOES
 *      NOT WRAP at a panorama's seam: the first and the last column are image borders to it.
 * A session takes camera frames and sensor frames in any order: a frame whose predecessor was of the other kind, or a sensor of
 * another model, takes no history (lookup NONE), and k goes on counting. Everything "Temporal accumulation" says of sessions holds: a
 * refused call leaves the session as it was, a scene change starts over, no allocation after the first frame, one stream per context;
 * rtu_temporal_history_device and rtu_temporal_reset work as before. Steered, gradient (enabled != 0), sparse and hole sessions refuse
 * a sensor with RTU_ERR_ARG — their ray generators go through the camera's sample rays — and go on as if the call had not been made.
 * The scene is at rest between sensor frames: there is no sensor form of rtu_temporal_frame_moved.
 * RTU_ERR_ARG: recipe W (samples 0), a sensor outside the rules of "Sensors" (so more than 2^25 pixels), a sensor of another size than
 * the session, a NULL or misaligned d_rgbz; RTU_ERR_NO_SCENE. */
int  rtu_sensor_project(const RtuSensorDesc* sensor, const float* points_xyz, size_t n, float* fxfy_out, uint8_t* ok_out);
int  rtu_temporal_accumulate_sensor(const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur, const float* h_rgbz,
                                    const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out);
int  rtu_temporal_accumulate_sensor_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur,
                                           const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                           void* d_rgbz_out, void* hip_stream);
int  rtu_temporal_accumulate_sensor_moments(const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur, const float* h_rgbz,
                                            const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out,
                                            float* h_rgbz_out);
int  rtu_temporal_accumulate_sensor_moments_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur,
                                                   const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev,
                                                   void* d_hist_out, void* d_rgbz_out, void* hip_stream);
int  rtu_temporal_sensor_frame_device(RtuTemporal* t, const RtuSensorDesc* sensor, void* d_rgbz, void* hip_stream);
int  rtu_temporal_sensor_frame(RtuTemporal* t, const RtuSensorDesc* sensor, float* h_rgbz);

/* Cancellation (StopRender(), main.cpp:70-72): a word the caller may set non-zero at any time; the context reads it between the
 * launch sequences of a sampled frame (recipes S / P: one sequence per batch of samples — a 64-sample 1080p frame is hundreds
 * of milliseconds) and returns RTU_ERR_CANCELLED from the render call. NULL: none. The word is read with a relaxed atomic load; a writer
 * on another thread stores it with __atomic_store_n(flag, 1, __ATOMIC_RELAXED) (rtu_stop_render does). A single launch sequence (a frame of
 * recipe W, a batch of frames in flight) is a fraction of a millisecond and is never interrupted. */
int  rtu_set_cancel_flag(RtuContext* ctx, const volatile int* flag);

/* ---- Several GPUs behind one handle (raytracer-utah_amd/csrc/rtu_multi.hip) ----------------------------------------------
 * What SpawnRenderThreads does with CPU workers (main.cpp:29-64): fan one frame out, wait, hand back one image. The frame is
 * sharded by interleaved RTU_BAND_ROWS-row bands (band b -> the b mod n-th device), the scene replicated on every GPU; the
 * float4 shards are gathered to the first GPU with one grouped RCCL send / receive over xGMI (n distinct GPUs, librccl.so
 * found) or by concurrent asynchronous copies into pinned host memory (several contexts on one GPU, or no RCCL), and land,
 * de-interleaved, in h_rgbz = height * width float4 in image order. device_ids may repeat (n contexts on one GPU: how the
 * one-GPU test box exercises this path). The RCCL branch with n > 1 distinct GPUs has not run on hardware.
 *
 * progress (may be NULL): `cancel` as rtu_set_cancel_flag (polled between sample batches on every GPU, between capacity
 * rounds and between the shards as they are handed over); rows_done(user, rows, row0, nrows) is called once per band as
 * the shards arrive, from the calling thread, with `rows` = nrows * width float4 of image rows [row0, row0 + nrows) — what
 * RenderImage::IncrementNumRenderPixel (scene.h:585-588) counts and the viewport polls (viewport.cpp:390-410). h_rgbz may be
 * NULL when rows_done consumes the rows. frame->shard_rank / shard_count are ignored. Synchronous; 0 or a negative RTU_ERR_*
 * (rtu_multi_last_error). */
typedef struct RtuMultiContext RtuMultiContext;
typedef struct RtuProgress {
    const volatile int* cancel;
    void (*rows_done)(void* user, const float* rows, int row0, int nrows);
    void* user;
} RtuProgress;
RtuMultiContext* rtu_create_context_multi(const int* device_ids, int n_devices, int* err_out);
void        rtu_destroy_context_multi(RtuMultiContext* m);
int         rtu_multi_size(const RtuMultiContext* m);
RtuContext* rtu_multi_context(RtuMultiContext* m, int i);            /* the i-th GPU's context (diagnostics, rtu_debug_*) */
const char* rtu_multi_last_error(const RtuMultiContext* m);
int         rtu_multi_upload_scene(RtuMultiContext* m, const RtuSceneDesc* scene);
int         rtu_multi_update_scene(RtuMultiContext* m, const RtuSceneDesc* scene);  /* rtu_update_scene on every context */
int         rtu_multi_update_meshes(RtuMultiContext* m, const RtuSceneDesc* scene, const uint32_t* mesh_ids, int n_meshes);  /* rtu_update_meshes on every context */
int         rtu_multi_render_frame(RtuMultiContext* m, const RtuFrameDesc* frame, float* h_rgbz, const RtuProgress* progress);
/* How the shards of the last rtu_multi_render_frame reached the host: 1 one context; 2 several contexts, asynchronous copies into
 * one pinned buffer, all in flight together; 3 RCCL (grouped ncclSend / ncclRecv to the first GPU, then one copy). */
int         rtu_multi_gather_kind(const RtuMultiContext* m);

/* Diagnostic: render one frame with every wavefront stamping the GPU's constant clock on entry
 * and exit, and return, per kernel launch that ran, its slot (0 primary, 1/2 primary stage 2
 * cooperative/wide, 3+4L.. trace, stage 2 cooperative, stage 2 wide, consume of level L,
 * 27+L combine of level L) and the first-entry / last-exit times in microseconds from the first
 * stamp. Unlike a profiler trace this neither serialises nor pads the launches. Returns the
 * number of entries (<= max_entries) or a negative RTU_ERR_*. Synchronous. */
int  rtu_render_timeline(RtuContext* ctx, const RtuFrameDesc* frame, void* d_rgbz, int max_entries, int* slot_out,
                         double* start_us_out, double* end_us_out);

/* Diagnostic, after rtu_render_timeline: the exit times (microseconds after the kernel's first entry) of
 * the wavefronts of the launch in timeline slot `slot` — one value per wavefront slot (index modulo
 * 8192; a later wavefront overwrites an earlier one). Shows whether a launch is a plateau or a tail.
 * Returns the number of values written. */
int  rtu_timeline_exits(RtuContext* ctx, int slot, int max_values, double* exit_us_out);

/* Test hook for the tail kernel. Recursion levels that were almost empty in the previous frame of a
 * scene are not launched kernel by kernel in the next one: one kernel evaluates every frame of the
 * first such level, subtree and all, with one wavefront per frame. Which level that is
 * comes from the counts of the previous launch of the same shape and is only a hint — any value renders the same image; if the
 * level turns out to hold thousands of frames (the view changed) the kernel refuses it on the device, the frame is reported
 * incomplete like a capacity overflow (rtu_frame_status) and rendered again level by level.
 * This sets the cut level for the NEXT launch only (taken as it is, never refused): 1..5, or 6 for "no tail". */
int  rtu_debug_tail_from(RtuContext* ctx, int level);
/* Test hook: the cut level the most recent launch of the recursion levels was made with — 1..5, or 6 for "no tail" (also what the
 * counting variant always uses) —, whether forced by rtu_debug_tail_from or learned. RTU_ERR_ARG for a NULL context. */
int  rtu_debug_last_tail_from(RtuContext* ctx);

/* Test hook: switch the node-level bounds of the fast variant off (0) or on (1, the default after an upload) until the next
 * upload: the world-space box per scene node and, for primary rays, its screen rectangle per camera, by which a ray skips
 * nodes it cannot touch before their transformation and exact test. Results must not change. */
int  rtu_debug_node_bounds(RtuContext* ctx, int on);

/* Experiment switches for performance work (which part of a kernel costs what): bits are defined next to their use in
 * render_impl.h; bits 0..7 render WRONG images: never set them in production paths or tests of results. Five bits only switch an
 * optimisation off and leave every result bit alone (tests compare the images with and without; 4096 below is a sixth): 256 = no tile occupancy
 * (k_primary tests every tile against the node rectangles and coverage masks itself), 512 = no stage-2 grid hints (both
 * stage-2 kernels of every tracing phase are launched at full size), 64 = the occluder lists of shadow rays only say "empty cell or
 * not" (every listed ray walks the BVH), 2048 = no Shade() call is settled without a frame record (every hit becomes a frame),
 * 4096 = a plane hit's normal through every transformation of its chain, as the reference writes it, instead of from the node's
 * table (csrc/rtu_device.h DevNode::plane_n),
 * 8192 = no side mode (stage 2 of the primary phase in the launch stream, before the recursion levels, instead of beside them),
 * 16384 = both stage-2 kernels of every phase are launched whatever the last launch's list lengths said (outside side mode).
 * 131072 (a wrong image; frames with collect_stats == 2 only) = stage 2 of the primary phase writes the work of each ray's BVH walk — two
 * units per inner step, one per triangle test — over the pixel's red channel (tools/scratch/walk_units.py). */
int  rtu_debug_flags(RtuContext* ctx, uint32_t bits);
/* A hint, never needed for correctness: how many launch sequences the caller keeps in flight on this GPU at once, over all of its
 * contexts together (bench.py alternates its batches over two contexts: 2). A context then sizes the grid of its long-running
 * primary kernel for its share of the machine instead of all of it (measured, two sequences in flight: 59.4 -> 62.5 Grays/s).
 * Default 1. Any value renders the same images. */
int  rtu_set_sequences_in_flight(RtuContext* ctx, int n);

/* Test hook: let the walks of the fast trees use at most `entries` stack entries from the next frame on
 * (until the next upload), so that tests can exercise the overflow path — a ray whose walk would
 * need more is finished on the reference's tree — on any scene. Results must not change. */
int  rtu_debug_walk_stack_limit(RtuContext* ctx, uint32_t entries);

/* Diagnostic: the acceleration structures built at upload for mesh `mesh`: out5 = {faces, depth of the
 * binned-SAH tree, deepest stack a walk of its 4-wide form can build (walks are given
 * min(that, RTU_MAX_BVH_STACK) entries; a ray that needs more finishes on the reference's tree),
 * 4-wide nodes, 8-wide nodes}. */
int  rtu_mesh_info(const RtuContext* ctx, uint32_t mesh, uint32_t* out5);

/* Diagnostic: the occluder lists of shadow rays built at upload (rtu_device.h DevLightMask), one per (non-ambient light < 4,
 * masked mesh node) pair that got one, in build order: out5 = {light slot, masked mesh slot, grid size G, entries of all
 * cells together, entries of the longest cell}. RTU_ERR_ARG past the last one. */
int  rtu_light_list_info(const RtuContext* ctx, uint32_t index, uint32_t* out5);

/* Test hook, pure host code (no GPU, no context): the occluder list rtu_upload_scene would build for the light_slot-th non-ambient
 * light and the cover_slot-th mesh node of the scene — frame, grid and, per cell, its entries as FACES of the node's mesh with the
 * depth in front of which an origin cannot see them (ascending per cell) — so that a CPU test can check ray by ray that every
 * triangle a shadow ray hits is listed in the cell of the ray's origin. cell = int((v - v0) * sv) * G + int((u - u0) * su) with
 * (u, v) = ((p - L) . X, (p - L) . Y) [/ ((p - L) . Z) for a point light]. usable == 0: no list from there (arrays NULL). */
typedef struct RtuLightListDump {
    int32_t  usable, node, light;
    uint32_t G, point, n_entries;
    float    X[3], Y[3], Z[3], L[3], u0, v0, su, sv;
    uint32_t* cell_off;     /* [G * G + 1] */
    uint32_t* entry_face;   /* [n_entries] */
    float*    entry_zmin;   /* [n_entries] */
} RtuLightListDump;
int  rtu_debug_light_list(const RtuSceneDesc* scene, uint32_t light_slot, uint32_t cover_slot, RtuLightListDump* out);
void rtu_debug_light_list_free(RtuLightListDump* dump);
/* Test hook: the list the context holds now (index as in rtu_light_list_info), copied back from the GPU into the same layout
 * (free with rtu_debug_light_list_free). Synchronous. */
int  rtu_debug_context_light_list(RtuContext* ctx, uint32_t index, RtuLightListDump* out);
/* Diagnostic: on != 0 times the phases of the device builder of later rtu_update_scene calls with HIP events (it synchronises
 * between phases); ms_out5 (may be NULL) gets the milliseconds spent since the previous call: {cover meshes and their extents,
 * corner pass, count passes, fill and offsets, radix sort}. */
int  rtu_debug_update_timing(RtuContext* ctx, int on, float* ms_out5);
/* Diagnostic: on != 0 times the phases of later rtu_update_meshes calls with HIP events on the context's stream. ms_out4 (may be
 * NULL) receives the milliseconds summed since the previous call: copies to HBM, triangle records, refit of bvh4 / bvh8, placement
 * (the rtu_update_scene part); they are reset. */
int  rtu_debug_mesh_update_timing(RtuContext* ctx, int on, float* ms_out4);

/* Test hooks of rtu_update_meshes: one array of what a mesh is on the device. */
#define RTU_MESH_BVH4          0  /* float4 [8 nodes4]: the fast tree collapsed to 4 children per node */
#define RTU_MESH_BVH8          1  /* float4 [16 nodes8]: ... to 8 */
#define RTU_MESH_FAST_TRI      2  /* float4 [4 nf]: triangle records in the fast tree's element order */
#define RTU_MESH_REF_TRI       3  /* float4 [4 nf]: ... in the `ref` tree's */
#define RTU_MESH_REF_BVH       4  /* RtuBvhNode [n_bvh_nodes]: the `ref` tree, renumbered breadth-first */
#define RTU_MESH_REF_ELEMENTS  5  /* uint32 [nf] */
#define RTU_MESH_V             6  /* float [3 nv] */
#define RTU_MESH_VN            7  /* float [3 nvn] */
#define RTU_MESH_HEADER        8  /* RtuMeshHeaderDump */
#define RTU_MESH_FAST_ELEMENTS 9  /* uint32 [nf]: element slot of the fast tree -> face */
typedef struct RtuMeshHeaderDump {
    float    bmin[3], bmax[3], scale;
    uint32_t n_bvh_nodes, any_empty_box;
} RtuMeshHeaderDump;
/* What the context holds for mesh `mesh` now, copied back from the GPU (synchronous). *bytes_out (may be NULL) is the size of the
 * array; RTU_ERR_ARG when capacity_bytes is smaller (nothing is copied: ask with capacity 0 first). */
int  rtu_debug_context_mesh(RtuContext* ctx, uint32_t mesh, int which, void* out, size_t capacity_bytes, size_t* bytes_out);
/* The same array as the HOST makes it — pure host code, no GPU and no context: the topology of the fast tree from the builders of
 * rtu_upload_scene on the mesh `uploaded`; boxes, records, vertices and `ref` tree from `now` (same nv / nf / nvn; its f is not read),
 * the boxes by the host restatement of the device refit. now == NULL: `uploaded` as rtu_upload_scene builds it, no refit — what
 * a refit with the uploaded vertices must reproduce (boxes as float values). */
int  rtu_debug_host_mesh(const RtuMesh* uploaded, const RtuMesh* now, int which, void* out, size_t capacity_bytes, size_t* bytes_out);
/* Test hooks of rtu_update_meshes_device, pure host code. rtu_debug_host_ref_build: the HOST FORM of the device builder (the same
 * passes, run in loops) on the connectivity of `uploaded` with the vertices v (float [3 nv]; NULL: uploaded->v). which:
 * RTU_MESH_REF_BVH, RTU_MESH_REF_ELEMENTS, RTU_MESH_VN (the normals RTU_MESH_EDIT_RECOMPUTE_NORMALS computes; needs nvn == nv), or
 * RTU_MESH_HEADER for an RtuRefBuildHeader. No depth bound: a tree deeper than RTU_MAX_BVH_STACK is built and its depth reported.
 * rtu_debug_partition_rule: the closed form of the builder's partition for the keep flags keep[n]; perm_out[i] is the position
 * whose element ends at position i. */
typedef struct RtuRefBuildHeader {
    float    bmin[3], bmax[3], scale;
    uint32_t n_bvh_nodes, any_empty_box, bvh_depth;
} RtuRefBuildHeader;
int  rtu_debug_host_ref_build(const RtuMesh* uploaded, const float* v, int which, void* out, size_t capacity_bytes, size_t* bytes_out);
int  rtu_debug_partition_rule(const uint8_t* keep, uint32_t n, uint32_t* perm_out);
/* Diagnostic: the milliseconds rtu_update_meshes_device spent per phase since the previous call (HIP events on the context's stream,
 * enabled by rtu_debug_mesh_update_timing): {tree build and normals, copies, triangle records and refit, placement}; reset. */
int  rtu_debug_mesh_update_device_timing(RtuContext* ctx, float* ms_out4);

/* Diagnostic: Shade() frames per recursion level (6 values) and rays deferred to stage 2 per phase
 * (7 values: primary, then levels 0..5) of the most recent frame (fast variant). Synchronises. */
int  rtu_frame_counts(RtuContext* ctx, uint32_t* frames_out, uint32_t* deferred_out);

/* Counters of the last frame rendered with collect_stats=1 (synchronises). */
int  rtu_get_stats(RtuContext* ctx, RtuStats* stats);

/* Touched-bytes mode (collect_stats == 2): what the kernels of the FAST variant — the ones bench.py times — read and write,
 * per kernel launch of the most recent launch sequence. A slot is a kernel's place in the sequence (rtu_kernel_slot_name:
 * "k_primary", "k_primary2c", "k_primary2", "k_trace(L0)", "k_trace2c(L0)", "k_trace2(L0)", "k_consume(L0)", ..., "k_combine(L0)", ...;
 * the tail kernel reports in the k_trace slot of its cut level). The images of this mode are those of the fast variant, bit for bit.
 * ALGORITHMIC bytes of a launch (rtu_touched_bytes; cache-agnostic, every access counted where it is made):
 *   24 bound_tests (a node's world-space box) + 48 node_tests (itm + pos) + 24 mesh_box_tests (bounding box) + 84 xform_levels (tm + pos + itm of FromNodeCoords)
 *   + 112 inner4 (7 float4 of a 4-wide node) + 256 inner8 (8 x 32 B child records) + 64 inner_ref (a sibling pair of the reference's
 *   tree: exact-tie / stack-overflow fallback) + 64 tri_tests (triangle record) + 100 winners (element, face and normal indices, three
 *   vertices, three normals; 148 with texture vertices) + record_bytes (frame records, lists, shadow results, pixels: counted at
 *   every load / store). SURVEY 8d's per-unit figures with the record sizes of THIS layout in place of the reference's.
 * Wave-uniform data — scene nodes and their bounds, mesh headers, screen rectangles — is read through the constant address space
 * by scalar loads, ONCE PER WAVEFRONT whatever the number of lanes that need it: bound_tests, node_tests and mesh_box_tests count
 * wavefronts, not lanes (the reference reads them once per ray; a GPU lane does not). Everything else is per lane. */
#define RTU_KERNEL_SLOTS 40
typedef struct RtuTouched {
    uint64_t rays;            /* Trace / ShadowTrace walks started by this launch */
    uint64_t node_tests, mesh_box_tests, inner4, inner8, inner_ref, tri_tests, winners, xform_levels;
    uint64_t record_bytes;
    uint64_t bound_tests;     /* node-level bounds tested (24 B each: the node's world-space box) */
    uint64_t inline_shadow_rays; /* of `rays`: shadow rays of childless Shade() calls fired by the lane that found the hit (no frame record) */
} RtuTouched;
int         rtu_get_touched(RtuContext* ctx, RtuTouched* per_slot, int n_slots);   /* synchronises; returns the slots written */
/* A sampled frame (recipes S / P) is many launch sequences — one per batch of samples, ten per batch for recipe P — and its counters are
 * the sums over all of them: per_slot[i] = the number of launches of slot i's kernel that went into the table since it was zeroed
 * (bytes per launch = rtu_touched_bytes / launches). Slot 33 is recipe P's k_gi_roots, slot 34 the k_tail launch of side mode (the few
 * frames stage 2 of the primary phase makes, evaluated on the helper stream beside the recursion levels). */
int         rtu_get_touched_launches(RtuContext* ctx, uint32_t* per_slot, int n_slots);
unsigned long long rtu_touched_bytes(const RtuTouched* t, int textured);
const char* rtu_kernel_slot_name(int slot);

/* Measurement helper for bench.py: bracket every launch of the kernel in `slot` with HIP events on the launch stream, from now on
 * (slot < 0: stop; what was measured stays until it is read). rtu_probe_read synchronises, returns the summed duration and the number of launches measured since the last
 * read (at most 64 are kept) and starts over. Recipe W launch sequences only. */
int  rtu_probe_kernel(RtuContext* ctx, int slot);
int  rtu_probe_read(RtuContext* ctx, float* total_ms_out, int* launches_out);

/* Measurement helper for bench.py: launch the render kernel `iters` times
 * back-to-back on `hip_stream`, bracketed by HIP events recorded on that same
 * stream, and return the AVERAGE kernel duration in milliseconds. */
int  rtu_time_render(RtuContext* ctx, const RtuFrameDesc* frame, void* d_rgbz, void* hip_stream,
                     int iters, float* avg_ms_out);

/* Self-test: the kernels replace binary32 divisions by a per-ray constant with an exact
 * binary64-reciprocal form (rtu_intersect.h); this runs n_pairs pseudo-random operand
 * pairs through both forms on the GPU and returns how many quotients differ in any bit
 * (must be 0). */
int  rtu_selftest_division(RtuContext* ctx, unsigned long long n_pairs, unsigned long long seed,
                           unsigned long long* mismatches_out);

/* Self-test of the sphere / plane intersection routines: the device path evaluates the
 * reference's expressions in a cheaper order (the bounding-box test last, and only when its
 * outcome is not already implied); this runs both orders on n_rays random and adversarial rays
 * (grazing, far away, axis-parallel, origin on the surface) and counts results that differ in
 * any bit. Expected: 0. */
int  rtu_selftest_primitives(RtuContext* ctx, unsigned long long n_rays, unsigned long long seed,
                             unsigned long long* mismatches_out);

/* Debug: the texture arithmetic of the kernels on n inputs, by the very __device__ functions the kernels call, for
 * bit-for-bit comparison with the oracle (tests/test_gpu_texcoords.py). h_in holds RTU_TEXOP_IN(op) floats per input,
 * h_out receives RTU_TEXOP_OUT(op). ATAN2F: {y, x} -> atan2f(y, x); ASINF: x -> asinf(x); SPHERE_UV: a unit normal ->
 * the sphere's uvw (objFunctions.cpp:38-41); ENV_UVW: a direction -> the uvw of SampleEnvironment (scene.h:425-431);
 * TILE_CLAMP: uvw -> Texture::TileClamp(uvw); TEXTURE: uvw -> Sample(uvw) of texture `index` of the uploaded scene;
 * MAP: uvw -> TextureMap::Sample(uvw) of material map `index` (4 * material + RTU_MAP_*), the background map (-1) or
 * the environment map (-2) of the uploaded scene. TEXTURE / MAP refuse (RTU_ERR_ARG) a scene without textures and a map
 * that is not present. The arrays are copied through the device in chunks. */
#define RTU_TEXOP_ATAN2F     0
#define RTU_TEXOP_ASINF      1
#define RTU_TEXOP_SPHERE_UV  2
#define RTU_TEXOP_ENV_UVW    3
#define RTU_TEXOP_TILE_CLAMP 4
#define RTU_TEXOP_TEXTURE    5
#define RTU_TEXOP_MAP        6
#define RTU_TEXOP_IN(op)  ((op) == RTU_TEXOP_ATAN2F ? 2 : (op) == RTU_TEXOP_ASINF ? 1 : 3)
#define RTU_TEXOP_OUT(op) ((op) <= RTU_TEXOP_ASINF ? 1 : 3)
int  rtu_debug_texcoords(RtuContext* ctx, int op, int index, const float* h_in, unsigned long long n, float* h_out);

/* ---- Irradiance map: the indirect term gathered at a refined grid of image points, interpolated per pixel (rtu_irradiance.h, -------
 * rtu_irradiance.hip) — the screen-space irradiance map of the reference's ExternalLibrary/cyIrradianceMap.h (its class
 * cyIrradianceMapColorZNormal), which the reference's renderer never reaches, restated for the GPU.
 * GRID. s = 2^-max_subdiv pixels lie between neighbouring points (max_subdiv <= 0; a positive one, several points per pixel, is
 * RTU_ERR_UNSUPPORTED); width and height must be multiples of s (RTU_ERR_ARG). The grid has (width / s + 1) x (height / s + 1) points,
 * point (x, y) — index x + grid_w * y — sits at the image position (x s, y s), a pixel CORNER, and its ray leaves the pinhole cam_pos
 * through (origin + u * (x s)) + v * (y s), normalised as rtu_camera_rays does; there is no lens. A point's record is two float4,
 * {E.r, E.g, E.b, z} {N.x, N.y, N.z, 0}, and one byte says whether it was COMPUTED (1) or ESTIMATED (0).
 *   computed   the point's ray is traced once: z = hInfo.z and N = hInfo.N, the bits of rtu_trace_rays; E = the sum, in the order of m,
 *              of the `samples` values c that rtu_gather_rays gives that ray with the keys rtu_sample_key(point index, first_sample + m),
 *              divided by (float)samples. A miss stores E = 0, z = tmax (RTU_BIGFLOAT), N = 0; a node without material E = 0.
 *   estimated  E, z and N are the average (((d0 + d1) + d2) + d3) * 0.25f of four earlier points.
 * PASSES, 1 + 2 (max_subdiv - min_subdiv) of them; a pass reads earlier passes only and visits its points in rising index:
 *   pass 0           computes every point whose x and y are multiples of 2^(max_subdiv - min_subdiv).
 *   then per level, skip = that spacing, halved from level to level, half = skip / 2:
 *   centre pass      visits (half + i skip, half + j skip); estimated from (x -+ half, y -+ half) in the order (-,-) (+,-) (-,+) (+,+)
 *   edge pass        visits (half + i skip, j skip) and (i skip, half + j skip); estimated from (x, y - half) (x - half, y)
 *                    (x + half, y) (x, y + half); a point with x == 0 or y == 0 is always computed
 *   In both, a point whose x + half or y + half lies beyond the grid is always computed (cells that a ragged grid cuts off).
 *   A point is estimated when the average is similar to each of the four: |dE| < threshold_color per channel, |dz| < threshold_z and
 *   dot(average N, N_i) > threshold_n, the average N not renormalised; otherwise it is computed. min_subdiv == max_subdiv computes
 *   every point. (The reference's iterator reads its spacing after leaving its lock, so the last point of each of its passes is
 *   visited with the next pass's spacing: a side effect of its threading that is not restated here)
 * LOOKUP at image position (px, py), the class's Sample(): xx = px * (1.0f / s), ix = (unsigned)xx, fx = xx - ix, likewise y; ix beyond
 * the last column: both columns the last; the four records are interpolated a * (1 - f) + b * f in x, then in y, every component
 * (the eight floats of a record), binary32, uncontracted. A negative or NaN coordinate is taken as 0.
 * rtu_irradiance_defaults: min_subdiv -5, max_subdiv 0, samples 64, first_sample 0, thresholds 1e30, 1e30, 1e30, 1e30, 0.7 (the class's
 * own: colour and depth never refuse), max_bounce 5. Rules (RTU_ERR_ARG): min_subdiv <= max_subdiv, min_subdiv >= -15, samples 1 ..
 * 4096, first_sample >= 0, thresholds not NaN, max_bounce 0 .. RTU_MAX_BOUNCE, reserved 0, at most 2^26 grid points. */
typedef struct RtuIrradianceDesc {   /* 64 B */
    int32_t  min_subdiv, max_subdiv;
    int32_t  samples;                /* M per computed point */
    int32_t  first_sample;
    float    threshold_color[3], threshold_z, threshold_n;
    int32_t  max_bounce;             /* of every Shade() tree of the gather, as RtuShadeDesc.max_bounce */
    uint32_t reserved[6];            /* must be 0 */
} RtuIrradianceDesc;
/* a built map, for the lookup and the frame: the image size it was built for, max_subdiv, and its records (host memory in the host
 * forms, device memory, 16-byte aligned, in the _device forms) */
typedef struct RtuIrradianceMap {    /* 32 B */
    int32_t     width, height, max_subdiv;
    uint32_t    reserved;            /* must be 0 */
    const void* records;             /* grid_w * grid_h records of two float4 */
    const void* reserved_ptr;        /* must be NULL */
} RtuIrradianceMap;
int  rtu_irradiance_defaults(RtuIrradianceDesc* out);
/* grid size and number of passes for a width x height image; any output may be NULL. Pure host code, as the next three. */
int  rtu_irradiance_grid(const RtuIrradianceDesc* desc, int width, int height, int* grid_w, int* grid_h, int* passes);
/* the rays of all grid points of `frame` (cam_pos, origin, u, v, width, height), index order, tmax = RTU_BIGFLOAT */
int  rtu_irradiance_rays(const RtuFrameDesc* frame, const RtuIrradianceDesc* desc, RtuRay* rays_out);
/* ONE PASS over given records: visit_out[k] = the index of the k-th point the pass visits, compute_out[k] = 1 if the pass wants it
 * computed, 0 if it estimated it — then its record in `records` is the average and its byte in `computed` 0; the record and byte of
 * a point to be computed are left alone (the caller computes and stores them before the next pass). *n_visit = the points visited.
 * visit_out / compute_out: room for grid_w * grid_h entries; the points with compute_out 1, in order, are the pass's list. */
int  rtu_irradiance_classify(const RtuIrradianceDesc* desc, int width, int height, int pass, float* records, uint8_t* computed, uint32_t* visit_out,
                             uint8_t* compute_out, uint32_t* n_visit);
/* the lookup at n image positions xy = {px, py} ...: eight floats per position to out */
int  rtu_irradiance_sample(const RtuIrradianceMap* map, const float* xy, size_t n, float* out);
int  rtu_irradiance_sample_device(RtuContext* ctx, const RtuIrradianceMap* map, const void* d_xy, size_t n, void* d_out, void* hip_stream);
/* BUILD the map of `frame` (its pinhole camera, width, height; eye = cam_pos; samples, lens, shards are not read — shard_count > 1 is
 * RTU_ERR_UNSUPPORTED): grid_w * grid_h records, as many bytes, *n_computed (may be NULL) the number of computed points, and per_pass
 * (may be NULL; 2 words per pass) {points visited, points computed}. Per pass: k_irr_classify writes the averages and flags the rest,
 * the flagged points become a device list in visiting order (the three scan kernels of rtu_steer.hip; no atomics), the list's length
 * is read back, and the list is computed in chunks of at most 2^22 chains — k_irr_roots, the chain and shading steps of
 * rtu_gather_rays, k_irr_store. THE CALL IS A RENDER (frame records, chain records, launch hints of rtu_shade_rays_paths; ONE STREAM
 * PER CONTEXT). Because of the read-back the _device form returns when the map is complete on hip_stream; a chunk that ran out of
 * frame records is shaded again by the call itself. The cancel flag is checked between chunks (RTU_ERR_CANCELLED).
 * RTU_ERR_NO_SCENE before rtu_upload_scene; d_records 16-byte aligned. */
int  rtu_irradiance_build_device(RtuContext* ctx, const RtuFrameDesc* frame, const RtuIrradianceDesc* desc, void* d_records, void* d_computed,
                                 uint32_t* n_computed, uint32_t* per_pass, void* hip_stream);
int  rtu_irradiance_build(RtuContext* ctx, const RtuFrameDesc* frame, const RtuIrradianceDesc* desc, float* h_records, uint8_t* h_computed,
                          uint32_t* n_computed, uint32_t* per_pass);
/* THE FRAME: a recipe-S frame of frame->samples samples (1 .. ; gather_bounces must be 0) whose root calls also get the AmbientLight
 * of the map at the pixel's centre (x + 0.5, y + 0.5). Per sample k: the rays and keys of rtu_camera_sample_rays_device(frame, k), the
 * lookup kernel, rtu_shade_rays_ambient_device of them (eye = cam_pos, frame->max_bounce), accumulated in sample order by the kernels
 * of a recipe-S frame: rgb = sum / (float)samples, z = the mean hInfo.z over the samples that hit, RTU_BIGFLOAT without one — a
 * recipe-S frame's z. A ray that misses shows the environment, as in every ray batch. map->width / height must be the frame's.
 * Sharded frames (shard_count > 1) are RTU_ERR_UNSUPPORTED; sensors and temporal sessions have no such entry. Synchronous on
 * hip_stream (a sample that ran out of frame records is shaded again). */
int  rtu_render_frame_irradiance_device(RtuContext* ctx, const RtuFrameDesc* frame, const RtuIrradianceMap* map, void* d_rgbz, void* hip_stream);
int  rtu_render_frame_irradiance(RtuContext* ctx, const RtuFrameDesc* frame, const RtuIrradianceMap* map, float* h_rgbz);

/* Debug: device allocations the library has made for its own buffers so far (every context together, the whole process).
 * rtu_device_alloc is not counted. */
unsigned long long rtu_debug_device_allocations(void);
/* Debug: bytes of device memory the library's own buffers hold now (every context and progressive session together). */
unsigned long long rtu_debug_device_bytes(void);

/* Device memory helpers so a C/C++ host needs no HIP headers. */
/* The context's own stream (a hipStream_t as void*) and device: a multi-GPU host (host/begin_render.cpp) renders every shard on
 * its context's stream and queues the collection — RCCL send / receive or an asynchronous copy into pinned host memory — behind
 * it on the same stream, so that the shards of all GPUs travel at the same time. */
void* rtu_context_stream(RtuContext* ctx);
int   rtu_context_device(const RtuContext* ctx);
int   rtu_context_sync(RtuContext* ctx);                       /* wait for the context's stream */
void* rtu_host_alloc_pinned(size_t bytes);                     /* page-locked host memory (asynchronous copies need it) */
void  rtu_host_free_pinned(void* p);
int   rtu_copy_to_host_async(RtuContext* ctx, void* h_dst, const void* d_src, size_t bytes, void* hip_stream);
void* rtu_device_alloc(RtuContext* ctx, size_t bytes);
void  rtu_device_free(RtuContext* ctx, void* d_ptr);
int   rtu_copy_to_host(RtuContext* ctx, void* h_dst, const void* d_src, size_t bytes);
int   rtu_copy_to_device(RtuContext* ctx, void* d_dst, const void* h_src, size_t bytes);   /* synchronous */

#ifdef __cplusplus
}
#endif
#endif /* RTU_RENDER_H_INCLUDED */
