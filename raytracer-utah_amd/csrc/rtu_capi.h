// rtu_capi.h — private to rtu_capi.hip and the files split off it (rtu_capi_build.hip: the host builders of an upload;
// rtu_capi_temporal.hip: the temporal accumulators and sessions; rtu_capi_sensor.hip: sensors and adaptive sensors), the host
// side of the C-ABI in include/rtu_render.h: the context, and what one of those files needs of another. Everything declared
// here has C++ linkage and hidden visibility: the library exports the rtu_* entries of include/rtu_render.h and nothing of this.
// A helper that only one file uses is not here but in that file, in an unnamed namespace or `static`.
#ifndef RTU_CAPI_H
#define RTU_CAPI_H
#include "rtu_camrays.h"
#include "rtu_devbuf.h"
#include "rtu_device.h"
#include "rtu_lightlist.h"
#include "rtu_ref_build.h"
#include "rtu_sensor.h"
#include "rtu_temporal.h"

#include <array>
#include <map>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

struct RtuProgressive;  // defined in rtu_capi.hip
struct RtuTemporal;     // defined in rtu_capi_temporal.hip

struct RtuContext {
    int         device = 0;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;        // side mode (rtu_device.h KernelArgs::fcnt0): stage 2 of the primary phase runs here, beside the levels
    hipEvent_t  aux_ev0 = nullptr, aux_ev1 = nullptr;
    hipEvent_t  ev0 = nullptr, ev1 = nullptr;
    std::string error;

    // scene
    bool     has_scene = false;
    uint32_t n_textures = 0;              // of the uploaded scene, and a host copy of its material maps: rtu_debug_texcoords
    std::vector<RtuTexMap> mat_maps_host; //   checks a texture / map before the kernel reads it
    std::vector<DevBuf<char>> scene_allocs;  // meshes and textures: live until the next upload
    std::vector<DevBuf<char>> place;      // what depends on node transformations, lights and materials, by slot (place_scene): an
                                          //   update rewrites these in place, growing one only when it is too small
    // the shape of the uploaded scene (rtu_update_scene refuses any other) and what an update builds from
    std::vector<RtuNode> shape_nodes;
    std::vector<RtuMesh> shape_meshes;       // headers only: the arrays stay NULL
    std::vector<RtuTexture> shape_textures;  // likewise
    uint32_t shape_materials = 0;
    bool     shape_maps = false;
    std::vector<std::vector<uint32_t>> fast_elements;  // per mesh: slot of the fast tree's leaf order -> face
    std::vector<DevMesh> dmeshes;            // host copy of the device mesh records (their f / v arrays)
    std::vector<const uint32_t*> slot_of;    // per mesh, device: face -> slot of the fast tree
    std::vector<DevLightMask> lmask_host;    // host copy of DevScene::lmask (rtu_debug_context_light_list)
    LlBuilder* llb = nullptr;                // the device builder of the occluder lists (rtu_scene_update.hip)
    // what rtu_update_meshes needs of a mesh beyond its device record: the node ranges of the levels of its collapsed fast trees
    // (root first, [levels + 1]) and which of scene_allocs holds its ref.bvh (the one per-mesh buffer whose size an update can change)
    struct MeshRefit { std::vector<uint32_t> lvl4, lvl8; size_t ref_bvh_alloc = 0, v_alloc = 0, vn_alloc = 0; };
    std::vector<MeshRefit> refit;
    // rtu_keep_previous_vertices: a mesh's positions and normals as they were before the last rtu_update_meshes — the buffers that
    // update swapped out of scene_allocs (valid), else "previous" is "current". df_*: the table the deform accumulator's kernels read
    // (TpDeformScene, rtu_temporal.h), rebuilt after an upload, an update or a change of the switch (df_dirty).
    bool keep_prev = false;
    struct PrevGen { DevBuf<char> v, vn; bool valid = false; };
    std::vector<PrevGen> prev_gen;
    DevBuf<TpDeformMesh> df_meshes;
    DevBuf<int32_t>      df_nodes;
    bool                 df_dirty = true;
    bool  mu_timing = false;                 // rtu_debug_mesh_update_timing: HIP events around the phases of rtu_update_meshes
    float mu_ms[4] = {};                     // copies, records, refit, placement: summed since the last read
    hipEvent_t mu_ev[5] = {};
    // rtu_update_meshes_device: the device builder of the `ref` tree (rtu_ref_build.hip; created on first use), the event that orders
    // its reads after the caller's stream, per mesh whether fn == f as uploaded (-1: not asked yet), and the phase times
    RefBuilder* rb = nullptr;
    hipEvent_t  mud_wait = nullptr;
    std::vector<int> fn_is_f;
    float mud_ms[4] = {};                    // build, copies, records and refit, placement: summed since the last read
    hipEvent_t mud_ev[5] = {};
    DevScene dscene{};
    uint32_t bvh_stack_needed = 1;

    // per-frame resources (grown on demand, reused)
    std::vector<DevBuf<char>> level_allocs;  // the storage of lv, lv_side and the defer lists
    LevelBuffers lv[RTU_MAX_LEVELS] = {};
    uint32_t level_nsl = 0;
    uint32_t want_cap_s[RTU_MAX_LEVELS] = {};  // per-shard capacity wanted for levels >= 1 (grown from the counts of an overflowed frame)
    uint32_t want_defer_s = 0;
    DevBuf<FrameCounters> fcnt;
    uint32_t* defer_list = nullptr;
    uint32_t  defer_cap_s = 0;
    DevBuf<FrameCounters> fcnt_side;         // side mode: counters of the primary phase's defer list and of the side level arrays
    int sequences_in_flight = 1;             // rtu_set_sequences_in_flight: launch sequences the caller keeps in flight on this GPU (all its contexts together)
    uint32_t* defer_list0 = nullptr;         // the primary phase's own defer list
    uint32_t  defer_cap0_s = 0;
    LevelBuffers lv_side[RTU_MAX_LEVELS] = {};
    std::map<uint64_t, bool> side_off;       // launch shapes whose stage 2 made more frames than the side arrays take: no side mode for them
    std::map<uint64_t, uint32_t> occ_hints;   // ... and how many 8x8 tiles had anything in them (k_tile_occ): the grid of k_primary
    std::map<uint64_t, uint64_t> side_frames; // ... and how many level-0 frames stage 2 of the primary phase made in the last launch of a shape
    bool     last_side = false;
    bool     mesh_hits_childless = false;    // no mesh node's material reflects or refracts: a mesh hit's Shade() call is settled by the lane that found it
    bool     any_recursive_material = true;
    bool     textured = false;
    bool     scene_stochastic = false;   // soft shadows / glossy bounces / depth of field: recipe S only
    std::string stochastic_what;
    DevBuf<float4>   acc;                // recipe S accumulators: rgb sum + z sum, hit count
    DevBuf<uint32_t> acc_hits;
    DevBuf<float4>   sample_buf;         // the images of one batch of samples, [sample][pixel]
    DevBuf<float4>   ad_sq;              // adaptive sampling (rtu_render_frame_adaptive): sums of squares and sample counts per pixel
    DevBuf<uint8_t>  ad_counts;
    DevBuf<uint4>    ad_list[2];         // ... the active-tile lists {tile, 0, lane mask}, double-buffered, and their lengths
    DevBuf<uint32_t> ad_n;               // [2] on the device
    PinnedBuf<uint32_t> ad_n_host;       // pinned: the length of the list the next batch walks
    DevBuf<float4>   gi_h;               // recipe P: chain records [5 depths][4][chains], results [2][chains]
    DevBuf<float4>   gi_res;
    bool      want_gi = false;           // level buffers carry famb
    // k_tail: the recursion level from which the previous frame of this scene was almost empty (a hint —
    // any value renders the same image); last_tail_from: what the most recent frame was launched with
    int      tail_hint = 0, last_tail_from = RTU_MAX_LEVELS;   // tail_hint: set by rtu_debug_tail_from for the next launch (0: none)
    std::map<uint64_t, int> tail_hints;   // per launch shape (tiles of the launch, feature set): learned cut level
    std::map<uint64_t, std::array<uint32_t, 8>> list_hints;  // ... and the rays deferred in every phase, + 1 (KernelArgs::list_n)
    uint64_t last_tail_key = 0;
    bool     last_stats = false;
    uint32_t n_meshes = 0;
    uint32_t nsl = 0;
    int32_t  shadow_light[RTU_MAX_SHADOW_LIGHTS] = {};
    float    nol_light[RTU_FI_NOL_LIGHTS][4] = {};
    DevBuf<float4> fb;
    DevBuf<unsigned long long> counters;     // 11 x u64 (RtuStats), or the touched-bytes table [RTU_TL_KERNELS][RTU_TOUCH_STRIDE]
    uint32_t slot_launches[RTU_TL_KERNELS] = {};  // touched-bytes mode: launches per slot that went into the table (rtu_get_touched_launches)
    // probe: HIP events around the launches of one timeline slot (rtu_probe_kernel)
    static const int kProbePairs = 64;
    int probe_slot = -1, probe_used = 0;
    hipEvent_t probe_ev[2 * kProbePairs] = {};
    struct MeshInfo { uint32_t faces, sah_depth, stack4, nodes4, nodes8; };
    std::vector<MeshInfo> mesh_info;
    struct LightListInfo { uint32_t light, cover, G, entries, longest; };  // the occluder lists built at upload (rtu_light_list_info)
    std::vector<LightListInfo> light_list_info;
    // cameras of a batch of frames: written into the next slot of a ring of pinned host slots, copied to d_cams on the launch
    // stream ahead of the kernels (stream order protects d_cams; an event per slot protects the slot from being rewritten
    // while its copy is still pending)
    static const int kCamSlots = 16;
    DevBuf<BatchCam> d_cams;
    PinnedBuf<BatchCam> h_cams;
    hipEvent_t cam_ev[kCamSlots] = {};
    int cam_slot = 0;
    uint32_t dbg = 0;
    const volatile int* cancel = nullptr;    // rtu_set_cancel_flag: polled between the launch sequences of a sampled frame
    uint64_t scene_gen = 0;                  // bumped by every upload and update: a progressive session of an older scene is stale
    std::vector<RtuProgressive*> sessions;   // the open progressive sessions (rtu_destroy_context frees their device memory)
    std::vector<RtuTemporal*> temporals;     // ... and the open temporal sessions (rtu_temporal_begin), likewise
    DevBuf<uint32_t> cover;                  // coverage masks of primary rays (KernelArgs::cover), grown on demand
    uint32_t  cover_faces = 0;
    DevBuf<uint32_t> occ;                    // tile occupancy of primary rays (KernelArgs::occ), grown on demand
    int4* node_rects = nullptr;              // [RTU_MAX_FRAME_BATCH][n_nodes] screen rectangles of the node-level bounds (k_node_rects); owned by the scene
    DevBuf<float4>  q_rays, q_hits;          // ray queries, host forms (rtu_trace_rays / rtu_occluded_rays): one chunk of rays and of answers
    DevBuf<uint8_t> q_occ;
    DevBuf<float4>  ft_albedo;               // first-hit features, host forms (rtu_ray_features / rtu_frame_features): one chunk of albedo (rays and hits: q_rays, q_hits)
    DevBuf<float4>  ft_surface;              // ... and of surface records (rtu_ray_surface / rtu_frame_surface), two float4 each: grown by those two only
    DevBuf<float4>  dn_planes;               // the denoising filter (rtu_denoise_device): its four planes gN, gP, e0, e1 of one frame
    DevBuf<float4>  sh_rays, sh_out;         // ray batches, host form (rtu_shade_rays): one chunk of rays and of {r, g, b, t}
    DevBuf<uint32_t> sh_keys;                // ... and of keys (rtu_shade_rays_sampled)
    float sort_box[6] = {};                  // ray sorting (rtu_raysort.h): the box the keys are quantised in, kept by place_scene
    DevBuf<uint32_t> so_scratch;             // ... keys and indices double-buffered, digit histograms (rtu_ray_order_device)
    DevBuf<float4>   so_rays;                // ... the host form's rays and order (rtu_ray_order)
    DevBuf<uint32_t> so_order;
    DevBuf<float4>   sn_rays, sn_out;        // sensors (rtu_render_sensor): the rays of one batch of samples, their {r, g, b, t} [sample][pixel],
    DevBuf<uint32_t> sn_keys, sn_hits;       // ... their keys; the hit counts and
    DevBuf<float4>   sn_acc, sn_img;         // ... the sums per pixel (none of the frame path's acc / acc_hits); the host form's image
    bool  sn_timing = false;                 // rtu_debug_sensor_timing: HIP events around the two kernels of rtu_sensor.hip and the whole render
    float sn_ms[3] = {};                     // k_sensor_rays, k_sensor_accumulate, the render: summed since the last read
    hipEvent_t sn_ev[6] = {};
    DevBuf<float4>   sa_s, sa_q, sa_img;     // adaptive sensors (rtu_render_sensor_adaptive): per pixel the sums and the sums of squares with the hit count; the host form's image
    DevBuf<uint32_t> sa_list[2], sa_packed;  // ... the live-pixel lists, double-buffered, the survivors packed per block,
    DevBuf<uint32_t> sa_blk, sa_n;           // ... their number per block and its scan, the length of the next list
    PinnedBuf<uint32_t> sa_n_host;           // ... and where the host reads it (pinned)
    DevBuf<uint8_t>  sa_counts;              // ... the host form's counts
    std::vector<uint32_t> sa_trace;          // {live pixels, samples} of every batch of the last adaptive sensor render (rtu_debug_sensor_adaptive_trace)
    DevBuf<uint32_t> st_scratch;            // steered sampling (rtu_sample_allocation_device): the weights, the tile sums, Wsum
    DevBuf<float4>   sh_amb;                 // the two halves of a recipe-P sample, host form (rtu_shade_rays_ambient): one chunk of AmbientLight intensities
    DevBuf<uint32_t> ir_scratch, ir_list;    // irradiance map (rtu_irradiance_build): the scratch of a pass (scan, counts, offsets, the list's length), its list,
    DevBuf<uint32_t> ir_keys, ir_hits;       // ... the key slots of a chunk's chain steps / the keys of a frame's sample; the frame's hit counts,
    DevBuf<float4>   ir_c, ir_rays;          // ... {c, t} per chain of a chunk / {r, g, b, t} of a frame's sample; its rays,
    DevBuf<float4>   ir_amb, ir_acc;         // ... the frame's AmbientLight per pixel and its sums,
    DevBuf<float4>   ir_rec, ir_img;         // ... the host forms' records and image,
    DevBuf<uint8_t>  ir_bytes;               // ... and computed bytes
    DevBuf<unsigned long long> tl;           // timeline stamps, RTU_TL_KERNELS x RTU_TL_STRIDE (rtu_render_timeline)
    bool stamp_next = false;
};

int fail(RtuContext* ctx, int code, const char* fmt, ...);  // rtu_capi.hip: sets the context's error string, returns `code`

#define RTU_HIP(ctx, call)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return fail(ctx, RTU_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// ---- constants and records that cross files ----
// placement buffers by slot
enum { P_NODES, P_MATERIALS, P_LIGHTS, P_MATMAPS, P_LMASK, P_COVER, P_LIST = P_COVER + RTU_MAX_COVER,
       P_SLOTS = P_LIST + 2 * RTU_LMASK_LIGHTS * RTU_MAX_COVER };

struct SahTree {
    std::vector<RtuBvhNode> nodes;
    std::vector<uint32_t>   elements;
    uint32_t depth = 0;
};

// The constants of the part of the cull margin that grows with the distance of a ray's origin, and of a sphere's slack along the
// ray (derived at cull_margin and sphere_slack, rtu_intersect.h): per node the condition numbers along its chain, root first.
struct WorldFar {
    float wnoise, wreach, sph_k, sph_r;
    float near_m0, near_c1;           // the margin of rays that start at hit points: c1 max(m0, pm) (rtu_intersect.h, THE NEAR MARGIN)
    float wlist;                      // the scale the occluder lists are built with: wscale itself, or more in a wide scene
};

struct CoverMesh {
    std::vector<float4> boxes;      // per face: world-space box {lo} {hi}, rounded outwards
    std::vector<double> verts;      // per face: 3 world-space vertices (9 doubles)
    std::vector<uint32_t> slot_of;  // face -> slot in the leaf order of the mesh's fast tree
};

struct HostLightList {
    DevLightMask m;                 // frame, offsets, scale, G, point (the device pointers stay null here)
    std::vector<uint32_t> off, ent;
};

// ---- internal functions that cross files, by the file that defines them (each is described there) ----
// rtu_capi.hip
int ensure_place(RtuContext* ctx, int slot, size_t bytes, void** out);
int check_adaptive_desc(RtuContext* ctx, const RtuAdaptiveDesc* ad, int samples);  // frame path
// ... its ray batches
int shade_args(RtuContext* ctx, const void* rays, const void* out, size_t n, const RtuShadeDesc* d, bool device, RtuFrameDesc* f, bool sampled = false,
               const void* keys = nullptr, bool paths = false);
int paths_chain(RtuContext* ctx, const RtuFrameDesc& f, float4* d_out, hipStream_t stream, const float4* d_rays, const uint32_t* d_keys, uint32_t n);
int shade_until_fits(RtuContext* ctx, const RtuFrameDesc& f, float4* d_out, hipStream_t stream, const float4* d_rays, const uint32_t* d_keys, uint32_t n,
                     bool paths, const char* counters_refusal, int (*behind)(void*) = nullptr, void* behind_arg = nullptr);
CamSample cam_sample(const RtuFrameDesc* frame, int sample);
void h_portable_sincos(float t, float& sn, float& cs);

// rtu_capi_sensor.hip
int check_sensor(RtuContext* ctx, const RtuSensorDesc* d);
int sensor_generate(RtuContext* ctx, const RtuSensorDesc* d, int k0, int n, float4* d_rays, uint32_t* d_keys, hipStream_t stream);

// rtu_capi_temporal.hip
void temporal_release(RtuTemporal* t);

// this header: the short helpers of rtu_capi.hip's frame path (check_frame, halton, cancel_raised), queries (misaligned) and ray
// batches (HostSinCos) that its neighbours use too, with their bodies, so that the frame path sees them as it did. check_frame is
// `static`: an internal function is emitted behind its first caller, which keeps rtu_capi.o's code for the rtu_render_frame*
// entries byte for byte what it was when check_frame sat in that file's unnamed namespace (NOTEBOOK 22); the temporal file has a copy.
static inline int check_frame(RtuContext* ctx, const RtuFrameDesc* f) {
    if (!f) return fail(ctx, RTU_ERR_ARG, "frame is NULL");
    if (f->width <= 0 || f->height <= 0 || f->width > 65536 || f->height > 65536) return fail(ctx, RTU_ERR_ARG, "bad resolution");
    if (f->shard_count < 1 || f->shard_rank < 0 || f->shard_rank >= f->shard_count) return fail(ctx, RTU_ERR_ARG, "bad shard");
    if (f->max_bounce < 0 || f->max_bounce > RTU_MAX_BOUNCE) return fail(ctx, RTU_ERR_ARG, "max_bounce out of range");
    if (f->samples < 0 || f->samples > 65536) return fail(ctx, RTU_ERR_ARG, "samples out of range");
    if (f->gather_bounces != 0 && (f->gather_bounces != RTU_GI_BOUNCES || f->samples < 1))
        return fail(ctx, RTU_ERR_ARG, "gather_bounces is 0 or %d (recipe P, with samples >= 1)", RTU_GI_BOUNCES);
    if (f->collect_stats < 0 || f->collect_stats > 2) return fail(ctx, RTU_ERR_ARG, "collect_stats is 0, 1 or 2");
    if (f->samples == 0 && ctx->has_scene && (ctx->scene_stochastic || f->dof != 0))
        return fail(ctx, RTU_ERR_STOCHASTIC, "the scene has %s: render it with frame.samples >= 1 (recipe S)",
                    ctx->scene_stochastic ? ctx->stochastic_what.c_str() : "depth of field");
    return RTU_OK;
}
// Halton (scene.h:130-139)
inline float halton(int index, int base) {
    float r = 0;
    float f = 1.0f / (float)base;
    for (int i = index; i > 0; i /= base) {
        r += f * (float)(i % base);
        f /= (float)base;
    }
    return r;
}
inline bool cancel_raised(const RtuContext* ctx) { return ctx->cancel && __atomic_load_n(ctx->cancel, __ATOMIC_RELAXED) != 0; }
inline bool misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }
struct HostSinCos {
    void operator()(float t, float& sn, float& cs) const { h_portable_sincos(t, sn, cs); }
};

// rtu_capi_build.hip
void build_sah(const RtuMesh& m, SahTree& out);
void dfs_order(SahTree& t, std::vector<uint32_t>& first, std::vector<uint32_t>& total);
void build_wide8(const SahTree& t, const std::vector<uint32_t>& first, const std::vector<uint32_t>& total, std::vector<float4>& out);
void build_wide4(const SahTree& t, std::vector<float4>& out, uint32_t& stack_need);
void build_tri_records(const RtuMesh& m, const uint32_t* elements, uint32_t n, std::vector<float4>& tri);
void renumber_bfs(const RtuMesh& m, std::vector<RtuBvhNode>& bfs, uint32_t& any_empty);
void world_far(const RtuSceneDesc* s, double wscale, WorldFar& out);
float world_bounds(const RtuSceneDesc* s, std::vector<DevNode>& nodes);
void sort_box_of(const std::vector<DevNode>& nodes, float wscale, float out[6]);
bool compute_light_list(const RtuLight& l, const CoverMesh& cm, float wscale, HostLightList& out);
// (rtu_capi.hip has an unrelated node_chain(s, i, Affine64&, Affine64&) in its unnamed namespace, beside scene_motion. Inside that
// namespace the local one hides this one; place_scene calls this one from ahead of it. Whoever moves scene_motion: rename one.)
LlChain node_chain(const RtuSceneDesc* s, uint32_t node);
void make_cover_mesh(const RtuSceneDesc* s, uint32_t node, const std::vector<uint32_t>& fast_elements, CoverMesh& cm);
int build_light_lists(RtuContext* ctx, const RtuSceneDesc* s, const std::vector<CoverMesh>& cover, float wscale, DevScene& ds);
int build_light_lists_device(RtuContext* ctx, const RtuSceneDesc* s, const std::vector<LlCover>& covers, const std::vector<double>& lohi, float wscale,
                             DevScene& ds);

template <class T>
int place_upload(RtuContext* ctx, int slot, const T* src, size_t count, const T** dst) {
    void* d = nullptr;
    int rc = ensure_place(ctx, slot, sizeof(T) * count, &d);
    *dst = static_cast<const T*>(d);
    if (rc != RTU_OK) return rc;
    if (count) RTU_HIP(ctx, hipMemcpy(d, src, sizeof(T) * count, hipMemcpyHostToDevice));
    return RTU_OK;
}

#pragma GCC visibility pop

#endif
