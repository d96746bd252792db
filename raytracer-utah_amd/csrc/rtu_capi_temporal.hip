// rtu_capi_temporal.hip — the temporal part of the host side of the C-ABI in include/rtu_render.h, split off rtu_capi.hip: the
// accumulators on device memory (rtu_temporal.h) with the variance, steering, gradient, sparse and hole entries around them, the
// host forms of their ray generators, and the sessions (RtuTemporal, rtu_temporal_begin* .. rtu_temporal_free) with their camera
// and sensor frames. What it uses of rtu_capi.hip and rtu_capi_sensor.hip is declared in rtu_capi.h; of itself it offers them
// temporal_release (rtu_destroy_context). Compiled like rtu_capi.hip with -ffp-contract=off: the host forms of the rays round
// as the kernels do.
#include "rtu_camrays.h"
#include "rtu_capi.h"
#include "rtu_denoise.h"
#include "rtu_features.h"
#include "rtu_gradient.h"
#include "rtu_holes.h"
#include "rtu_query.h"
#include "rtu_sensor.h"
#include "rtu_sparse.h"
#include "rtu_steer.h"
#include "rtu_temporal.h"
#include "rtu_variance.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

// A temporal session (rtu_temporal_*): one new sample per frame, accumulated over a moving camera. It owns every buffer a frame
// writes; the frame-record arrays it shades through are the context's scratch within one call.
struct RtuTemporal {
    RtuContext*     ctx = nullptr;    // nullptr once the context is destroyed
    RtuTemporalDesc desc{};
    size_t          pixels = 0;
    uint64_t        scene_gen = 0;    // the context's scene generation at the last frame: another one starts the history over
    int             k = 0;            // frames since begin / reset
    bool            has_hist = false; // hist[cur] and prev_cam are those of the previous frame
    int             cur = 0;
    RtuFrameDesc    prev_cam{};
    bool            prev_is_sensor = false;  // the previous frame was a sensor frame (rtu_temporal_sensor_frame): prev_sensor, not prev_cam, is its
    RtuSensorDesc   prev_sensor{};           // ... and a camera frame that follows takes no history, as a sensor frame after a camera frame
    DevBuf<float4>   rays, img, hits, albedo, hist[2];
    DevBuf<uint32_t> keys;
    DevBuf<RtuNodeMotion>    motion;      // rtu_temporal_frame_moved: the table of the frame, grown at the first frame that needs it ...
    PinnedBuf<RtuNodeMotion> motion_host; // ... and the staging memory it is copied through
    bool             variance = false;    // rtu_temporal_begin_variance: hist[] have four planes, a frame ends with k_variance and the filter
    RtuVarianceDesc  vdesc{};
    DevBuf<float>    var;                 // ... the variance of the frame
    DevBuf<float4>   surface;             // rtu_temporal_frame_deformed: the frame's surface records (two float4 per pixel), grown by the first such frame
    bool             steered = false;     // rtu_temporal_begin_steered: a frame goes on with the allocation, the extra rays and the fold
    RtuSteerDesc     sdesc{};
    size_t           st_cap = 0;          // ... rays of a frame at most: min(budget, pixels * max_extra)
    uint32_t         st_total = 0;        // ... of the last frame
    DevBuf<uint32_t> st_counts, st_offsets, st_total_dev, st_keys, st_owner;
    DevBuf<float4>   st_rays, st_img;
    PinnedBuf<uint32_t> st_total_host;
    bool             gradient = false;    // rtu_temporal_begin_gradient with enabled != 0: a frame with a previous frame shades the gradient rays
    RtuGradientDesc  gdesc{};             // ... behind its own (rays, keys and img hold pixels + strata) and caps the history by their lambda
    size_t           strata = 0;
    bool             has_lambda = false;  // ... gr_lambda is that of the last frame
    int              lcur = 0;            // ... lum[lcur] is the luminance plane of the last frame's sample
    DevBuf<float>    lum[2], gr_lambda;
    DevBuf<uint32_t> gr_owner;
    DevBuf<float4>   gr_diff;
    bool             sparse_session = false;  // rtu_temporal_begin_sparse
    bool             sparse = false;      // ... with block > 1: a frame shades one ray per block (the first `blocks` entries of rays, keys and img) ...
    RtuSparseDesc    spdesc{};            // ... and goes through the sparse accumulator and the fill
    size_t           blocks = 0;
    DevBuf<uint32_t> sp_owner;
    DevBuf<uint8_t>  sp_hole;
    PinnedBuf<uint8_t> sp_hole_host;      // rtu_temporal_holes counts here
    hipEvent_t       sp_done = nullptr;   // ... recorded behind the last frame's fill: the copy waits for it on the context's stream
    bool             sparse_holes = false;    // rtu_temporal_begin_sparse_holes
    RtuHoleDesc      hdesc{};             // ... with block > 1 and budget > 0 (hl_cap > 0): a frame shades its holes behind the owners' rays
    size_t           hl_cap = 0;          // ... rays of a frame at most: pixels - blocks
    uint32_t         hl_total = 0;        // ... of the last frame
    DevBuf<uint32_t> hl_counts, hl_offsets, hl_owner, hl_total_dev;
    PinnedBuf<uint32_t> hl_total_host;
};

void temporal_release(RtuTemporal* t) {
    t->rays.reset();
    t->img.reset();
    t->hits.reset();
    t->albedo.reset();
    for (DevBuf<float4>& h : t->hist) h.reset();
    t->keys.reset();
    t->motion.reset();
    t->motion_host.reset();
    t->var.reset();
    t->surface.reset();
    t->st_counts.reset();
    t->st_offsets.reset();
    t->st_total_dev.reset();
    t->st_keys.reset();
    t->st_owner.reset();
    t->st_rays.reset();
    t->st_img.reset();
    t->st_total_host.reset();
    t->st_total = 0;
    for (DevBuf<float>& l : t->lum) l.reset();
    t->gr_lambda.reset();
    t->gr_owner.reset();
    t->gr_diff.reset();
    t->sp_owner.reset();
    t->sp_hole.reset();
    t->sp_hole_host.reset();
    if (t->sp_done) (void)hipEventDestroy(t->sp_done);
    t->sp_done = nullptr;
    t->hl_counts.reset();
    t->hl_offsets.reset();
    t->hl_owner.reset();
    t->hl_total_dev.reset();
    t->hl_total_host.reset();
    t->hl_total = 0;
    t->has_lambda = false;
    t->has_hist = false;
    t->ctx = nullptr;
}
extern "C" {

// ---- temporal accumulation (rtu_temporal.h, rtu_temporal.hip): the accumulator on device memory, and the session that drives it ----
static_assert(sizeof(RtuTemporalDesc) == 32, "RtuTemporalDesc is 32 bytes");

static const char* const kTemporalDescRules =
    "temporal: width, height 1 .. 65536 (2^26 pixels), max_history 1 .. 65535, sigma_plane > 0, normal_min -1 .. 1, known flags, reserved words 0";

// The checks the three rtu_temporal_accumulate*_device entries share, in their order of precedence: `planes` 3 or 4 float4 per pixel
// of a history; has_motion: the entry takes a table and a history_cap. prev_cam: NULL becomes cur_cam. RTU_OK: the device is set.
static int temporal_device_args(RtuContext* ctx, int planes, bool has_motion, const RtuTemporalDesc* desc, const RtuFrameDesc*& prev_cam,
                                const RtuFrameDesc* cur_cam, const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev,
                                const void* d_hist_out, const void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_temporal_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kTemporalDescRules);
    if (has_motion && rtu_temporal_check_motion(nullptr, n_nodes, history_cap) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "temporal: history_cap is 0 .. 65535");
    if (!cur_cam || (d_hist_prev && !prev_cam)) return fail(ctx, RTU_ERR_ARG, "temporal: a camera is NULL");
    if (!prev_cam) prev_cam = cur_cam;
    if (cur_cam->width != desc->width || cur_cam->height != desc->height || prev_cam->width != desc->width || prev_cam->height != desc->height)
        return fail(ctx, RTU_ERR_ARG, "temporal: the cameras must have the desc's width and height");
    if (!d_rgbz || !d_hits || !d_albedo || !d_hist_out || !d_rgbz_out || (has_motion && !d_motion)) return fail(ctx, RTU_ERR_ARG, "temporal: a device pointer is NULL");
    if (misaligned(d_rgbz) || misaligned(d_hits) || misaligned(d_albedo) || misaligned(d_hist_prev) || misaligned(d_hist_out) || misaligned(d_rgbz_out) ||
        misaligned(d_motion))
        return fail(ctx, RTU_ERR_ARG, "temporal: device buffers must be 16-byte aligned");
    if (d_hist_prev) {
        const uintptr_t a = (uintptr_t)d_hist_prev, b = (uintptr_t)d_hist_out, bytes = (uintptr_t)(16 * planes) * (uintptr_t)desc->width * (uintptr_t)desc->height;
        if (a < b + bytes && b < a + bytes) return fail(ctx, RTU_ERR_ARG, "temporal: hist_out overlaps hist_prev");
    }
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    return RTU_OK;
}

int rtu_temporal_accumulate_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                   const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                   void* d_rgbz_out, void* hip_stream) {
    const int rc = temporal_device_args(ctx, 3, false, desc, prev_cam, cur_cam, d_rgbz, d_hits, d_albedo, d_hist_prev, d_hist_out, d_rgbz_out, nullptr, 0, 0);
    if (rc != RTU_OK) return rc;
    const hipError_t e = (hipError_t)rtu_launch_temporal(tp_setup(*desc, *prev_cam, *cur_cam, d_hist_prev != nullptr), (const float4*)d_rgbz, (const float4*)d_hits,
                                                         (const float4*)d_albedo, (const float4*)d_hist_prev, (float4*)d_hist_out, (float4*)d_rgbz_out,
                                                         (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "temporal launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

static RtuTemporal* temporal_begin(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuVarianceDesc* vdesc, int* err_out) {
    auto refuse = [&](int rc) -> RtuTemporal* {
        if (err_out) *err_out = rc;
        return nullptr;
    };
    if (!ctx) return refuse(RTU_ERR_ARG);
    if (rtu_temporal_check_desc(desc) != RTU_OK)
        return refuse(fail(ctx, RTU_ERR_ARG, "%s", kTemporalDescRules));
    if (vdesc && (desc->flags & RTU_TEMPORAL_DENOISE))
        return refuse(fail(ctx, RTU_ERR_ARG, "temporal: a variance session has its own filter (RTU_TEMPORAL_DENOISE must not be set)"));
    if (hipSetDevice(ctx->device) != hipSuccess) return refuse(fail(ctx, RTU_ERR_HIP, "hipSetDevice failed"));
    std::unique_ptr<RtuTemporal> t(new RtuTemporal);
    t->desc = *desc;
    if (vdesc) {
        t->variance = true;
        t->vdesc = *vdesc;
    }
    t->pixels = (size_t)desc->width * (size_t)desc->height;
    t->scene_gen = ctx->scene_gen;
    const size_t n = t->pixels;
    hipError_t e = t->rays.grow(2 * n);
    if (e == hipSuccess) e = t->keys.grow(n);
    if (e == hipSuccess) e = t->img.grow(n);
    if (e == hipSuccess) e = t->hits.grow(3 * n);
    if (e == hipSuccess) e = t->albedo.grow(n);
    for (DevBuf<float4>& h : t->hist)
        if (e == hipSuccess) e = h.grow((vdesc ? 4 : 3) * n);
    if (e == hipSuccess && vdesc) e = t->var.grow(n);
    if (e == hipSuccess && (vdesc || (desc->flags & RTU_TEMPORAL_DENOISE))) e = ctx->dn_planes.grow(4 * n);  // the filter's planes are the context's
    if (e != hipSuccess) return refuse(fail(ctx, RTU_ERR_HIP, "session buffers: %s", hipGetErrorString(e)));
    t->ctx = ctx;
    ctx->temporals.push_back(t.get());
    if (err_out) *err_out = RTU_OK;
    return t.release();
}

RtuTemporal* rtu_temporal_begin(RtuContext* ctx, const RtuTemporalDesc* desc, int* err_out) { return temporal_begin(ctx, desc, nullptr, err_out); }

static const char* const kVarianceDescRules =
    "variance: width, height 1 .. 65536 (2^26 pixels), n_passes 1 .. 8, normal_log2_power 0 .. 7, sigmas > 0, min_history 1 .. 65535, reserved words 0";

RtuTemporal* rtu_temporal_begin_variance(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuVarianceDesc* vdesc, int* err_out) {
    auto refuse = [&](int rc) -> RtuTemporal* {
        if (err_out) *err_out = rc;
        return nullptr;
    };
    if (!ctx) return refuse(RTU_ERR_ARG);
    if (!vdesc || !desc) return refuse(fail(ctx, RTU_ERR_ARG, "temporal: a descriptor is NULL"));
    RtuVarianceDesc vd = *vdesc;  // (its size is the session's)
    vd.width = desc->width;
    vd.height = desc->height;
    if (rtu_temporal_check_desc(desc) == RTU_OK && rtu_variance_check_desc(&vd) != RTU_OK) return refuse(fail(ctx, RTU_ERR_ARG, "%s", kVarianceDescRules));
    return temporal_begin(ctx, desc, &vd, err_out);
}

static_assert(sizeof(RtuNodeMotion) == 96, "RtuNodeMotion is 96 bytes");
static_assert(sizeof(RtuVarianceDesc) == 40, "RtuVarianceDesc is 40 bytes");

int rtu_temporal_accumulate_moments_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                           const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                           void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap, void* hip_stream) {
    const int rc = temporal_device_args(ctx, 4, true, desc, prev_cam, cur_cam, d_rgbz, d_hits, d_albedo, d_hist_prev, d_hist_out, d_rgbz_out, d_motion, n_nodes,
                                        history_cap);
    if (rc != RTU_OK) return rc;
    const hipError_t e = (hipError_t)rtu_launch_temporal_moments(tp_motion_setup(*desc, *prev_cam, *cur_cam, d_hist_prev != nullptr, n_nodes, history_cap),
                                                                 (const float4*)d_rgbz, (const float4*)d_hits, (const float4*)d_albedo, (const float4*)d_hist_prev,
                                                                 (float4*)d_hist_out, (float4*)d_rgbz_out, d_motion, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "temporal launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_variance_device(RtuContext* ctx, const RtuVarianceDesc* desc, const void* d_hist, const void* d_hits, void* d_v, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_variance_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kVarianceDescRules);
    if (!d_hist || !d_hits || !d_v) return fail(ctx, RTU_ERR_ARG, "variance: a device pointer is NULL");
    if (misaligned(d_hist) || misaligned(d_hits) || ((uintptr_t)d_v & 3u))
        return fail(ctx, RTU_ERR_ARG, "variance: device buffers must be 16-byte aligned (d_v: 4-byte)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_variance(vr_setup(*desc), (const float4*)d_hist, (const float4*)d_hits, (float*)d_v, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "variance launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_denoise_variance_device(RtuContext* ctx, const RtuVarianceDesc* desc, const void* d_in, const void* d_hits, const void* d_albedo, const void* d_v,
                                void* d_out, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_variance_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kVarianceDescRules);
    if (!d_in || !d_hits || !d_albedo || !d_v || !d_out) return fail(ctx, RTU_ERR_ARG, "variance: a device pointer is NULL");
    if (misaligned(d_in) || misaligned(d_hits) || misaligned(d_albedo) || misaligned(d_out) || ((uintptr_t)d_v & 3u))
        return fail(ctx, RTU_ERR_ARG, "variance: device buffers must be 16-byte aligned (d_v: 4-byte)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->dn_planes.grow(4 * (size_t)desc->width * (size_t)desc->height));
    const hipError_t e = (hipError_t)rtu_launch_denoise_variance(*desc, (const float4*)d_in, (const float4*)d_hits, (const float4*)d_albedo, (const float*)d_v,
                                                                 (float4*)d_out, ctx->dn_planes.get(), (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "variance filter launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_temporal_accumulate_motion_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                          const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                          void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap, void* hip_stream) {
    const int rc = temporal_device_args(ctx, 3, true, desc, prev_cam, cur_cam, d_rgbz, d_hits, d_albedo, d_hist_prev, d_hist_out, d_rgbz_out, d_motion, n_nodes,
                                        history_cap);
    if (rc != RTU_OK) return rc;
    const hipError_t e = (hipError_t)rtu_launch_temporal_motion(tp_motion_setup(*desc, *prev_cam, *cur_cam, d_hist_prev != nullptr, n_nodes, history_cap),
                                                                (const float4*)d_rgbz, (const float4*)d_hits, (const float4*)d_albedo, (const float4*)d_hist_prev,
                                                                (float4*)d_hist_out, (float4*)d_rgbz_out, d_motion, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "temporal launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

// The deform forms on the device: the motion / moments form with the surface records, the context's own connectivity and the previous
// vertices it kept. RTU_OK: *D is the table the kernels read (rebuilt here after an upload, an update or a change of the switch).
static int deform_scene(RtuContext* ctx, uint32_t n_nodes, const void* d_surface, TpDeformScene* D) {
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (!ctx->keep_prev) return fail(ctx, RTU_ERR_ARG, "deform: rtu_keep_previous_vertices is off");
    if (!d_surface || misaligned(d_surface)) return fail(ctx, RTU_ERR_ARG, "deform: the surface records are NULL or not 16-byte aligned");
    if ((size_t)n_nodes != ctx->shape_nodes.size()) return fail(ctx, RTU_ERR_ARG, "deform: n_nodes is not the uploaded scene's node count");
    const size_t nm = ctx->dmeshes.size();
    if (ctx->df_dirty) {
        std::vector<TpDeformMesh> meshes(nm);
        for (size_t i = 0; i < nm; i++) {
            const DevMesh& d = ctx->dmeshes[i];
            const bool prev = i < ctx->prev_gen.size() && ctx->prev_gen[i].valid;
            meshes[i] = TpDeformMesh{d.f, d.fn, prev ? reinterpret_cast<const float*>(ctx->prev_gen[i].v.get()) : d.v,
                                     prev ? reinterpret_cast<const float*>(ctx->prev_gen[i].vn.get()) : d.vn, ctx->shape_meshes[i].nf, 0};
        }
        std::vector<int32_t> node_mesh(n_nodes);
        for (uint32_t i = 0; i < n_nodes; i++) node_mesh[i] = ctx->shape_nodes[i].mesh_id;
        RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
        RTU_HIP(ctx, ctx->df_meshes.grow(nm ? nm : 1));
        RTU_HIP(ctx, ctx->df_nodes.grow(n_nodes ? n_nodes : 1));
        if (nm) RTU_HIP(ctx, hipMemcpy(ctx->df_meshes.get(), meshes.data(), sizeof(TpDeformMesh) * nm, hipMemcpyHostToDevice));
        if (n_nodes) RTU_HIP(ctx, hipMemcpy(ctx->df_nodes.get(), node_mesh.data(), sizeof(int32_t) * n_nodes, hipMemcpyHostToDevice));
        ctx->df_dirty = false;
    }
    *D = TpDeformScene{ctx->df_meshes.get(), ctx->df_nodes.get(), (uint32_t)nm, 0};
    return RTU_OK;
}

static int temporal_deform_device(RtuContext* ctx, bool moments, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                  const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_surface, const void* d_hist_prev,
                                  void* d_hist_out, void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap, void* hip_stream) {
    int rc = temporal_device_args(ctx, moments ? 4 : 3, true, desc, prev_cam, cur_cam, d_rgbz, d_hits, d_albedo, d_hist_prev, d_hist_out, d_rgbz_out, d_motion,
                                  n_nodes, history_cap);
    if (rc != RTU_OK) return rc;
    TpDeformScene D;
    if ((rc = deform_scene(ctx, n_nodes, d_surface, &D)) != RTU_OK) return rc;
    const hipError_t e = (hipError_t)rtu_launch_temporal_deform(tp_motion_setup(*desc, *prev_cam, *cur_cam, d_hist_prev != nullptr, n_nodes, history_cap), moments,
                                                                D, (const float4*)d_rgbz, (const float4*)d_hits, (const float4*)d_albedo,
                                                                (const float4*)d_surface, (const float4*)d_hist_prev, (float4*)d_hist_out, (float4*)d_rgbz_out,
                                                                d_motion, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "temporal launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_temporal_accumulate_deform_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                          const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_surface, const void* d_hist_prev,
                                          void* d_hist_out, void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap,
                                          void* hip_stream) {
    return temporal_deform_device(ctx, false, desc, prev_cam, cur_cam, d_rgbz, d_hits, d_albedo, d_surface, d_hist_prev, d_hist_out, d_rgbz_out, d_motion, n_nodes,
                                  history_cap, hip_stream);
}

int rtu_temporal_accumulate_deform_moments_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                                  const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_surface,
                                                  const void* d_hist_prev, void* d_hist_out, void* d_rgbz_out, const RtuNodeMotion* d_motion,
                                                  uint32_t n_nodes, int32_t history_cap, void* hip_stream) {
    return temporal_deform_device(ctx, true, desc, prev_cam, cur_cam, d_rgbz, d_hits, d_albedo, d_surface, d_hist_prev, d_hist_out, d_rgbz_out, d_motion, n_nodes,
                                  history_cap, hip_stream);
}

int rtu_motion_vectors_deform_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const void* d_hits, const void* d_surface,
                                     const RtuNodeMotion* d_motion, uint32_t n_nodes, void* d_mv, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_temporal_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kTemporalDescRules);
    if (!prev_cam || prev_cam->width != desc->width || prev_cam->height != desc->height)
        return fail(ctx, RTU_ERR_ARG, "motion vectors: the previous camera must have the desc's width and height");
    if (!d_hits || !d_motion || !d_mv) return fail(ctx, RTU_ERR_ARG, "motion vectors: a device pointer is NULL");
    if (misaligned(d_hits) || misaligned(d_motion) || misaligned(d_mv)) return fail(ctx, RTU_ERR_ARG, "motion vectors: device buffers must be 16-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    TpDeformScene D;
    const int rc = deform_scene(ctx, n_nodes, d_surface, &D);
    if (rc != RTU_OK) return rc;
    const hipError_t e = (hipError_t)rtu_launch_motion_vectors_deform(tp_setup(*desc, *prev_cam, *prev_cam, true), n_nodes, D, (const float4*)d_hits,
                                                                      (const float4*)d_surface, d_motion, (float4*)d_mv, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "motion vector launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_motion_vectors_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const void* d_hits, const RtuNodeMotion* d_motion,
                              uint32_t n_nodes, void* d_mv, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_temporal_check_desc(desc) != RTU_OK)
        return fail(ctx, RTU_ERR_ARG, "%s", kTemporalDescRules);
    if (!prev_cam || prev_cam->width != desc->width || prev_cam->height != desc->height)
        return fail(ctx, RTU_ERR_ARG, "motion vectors: the previous camera must have the desc's width and height");
    if (!d_hits || !d_motion || !d_mv) return fail(ctx, RTU_ERR_ARG, "motion vectors: a device pointer is NULL");
    if (misaligned(d_hits) || misaligned(d_motion) || misaligned(d_mv)) return fail(ctx, RTU_ERR_ARG, "motion vectors: device buffers must be 16-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_motion_vectors(tp_setup(*desc, *prev_cam, *prev_cam, true), n_nodes, (const float4*)d_hits, d_motion, (float4*)d_mv,
                                                               (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "motion vector launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

// ---- steered sampling (rtu_steer.h, rtu_steer.hip): the allocation, the extra rays and the fold on device memory ----
static_assert(sizeof(RtuSteerDesc) == 32, "RtuSteerDesc is 32 bytes");

static const char* const kSteerDescRules =
    "steer: width, height 1 .. 65536 (2^26 pixels), budget 0 .. 2^26, max_extra 1 .. 15, reserved words 0";
static bool misaligned4(const void* p) { return ((uintptr_t)p & 3u) != 0; }

// What st_extra_ray takes of `frame` for the extra samples of frame `d.frame_index`: the camera, and the pixel offsets of the samples
// S + (k mod S) * E + j of the frame with S * (1 + E) samples, by launch()'s expressions (cam_sample). false: the frame is refused.
static bool steer_rays_setup(const RtuSteerDesc& d, const RtuFrameDesc* frame, StRays* r) {
    if (!frame || frame->width != d.width || frame->height != d.height || frame->samples < 1) return false;
    const long long S = frame->samples, E = d.max_extra;
    if (S * (1 + E) > 65536) return false;
    RtuFrameDesc f = *frame;
    f.samples = (int32_t)(S * (1 + E));
    const uint32_t sample0 = (uint32_t)(S + (long long)(d.frame_index % (uint32_t)S) * E);
    memset(r, 0, sizeof *r);
    r->c = cam_sample(&f, (int)sample0);
    for (int j = 0; j < d.max_extra; j++) {
        const CamSample cj = cam_sample(&f, (int)sample0 + j);
        r->ox[j] = cj.ox;
        r->oy[j] = cj.oy;
    }
    r->sample0 = sample0;
    return true;
}

int rtu_extra_sample_rays(const RtuSteerDesc* desc, const RtuFrameDesc* frame, const uint32_t* counts, const uint32_t* offsets, size_t capacity,
                          RtuRay* rays_out, uint32_t* keys_out, uint32_t* owner_out) {
    StRays r;
    if (rtu_steer_check_desc(desc) != RTU_OK || !steer_rays_setup(*desc, frame, &r) || !counts || !offsets || capacity > ((size_t)1 << 26))
        return RTU_ERR_ARG;
    if (capacity && (!rays_out || !keys_out || !owner_out)) return RTU_ERR_ARG;
    const size_t n = (size_t)desc->width * (size_t)desc->height;
    for (size_t p = 0; p < n; p++)
        if (counts[p] > (uint32_t)desc->max_extra || (unsigned long long)offsets[p] + counts[p] > capacity) return RTU_ERR_ARG;
    for (size_t p = 0; p < n; p++) {
        const int y = (int)(p / (size_t)desc->width), x = (int)(p - (size_t)y * (size_t)desc->width);
        for (uint32_t j = 0; j < counts[p]; j++) {
            f3 org, dir;
            uint32_t key;
            st_extra_ray(r.c, r.ox[j], r.oy[j], r.sample0 + j, x, y, HostSinCos(), org, dir, key);
            const size_t i = (size_t)offsets[p] + j;
            RtuRay& ray = rays_out[i];
            ray.org[0] = org.x; ray.org[1] = org.y; ray.org[2] = org.z;
            ray.tmax = RTU_BIGFLOAT;
            ray.dir[0] = dir.x; ray.dir[1] = dir.y; ray.dir[2] = dir.z;
            ray.reserved = 0;
            keys_out[i] = key;
            owner_out[i] = (uint32_t)p;
        }
    }
    return RTU_OK;
}

int rtu_sample_allocation_device(RtuContext* ctx, const RtuSteerDesc* desc, const void* d_hist, const void* d_hits, const void* d_v, void* d_counts,
                                 void* d_offsets, void* d_total, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_steer_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kSteerDescRules);
    if (!d_hist || !d_hits || !d_v || !d_counts || !d_offsets || !d_total) return fail(ctx, RTU_ERR_ARG, "steer: a device pointer is NULL");
    if (misaligned(d_hist) || misaligned(d_hits) || misaligned4(d_v) || misaligned4(d_counts) || misaligned4(d_offsets) || misaligned4(d_total))
        return fail(ctx, RTU_ERR_ARG, "steer: device buffers must be 16-byte aligned (d_v, d_counts, d_offsets, d_total: 4-byte)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->st_scratch.grow(rtu_steer_scratch_words((size_t)desc->width * (size_t)desc->height)));
    const hipError_t e = (hipError_t)rtu_launch_sample_allocation(*desc, (const float4*)d_hist, (const float4*)d_hits, (const float*)d_v, (uint32_t*)d_counts,
                                                                  (uint32_t*)d_offsets, (uint32_t*)d_total, ctx->st_scratch.get(), (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "allocation launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_extra_sample_rays_device(RtuContext* ctx, const RtuSteerDesc* desc, const RtuFrameDesc* frame, const void* d_counts, const void* d_offsets,
                                 size_t capacity, void* d_rays, void* d_keys, void* d_owner, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_steer_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kSteerDescRules);
    StRays r;
    if (!steer_rays_setup(*desc, frame, &r))
        return fail(ctx, RTU_ERR_ARG, "steer: the frame must have the desc's size, samples >= 1 and samples * (1 + max_extra) <= 65536");
    if (capacity > ((size_t)1 << 26)) return fail(ctx, RTU_ERR_ARG, "steer: more than 2^26 rays");
    if (!d_counts || !d_offsets || (capacity && (!d_rays || !d_keys || !d_owner))) return fail(ctx, RTU_ERR_ARG, "steer: a device pointer is NULL");
    if (misaligned(d_rays) || misaligned4(d_keys) || misaligned4(d_owner) || misaligned4(d_counts) || misaligned4(d_offsets))
        return fail(ctx, RTU_ERR_ARG, "steer: the ray buffer must be 16-byte, the other buffers 4-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_extra_sample_rays(r, (uint32_t)desc->max_extra, (const uint32_t*)d_counts, (const uint32_t*)d_offsets,
                                                                  (float4*)d_rays, (uint32_t*)d_keys, (uint32_t*)d_owner, (uint32_t)capacity, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "extra ray launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_temporal_refine_device(RtuContext* ctx, const RtuTemporalDesc* desc, void* d_hist, const void* d_hits, const void* d_albedo, const void* d_counts,
                               const void* d_offsets, const void* d_rgbt, size_t n_rays, void* d_rgbz, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_temporal_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kTemporalDescRules);
    if (n_rays > ((size_t)1 << 26)) return fail(ctx, RTU_ERR_ARG, "refine: more than 2^26 samples");
    if (!d_hist || !d_hits || !d_albedo || !d_counts || !d_offsets || !d_rgbz || (n_rays && !d_rgbt)) return fail(ctx, RTU_ERR_ARG, "refine: a device pointer is NULL");
    if (misaligned(d_hist) || misaligned(d_hits) || misaligned(d_albedo) || misaligned(d_rgbt) || misaligned(d_rgbz) || misaligned4(d_counts) ||
        misaligned4(d_offsets))
        return fail(ctx, RTU_ERR_ARG, "refine: device buffers must be 16-byte aligned (d_counts, d_offsets: 4-byte)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_temporal_refine((size_t)desc->width * (size_t)desc->height, (float)desc->max_history, (float4*)d_hist,
                                                                (const float4*)d_hits, (const float4*)d_albedo, (const uint32_t*)d_counts,
                                                                (const uint32_t*)d_offsets, (const float4*)d_rgbt, (uint32_t)n_rays, (float4*)d_rgbz,
                                                                (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "refine launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

RtuTemporal* rtu_temporal_begin_steered(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuVarianceDesc* vdesc, const RtuSteerDesc* sdesc, int* err_out) {
    auto refuse = [&](int rc) -> RtuTemporal* {
        if (err_out) *err_out = rc;
        return nullptr;
    };
    if (!ctx) return refuse(RTU_ERR_ARG);
    if (!sdesc || !desc || !vdesc) return refuse(fail(ctx, RTU_ERR_ARG, "temporal: a descriptor is NULL"));
    RtuSteerDesc sd = *sdesc;  // (its size is the session's, its frame_index the frame's)
    sd.width = desc->width;
    sd.height = desc->height;
    sd.frame_index = 0;
    if (rtu_temporal_check_desc(desc) == RTU_OK && rtu_steer_check_desc(&sd) != RTU_OK) return refuse(fail(ctx, RTU_ERR_ARG, "%s", kSteerDescRules));
    RtuTemporal* t = rtu_temporal_begin_variance(ctx, desc, vdesc, err_out);
    if (!t) return nullptr;
    t->steered = true;
    t->sdesc = sd;
    const size_t n = t->pixels, most = n * (size_t)sd.max_extra;
    t->st_cap = sd.budget < most ? sd.budget : most;
    hipError_t e = t->st_counts.grow(n);
    if (e == hipSuccess) e = hipMemset(t->st_counts.get(), 0, n * sizeof(uint32_t));  // (before the first frame: zeros)
    if (e == hipSuccess && t->st_cap) {
        e = t->st_offsets.grow(n);
        if (e == hipSuccess) e = t->st_total_dev.grow(1);
        if (e == hipSuccess) e = t->st_total_host.grow(1);
        if (e == hipSuccess) e = t->st_rays.grow(2 * t->st_cap);
        if (e == hipSuccess) e = t->st_keys.grow(t->st_cap);
        if (e == hipSuccess) e = t->st_owner.grow(t->st_cap);
        if (e == hipSuccess) e = t->st_img.grow(t->st_cap);
        if (e == hipSuccess) e = ctx->st_scratch.grow(rtu_steer_scratch_words(n));
    }
    if (e != hipSuccess) {
        const int rc = fail(ctx, RTU_ERR_HIP, "session buffers: %s", hipGetErrorString(e));
        rtu_temporal_free(t);
        return refuse(rc);
    }
    return t;
}

// a steered session's frame after the accumulator and the first rtu_variance_device: the extra rays of the frame, folded into the new
// history and d_rgbz, and the variance of the folded history
static int temporal_steer(RtuTemporal* t, const RtuFrameDesc* frame, uint32_t k, void* d_rgbz, void* hip_stream) {
    RtuContext* ctx = t->ctx;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool paths = frame->gather_bounces != 0;
    RtuSteerDesc sd = t->sdesc;
    sd.frame_index = k;
    float4* hist = t->hist[t->cur].get();
    int rc = rtu_sample_allocation_device(ctx, &sd, hist, t->hits.get(), t->var.get(), t->st_counts.get(), t->st_offsets.get(), t->st_total_dev.get(), hip_stream);
    if (rc != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpyAsync(t->st_total_host.get(), t->st_total_dev.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    RTU_HIP(ctx, hipStreamSynchronize(stream));
    const uint32_t total = *t->st_total_host.get();
    if ((size_t)total > t->st_cap) return fail(ctx, RTU_ERR_HIP, "steer: %u rays allocated, the session holds %zu", total, t->st_cap);
    t->st_total = total;
    if (total == 0) return RTU_OK;
    if ((rc = rtu_extra_sample_rays_device(ctx, &sd, frame, t->st_counts.get(), t->st_offsets.get(), total, t->st_rays.get(), t->st_keys.get(),
                                           t->st_owner.get(), hip_stream)) != RTU_OK)
        return rc;
    RtuShadeDesc shd;
    rtu_shade_defaults(&shd);
    memcpy(shd.eye, frame->cam_pos, sizeof shd.eye);
    shd.max_bounce = frame->max_bounce;
    RtuFrameDesc f;
    if ((rc = shade_args(ctx, t->st_rays.get(), t->st_img.get(), total, &shd, true, &f, true, t->st_keys.get(), paths)) != RTU_OK) return rc;
    if (paths && (rc = paths_chain(ctx, f, t->st_img.get(), stream, t->st_rays.get(), t->st_keys.get(), total)) != RTU_OK) return rc;
    if ((rc = shade_until_fits(ctx, f, t->st_img.get(), stream, t->st_rays.get(), t->st_keys.get(), total, paths, nullptr)) != RTU_OK) return rc;
    if ((rc = rtu_temporal_refine_device(ctx, &t->desc, hist, t->hits.get(), t->albedo.get(), t->st_counts.get(), t->st_offsets.get(), t->st_img.get(),
                                         total, d_rgbz, hip_stream)) != RTU_OK)
        return rc;
    return rtu_variance_device(ctx, &t->vdesc, hist, t->hits.get(), t->var.get(), hip_stream);
}

int rtu_temporal_extra_counts_device(RtuTemporal* t, void* d_counts, void* hip_stream) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = t->ctx;
    if (!t->steered) return fail(ctx, RTU_ERR_ARG, "not a steered session");
    if (!d_counts) return fail(ctx, RTU_ERR_ARG, "d_counts is NULL");
    if (misaligned4(d_counts)) return fail(ctx, RTU_ERR_ARG, "d_counts must be 4-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    if (t->has_hist)
        RTU_HIP(ctx, hipMemcpyAsync(d_counts, t->st_counts.get(), t->pixels * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
    else
        RTU_HIP(ctx, hipMemsetAsync(d_counts, 0, t->pixels * sizeof(uint32_t), (hipStream_t)hip_stream));
    return RTU_OK;
}

int rtu_temporal_steer_total(RtuTemporal* t, uint32_t* total_out) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    if (!t->steered) return fail(t->ctx, RTU_ERR_ARG, "not a steered session");
    if (!total_out) return fail(t->ctx, RTU_ERR_ARG, "total_out is NULL");
    *total_out = t->st_total;
    return RTU_OK;
}

// ---- temporal gradients (rtu_gradient.h, rtu_gradient.hip): the gradient rays, the luminance plane, lambda and the capped accumulator ----
static_assert(sizeof(RtuGradientDesc) == 32, "RtuGradientDesc is 32 bytes");

static const char* const kGradientDescRules =
    "gradient: width, height 1 .. 65536 (2^26 pixels), radius 0 .. 3, kappa >= 0 and finite, enabled 0 or 1, reserved words 0";

static bool gradient_rays_args(const RtuGradientDesc* desc, const RtuFrameDesc* frame, int sample) {
    return rtu_gradient_check_desc(desc) == RTU_OK && frame && frame->width == desc->width && frame->height == desc->height && frame->samples >= 1 &&
           sample >= 0 && sample < frame->samples;
}

int rtu_gradient_rays(const RtuGradientDesc* desc, const RtuFrameDesc* frame, int sample, RtuRay* rays_out, uint32_t* keys_out, uint32_t* owner_out) {
    if (!gradient_rays_args(desc, frame, sample) || !rays_out || !keys_out || !owner_out) return RTU_ERR_ARG;
    const CamSample c = cam_sample(frame, sample);
    const int32_t sw = gr_strata(desc->width), sh = gr_strata(desc->height);
    for (uint32_t s = 0; s < (uint32_t)sw * (uint32_t)sh; s++) {
        int x, y;
        gr_owner(desc->width, desc->height, sw, s, desc->frame_index, x, y);
        f3 org, dir;
        uint32_t key;
        camera_sample_ray(c, x, y, HostSinCos(), org, dir, key);
        RtuRay& r = rays_out[s];
        r.org[0] = org.x; r.org[1] = org.y; r.org[2] = org.z;
        r.tmax = RTU_BIGFLOAT;
        r.dir[0] = dir.x; r.dir[1] = dir.y; r.dir[2] = dir.z;
        r.reserved = 0;
        keys_out[s] = key;
        owner_out[s] = (uint32_t)x + (uint32_t)desc->width * (uint32_t)y;
    }
    return RTU_OK;
}

int rtu_gradient_rays_device(RtuContext* ctx, const RtuGradientDesc* desc, const RtuFrameDesc* frame, int sample, void* d_rays, void* d_keys, void* d_owner,
                             void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_gradient_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kGradientDescRules);
    if (!gradient_rays_args(desc, frame, sample)) return fail(ctx, RTU_ERR_ARG, "gradient: the frame must have the desc's size and 0 <= sample < samples");
    if (!d_rays || !d_keys || !d_owner) return fail(ctx, RTU_ERR_ARG, "gradient: a device pointer is NULL");
    if (misaligned(d_rays) || misaligned4(d_keys) || misaligned4(d_owner))
        return fail(ctx, RTU_ERR_ARG, "gradient: the ray buffer must be 16-byte, the other buffers 4-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_gradient_rays(cam_sample(frame, sample), desc->frame_index, (float4*)d_rays, (uint32_t*)d_keys,
                                                              (uint32_t*)d_owner, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "gradient ray launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_sample_luminance_device(RtuContext* ctx, const RtuGradientDesc* desc, const void* d_rgbz, const void* d_hits, const void* d_albedo, void* d_lum,
                                void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_gradient_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kGradientDescRules);
    if (!d_rgbz || !d_hits || !d_albedo || !d_lum) return fail(ctx, RTU_ERR_ARG, "gradient: a device pointer is NULL");
    if (misaligned(d_rgbz) || misaligned(d_hits) || misaligned(d_albedo) || misaligned4(d_lum))
        return fail(ctx, RTU_ERR_ARG, "gradient: device buffers must be 16-byte aligned (d_lum: 4-byte)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_sample_luminance((size_t)desc->width * (size_t)desc->height, (const float4*)d_rgbz, (const float4*)d_hits,
                                                                 (const float4*)d_albedo, (float*)d_lum, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "luminance launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_temporal_gradient_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuGradientDesc* gdesc, const RtuFrameDesc* prev_cam,
                                 const RtuFrameDesc* cur_cam, const void* d_hits, const void* d_albedo, const RtuNodeMotion* d_motion, uint32_t n_nodes,
                                 const void* d_hist_prev, const void* d_lum_prev, const void* d_owner, const void* d_rgbt, void* d_diff_out,
                                 void* d_lambda_out, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_temporal_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kTemporalDescRules);
    if (rtu_gradient_check_desc(gdesc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kGradientDescRules);
    if (gdesc->width != desc->width || gdesc->height != desc->height) return fail(ctx, RTU_ERR_ARG, "gradient: the two descs must have one size");
    if (!cur_cam || (d_hist_prev && !prev_cam)) return fail(ctx, RTU_ERR_ARG, "gradient: a camera is NULL");
    if (!prev_cam) prev_cam = cur_cam;
    if (cur_cam->width != desc->width || cur_cam->height != desc->height || prev_cam->width != desc->width || prev_cam->height != desc->height)
        return fail(ctx, RTU_ERR_ARG, "gradient: the cameras must have the desc's width and height");
    if (!d_hits || !d_albedo || !d_motion || !d_owner || !d_rgbt || !d_diff_out || !d_lambda_out || (d_hist_prev && !d_lum_prev))
        return fail(ctx, RTU_ERR_ARG, "gradient: a device pointer is NULL");
    if (misaligned(d_hits) || misaligned(d_albedo) || misaligned(d_motion) || misaligned(d_hist_prev) || misaligned(d_rgbt) || misaligned(d_diff_out) ||
        misaligned4(d_lum_prev) || misaligned4(d_owner) || misaligned4(d_lambda_out))
        return fail(ctx, RTU_ERR_ARG, "gradient: device buffers must be 16-byte aligned (luminance, owners, lambda: 4-byte)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    GrParams G{};
    G.M = tp_motion_setup(*desc, *prev_cam, *cur_cam, d_hist_prev != nullptr, n_nodes, 0);
    G.sw = gr_strata(desc->width);
    G.sh = gr_strata(desc->height);
    G.radius = gdesc->radius;
    G.kappa = gdesc->kappa;
    const hipError_t e = (hipError_t)rtu_launch_temporal_gradient(G, (const float4*)d_hits, (const float4*)d_albedo, d_motion, (const float4*)d_hist_prev,
                                                                  (const float*)d_lum_prev, (const uint32_t*)d_owner, (const float4*)d_rgbt,
                                                                  (float4*)d_diff_out, (float*)d_lambda_out, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "gradient launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_temporal_accumulate_gradient_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                            const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                            void* d_rgbz_out, const RtuNodeMotion* d_motion, uint32_t n_nodes, int32_t history_cap, const void* d_lambda,
                                            void* hip_stream) {
    const int rc = temporal_device_args(ctx, 4, true, desc, prev_cam, cur_cam, d_rgbz, d_hits, d_albedo, d_hist_prev, d_hist_out, d_rgbz_out, d_motion, n_nodes,
                                        history_cap);
    if (rc != RTU_OK) return rc;
    if (misaligned4(d_lambda)) return fail(ctx, RTU_ERR_ARG, "temporal: lambda must be 4-byte aligned");
    const TpGradientParams g{tp_motion_setup(*desc, *prev_cam, *cur_cam, d_hist_prev != nullptr, n_nodes, history_cap), (const float*)d_lambda,
                             gr_strata(desc->width)};
    const hipError_t e = (hipError_t)rtu_launch_temporal_capped(g, (const float4*)d_rgbz, (const float4*)d_hits, (const float4*)d_albedo,
                                                                (const float4*)d_hist_prev, (float4*)d_hist_out, (float4*)d_rgbz_out, d_motion,
                                                                (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "temporal launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

RtuTemporal* rtu_temporal_begin_gradient(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuVarianceDesc* vdesc, const RtuSteerDesc* sdesc,
                                         const RtuGradientDesc* gdesc, int* err_out) {
    auto refuse = [&](int rc) -> RtuTemporal* {
        if (err_out) *err_out = rc;
        return nullptr;
    };
    if (!ctx) return refuse(RTU_ERR_ARG);
    if (!gdesc || !desc || !vdesc) return refuse(fail(ctx, RTU_ERR_ARG, "temporal: a descriptor is NULL"));
    RtuGradientDesc gd = *gdesc;  // (its size is the session's, its frame_index the frame's)
    gd.width = desc->width;
    gd.height = desc->height;
    gd.frame_index = 0;
    if (rtu_temporal_check_desc(desc) == RTU_OK && rtu_gradient_check_desc(&gd) != RTU_OK) return refuse(fail(ctx, RTU_ERR_ARG, "%s", kGradientDescRules));
    RtuTemporal* t = sdesc ? rtu_temporal_begin_steered(ctx, desc, vdesc, sdesc, err_out) : rtu_temporal_begin_variance(ctx, desc, vdesc, err_out);
    if (!t || !gd.enabled) return t;
    t->gradient = true;
    t->gdesc = gd;
    t->strata = (size_t)gr_strata(gd.width) * (size_t)gr_strata(gd.height);
    const size_t n = t->pixels, m = t->strata;
    hipError_t e = t->rays.grow(2 * (n + m));
    if (e == hipSuccess) e = t->keys.grow(n + m);
    if (e == hipSuccess) e = t->img.grow(n + m);
    for (DevBuf<float>& l : t->lum)
        if (e == hipSuccess) e = l.grow(n);
    if (e == hipSuccess) e = t->gr_lambda.grow(m);
    if (e == hipSuccess) e = t->gr_owner.grow(m);
    if (e == hipSuccess) e = t->gr_diff.grow(m);
    if (e != hipSuccess) {
        const int rc = fail(ctx, RTU_ERR_HIP, "session buffers: %s", hipGetErrorString(e));
        rtu_temporal_free(t);
        return refuse(rc);
    }
    return t;
}

int rtu_temporal_lambda_device(RtuTemporal* t, void* d_lambda, void* hip_stream) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = t->ctx;
    if (!d_lambda) return fail(ctx, RTU_ERR_ARG, "d_lambda is NULL");
    if (misaligned4(d_lambda)) return fail(ctx, RTU_ERR_ARG, "d_lambda must be 4-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const bool live = t->gradient && t->has_lambda && t->has_hist;
    const hipError_t e = (hipError_t)rtu_launch_lambda_image(t->desc.width, t->desc.height, live ? t->gr_lambda.get() : nullptr, (float*)d_lambda,
                                                             (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "lambda launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

// ---- sparse sessions (rtu_sparse.h, rtu_sparse.hip): the owners' rays, the sparse accumulator and the fill ----
static_assert(sizeof(RtuSparseDesc) == 32, "RtuSparseDesc is 32 bytes");

static const char* const kSparseDescRules = "sparse: width, height 1 .. 65536 (2^26 pixels), block 1 .. 4, reserved words 0";

// What sp_ray takes of `frame` for frame d.frame_index: the camera and, per class of blocks, the sample (k div m) mod S with its pixel
// offsets by launch()'s expressions (cam_sample). false: the frame is refused.
static bool sparse_rays_setup(const RtuSparseDesc& d, const RtuFrameDesc* frame, SpRays* r) {
    if (!frame || frame->width != d.width || frame->height != d.height || frame->samples < 1) return false;
    memset(r, 0, sizeof *r);
    r->c = cam_sample(frame, 0);
    uint32_t m[4];
    sp_class_sizes(d.width, d.height, d.block, m);
    for (int c = 0; c < 4; c++) {
        const CamSample cs = cam_sample(frame, (int)((d.frame_index / m[c]) % (uint32_t)frame->samples));
        r->ox[c] = cs.ox;
        r->oy[c] = cs.oy;
        r->sample[c] = cs.sample;
    }
    r->block = d.block;
    r->sw = sp_blocks(d.width, d.block);
    r->blocks = (uint32_t)r->sw * (uint32_t)sp_blocks(d.height, d.block);
    r->frame_index = d.frame_index;
    return true;
}

int rtu_sparse_rays(const RtuSparseDesc* desc, const RtuFrameDesc* frame, RtuRay* rays_out, uint32_t* keys_out, uint32_t* owner_out) {
    SpRays R;
    if (rtu_sparse_check_desc(desc) != RTU_OK || !sparse_rays_setup(*desc, frame, &R) || !rays_out || !keys_out || !owner_out) return RTU_ERR_ARG;
    for (uint32_t b = 0; b < R.blocks; b++) {
        f3 org, dir;
        uint32_t key, own;
        sp_ray(R, b, HostSinCos(), org, dir, key, own);
        RtuRay& r = rays_out[b];
        r.org[0] = org.x; r.org[1] = org.y; r.org[2] = org.z;
        r.tmax = RTU_BIGFLOAT;
        r.dir[0] = dir.x; r.dir[1] = dir.y; r.dir[2] = dir.z;
        r.reserved = 0;
        keys_out[b] = key;
        owner_out[b] = own;
    }
    return RTU_OK;
}

int rtu_sparse_rays_device(RtuContext* ctx, const RtuSparseDesc* desc, const RtuFrameDesc* frame, void* d_rays, void* d_keys, void* d_owner, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_sparse_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kSparseDescRules);
    SpRays R;
    if (!sparse_rays_setup(*desc, frame, &R)) return fail(ctx, RTU_ERR_ARG, "sparse: the frame must have the desc's size and samples >= 1");
    if (!d_rays || !d_keys || !d_owner) return fail(ctx, RTU_ERR_ARG, "sparse: a device pointer is NULL");
    if (misaligned(d_rays) || misaligned4(d_keys) || misaligned4(d_owner))
        return fail(ctx, RTU_ERR_ARG, "sparse: the ray buffer must be 16-byte, the other buffers 4-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_sparse_rays(R, (float4*)d_rays, (uint32_t*)d_keys, (uint32_t*)d_owner, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "sparse ray launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_temporal_accumulate_sparse_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuSparseDesc* sparse_desc, const RtuFrameDesc* prev_cam,
                                          const RtuFrameDesc* cur_cam, const void* d_rgbt, const void* d_owner, const void* d_hits, const void* d_albedo,
                                          const void* d_hist_prev, void* d_hist_out, void* d_rgbz_out, void* d_hole_out, const RtuNodeMotion* d_motion,
                                          uint32_t n_nodes, int32_t history_cap, void* hip_stream) {
    // (d_rgbt stands where the other forms have their image of samples: NULL and misaligned are refused alike)
    const int rc = temporal_device_args(ctx, 4, true, desc, prev_cam, cur_cam, d_rgbt, d_hits, d_albedo, d_hist_prev, d_hist_out, d_rgbz_out, d_motion, n_nodes,
                                        history_cap);
    if (rc != RTU_OK) return rc;
    if (rtu_sparse_check_desc(sparse_desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kSparseDescRules);
    if (sparse_desc->width != desc->width || sparse_desc->height != desc->height) return fail(ctx, RTU_ERR_ARG, "sparse: the two descs must have one size");
    if (!d_owner || !d_hole_out) return fail(ctx, RTU_ERR_ARG, "sparse: a device pointer is NULL");
    if (misaligned4(d_owner)) return fail(ctx, RTU_ERR_ARG, "sparse: the owners must be 4-byte aligned");
    const TpSparseParams s{tp_motion_setup(*desc, *prev_cam, *cur_cam, d_hist_prev != nullptr, n_nodes, history_cap), (const float4*)d_rgbt,
                           (const uint32_t*)d_owner, (uint8_t*)d_hole_out, sparse_desc->block, sp_blocks(desc->width, sparse_desc->block)};
    const hipError_t e = (hipError_t)rtu_launch_temporal_sparse(s, (const float4*)d_hits, (const float4*)d_albedo, (const float4*)d_hist_prev, (float4*)d_hist_out,
                                                                (float4*)d_rgbz_out, d_motion, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "temporal launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_sparse_fill_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuSparseDesc* sparse_desc, const void* d_hits, const void* d_albedo,
                           const void* d_owner, const void* d_rgbt, const void* d_hole, void* d_rgbz, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_temporal_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kTemporalDescRules);
    if (rtu_sparse_check_desc(sparse_desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kSparseDescRules);
    if (sparse_desc->width != desc->width || sparse_desc->height != desc->height) return fail(ctx, RTU_ERR_ARG, "sparse: the two descs must have one size");
    if (!d_hits || !d_albedo || !d_owner || !d_rgbt || !d_hole || !d_rgbz) return fail(ctx, RTU_ERR_ARG, "sparse: a device pointer is NULL");
    if (misaligned(d_hits) || misaligned(d_albedo) || misaligned(d_rgbt) || misaligned(d_rgbz) || misaligned4(d_owner))
        return fail(ctx, RTU_ERR_ARG, "sparse: device buffers must be 16-byte aligned (owners: 4-byte)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const int B = sparse_desc->block;
    const SpFill F{desc->width, desc->height, B, sp_blocks(desc->width, B), sp_blocks(desc->height, B), desc->sigma_plane, desc->normal_min};
    const hipError_t e = (hipError_t)rtu_launch_sparse_fill(F, (const float4*)d_hits, (const float4*)d_albedo, (const uint32_t*)d_owner, (const float4*)d_rgbt,
                                                            (const uint8_t*)d_hole, (float4*)d_rgbz, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "sparse fill launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

RtuTemporal* rtu_temporal_begin_sparse(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuVarianceDesc* vdesc, const RtuSparseDesc* spdesc, int* err_out) {
    auto refuse = [&](int rc) -> RtuTemporal* {
        if (err_out) *err_out = rc;
        return nullptr;
    };
    if (!ctx) return refuse(RTU_ERR_ARG);
    if (!spdesc || !desc || !vdesc) return refuse(fail(ctx, RTU_ERR_ARG, "temporal: a descriptor is NULL"));
    RtuSparseDesc sd = *spdesc;  // (its frame_index is the frame's)
    sd.frame_index = 0;
    if (sd.width == 0 && sd.height == 0) {
        sd.width = desc->width;
        sd.height = desc->height;
    }
    if (rtu_temporal_check_desc(desc) == RTU_OK) {
        if (rtu_sparse_check_desc(&sd) != RTU_OK) return refuse(fail(ctx, RTU_ERR_ARG, "%s", kSparseDescRules));
        if (sd.width != desc->width || sd.height != desc->height) return refuse(fail(ctx, RTU_ERR_ARG, "sparse: the desc has not the session's size"));
    }
    RtuTemporal* t = rtu_temporal_begin_variance(ctx, desc, vdesc, err_out);
    if (!t) return nullptr;
    t->sparse_session = true;
    if (sd.block == 1) return t;
    t->sparse = true;
    t->spdesc = sd;
    t->blocks = (size_t)sp_blocks(sd.width, sd.block) * (size_t)sp_blocks(sd.height, sd.block);
    hipError_t e = t->sp_owner.grow(t->blocks);
    if (e == hipSuccess) e = t->sp_hole.grow(t->pixels);
    if (e == hipSuccess) e = t->sp_hole_host.grow(t->pixels);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->sp_done, hipEventDisableTiming);
    if (e != hipSuccess) {
        const int rc = fail(ctx, RTU_ERR_HIP, "session buffers: %s", hipGetErrorString(e));
        rtu_temporal_free(t);
        return refuse(rc);
    }
    return t;
}

int rtu_temporal_holes(RtuTemporal* t, uint32_t* count_out) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = t->ctx;
    if (!t->sparse_session) return fail(ctx, RTU_ERR_ARG, "not a sparse session");
    if (!count_out) return fail(ctx, RTU_ERR_ARG, "count_out is NULL");
    *count_out = 0;
    if (!t->sparse || !t->has_hist) return RTU_OK;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    // on the context's own stream, behind the event of the last frame: the caller's stream of that frame may be gone by now
    RTU_HIP(ctx, hipStreamWaitEvent(ctx->stream, t->sp_done, 0));
    RTU_HIP(ctx, hipMemcpyAsync(t->sp_hole_host.get(), t->sp_hole.get(), t->pixels, hipMemcpyDeviceToHost, ctx->stream));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t count = 0;
    const uint8_t* h = t->sp_hole_host.get();
    for (size_t i = 0; i < t->pixels; i++) count += h[i];
    *count_out = count;
    return RTU_OK;
}

// ---- hole rays (rtu_holes.h, rtu_holes.hip): the allocation and the fold on device memory, and the sparse session that shades its holes ----
static_assert(sizeof(RtuHoleDesc) == 32, "RtuHoleDesc is 32 bytes");

static const char* const kHoleDescRules = "holes: width, height 1 .. 65536 (2^26 pixels), budget 0 .. 2^26, reserved words 0";

int rtu_hole_allocation_device(RtuContext* ctx, const RtuHoleDesc* desc, const void* d_hole, const void* d_hits, void* d_counts, void* d_offsets,
                               void* d_total, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_hole_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kHoleDescRules);
    if (!d_hole || !d_hits || !d_counts || !d_offsets || !d_total) return fail(ctx, RTU_ERR_ARG, "holes: a device pointer is NULL");
    if (misaligned(d_hits) || misaligned4(d_counts) || misaligned4(d_offsets) || misaligned4(d_total))
        return fail(ctx, RTU_ERR_ARG, "holes: d_hits must be 16-byte, d_counts, d_offsets and d_total 4-byte aligned (the hole plane: any)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->st_scratch.grow(rtu_steer_scratch_words((size_t)desc->width * (size_t)desc->height)));
    const hipError_t e = (hipError_t)rtu_launch_hole_allocation(*desc, (const uint8_t*)d_hole, (const float4*)d_hits, (uint32_t*)d_counts, (uint32_t*)d_offsets,
                                                                (uint32_t*)d_total, ctx->st_scratch.get(), (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "hole allocation launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_hole_fold_device(RtuContext* ctx, const RtuHoleDesc* desc, void* d_hist, void* d_rgbz, void* d_hole, const void* d_hits, const void* d_albedo,
                         const void* d_counts, const void* d_offsets, const void* d_rgbt, size_t n_rays, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_hole_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kHoleDescRules);
    if (n_rays > ((size_t)1 << 26)) return fail(ctx, RTU_ERR_ARG, "holes: more than 2^26 samples");
    if (!d_hist || !d_rgbz || !d_hole || !d_hits || !d_albedo || !d_counts || !d_offsets || (n_rays && !d_rgbt))
        return fail(ctx, RTU_ERR_ARG, "holes: a device pointer is NULL");
    if (misaligned(d_hist) || misaligned(d_rgbz) || misaligned(d_hits) || misaligned(d_albedo) || misaligned(d_rgbt) || misaligned4(d_counts) ||
        misaligned4(d_offsets))
        return fail(ctx, RTU_ERR_ARG, "holes: device buffers must be 16-byte aligned (d_counts, d_offsets: 4-byte; the hole plane: any)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_hole_fold((size_t)desc->width * (size_t)desc->height, (float4*)d_hist, (float4*)d_rgbz, (uint8_t*)d_hole,
                                                          (const float4*)d_hits, (const float4*)d_albedo, (const uint32_t*)d_counts,
                                                          (const uint32_t*)d_offsets, (const float4*)d_rgbt, (uint32_t)n_rays, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "hole fold launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

RtuTemporal* rtu_temporal_begin_sparse_holes(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuVarianceDesc* vdesc, const RtuSparseDesc* spdesc,
                                             const RtuHoleDesc* hdesc, int* err_out) {
    auto refuse = [&](int rc) -> RtuTemporal* {
        if (err_out) *err_out = rc;
        return nullptr;
    };
    if (!ctx) return refuse(RTU_ERR_ARG);
    if (!hdesc || !spdesc || !desc || !vdesc) return refuse(fail(ctx, RTU_ERR_ARG, "temporal: a descriptor is NULL"));
    RtuHoleDesc hd = *hdesc;  // (its frame_index is the frame's)
    hd.frame_index = 0;
    if (hd.width == 0 && hd.height == 0) {
        hd.width = desc->width;
        hd.height = desc->height;
    }
    if (rtu_temporal_check_desc(desc) == RTU_OK) {
        if (rtu_hole_check_desc(&hd) != RTU_OK) return refuse(fail(ctx, RTU_ERR_ARG, "%s", kHoleDescRules));
        if (hd.width != desc->width || hd.height != desc->height) return refuse(fail(ctx, RTU_ERR_ARG, "holes: the desc has not the session's size"));
    }
    RtuTemporal* t = rtu_temporal_begin_sparse(ctx, desc, vdesc, spdesc, err_out);
    if (!t) return nullptr;
    t->sparse_holes = true;
    t->hdesc = hd;
    if (!t->sparse || hd.budget == 0) return t;  // a sparse session's frames
    const size_t n = t->pixels;
    t->hl_cap = n - t->blocks;  // (block > 1: the image has more pixels than blocks unless it is 1 x 1, which has no hole)
    hipError_t e = hipSuccess;
    if (t->hl_cap) {
        e = t->hl_counts.grow(n);
        if (e == hipSuccess) e = t->hl_offsets.grow(n);
        if (e == hipSuccess) e = t->hl_owner.grow(n);
        if (e == hipSuccess) e = t->hl_total_dev.grow(1);
        if (e == hipSuccess) e = t->hl_total_host.grow(1);
        if (e == hipSuccess) e = ctx->st_scratch.grow(rtu_steer_scratch_words(n));
    }
    if (e != hipSuccess) {
        const int rc = fail(ctx, RTU_ERR_HIP, "session buffers: %s", hipGetErrorString(e));
        rtu_temporal_free(t);
        return refuse(rc);
    }
    return t;
}

// A sparse session's frame between the sparse accumulator and the fill: the pixels `hole` marks shaded by rays of their own — behind
// the owners' batch in the session's ray, key and result buffers — and made the history of those pixels in `hist` and d_rgbz. *total_out:
// the rays of the frame; the session's own word is set at the commit.
static int temporal_hole_rays(RtuTemporal* t, const RtuFrameDesc* frame, uint32_t k, float4* hist, void* d_rgbz, void* hip_stream, uint32_t* total_out) {
    RtuContext* ctx = t->ctx;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool paths = frame->gather_bounces != 0;
    RtuHoleDesc hd = t->hdesc;
    hd.frame_index = k;
    int rc = rtu_hole_allocation_device(ctx, &hd, t->sp_hole.get(), t->hits.get(), t->hl_counts.get(), t->hl_offsets.get(), t->hl_total_dev.get(), hip_stream);
    if (rc != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpyAsync(t->hl_total_host.get(), t->hl_total_dev.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    RTU_HIP(ctx, hipStreamSynchronize(stream));
    const uint32_t total = *t->hl_total_host.get();
    if ((size_t)total > t->hl_cap) return fail(ctx, RTU_ERR_HIP, "holes: %u rays allocated, the session holds %zu", total, t->hl_cap);
    *total_out = total;
    if (total == 0) return RTU_OK;
    float4*   rays = t->rays.get() + 2 * t->blocks;
    uint32_t* keys = t->keys.get() + t->blocks;
    float4*   img = t->img.get() + t->blocks;
    const RtuSteerDesc sd = hl_steer_desc(hd);
    if ((rc = rtu_extra_sample_rays_device(ctx, &sd, frame, t->hl_counts.get(), t->hl_offsets.get(), total, rays, keys, t->hl_owner.get(), hip_stream)) != RTU_OK)
        return rc;
    RtuShadeDesc shd;
    rtu_shade_defaults(&shd);
    memcpy(shd.eye, frame->cam_pos, sizeof shd.eye);
    shd.max_bounce = frame->max_bounce;
    RtuFrameDesc f;
    if ((rc = shade_args(ctx, rays, img, total, &shd, true, &f, true, keys, paths)) != RTU_OK) return rc;
    if (paths && (rc = paths_chain(ctx, f, img, stream, rays, keys, total)) != RTU_OK) return rc;
    if ((rc = shade_until_fits(ctx, f, img, stream, rays, keys, total, paths, nullptr)) != RTU_OK) return rc;
    return rtu_hole_fold_device(ctx, &hd, hist, d_rgbz, t->sp_hole.get(), t->hits.get(), t->albedo.get(), t->hl_counts.get(), t->hl_offsets.get(), img, total,
                                hip_stream);
}

int rtu_temporal_hole_rays(RtuTemporal* t, uint32_t* count_out) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    if (!t->sparse_holes) return fail(t->ctx, RTU_ERR_ARG, "not a sparse session with hole rays");
    if (!count_out) return fail(t->ctx, RTU_ERR_ARG, "count_out is NULL");
    *count_out = t->has_hist ? t->hl_total : 0u;
    return RTU_OK;
}

// what a moved frame has beyond a plain one (rtu_temporal_frame_moved_device)
struct TemporalMoved {
    const RtuNodeMotion* h_motion;
    uint32_t n_nodes;
    int32_t  history_cap;
    bool     deformed;  // rtu_temporal_frame_deformed: the guides with surface records, the deform accumulator
};

static int temporal_frame(RtuTemporal* t, const RtuFrameDesc* frame, void* d_rgbz, void* hip_stream, const TemporalMoved* moved);

int rtu_temporal_frame_device(RtuTemporal* t, const RtuFrameDesc* frame, void* d_rgbz, void* hip_stream) {
    return temporal_frame(t, frame, d_rgbz, hip_stream, nullptr);
}

int rtu_temporal_frame_moved_device(RtuTemporal* t, const RtuFrameDesc* frame, const RtuNodeMotion* h_motion, uint32_t n_nodes, int32_t history_cap,
                                    void* d_rgbz, void* hip_stream) {
    const TemporalMoved moved{h_motion, n_nodes, history_cap, false};
    return temporal_frame(t, frame, d_rgbz, hip_stream, &moved);
}

int rtu_temporal_frame_deformed_device(RtuTemporal* t, const RtuFrameDesc* frame, const RtuNodeMotion* h_motion, uint32_t n_nodes, int32_t history_cap,
                                       void* d_rgbz, void* hip_stream) {
    const TemporalMoved moved{h_motion, n_nodes, history_cap, true};
    return temporal_frame(t, frame, d_rgbz, hip_stream, &moved);
}

static int temporal_frame(RtuTemporal* t, const RtuFrameDesc* frame, void* d_rgbz, void* hip_stream, const TemporalMoved* moved) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = t->ctx;
    if (!frame) return fail(ctx, RTU_ERR_ARG, "frame is NULL");
    const bool deformed = moved && moved->deformed;
    if (deformed && (t->steered || t->gradient || t->sparse || t->hl_cap))
        return fail(ctx, RTU_ERR_UNSUPPORTED, "a deformed frame: plain, RTU_TEMPORAL_DENOISE and variance sessions only");
    if (deformed && !ctx->keep_prev) return fail(ctx, RTU_ERR_ARG, "a deformed frame needs rtu_keep_previous_vertices");
    if (frame->width != t->desc.width || frame->height != t->desc.height) return fail(ctx, RTU_ERR_ARG, "the frame has not the session's width and height");
    if (frame->shard_count != 1 || frame->shard_rank != 0) return fail(ctx, RTU_ERR_ARG, "a temporal session renders the whole image: shard_count must be 1");
    if (frame->samples < 1) return fail(ctx, RTU_ERR_ARG, "a temporal frame is a recipe S / P frame (samples >= 1)");
    if (frame->gather_bounces != 0 && frame->gather_bounces != RTU_GI_BOUNCES) return fail(ctx, RTU_ERR_ARG, "gather_bounces is 0 or %d", RTU_GI_BOUNCES);
    if (frame->collect_stats != 0) return fail(ctx, RTU_ERR_ARG, "a temporal frame has no counters (collect_stats == 0)");
    // A REFUSED CALL LEAVES THE SESSION AS IT WAS. Whatever an entry further down refuses — max_bounce, a camera that is not finite, too
    // many chains of recipe P — it refuses before THE COMMIT below: until there the frame works on copies of the counter and of the
    // history flag, and writes only buffers that hold nothing between two frames. What is refused behind the commit (a steered frame's
    // samples * (1 + max_extra), in temporal_steer) is therefore refused here; so is what the hole rays would refuse, though they run
    // before the commit.
    if (const int rc = check_frame(ctx, frame)) return rc;
    if (t->steered && t->st_cap && (long long)frame->samples * (1 + t->sdesc.max_extra) > 65536)
        return fail(ctx, RTU_ERR_ARG, "a steered frame needs samples * (1 + max_extra) <= 65536");
    if (t->hl_cap && 2ll * frame->samples > 65536) return fail(ctx, RTU_ERR_ARG, "a frame with hole rays needs 2 * samples <= 65536");
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "d_rgbz is NULL");
    if (misaligned(d_rgbz)) return fail(ctx, RTU_ERR_ARG, "d_rgbz must be 16-byte aligned");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool paths = frame->gather_bounces != 0;
    const size_t n = t->pixels;
    if (moved) {
        if (moved->n_nodes != (uint32_t)ctx->shape_nodes.size())
            return fail(ctx, RTU_ERR_ARG, "the motion table has %u entries, the uploaded scene %u nodes", moved->n_nodes, (uint32_t)ctx->shape_nodes.size());
        if (!moved->h_motion && t->has_hist) return fail(ctx, RTU_ERR_ARG, "the motion table is NULL");
        if (rtu_temporal_check_motion(moved->h_motion, moved->n_nodes, moved->history_cap, deformed) != RTU_OK)
            return fail(ctx, RTU_ERR_ARG, "motion: history_cap 0 .. 65535, known flags and reserved words 0 in every table entry");
    }
    if (deformed) {
        RTU_HIP(ctx, hipSetDevice(ctx->device));
        RTU_HIP(ctx, t->surface.grow(2 * n));
    }
    // the table of the frame: a moved frame's (== the scene's node count), or a variance session's all-STATIC one for a plain frame —
    // at least one entry there, the moments form refuses a NULL table. Also on frame 0, which does not use it: a later frame allocates nothing.
    const uint32_t n_static = (uint32_t)ctx->shape_nodes.size();
    if (moved || t->variance) {
        const size_t entries = (t->variance && n_static == 0) ? 1 : n_static;
        RTU_HIP(ctx, hipSetDevice(ctx->device));
        RTU_HIP(ctx, t->motion.grow(entries));
        RTU_HIP(ctx, t->motion_host.grow(entries));
    }
    // another scene generation: a moved frame adopts it; a plain frame starts over — moved geometry or lights: what was accumulated
    // shows another scene. Both take effect at the commit.
    const bool start_over = !moved && t->scene_gen != ctx->scene_gen;
    const bool has_hist = t->has_hist && !start_over && !t->prev_is_sensor;  // (a sensor's history is of another image: none is taken, k goes on)
    const int  k = start_over ? 0 : t->k;
    int rc;
    uint32_t hole_total = 0;
    if (t->sparse) {  // one ray per block: the block's owner of frame k in the sample the block has reached
        t->spdesc.frame_index = (uint32_t)k;
        rc = rtu_sparse_rays_device(ctx, &t->spdesc, frame, t->rays.get(), t->keys.get(), t->sp_owner.get(), hip_stream);
    } else {
        rc = rtu_camera_sample_rays_device(ctx, frame, k % frame->samples, t->rays.get(), t->keys.get(), hip_stream);
    }
    if (rc != RTU_OK) return rc;
    // A gradient session: the gradient rays behind the frame's own, shaded with them in the one launch sequence. A frame without a
    // previous one shades them too and uses none of their results — the batch of every frame has one size, so the context's frame
    // records grow in the first frame and no later frame allocates.
    const bool grad = t->gradient && has_hist;
    const size_t shaded = t->sparse ? t->blocks : (t->gradient ? n + t->strata : n);
    if (t->gradient) {
        t->gdesc.frame_index = (uint32_t)k;
        if ((rc = rtu_gradient_rays_device(ctx, &t->gdesc, frame, (k + frame->samples - 1) % frame->samples, t->rays.get() + 2 * n, t->keys.get() + n,
                                           t->gr_owner.get(), hip_stream)) != RTU_OK)
            return rc;
    }
    RtuShadeDesc sd;
    rtu_shade_defaults(&sd);
    memcpy(sd.eye, frame->cam_pos, sizeof sd.eye);
    sd.max_bounce = frame->max_bounce;
    RtuFrameDesc f;
    if ((rc = shade_args(ctx, t->rays.get(), t->img.get(), shaded, &sd, true, &f, true, t->keys.get(), paths)) != RTU_OK) return rc;
    // as shade_host: the chain of recipe P is traced once, the shading is what is repeated when the frame records ran out
    if (paths && (rc = paths_chain(ctx, f, t->img.get(), stream, t->rays.get(), t->keys.get(), (uint32_t)shaded)) != RTU_OK) return rc;
    if ((rc = shade_until_fits(ctx, f, t->img.get(), stream, t->rays.get(), t->keys.get(), (uint32_t)shaded, paths, nullptr)) != RTU_OK) return rc;
    if (deformed) rc = rtu_frame_surface_device(ctx, frame, t->hits.get(), t->albedo.get(), t->surface.get(), hip_stream);
    else rc = rtu_frame_features_device(ctx, frame, t->hits.get(), t->albedo.get(), hip_stream);
    if (rc != RTU_OK) return rc;
    RtuTemporalDesc td = t->desc;
    td.flags = 0;
    if (t->variance) {
        // the stream was waited for above: the copy of the frame before has left the staging memory (ONE STREAM PER CONTEXT)
        const uint32_t n_nodes = moved ? moved->n_nodes : n_static;
        if (moved && has_hist) {
            memcpy(t->motion_host.get(), moved->h_motion, n_nodes * sizeof(RtuNodeMotion));
        } else {
            RtuNodeMotion id{};
            const TpMotion T = tp_motion_identity();
            memcpy(id.m, T.m, sizeof id.m);
            memcpy(id.g, T.g, sizeof id.g);
            id.flags = RTU_MOTION_STATIC;
            for (uint32_t i = 0; i < n_nodes; i++) t->motion_host.get()[i] = id;
        }
        if (n_nodes > 0)
            RTU_HIP(ctx, hipMemcpyAsync(t->motion.get(), t->motion_host.get(), n_nodes * sizeof(RtuNodeMotion), hipMemcpyHostToDevice, stream));
        if (t->sparse) {
            rc = rtu_temporal_accumulate_sparse_device(ctx, &td, &t->spdesc, has_hist ? &t->prev_cam : nullptr, frame, t->img.get(), t->sp_owner.get(),
                                                       t->hits.get(), t->albedo.get(), has_hist ? t->hist[t->cur].get() : nullptr,
                                                       t->hist[t->cur ^ 1].get(), d_rgbz, t->sp_hole.get(), t->motion.get(), n_nodes,
                                                       moved ? moved->history_cap : 0, hip_stream);
            if (rc == RTU_OK && t->hl_cap) rc = temporal_hole_rays(t, frame, (uint32_t)k, t->hist[t->cur ^ 1].get(), d_rgbz, hip_stream, &hole_total);
            if (rc == RTU_OK)
                rc = rtu_sparse_fill_device(ctx, &td, &t->spdesc, t->hits.get(), t->albedo.get(), t->sp_owner.get(), t->img.get(), t->sp_hole.get(), d_rgbz,
                                            hip_stream);
            if (rc == RTU_OK) RTU_HIP(ctx, hipEventRecord(t->sp_done, stream));  // rtu_temporal_holes reads the hole plane behind it
        } else if (grad) {
            rc = rtu_temporal_gradient_device(ctx, &td, &t->gdesc, &t->prev_cam, frame, t->hits.get(), t->albedo.get(), t->motion.get(), n_nodes,
                                              t->hist[t->cur].get(), t->lum[t->lcur].get(), t->gr_owner.get(), t->img.get() + n, t->gr_diff.get(),
                                              t->gr_lambda.get(), hip_stream);
            if (rc == RTU_OK)
                rc = rtu_temporal_accumulate_gradient_device(ctx, &td, &t->prev_cam, frame, t->img.get(), t->hits.get(), t->albedo.get(),
                                                             t->hist[t->cur].get(), t->hist[t->cur ^ 1].get(), d_rgbz, t->motion.get(), n_nodes,
                                                             moved ? moved->history_cap : 0, t->gr_lambda.get(), hip_stream);
        } else if (deformed) {
            rc = rtu_temporal_accumulate_deform_moments_device(ctx, &td, has_hist ? &t->prev_cam : nullptr, frame, t->img.get(), t->hits.get(),
                                                               t->albedo.get(), t->surface.get(), has_hist ? t->hist[t->cur].get() : nullptr,
                                                               t->hist[t->cur ^ 1].get(), d_rgbz, t->motion.get(), n_nodes, moved->history_cap, hip_stream);
        } else {
            rc = rtu_temporal_accumulate_moments_device(ctx, &td, has_hist ? &t->prev_cam : nullptr, frame, t->img.get(), t->hits.get(), t->albedo.get(),
                                                        has_hist ? t->hist[t->cur].get() : nullptr, t->hist[t->cur ^ 1].get(), d_rgbz, t->motion.get(),
                                                        n_nodes, moved ? moved->history_cap : 0, hip_stream);
        }
        if (rc == RTU_OK && t->gradient) {  // the luminance of this frame's sample: what the next frame's gradients are taken against
            rc = rtu_sample_luminance_device(ctx, &t->gdesc, t->img.get(), t->hits.get(), t->albedo.get(), t->lum[t->lcur ^ 1].get(), hip_stream);
            t->lcur ^= 1;
            t->has_lambda = grad;
        }
    } else if (moved && has_hist) {
        // the stream was waited for above: the copy of the frame before has left the staging memory (ONE STREAM PER CONTEXT)
        memcpy(t->motion_host.get(), moved->h_motion, moved->n_nodes * sizeof(RtuNodeMotion));
        RTU_HIP(ctx, hipMemcpyAsync(t->motion.get(), t->motion_host.get(), moved->n_nodes * sizeof(RtuNodeMotion), hipMemcpyHostToDevice, stream));
        if (deformed)
            rc = rtu_temporal_accumulate_deform_device(ctx, &td, &t->prev_cam, frame, t->img.get(), t->hits.get(), t->albedo.get(), t->surface.get(),
                                                       t->hist[t->cur].get(), t->hist[t->cur ^ 1].get(), d_rgbz, t->motion.get(), moved->n_nodes,
                                                       moved->history_cap, hip_stream);
        else
            rc = rtu_temporal_accumulate_motion_device(ctx, &td, &t->prev_cam, frame, t->img.get(), t->hits.get(), t->albedo.get(), t->hist[t->cur].get(),
                                                       t->hist[t->cur ^ 1].get(), d_rgbz, t->motion.get(), moved->n_nodes, moved->history_cap, hip_stream);
    } else {  // (frame 0 of a moved session has nothing to look up: the plain form gives its bits)
        rc = rtu_temporal_accumulate_device(ctx, &td, has_hist ? &t->prev_cam : nullptr, frame, t->img.get(), t->hits.get(), t->albedo.get(),
                                            has_hist ? t->hist[t->cur].get() : nullptr, t->hist[t->cur ^ 1].get(), d_rgbz, hip_stream);
    }
    if (rc != RTU_OK) return rc;
    // THE COMMIT: nothing behind it refuses
    t->scene_gen = ctx->scene_gen;
    t->cur ^= 1;
    t->has_hist = true;
    t->prev_cam = *frame;
    t->prev_is_sensor = false;
    t->k = k + 1;
    t->hl_total = hole_total;
    if (t->variance) {
        if ((rc = rtu_variance_device(ctx, &t->vdesc, t->hist[t->cur].get(), t->hits.get(), t->var.get(), hip_stream)) != RTU_OK) return rc;
        if (t->steered && t->st_cap && (rc = temporal_steer(t, frame, (uint32_t)k, d_rgbz, hip_stream)) != RTU_OK) return rc;
        return rtu_denoise_variance_device(ctx, &t->vdesc, d_rgbz, t->hits.get(), t->albedo.get(), t->var.get(), d_rgbz, hip_stream);  // in place
    }
    if (t->desc.flags & RTU_TEMPORAL_DENOISE) {
        RtuDenoiseDesc dd;
        rtu_denoise_defaults(&dd);
        dd.width = t->desc.width;
        dd.height = t->desc.height;
        return rtu_denoise_device(ctx, &dd, d_rgbz, t->hits.get(), t->albedo.get(), d_rgbz, hip_stream);  // in place; the history stays unfiltered
    }
    return RTU_OK;
}

// the host forms: the frame into the context's frame buffer, then its copy to h_rgbz
static int temporal_frame_host(RtuTemporal* t, const RtuFrameDesc* frame, float* h_rgbz, const TemporalMoved* moved) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = t->ctx;
    if (!h_rgbz) return fail(ctx, RTU_ERR_ARG, "h_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->fb.grow(t->pixels));
    const int rc = temporal_frame(t, frame, ctx->fb.get(), ctx->stream, moved);
    if (rc != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpyAsync(h_rgbz, ctx->fb.get(), t->pixels * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTU_OK;
}

int rtu_temporal_frame(RtuTemporal* t, const RtuFrameDesc* frame, float* h_rgbz) { return temporal_frame_host(t, frame, h_rgbz, nullptr); }

int rtu_temporal_frame_moved(RtuTemporal* t, const RtuFrameDesc* frame, const RtuNodeMotion* h_motion, uint32_t n_nodes, int32_t history_cap, float* h_rgbz) {
    const TemporalMoved moved{h_motion, n_nodes, history_cap, false};
    return temporal_frame_host(t, frame, h_rgbz, &moved);
}

int rtu_temporal_frame_deformed(RtuTemporal* t, const RtuFrameDesc* frame, const RtuNodeMotion* h_motion, uint32_t n_nodes, int32_t history_cap,
                                float* h_rgbz) {
    const TemporalMoved moved{h_motion, n_nodes, history_cap, true};
    return temporal_frame_host(t, frame, h_rgbz, &moved);
}

int rtu_temporal_history_device(RtuTemporal* t, void* d_n, void* hip_stream) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = t->ctx;
    if (!d_n) return fail(ctx, RTU_ERR_ARG, "d_n is NULL");
    if ((uintptr_t)d_n & 3u) return fail(ctx, RTU_ERR_ARG, "d_n must be 4-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const bool live = t->has_hist && t->scene_gen == ctx->scene_gen;
    const hipError_t e = (hipError_t)rtu_launch_temporal_history(live ? t->hist[t->cur].get() : nullptr, (float*)d_n, t->pixels, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "temporal history launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_temporal_reset(RtuTemporal* t) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    t->has_hist = false;
    t->k = 0;
    t->st_total = 0;
    t->hl_total = 0;
    t->has_lambda = false;
    return RTU_OK;
}

void rtu_temporal_free(RtuTemporal* t) {
    if (!t) return;
    if (RtuContext* ctx = t->ctx) {
        (void)hipSetDevice(ctx->device);
        ctx->temporals.erase(std::remove(ctx->temporals.begin(), ctx->temporals.end(), t), ctx->temporals.end());
    }
    delete t;
}

// ---- temporal accumulation for sensors (rtu_sensor.h sensor_project, rtu_temporal.hip k_temporal_sensor): the accumulator on device
// memory, and the sensor frames of a session. (The projection's host form, rtu_sensor_project, is in rtu_capi_sensor.hip.) -----------
// the two _device forms: `moments` — histories of four planes. The order of the checks is that of temporal_device_args.
static int temporal_sensor_device(RtuContext* ctx, bool moments, const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur,
                                  const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out, void* d_rgbz_out,
                                  void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_temporal_check_desc(desc) != RTU_OK) return fail(ctx, RTU_ERR_ARG, "%s", kTemporalDescRules);
    if (!cur || (d_hist_prev && !prev)) return fail(ctx, RTU_ERR_ARG, "temporal: a sensor is NULL");
    if (!prev) prev = cur;
    int rc = check_sensor(ctx, cur);
    if (rc == RTU_OK) rc = check_sensor(ctx, prev);
    if (rc != RTU_OK) return rc;
    if (cur->width != desc->width || cur->height != desc->height) return fail(ctx, RTU_ERR_ARG, "temporal: the sensor must have the desc's width and height");
    if (!d_rgbz || !d_hits || !d_albedo || !d_hist_out || !d_rgbz_out) return fail(ctx, RTU_ERR_ARG, "temporal: a device pointer is NULL");
    if (misaligned(d_rgbz) || misaligned(d_hits) || misaligned(d_albedo) || misaligned(d_hist_prev) || misaligned(d_hist_out) || misaligned(d_rgbz_out))
        return fail(ctx, RTU_ERR_ARG, "temporal: device buffers must be 16-byte aligned");
    if (d_hist_prev) {
        const uintptr_t a = (uintptr_t)d_hist_prev, b = (uintptr_t)d_hist_out,
                        bytes = (uintptr_t)(moments ? 64 : 48) * (uintptr_t)desc->width * (uintptr_t)desc->height;
        if (a < b + bytes && b < a + bytes) return fail(ctx, RTU_ERR_ARG, "temporal: hist_out overlaps hist_prev");
    }
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const TpParams p = tp_sensor_setup(*desc, *prev, *cur, d_hist_prev != nullptr);
    const hipError_t e = (hipError_t)rtu_launch_temporal_sensor(p, *prev, moments, (const float4*)d_rgbz, (const float4*)d_hits, (const float4*)d_albedo,
                                                                p.lookup != TP_LOOKUP_NONE ? (const float4*)d_hist_prev : nullptr, (float4*)d_hist_out,
                                                                (float4*)d_rgbz_out, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "temporal launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_temporal_accumulate_sensor_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur, const void* d_rgbz,
                                          const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out, void* d_rgbz_out,
                                          void* hip_stream) {
    return temporal_sensor_device(ctx, false, desc, prev, cur, d_rgbz, d_hits, d_albedo, d_hist_prev, d_hist_out, d_rgbz_out, hip_stream);
}

int rtu_temporal_accumulate_sensor_moments_device(RtuContext* ctx, const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur,
                                                  const void* d_rgbz, const void* d_hits, const void* d_albedo, const void* d_hist_prev, void* d_hist_out,
                                                  void* d_rgbz_out, void* hip_stream) {
    return temporal_sensor_device(ctx, true, desc, prev, cur, d_rgbz, d_hits, d_albedo, d_hist_prev, d_hist_out, d_rgbz_out, hip_stream);
}

// A sensor frame of a session: temporal_frame with the sensor's rays, guides and accumulator. The scene is at rest: no table.
int rtu_temporal_sensor_frame_device(RtuTemporal* t, const RtuSensorDesc* sensor, void* d_rgbz, void* hip_stream) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = t->ctx;
    int rc = check_sensor(ctx, sensor);
    if (rc != RTU_OK) return rc;
    if (t->steered || t->gradient || t->sparse_session)
        return fail(ctx, RTU_ERR_ARG, "a steered, gradient or sparse session takes camera frames only: its ray generators have no sensor form");
    if (sensor->width != t->desc.width || sensor->height != t->desc.height) return fail(ctx, RTU_ERR_ARG, "the sensor has not the session's width and height");
    if (sensor->samples < 1) return fail(ctx, RTU_ERR_ARG, "a temporal frame is a recipe S / P frame (samples >= 1)");
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "d_rgbz is NULL");
    if (misaligned(d_rgbz)) return fail(ctx, RTU_ERR_ARG, "d_rgbz must be 16-byte aligned");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool paths = sensor->gather_bounces != 0;
    const size_t n = t->pixels;
    // A REFUSED CALL LEAVES THE SESSION AS IT WAS, as in temporal_frame: copies of the counter and of the history flag until the commit.
    if (t->variance) {  // what a later camera frame of this session needs: no frame after the first allocates
        const size_t entries = ctx->shape_nodes.empty() ? 1 : ctx->shape_nodes.size();
        RTU_HIP(ctx, hipSetDevice(ctx->device));
        RTU_HIP(ctx, t->motion.grow(entries));
        RTU_HIP(ctx, t->motion_host.grow(entries));
    }
    const bool start_over = t->scene_gen != ctx->scene_gen;
    // the history of a camera frame, or of a sensor of another model, is of another image: none is taken, k goes on
    const bool has_hist = t->has_hist && !start_over && t->prev_is_sensor && t->prev_sensor.model == sensor->model;
    const int  k = start_over ? 0 : t->k;
    if ((rc = rtu_sensor_rays_device(ctx, sensor, k % sensor->samples, 1, t->rays.get(), t->keys.get(), hip_stream)) != RTU_OK) return rc;
    RtuShadeDesc sd;
    rtu_shade_defaults(&sd);
    memcpy(sd.eye, sensor->pos, sizeof sd.eye);
    sd.max_bounce = sensor->max_bounce;
    sd.flags = sensor->flags;
    RtuFrameDesc f;
    if ((rc = shade_args(ctx, t->rays.get(), t->img.get(), n, &sd, true, &f, true, t->keys.get(), paths)) != RTU_OK) return rc;
    if (paths && (rc = paths_chain(ctx, f, t->img.get(), stream, t->rays.get(), t->keys.get(), (uint32_t)n)) != RTU_OK) return rc;
    if ((rc = shade_until_fits(ctx, f, t->img.get(), stream, t->rays.get(), t->keys.get(), (uint32_t)n, paths,
                               "recipe P with counters: frame records ran out; run the frame once without RTU_QUERY_REFERENCE_WALK first")) != RTU_OK)
        return rc;
    // the guides: the pixel-centre rays — the sensor's rays with samples == 0 — over the sample's rays, which are shaded (the stream was
    // waited for above)
    RtuSensorDesc centre = *sensor;
    centre.samples = 0;
    centre.gather_bounces = 0;
    if ((rc = sensor_generate(ctx, &centre, 0, 1, t->rays.get(), nullptr, stream)) != RTU_OK) return rc;
    if ((rc = rtu_ray_features_device(ctx, t->rays.get(), n, 0, t->hits.get(), t->albedo.get(), hip_stream)) != RTU_OK) return rc;
    RtuTemporalDesc td = t->desc;
    td.flags = 0;
    rc = temporal_sensor_device(ctx, t->variance, &td, has_hist ? &t->prev_sensor : nullptr, sensor, t->img.get(), t->hits.get(), t->albedo.get(),
                                has_hist ? t->hist[t->cur].get() : nullptr, t->hist[t->cur ^ 1].get(), d_rgbz, hip_stream);
    if (rc != RTU_OK) return rc;
    // THE COMMIT: nothing behind it refuses
    t->scene_gen = ctx->scene_gen;
    t->cur ^= 1;
    t->has_hist = true;
    t->prev_sensor = *sensor;
    t->prev_is_sensor = true;
    t->k = k + 1;
    if (t->variance) {
        if ((rc = rtu_variance_device(ctx, &t->vdesc, t->hist[t->cur].get(), t->hits.get(), t->var.get(), hip_stream)) != RTU_OK) return rc;
        return rtu_denoise_variance_device(ctx, &t->vdesc, d_rgbz, t->hits.get(), t->albedo.get(), t->var.get(), d_rgbz, hip_stream);  // in place
    }
    if (t->desc.flags & RTU_TEMPORAL_DENOISE) {
        RtuDenoiseDesc dd;
        rtu_denoise_defaults(&dd);
        dd.width = t->desc.width;
        dd.height = t->desc.height;
        return rtu_denoise_device(ctx, &dd, d_rgbz, t->hits.get(), t->albedo.get(), d_rgbz, hip_stream);  // in place; the history stays unfiltered
    }
    return RTU_OK;
}

int rtu_temporal_sensor_frame(RtuTemporal* t, const RtuSensorDesc* sensor, float* h_rgbz) {
    if (!t || !t->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = t->ctx;
    if (!h_rgbz) return fail(ctx, RTU_ERR_ARG, "h_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->fb.grow(t->pixels));
    const int rc = rtu_temporal_sensor_frame_device(t, sensor, ctx->fb.get(), ctx->stream);
    if (rc != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpyAsync(h_rgbz, ctx->fb.get(), t->pixels * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTU_OK;
}
}  // extern "C"
