// rtu_capi.hip — host side of the C-ABI in include/rtu_render.h: context, scene
// validation + upload into the HBM layout of rtu_device.h, frame set-up and
// kernel launch. What an upload builds on the host without a GPU (trees, triangle
// records, world bounds, occluder lists) is in rtu_capi_build.hip; the temporal
// accumulators and sessions are in rtu_capi_temporal.hip, sensors and adaptive
// sensors in rtu_capi_sensor.hip; rtu_capi.h is what the four share. All are
// compiled by hipcc with -ffp-contract=off so the few host-side float computations
// (triangle normals in the builders, the camera frame here, the host forms of the
// ray generators) round exactly like the reference's CPU code.
//
// The five concerns this file still holds, and all that one uses of another (the rest of each is its own). "The neighbours" are
// rtu_capi_temporal.hip and rtu_capi_sensor.hip: what they use is declared in rtu_capi.h and defined here outside the unnamed
// namespaces, or, where it is a few lines (check_frame, halton, cancel_raised, misaligned, HostSinCos), defined in rtu_capi.h.
//   scene        validation, place_scene, upload, updates in place, scene motion, mesh and light-list dumps, sort boxes
//   frame path   level buffers, launch(), check_overflow, the sampled / adaptive / progressive paths, every rtu_render_frame*,
//                statistics, probes, switches, self-tests. Used from outside: launch (ray batches, the halves, the irradiance
//                build), check_overflow (ray batches). The neighbours: check_adaptive_desc (adaptive sensors)
//   queries      ray queries, first-hit features, surface records, rtu_denoise_device. Used from outside: query_scene and
//                feature_cam (the denoised progressive snapshot), kQueryChunk (ray batches). (misaligned, which the frame path
//                and the temporal file use too, is in rtu_capi.h.)
//   ray batches  shade_args, paths_chain, shade_until_fits, the host sample streams, cam_sample, the half_* family, ray ordering.
//                Used from outside: shade_args, half_scene, half_chain, half_until_fits, kPathChains, cam_sample (irradiance). The
//                neighbours: shade_args, paths_chain, shade_until_fits (both), cam_sample (temporal), h_portable_sincos behind
//                HostSinCos of rtu_capi.h (both)
//   irradiance   the map's build, sample and frame; nothing of it is used elsewhere
// Of the neighbours this file uses temporal_release alone (rtu_destroy_context). Beyond these, one concern calls another only
// through its public rtu_* entries. launch, check_overflow, sample_batches, render_sampled, the rtu_render_frame* entries and the
// progressive session are the benchmarked path and stay one translation unit.
#include "rtu_camrays.h"
#include "rtu_capi.h"
#include "rtu_denoise.h"
#include "rtu_devbuf.h"
#include "rtu_device.h"
#include "rtu_features.h"
#include "rtu_lightlist.h"
#include "rtu_meshrec.h"
#include "rtu_query.h"
#include "rtu_raysort.h"
#include "rtu_irradiance.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace {

const size_t kCounterBytes = (size_t)RTU_TL_KERNELS * RTU_TOUCH_STRIDE * sizeof(unsigned long long);

}  // namespace

int fail(RtuContext* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->error = buf;
    return code;
}

namespace {

void free_scene(RtuContext* ctx) {
    ctx->scene_allocs.clear();
    ctx->prev_gen.clear();  // after an upload "previous" is "current"
    ctx->df_dirty = true;
    ctx->place.clear();
    ctx->has_scene = false;
}

}  // namespace

int ensure_place(RtuContext* ctx, int slot, size_t bytes, void** out) {
    if (ctx->place.size() < (size_t)P_SLOTS) ctx->place.resize(P_SLOTS);
    DevBuf<char>& b = ctx->place[(size_t)slot];
    RTU_HIP(ctx, b.grow(bytes ? bytes : 16));  // keep pointers valid for empty arrays
    *out = b.get();
    return RTU_OK;
}

namespace {

// a new device allocation of `bytes`, owned by `list` (the scene's or the level arrays' storage) until it is cleared
template <class T>
int alloc_owned(RtuContext* ctx, std::vector<DevBuf<char>>& list, size_t bytes, T** dst) {
    list.emplace_back();
    RTU_HIP(ctx, list.back().grow(bytes));
    *dst = reinterpret_cast<T*>(list.back().get());
    return RTU_OK;
}

template <class T>
int upload(RtuContext* ctx, const T* src, size_t count, const T** dst) {
    *dst = nullptr;
    T* d = nullptr;
    int rc = alloc_owned(ctx, ctx->scene_allocs, count ? sizeof(T) * count : 16, &d);  // keep pointers valid for empty arrays
    if (rc != RTU_OK) return rc;
    if (count) RTU_HIP(ctx, hipMemcpy(d, src, sizeof(T) * count, hipMemcpyHostToDevice));
    *dst = d;
    return RTU_OK;
}

// The node ranges of the levels of a collapsed tree (build_wide4 / build_wide8 number breadth-first: a level is a range of nodes),
// root first: level L = nodes [out[L], out[L + 1]). A function of the ref words only.
template <int W>
void wide_levels(const std::vector<float4>& tree, std::vector<uint32_t>& out) {
    const float* t = reinterpret_cast<const float*>(tree.data());
    const uint32_t n_nodes = (uint32_t)(tree.size() * 4 / MuWide<W>::kNodeFloats);
    std::vector<uint32_t> level(n_nodes, 0u);
    out.clear();
    for (uint32_t i = 0; i < n_nodes; i++) {  // parents come before their children
        if (i == 0 || level[i] != level[i - 1]) out.push_back(i);
        for (uint32_t c = 0; c < (uint32_t)W; c++) {
            const uint32_t ref = mu_ref<W>(t, i, c);
            if (mu_is_inner(ref) && ref < n_nodes) level[ref] = level[i] + 1;
        }
    }
    out.push_back(n_nodes);
}

// the boxes of a collapsed tree from the vertices of `m` through the fast tree's element order: what the device refit writes
template <int W>
void refit_host(std::vector<float4>& tree, const RtuMesh& m, const std::vector<uint32_t>& elements) {
    float* t = reinterpret_cast<float*>(tree.data());
    const uint32_t n_nodes = (uint32_t)(tree.size() * 4 / MuWide<W>::kNodeFloats);
    for (uint32_t i = n_nodes; i-- > 0;)  // children have larger numbers than their parents
        for (uint32_t c = 0; c < (uint32_t)W; c++) {
            mu_leaf_slot<W>(t, i, c, m.f, m.v, elements.data(), (uint32_t)elements.size());
            mu_inner_slot<W>(t, n_nodes, i, c);
        }
}

// The checks of a mesh's `ref` tree and element list (validate, and rtu_update_meshes for the trees it takes): element ids, and every
// node reachable from the root well formed; children have larger ids than their parent (cyBVH.h:242-251), which also rules out
// cycles.
int validate_tree(RtuContext* ctx, const RtuMesh& m, uint32_t mi) {
    for (uint32_t i = 0; i < m.n_elements; i++)
        if (m.elements[i] >= m.nf) return fail(ctx, RTU_ERR_ARG, "mesh %u: element out of range", mi);
    std::vector<std::pair<uint32_t, uint32_t>> st;  // node, level
    st.push_back({1u, 1u});
    uint32_t depth = 0;
    while (!st.empty()) {
        auto [id, lvl] = st.back();
        st.pop_back();
        if (lvl > depth) depth = lvl;
        const RtuBvhNode& n = m.bvh[id];
        if (n.count == 0) {
            if (n.index <= id || n.index + 1 >= m.n_bvh_nodes) return fail(ctx, RTU_ERR_ARG, "mesh %u: bad child index at node %u", mi, id);
            st.push_back({n.index, lvl + 1});
            st.push_back({n.index + 1, lvl + 1});
        } else {
            if (n.count > 8 || n.index + n.count > m.n_elements) return fail(ctx, RTU_ERR_ARG, "mesh %u: bad leaf at node %u", mi, id);
        }
    }
    if (depth > m.bvh_depth) return fail(ctx, RTU_ERR_ARG, "mesh %u: bvh_depth %u understates the tree (%u)", mi, m.bvh_depth, depth);
    return RTU_OK;
}

// Reject anything the kernel's indexing does not expect, so that a malformed
// scene is an error code and never an out-of-bounds access on the GPU. placement: the mesh and texture arrays are the uploaded
// ones (rtu_update_scene): only what an update may change is checked.
int validate(RtuContext* ctx, const RtuSceneDesc* s, bool placement = false) {
    if (!s || !s->nodes || s->n_nodes == 0) return fail(ctx, RTU_ERR_ARG, "scene has no nodes");
    if (s->n_materials && !s->materials) return fail(ctx, RTU_ERR_ARG, "materials is NULL");
    if (s->n_lights && !s->lights) return fail(ctx, RTU_ERR_ARG, "lights is NULL");
    if (s->n_meshes && !s->meshes) return fail(ctx, RTU_ERR_ARG, "meshes is NULL");
    for (uint32_t i = 0; i < s->n_textures && !placement; i++) {
        const RtuTexture& t = s->textures[i];
        if (t.type != RTU_TEX_FILE && t.type != RTU_TEX_CHECKER) return fail(ctx, RTU_ERR_ARG, "texture %u: unknown type", i);
        if (t.type == RTU_TEX_FILE && (t.width < 0 || t.height < 0 || ((size_t)t.width * t.height > 0 && !t.rgb)))
            return fail(ctx, RTU_ERR_ARG, "texture %u: bad image", i);
        // one side 0, the other not: TextureFile::Sample divides by the 0 (the reference faults) and reads an image that is not there
        if (t.type == RTU_TEX_FILE && (t.width == 0) != (t.height == 0)) return fail(ctx, RTU_ERR_ARG, "texture %u: %d x %d image", i, t.width, t.height);
    }
    auto map_ok = [&](const RtuTexMap& m) { return !m.present || m.texture < (int32_t)s->n_textures; };
    if (!map_ok(s->background_map) || !map_ok(s->environment_map)) return fail(ctx, RTU_ERR_ARG, "background/environment map: bad texture index");
    if (s->material_maps)
        for (uint32_t i = 0; i < s->n_materials * 4; i++)
            if (!map_ok(s->material_maps[i])) return fail(ctx, RTU_ERR_ARG, "material map %u: bad texture index", i);
    if (((s->background.has_map && !s->background.map_is_null) && !s->background_map.present) ||
        ((s->environment.has_map && !s->environment.map_is_null) && !s->environment_map.present))
        return fail(ctx, RTU_ERR_ARG, "textured background/environment without its texture map");
    for (uint32_t i = 0; i < s->n_lights; i++) {
        const RtuLight& l = s->lights[i];
        if (l.type < RTU_LIGHT_AMBIENT || l.type > RTU_LIGHT_POINT) return fail(ctx, RTU_ERR_ARG, "light %u: bad type", i);
    }
    uint32_t n_shadow = 0;
    for (uint32_t i = 0; i < s->n_lights; i++)
        if (s->lights[i].type != RTU_LIGHT_AMBIENT) n_shadow++;
    if (n_shadow > RTU_MAX_SHADOW_LIGHTS) return fail(ctx, RTU_ERR_UNSUPPORTED, "more than %d non-ambient lights", RTU_MAX_SHADOW_LIGHTS);
    if (s->n_materials > RTU_FI_MTL_MASK) return fail(ctx, RTU_ERR_UNSUPPORTED, "too many materials");
    for (uint32_t i = 0; i < s->n_nodes; i++) {
        const RtuNode& n = s->nodes[i];
        if (i == 0 ? n.parent != -1 : (n.parent < 0 || (uint32_t)n.parent >= i))
            return fail(ctx, RTU_ERR_ARG, "node %u: parent %d breaks pre-order", i, n.parent);
        int depth = i == 0 ? 0 : s->nodes[n.parent].depth + 1;
        if (n.depth != depth) return fail(ctx, RTU_ERR_ARG, "node %u: depth %d != %d", i, n.depth, depth);
        if (depth >= RTU_MAX_NODE_DEPTH) return fail(ctx, RTU_ERR_UNSUPPORTED, "node %u deeper than %d", i, RTU_MAX_NODE_DEPTH - 1);
        if (n.obj_type < RTU_OBJ_NONE || n.obj_type > RTU_OBJ_TRIMESH) return fail(ctx, RTU_ERR_ARG, "node %u: bad type", i);
        if (n.obj_type == RTU_OBJ_TRIMESH && (n.mesh_id < 0 || (uint32_t)n.mesh_id >= s->n_meshes))
            return fail(ctx, RTU_ERR_ARG, "node %u: bad mesh id", i);
        if (n.material_id >= (int)s->n_materials) return fail(ctx, RTU_ERR_ARG, "node %u: bad material id", i);
    }
    for (uint32_t mi = 0; mi < s->n_meshes && !placement; mi++) {
        const RtuMesh& m = s->meshes[mi];
        if (!m.v || !m.f || !m.vn || !m.fn || !m.bvh || !m.elements)
            return fail(ctx, RTU_ERR_ARG, "mesh %u: missing array (normals are required, objects.h:56)", mi);
        if (m.n_bvh_nodes < 2 || m.n_elements != m.nf || m.nf == 0) return fail(ctx, RTU_ERR_ARG, "mesh %u: empty", mi);
        if (m.n_bvh_nodes >= (1u << 28) || m.n_elements >= (1u << 28)) return fail(ctx, RTU_ERR_UNSUPPORTED, "mesh %u: more than 2^28 nodes/elements", mi);
        // the fast walk addresses its triangle records (64 B) and 4-wide nodes (128 B, fewer than triangles) with 32-bit byte offsets
        if (m.nf >= (1u << 26) || m.n_elements >= (1u << 26)) return fail(ctx, RTU_ERR_UNSUPPORTED, "mesh %u: more than 2^26 triangles", mi);
        if (m.bvh_depth > RTU_MAX_BVH_STACK) return fail(ctx, RTU_ERR_UNSUPPORTED, "mesh %u: BVH depth %u > %d", mi, m.bvh_depth, RTU_MAX_BVH_STACK);
        for (uint32_t i = 0; i < m.nf * 3; i++) {
            if (m.f[i] >= m.nv) return fail(ctx, RTU_ERR_ARG, "mesh %u: vertex index out of range", mi);
            if (m.fn[i] >= m.nvn) return fail(ctx, RTU_ERR_ARG, "mesh %u: normal index out of range", mi);
        }
        // texture coordinates are optional, but half a set or an index past nvt would be read on every accepted hit
        if ((m.vt != nullptr) != (m.ft != nullptr) || ((m.vt || m.ft) && m.nvt == 0) || (m.nvt != 0 && !m.vt))
            return fail(ctx, RTU_ERR_ARG, "mesh %u: texture vertices and texture faces must come together (nvt %u)", mi, m.nvt);
        if (m.ft)
            for (uint32_t i = 0; i < m.nf * 3; i++)
                if (m.ft[i] >= m.nvt) return fail(ctx, RTU_ERR_ARG, "mesh %u: texture-vertex index out of range", mi);
        if (int rc = validate_tree(ctx, m, mi); rc != RTU_OK) return rc;
    }
    return RTU_OK;
}

// background.Sample / environment.SampleEnvironment for the supported cases
// (scene.h:421-431): untextured -> colour; TextureMap(NULL) -> colour * black.
void env_value(const RtuEnvColor& e, float out[3]) {
    for (int k = 0; k < 3; k++) out[k] = e.has_map ? e.color[k] * 0.0f : e.color[k];
}

int shard_bands(int height, int rank, int count) {
    int nb = (height + RTU_BAND_ROWS - 1) / RTU_BAND_ROWS;
    if (rank >= nb) return 0;
    return (nb - rank + count - 1) / count;
}

void free_levels(RtuContext* ctx) {
    ctx->level_allocs.clear();
    memset(ctx->lv, 0, sizeof ctx->lv);
    memset(ctx->lv_side, 0, sizeof ctx->lv_side);
    ctx->defer_list0 = nullptr;
    ctx->defer_cap0_s = 0;
}

template <class T>
int alloc_level(RtuContext* ctx, T** dst, size_t count) {
    return alloc_owned(ctx, ctx->level_allocs, sizeof(T) * (count ? count : 1), dst);
}

// one set of level arrays, cap_s frames per shard: famb only if `amb`, fuv / fsuv only for a textured scene
int alloc_level_set(RtuContext* ctx, LevelBuffers& lv, size_t cap_s, bool amb) {
    const size_t cap = cap_s * RTU_SHARDS;
    int rc = RTU_OK;
    auto a = [&](auto** dst, size_t count) { if (rc == RTU_OK) rc = alloc_level(ctx, dst, count); };
    a(&lv.fa, cap);
    a(&lv.fb, cap);
    a(&lv.fc, cap);
    a(&lv.fres, cap);
    a(&lv.fchild, cap);
    a(&lv.fsh, cap * (ctx->nsl ? ctx->nsl : 1));
    a(&lv.fslot, cap * 6);
    a(&lv.fpend, cap);
    if (amb) a(&lv.famb, cap);
    if (ctx->textured) {
        a(&lv.fuv, cap);
        a(&lv.fsuv, cap * 3);
    }
    a(&lv.lmain, cap);
    a(&lv.lrefl, cap);
    if (rc == RTU_OK) lv.cap_s = (uint32_t)cap_s;
    return rc;
}

// Frame arrays of every recursion level (rtu_device.h). Level 0 holds at most one frame per
// pixel; a deeper level starts with the same capacity — a QUARTER of it in launches of more than 16 M pixels (batches of frames) —
// and is grown to what an overflowed frame reported (check_overflow): a frame can hold up to 3^L frames per pixel at level L in
// theory, a tenth of a frame per pixel in the reference's scenes. (Round 3: every level as large as level 0 was 80 GB per context
// with 32 frames of 1920 x 1080 in flight — a fourth context on one GPU ran out of memory; now 30 GB.)
int ensure_levels(RtuContext* ctx, uint32_t n_tiles, bool gi = false) {
    if (gi) ctx->want_gi = true;
    // one shard of level 0 receives the frames of every RTU_SHARDS-th 8x8 tile of the launch (ragged right /
    // bottom tiles included), so level 0 cannot overflow
    size_t tiles = n_tiles;
    size_t cap_s0 = ((tiles + RTU_SHARDS - 1) / RTU_SHARDS) * 64;
    size_t want[RTU_MAX_LEVELS];
    size_t maxcap = cap_s0;
    bool fits = ctx->level_nsl == ctx->nsl && (!ctx->textured || ctx->lv[0].fuv) && (!ctx->want_gi || ctx->lv[0].famb);
    const size_t cap_deep = cap_s0 * RTU_SHARDS > ((size_t)16 << 20) ? ((cap_s0 / 4 + 63) / 64) * 64 : cap_s0;
    for (int L = 0; L < RTU_MAX_LEVELS; L++) {
        want[L] = L == 0 ? cap_s0 : std::max<size_t>(cap_deep, ctx->want_cap_s[L]);
        if (want[L] > maxcap) maxcap = want[L];
        fits = fits && ctx->lv[L].cap_s >= want[L];
    }
    // defer list: at most every ray of the largest phase (all slots of the largest level)
    size_t dcap_s = maxcap * (ctx->nsl + 3);
    if (ctx->want_defer_s > dcap_s) dcap_s = ctx->want_defer_s;
    if (fits && ctx->defer_cap_s >= dcap_s && ctx->defer_list0 && ctx->defer_cap0_s >= cap_s0) return RTU_OK;
    // GROW ONLY: a caller that alternates launch shapes (a batch of 24 frames, then the last 8 of its run: the smaller one wants MORE at
    // the deep levels — it is below the quarter rule's 16 M pixels — and less at level 0) must not make the arrays swing between the two
    // (found as a 2.4 s stall per timed region: every launch freed and allocated 20 GB). Every capacity is the larger of what it was and
    // what is wanted now.
    size_t cap_s0_alloc = cap_s0 > ctx->defer_cap0_s ? cap_s0 : ctx->defer_cap0_s;
    for (int L = 0; L < RTU_MAX_LEVELS; L++) {
        if (ctx->lv[L].cap_s > want[L]) want[L] = ctx->lv[L].cap_s;
        if (want[L] > maxcap) maxcap = want[L];
    }
    if (maxcap * (ctx->nsl + 3) > dcap_s) dcap_s = maxcap * (ctx->nsl + 3);
    if (ctx->defer_cap_s > dcap_s) dcap_s = ctx->defer_cap_s;
    free_levels(ctx);
    int rc;
    size_t total = 0;
    for (int L = 0; L < RTU_MAX_LEVELS; L++) total += want[L] * RTU_SHARDS * (size_t)(16 * 11 + 4 * (ctx->nsl ? ctx->nsl : 1) + 12);
    if (total > ((size_t)160 << 30)) return fail(ctx, RTU_ERR_CAPACITY, "the recursion of this frame needs %zu GB of frame records", total >> 30);
    for (int L = 0; L < RTU_MAX_LEVELS; L++) {
        if (want[L] * RTU_SHARDS > 0x0FFFFFF0u) return fail(ctx, RTU_ERR_CAPACITY, "more than 2^28 frames in one recursion level");
        if ((rc = alloc_level_set(ctx, ctx->lv[L], want[L], ctx->want_gi)) != RTU_OK) return rc;
    }
    if ((rc = alloc_level(ctx, &ctx->defer_list, dcap_s * RTU_SHARDS)) != RTU_OK) return rc;
    ctx->defer_cap_s = (uint32_t)dcap_s;
    // the primary phase's own defer list (at most every pixel of the launch) and the side set of level arrays (rtu_device.h
    // KernelArgs::fcnt0): small — a k_tail launch refuses more than RTU_TAIL_DECLINE frames anyway
    if ((rc = alloc_level(ctx, &ctx->defer_list0, cap_s0_alloc * RTU_SHARDS)) != RTU_OK) return rc;
    ctx->defer_cap0_s = (uint32_t)cap_s0_alloc;
    for (int L = 0; L < RTU_MAX_LEVELS; L++)
        if ((rc = alloc_level_set(ctx, ctx->lv_side[L], 256, false)) != RTU_OK) return rc;
    ctx->level_nsl = ctx->nsl;
    return RTU_OK;
}

// One launch sequence: the whole frame of recipe W, or samples [sample_index, sample_index + batch) of
// recipe S into d_out as [sample][pixel of the shard].
// frames_batch: `batch` frames of recipe W with their own cameras (frame == &frames_batch[0]).
// gi_mode RTU_LAUNCH_CHAIN / RTU_LAUNCH_SHADE: one step of recipe P at chain depth gi_depth (render_sampled).
// adaptive: a launch of an adaptive frame (hint keys of its own: its shape changes every batch); act_list / act_n: the active-tile list
// its primary phase walks (KernelArgs::act_list), nullptr for every tile (act_n then only keys the hints).
// d_rays / n_rays: a RAY BATCH (rtu_shade_rays): the roots are the Shade() calls of n_rays caller-supplied rays in device memory, d_out has
// one float4 per ray; `frame` carries the eye (cam_pos), max_bounce and collect_stats (0 / 1) of a recipe-W frame and no camera. A
// "tile" is a chunk of 64 rays (k_ray_roots): no screen rectangles, coverage masks or tile occupancy, no side mode, hint keys of its own.
// d_keys: the ray batch is SAMPLED (rtu_shade_rays_sampled): `frame` is a recipe-S frame with samples = 1, d_keys[i] the key of ray i's root
// Shade() call; the pointer travels in KernelArgs::cam (ray_keys, render_impl.h), which a ray batch leaves idle.
// d_rays with d_keys and a gi_mode: one step of a PATH-TRACED ray batch (rtu_shade_rays_paths): chain i is ray i, gi_total = n_rays.
// RTU_LAUNCH_CHAIN at depth 0 traces the roots (render_rays4.hip / render_rays5.hip), at depth 1 .. 4 the gather rays; RTU_LAUNCH_SHADE
// is the frame path's own (k_gi_roots, the levels, k_gi_final), which knows chains and no pixels.
int launch(RtuContext* ctx, const RtuFrameDesc* frame, float4* d_out, hipStream_t stream, bool zero_counters, int sample_index = 0, int batch = 1,
           const RtuFrameDesc* frames_batch = nullptr, int gi_mode = RTU_LAUNCH_ALL, int gi_depth = 0, bool adaptive = false,
           const uint4* act_list = nullptr, uint32_t act_n = 0, const float4* d_rays = nullptr, uint32_t n_rays = 0, const uint32_t* d_keys = nullptr) {
    const bool rays = d_rays != nullptr;
    uint32_t tiles_x = (uint32_t)((frame->width + 7) / 8);
    uint32_t bands = (uint32_t)shard_bands(frame->height, frame->shard_rank, frame->shard_count);
    uint32_t n_tiles = rays ? (n_rays + 63u) / 64u : tiles_x * bands * (uint32_t)batch;
    uint32_t pixels = (uint32_t)rtu_shard_rows(frame) * (uint32_t)frame->width;
    const bool gi = gi_mode != RTU_LAUNCH_ALL;
    // recipe P: every chain hit is the root of two Shade() trees
    int rc = ensure_levels(ctx, gi ? 2u * (n_tiles + RTU_SHARDS) : n_tiles, gi);
    if (rc != RTU_OK) return rc;
    if (gi) {
        const size_t chains = rays ? (size_t)n_rays : (size_t)pixels * (size_t)batch;
        RTU_HIP(ctx, ctx->gi_h.grow(chains * (RTU_GI_BOUNCES + 1) * 4));
        RTU_HIP(ctx, ctx->gi_res.grow(chains * 2));
        // adaptive: the chains of stopped pixels are not traced; a zero depth-0 record is "no hit" to every later depth, k_gi_roots
        // and k_gi_final
        if (act_list && gi_mode == RTU_LAUNCH_CHAIN && gi_depth == 0)
            RTU_HIP(ctx, hipMemsetAsync(ctx->gi_h.get() + chains, 0, chains * sizeof(float4), stream));
    }
    const int stats = frame->collect_stats;  // 0 fast, 1 reference counting, 2 touched bytes of the fast variant
    if (stats && zero_counters) {
        RTU_HIP(ctx, hipMemsetAsync(ctx->counters.get(), 0, kCounterBytes, stream));
        memset(ctx->slot_launches, 0, sizeof ctx->slot_launches);
    }
    // the append counters start at zero; `overflow` is STICKY — launches only ever set it, check_overflow reads and clears
    // it — so that a frame that ran out of capacity is reported even when later launch sequences were queued behind it
    RTU_HIP(ctx, hipMemsetAsync(ctx->fcnt.get(), 0, offsetof(FrameCounters, overflow), stream));
    KernelArgs a;
    memset(&a, 0, sizeof a);
    a.scene = ctx->dscene;
    a.frame = *frame;
    if (!ctx->any_recursive_material) a.frame.max_bounce = 0;  // no reflection/refraction anywhere: Shade() never recurses
    a.out = d_out;
    memcpy(a.lv, ctx->lv, sizeof a.lv);
    a.fcnt = ctx->fcnt.get();
    a.tl = ctx->stamp_next ? ctx->tl.get() : nullptr;
    a.defer_list = ctx->defer_list;
    a.defer_cap_s = ctx->defer_cap_s;
    a.defer_list0 = ctx->defer_list0;
    a.defer_cap0_s = ctx->defer_cap0_s;
    a.fcnt0 = ctx->fcnt.get();
    a.dbg = ctx->dbg;
    a.scene.dbg = ctx->dbg;
    a.counters = stats ? ctx->counters.get() : nullptr;
    a.host_launches = stats == 2 ? ctx->slot_launches : nullptr;
    a.node_rects = (stats != 1 && frame->samples == 0 && ctx->dscene.node_bounds && !rays) ? ctx->node_rects : nullptr;  // (a ray has no pixel)
    if (a.node_rects && (ctx->dscene.n_cover + ctx->dscene.n_pcover) && !gi && ((size_t)((frame->width + 7) / 8) * (size_t)((frame->height + 7) / 8) + 31u) / 32u <= 12288u) {  // (the mask has to fit k_mesh_cover's LDS copy)
        a.tiles_xf = (uint32_t)((frame->width + 7) / 8);
        a.cover_words = (a.tiles_xf * (uint32_t)((frame->height + 7) / 8) + 31u) / 32u;
        a.cover_faces = ctx->cover_faces;
        const size_t need = (size_t)batch * (ctx->dscene.n_cover + ctx->dscene.n_pcover) * (1u + a.cover_words);
        if (need > ctx->cover.size()) {
            RTU_HIP(ctx, hipStreamSynchronize(stream));  // (first launch at this size only) nothing may still read the old masks
            RTU_HIP(ctx, ctx->cover.grow(need));
        }
        RTU_HIP(ctx, hipMemsetAsync(ctx->cover.get(), 0, need * sizeof(uint32_t), stream));
        a.cover = ctx->cover.get();
    }
    if (a.node_rects && !gi && ctx->dscene.n_nodes <= 64u && stats != 1 && !(ctx->dbg & 256u)) {  // tile occupancy: every word is written by k_tile_occ on this launch
        a.occ_words = ((tiles_x * bands + 63u) / 64u) * 2u;
        const size_t need = (size_t)batch * a.occ_words;
        if (need > ctx->occ.size()) {
            RTU_HIP(ctx, hipStreamSynchronize(stream));  // (first launch at this size only) nothing may still read the old words
            RTU_HIP(ctx, ctx->occ.grow(need));
        }
        a.occ = a.occ_words ? ctx->occ.get() : nullptr;  // (a shard without rows has no tiles: nothing is launched at all)
    }
    a.tiles_x = tiles_x;
    a.tiles_per_image = tiles_x * bands;
    a.nsl = ctx->nsl;
    a.n_meshes = ctx->n_meshes;
    // the cut level for k_tail: what a launch of the same shape showed last time (a hint: any value renders the same image, a
    // wrong one is refused on the device and reported like an overflow); rtu_debug_tail_from overrides it once
    // (adaptive frames: keys of their own — the fixed path's hints are not theirs — by the power of two of the tiles still sampling,
    // so that a batch learns from batches of about its size and the maps stay small)
    const uint32_t act_tiles = act_n ? act_n * (uint32_t)batch : n_tiles;
    const uint64_t tail_key = adaptive ? ((uint64_t)(32 - __builtin_clz(act_tiles | 1u)) << 8) | (uint64_t)(16 | 2 | (gi ? 8 : 0))
                                       : ((uint64_t)n_tiles << 8) | (uint64_t)((frame->samples ? 2 : 0) | (frames_batch ? 4 : 0) | (gi ? 8 : 0) | (rays ? 32 : 0));  // (32: a ray batch and a frame of as many tiles teach each other nothing; a sampled ray batch has 2 | 32: neither a sampled frame's hints nor an unsampled batch's)
    int hint = RTU_MAX_LEVELS;
    bool forced = false;
    if (ctx->tail_hint != 0) { hint = ctx->tail_hint; ctx->tail_hint = 0; forced = true; }
    else if (ctx->tail_hints.count(tail_key)) hint = ctx->tail_hints[tail_key];
    a.tail_from = stats == 1 ? RTU_MAX_LEVELS : hint;
    ctx->last_tail_key = tail_key;
    // (not for recipe P: its chain and shading launches share one shape and have lists of very different lengths)
    if (stats == 0 && !gi && !(ctx->dbg & 512u) && ctx->list_hints.count(tail_key)) memcpy(a.list_n, ctx->list_hints[tail_key].data(), sizeof a.list_n);
    if (forced) a.dbg |= 128u;  // a cut level set by the test hook is taken as it is (k_tail does not refuse it)
    if (frame->samples >= 1) {
        const float pixelIncrement = (float)(1.0 / frame->samples);  // RenderFunctions.cpp:68
        a.sampling = 1;
        a.sample_index = (uint32_t)sample_index;
        a.batch = (uint32_t)batch;
        a.batch_pixels = pixels;
        a.tiles_per_image = tiles_x * bands;
        for (int b = 0; b < batch; b++) {
            const int index = sample_index + b;
            const float currentOffset = (float)index * pixelIncrement;  // :80
            a.pix_off_x[b] = currentOffset + halton(index, 4);          // :84, :96
            a.pix_off_y[b] = currentOffset + halton(index, 5);          // :85, :96
        }
    }
    if (frames_batch) {
        a.frame_batch = 1;
        a.batch = (uint32_t)batch;
        a.batch_pixels = pixels;
        a.tiles_per_image = tiles_x * bands;
        if (!ctx->d_cams.get()) {
            RTU_HIP(ctx, ctx->d_cams.grow(RTU_MAX_FRAME_BATCH));
            RTU_HIP(ctx, ctx->h_cams.grow((size_t)RTU_MAX_FRAME_BATCH * RtuContext::kCamSlots));
            for (hipEvent_t& e : ctx->cam_ev) RTU_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        const int slot = ctx->cam_slot;
        ctx->cam_slot = (slot + 1) % RtuContext::kCamSlots;
        RTU_HIP(ctx, hipEventSynchronize(ctx->cam_ev[slot]));  // the copy that last read this slot (16 launches ago) is done; a fresh event is "done"
        BatchCam* hc = ctx->h_cams.get() + (size_t)slot * RTU_MAX_FRAME_BATCH;
        for (int b = 0; b < batch; b++) {
            memcpy(hc[b].pos, frames_batch[b].cam_pos, sizeof hc[b].pos);
            memcpy(hc[b].origin, frames_batch[b].origin, sizeof hc[b].origin);
            memcpy(hc[b].u, frames_batch[b].u, sizeof hc[b].u);
            memcpy(hc[b].v, frames_batch[b].v, sizeof hc[b].v);
        }
        RTU_HIP(ctx, hipMemcpyAsync(ctx->d_cams.get(), hc, sizeof(BatchCam) * (size_t)batch, hipMemcpyHostToDevice, stream));
        RTU_HIP(ctx, hipEventRecord(ctx->cam_ev[slot], stream));
        a.cam = ctx->d_cams.get();
    }
    if (d_keys) a.cam = reinterpret_cast<const BatchCam*>(d_keys);  // (ray_keys: no batch of frames here — frames_batch is NULL —, so nothing reads it as cameras)
    if (gi) {
        a.gi_h = ctx->gi_h.get();
        a.gi_res = ctx->gi_res.get();
        a.gi_depth = (uint32_t)gi_depth;
        a.gi_total = rays ? n_rays : pixels * (uint32_t)batch;
    }
    const uint32_t launch_tiles = act_list ? act_n * (uint32_t)batch : n_tiles;
    a.act_list = act_list;
    a.act_n = act_n;
    // side mode (rtu_device.h KernelArgs::fcnt0): recipe W's fast variant on a scene with meshes, unless this launch shape has shown that
    // its stage 2 makes more frames than a k_tail launch takes (rtu_debug_flags 8192: never — results must not change)
    // Only where it pays and cannot surprise: every mesh node's material is childless (stage 2's frames are then the rare hits whose
    // shadow rays could not be settled inline — a mirror teapot would send every hit through the k_tail launch), and the last launch of
    // this shape deferred enough primary rays for the one-lane-per-ray stage 2 (a first launch, or a short list: the old order).
    ctx->last_side = false;
    const uint32_t thr0 = (uint32_t)(frame->coop_threshold > 0 ? frame->coop_threshold : 70000);
    if (stats != 1 && !gi && !rays && frame->samples == 0 && ctx->n_meshes > 0 && ctx->mesh_hits_childless && !ctx->stamp_next && !(ctx->dbg & (8192u | 2048u | 64u)) &&
        ctx->dscene.node_bounds && ctx->dscene.lmask &&  // (the occluder lists are what settles a mesh hit's shadow rays inline)
        !ctx->side_off.count(tail_key) && ctx->list_hints.count(tail_key) && ctx->list_hints[tail_key][0] - 1u > thr0 &&
        ctx->side_frames.count(tail_key) && ctx->side_frames[tail_key] <= 256u) {
        if (!ctx->aux_stream) {
            // created at first use: the helper stream of side mode, lowest priority. (A context that never uses side mode creates no stream
            // for it: HIP deals its hardware queues out in creation order — four by default, GPU_MAX_HW_QUEUES —, and a stream too many makes
            // two streams that are meant to overlap share a queue: two contexts alternating, 56.8 -> 47.5 Grays/s, measured.)
            int prio_least = 0, prio_greatest = 0;
            RTU_HIP(ctx, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
            RTU_HIP(ctx, hipStreamCreateWithPriority(&ctx->aux_stream, hipStreamNonBlocking, prio_least));
            RTU_HIP(ctx, hipEventCreateWithFlags(&ctx->aux_ev0, hipEventDisableTiming));
            RTU_HIP(ctx, hipEventCreateWithFlags(&ctx->aux_ev1, hipEventDisableTiming));
        }
        a.side = 1;
        a.fcnt0 = ctx->fcnt_side.get();
        memcpy(a.lv_side, ctx->lv_side, sizeof a.lv_side);
        a.aux_stream = ctx->aux_stream;
        a.aux_ev0 = ctx->aux_ev0;
        a.aux_ev1 = ctx->aux_ev1;
        RTU_HIP(ctx, hipMemsetAsync(ctx->fcnt_side.get(), 0, offsetof(FrameCounters, overflow), stream));  // (ahead of k_primary, which fills its defer counters)
        ctx->last_side = true;
    }
    // k_primary's grid (render_impl.h launch_all): few, long-lived workgroups when the last launch of this shape found most tiles empty
    a.pgrid = 32768u;
    if (a.occ && !(ctx->dbg & 512u) && ctx->occ_hints.count(tail_key) && (uint64_t)ctx->occ_hints[tail_key] * 3u < (uint64_t)n_tiles)
        // (alone: four rounds of resident wavefronts balance themselves; beside another sequence — rtu_set_sequences_in_flight —: ONE resident
        // set, which the other sequence's kernels fill in around. Two sequences in flight: 2048 / 1536 / 1024 / 768 workgroups: 59.4 / 61.4 /
        // 62.5 / 61.4 Grays/s; three: 60 - 61 whatever the grid.)
        a.pgrid = ctx->sequences_in_flight >= 2 ? 1024u : 4096u;
    ctx->last_tail_from = a.tail_from;
    ctx->last_stats = stats == 1;
    memcpy(a.shadow_light, ctx->shadow_light, sizeof a.shadow_light);
    memcpy(a.nol_light, ctx->nol_light, sizeof a.nol_light);
    int probe_recorded = 0;
    LaunchProbe probe{-1, nullptr, nullptr, &probe_recorded};
    const bool probing = ctx->probe_slot >= 0 && ctx->probe_used < RtuContext::kProbePairs;
    if (probing) {
        probe.slot = ctx->probe_slot;
        probe.ev0 = ctx->probe_ev[2 * ctx->probe_used];
        probe.ev1 = ctx->probe_ev[2 * ctx->probe_used + 1];
    }
    if (gi_mode == RTU_LAUNCH_SHADE && gi_depth == 0) {
        hipError_t e0 = (hipError_t)rtu_launch_frame(a, launch_tiles, ctx->bvh_stack_needed, stats, stream, gi_mode, probing ? &probe : nullptr);
        if (probing && probe_recorded) ctx->probe_used++;
        if (e0 != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e0));
        e0 = (hipError_t)rtu_launch_gi_final(a, stream);  // harmless if this step has to be repeated: it only reads the results
        if (e0 != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e0));
        return RTU_OK;
    }
    hipError_t e = (rays && gi_mode == RTU_LAUNCH_CHAIN) ? (hipError_t)rtu_launch_ray_batch_chain(a, d_rays, ctx->bvh_stack_needed, stats == 1, stream)
                 : (rays && !gi) ? (d_keys ? (hipError_t)rtu_launch_ray_batch_sampled(a, d_rays, n_rays, ctx->bvh_stack_needed, stats == 1, stream, probing ? &probe : nullptr)
                                           : (hipError_t)rtu_launch_ray_batch(a, d_rays, n_rays, ctx->bvh_stack_needed, stats == 1, stream, probing ? &probe : nullptr))
                                 : (hipError_t)rtu_launch_frame(a, launch_tiles, ctx->bvh_stack_needed, stats, stream, gi_mode, probing ? &probe : nullptr);
    if (probing && probe_recorded) ctx->probe_used++;
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

// After the stream has drained: did any recursion level run out of frame capacity?
// Frames per level of the frame just finished -> where k_tail may take over in the next one.
uint64_t stage2_total(const FrameCounters& h) {
    uint64_t n = 0;
    for (int s = 0; s < RTU_SHARDS; s++) n += h.stage2_frames[s * RTU_CSTRIDE];
    return n;
}

void learn_tail(RtuContext* ctx, const FrameCounters& h, const FrameCounters* side) {
    static const uint32_t kTailEnv = [] { const char* e = getenv("RTU_TAIL_LEARN"); return e ? (uint32_t)strtoul(e, nullptr, 10) : 0u; }();  // tuning knob
    const uint32_t kTailMax = kTailEnv ? kTailEnv : RTU_TAIL_LEARN;  // frames of the cut level, one wavefront each: measured, a few thousand subtrees evaluated
                                               // wavefront by wavefront are slower than their levels kernel by kernel
    uint32_t frames[RTU_MAX_LEVELS];
    for (int L = 0; L < RTU_MAX_LEVELS; L++) {
        frames[L] = 0;
        for (int s = 0; s < RTU_SHARDS; s++) frames[L] += h.n_frames[L][(s) * RTU_CSTRIDE];
    }
    const int used = ctx->last_tail_from;  // levels > used were not materialised: their counts are unknown (zero)
    const int top = used < RTU_MAX_LEVELS ? used : RTU_MAX_LEVELS - 1;
    int hint = RTU_MAX_LEVELS;
    for (int L = 1; L <= top; L++)
        if (frames[L] <= kTailMax) { hint = L; break; }
    // the launch had a tail and its cut level was not small after all: deeper counts are unknown, learn them from a launch without
    ctx->tail_hints[ctx->last_tail_key] = hint;
    // the rays deferred in every phase (+ 1): what the next launch of this shape sizes its idle stage-2 kernels by
    std::array<uint32_t, 8> lh{};
    for (int p = 0; p <= RTU_MAX_LEVELS && p < 8; p++) {
        uint64_t n = 0;
        const FrameCounters& from = (p == 0 && side) ? *side : h;  // (side mode: the primary phase counts in the side counters)
        for (int s = 0; s < RTU_SHARDS; s++) n += from.n_defer[p][(s) * RTU_CSTRIDE];
        lh[p] = (uint32_t)(n < 0xFFFFFFF0ull ? n : 0xFFFFFFF0ull) + 1u;
    }
    ctx->list_hints[ctx->last_tail_key] = lh;
}

// The append counters keep counting past the capacity, so an overflowed frame tells how much its
// first overflowing level really needs (deeper levels may need another round: their parents were
// dropped). Wanted capacities grow to the reported counts (+25 %, at least x2 for the level below).
int check_overflow(RtuContext* ctx, bool* overflow) {
    std::unique_ptr<FrameCounters> hp(new FrameCounters);  // a quarter of a megabyte: not on the stack
    FrameCounters& h = *hp;
    RTU_HIP(ctx, hipMemcpy(&h, ctx->fcnt.get(), sizeof h, hipMemcpyDeviceToHost));
    // side mode: stage 2 of the primary phase made more frames than its k_tail launch takes (or than the side arrays hold): the
    // frames of this report are incomplete, and this launch shape goes without side mode from now on
    std::unique_ptr<FrameCounters> sp;
    bool side_failed = false;
    {
        uint32_t flags[2] = {0, 0};
        RTU_HIP(ctx, hipMemcpy(flags, &ctx->fcnt_side.get()->overflow, sizeof flags, hipMemcpyDeviceToHost));
        if (flags[0] || flags[1]) {
            side_failed = true;
            ctx->side_off[ctx->last_tail_key] = true;
            RTU_HIP(ctx, hipMemset(&ctx->fcnt_side.get()->overflow, 0, 2 * sizeof(uint32_t)));
        }
        if (ctx->last_side) {
            sp.reset(new FrameCounters);
            RTU_HIP(ctx, hipMemcpy(sp.get(), ctx->fcnt_side.get(), sizeof(FrameCounters), hipMemcpyDeviceToHost));
            ctx->side_frames[ctx->last_tail_key] = stage2_total(*sp);
            static const bool kSideVerbose = getenv("RTU_SIDE_VERBOSE") != nullptr;  // diagnostics: what side mode's stage 2 made, per status check
            if (kSideVerbose) {
                unsigned long long f[RTU_MAX_LEVELS] = {}, d0 = 0;
                for (int L = 0; L < RTU_MAX_LEVELS; L++)
                    for (int s = 0; s < RTU_SHARDS; s++) f[L] += sp->n_frames[L][s * RTU_CSTRIDE];
                for (int s = 0; s < RTU_SHARDS; s++) d0 += sp->n_defer[0][s * RTU_CSTRIDE];
                fprintf(stderr, "[side] deferred pixels %llu, side frames per level %llu %llu %llu %llu %llu %llu, failed %d\n", d0, f[0], f[1], f[2], f[3], f[4], f[5], (int)side_failed);
            }
        }
    }
    {
        uint64_t occ = 0;
        for (int s = 0; s < RTU_SHARDS; s++) occ += h.occ_tiles[s * RTU_CSTRIDE];
        if (!ctx->last_stats) ctx->occ_hints[ctx->last_tail_key] = (uint32_t)(occ < 0xFFFFFFFFull ? occ : 0xFFFFFFFFull);
    }
    if (!ctx->last_side && !ctx->last_stats) ctx->side_frames[ctx->last_tail_key] = stage2_total(h);  // (the fast variant without side mode: counted in the main counters)
    *overflow = h.overflow != 0 || h.tail_declined != 0 || side_failed;
    if (!*overflow) {
        learn_tail(ctx, h, sp.get());
        return RTU_OK;
    }
    RTU_HIP(ctx, hipMemset(&ctx->fcnt.get()->overflow, 0, 2 * sizeof(uint32_t)));  // reported: the next status starts clean (overflow, tail_declined)
    if (h.tail_declined) ctx->tail_hints[ctx->last_tail_key] = RTU_MAX_LEVELS;  // this shape is rendered level by level from now on
    if (!h.overflow) return RTU_OK;  // nothing ran out of capacity: render again, that is all
    bool grew = false;
    for (int L = 1; L < RTU_MAX_LEVELS; L++) {
        uint32_t need = 0;
        for (int s = 0; s < RTU_SHARDS; s++) need = h.n_frames[L][(s) * RTU_CSTRIDE] > need ? h.n_frames[L][(s) * RTU_CSTRIDE] : need;
        if (need > ctx->lv[L].cap_s) {
            size_t w = ((size_t)need + need / 4 + 63) / 64 * 64;
            if (w > ctx->want_cap_s[L]) ctx->want_cap_s[L] = (uint32_t)w;
            // its children were not all created: start the next level at least as large
            if (L + 1 < RTU_MAX_LEVELS && ctx->want_cap_s[L + 1] < w && ctx->lv[L + 1].cap_s < w) ctx->want_cap_s[L + 1] = (uint32_t)w;
            grew = true;
        }
    }
    uint32_t dneed = 0;
    for (int p = 0; p <= RTU_MAX_LEVELS; p++)
        for (int s = 0; s < RTU_SHARDS; s++) dneed = h.n_defer[p][(s) * RTU_CSTRIDE] > dneed ? h.n_defer[p][(s) * RTU_CSTRIDE] : dneed;
    if (dneed > ctx->defer_cap_s) {
        ctx->want_defer_s = dneed + dneed / 4;
        grew = true;
    }
    if (!grew) {  // the overflow was an EARLIER launch sequence's (the counts are the last one's): grow every level
        for (int L = 1; L < RTU_MAX_LEVELS; L++) ctx->want_cap_s[L] = ctx->lv[L].cap_s * 2;
    }
    return RTU_OK;
}

// What render_sampled does besides the fixed-count mean of frame->samples samples.
struct SampledRun {
    const RtuAdaptiveDesc* ad = nullptr;  // adaptive sampling (validated): stop every pixel at its first checkpoint that passes
    uint8_t* d_counts = nullptr;          // ... and write its count here (may be nullptr)
    float*   h_dump = nullptr;            // rtu_debug_sample_images: copy the images of samples [first, end) here, accumulate nothing
    int      first = 0, end = 0;
};

// The running sums a run of batches adds to — the context's own (render_sampled) or a progressive session's (rtu_progressive_*) —
// and, adaptive, where the run stands: the active-tile lists, the one the next batch walks (cur) and its length (n_act).
struct SampleSums {
    float4*   acc = nullptr;
    uint32_t* hits = nullptr;
    float4*   sq = nullptr;        // adaptive only, from here on
    uint8_t*  counts = nullptr;
    uint4*    list[2] = {nullptr, nullptr};
    uint32_t* n_dev = nullptr;     // [2] on the device
    uint32_t* n_host = nullptr;    // pinned
    int       cur = 0;
    uint32_t  n_act = 0;
};

int ensure_adaptive(RtuContext* ctx, size_t pixels, size_t tiles) {  // grow-only, like acc
    RTU_HIP(ctx, ctx->ad_sq.grow(pixels));
    RTU_HIP(ctx, ctx->ad_counts.grow(pixels));
    for (DevBuf<uint4>& l : ctx->ad_list) RTU_HIP(ctx, l.grow(tiles));
    RTU_HIP(ctx, ctx->ad_n.grow(2));
    RTU_HIP(ctx, ctx->ad_n_host.grow(1));
    return RTU_OK;
}

// Samples per launch sequence of a recipe S / P frame: as many as fit 2^25 pixels, at most RTU_MAX_BATCH (and max_batch, adaptive).
int sampled_batch(const RtuFrameDesc* frame, const RtuAdaptiveDesc* ad, size_t pixels) {
    static const int kGiLog2 = [] { const char* e = getenv("RTU_GI_BATCH_LOG2"); return e ? atoi(e) : 25; }();  // tuning knob (23 / 24 / 25: 138.2 / 131.9 / 130.6 ms for config 5 at 64 spp)
    const bool gi = frame->gather_bounces != 0;
    int batch = (int)(((size_t)1 << (gi ? kGiLog2 : 25)) / pixels);  // recipe P keeps 22 float4 per chain and two roots per chain hit (a larger batch buys nothing: measured)
    if (batch > RTU_MAX_BATCH) batch = RTU_MAX_BATCH;
    if (ad && ad->max_batch > 0 && batch > ad->max_batch) batch = ad->max_batch;
    if (batch > frame->samples) batch = frame->samples;
    if (batch < 1) batch = 1;
    return batch;
}

// The batch loop of recipes S / P: samples [i_begin, i_end) in batches of `batch`, one launch sequence each, each checked for
// frame-capacity overflow before its images are added to `sums` in sample order. Synchronises per batch. *reached: the end of the
// last batch added (i_end once an adaptive run's list is empty). The cancel word is polled before every batch.
// Adaptive (run->ad): the primary phase of a batch walks the list of tiles that still have a pixel sampling; k_adaptive_step,
// queued behind the batch and ahead of the batch's synchronisation, adds the samples of those pixels up to their stop and writes
// the next list, whose length the host reads in that same synchronisation. A batch that has to be rendered again (capacity) is
// not added (the step kernel sees the overflow flags the host will see).
int sample_batches(RtuContext* ctx, const RtuFrameDesc* frame, hipStream_t stream, bool zero_counters, const SampledRun* run, SampleSums& sums,
                   int i_begin, int i_end, int batch, int* reached) {
    const size_t pixels = (size_t)rtu_shard_rows(frame) * (size_t)frame->width;
    const bool gi = frame->gather_bounces != 0;
    const RtuAdaptiveDesc* ad = run ? run->ad : nullptr;
    float* const h_dump = run ? run->h_dump : nullptr;
    const uint32_t tiles_x = (uint32_t)((frame->width + 7) / 8);
    const uint32_t tiles = tiles_x * (uint32_t)shard_bands(frame->height, frame->shard_rank, frame->shard_count);
    int& cur = sums.cur;          // adaptive: the list the next batch walks ...
    uint32_t& n_act = sums.n_act; // ... and its length
    *reached = i_begin;
    auto adaptive_start = [&]() -> int {  // (again after the counting variant starts over)
        cur = 0;
        n_act = tiles;
        hipError_t e = (hipError_t)rtu_launch_adaptive_init(sums.list[0], tiles, tiles_x, frame->width, frame->height, frame->shard_rank, frame->shard_count, stream);
        return e == hipSuccess ? RTU_OK : fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    };
    auto adaptive_step = [&](int i, int nb) -> int {
        RTU_HIP(ctx, hipMemsetAsync(sums.n_dev + (cur ^ 1), 0, sizeof(uint32_t), stream));
        AdaptiveStep p;
        p.samples = ctx->sample_buf.get();
        p.acc = sums.acc;
        p.sq = sums.sq;
        p.hits = sums.hits;
        p.counts = sums.counts;
        p.list_in = sums.list[cur];
        p.list_out = sums.list[cur ^ 1];
        p.n_out = sums.n_dev + (cur ^ 1);
        p.skip_if = &ctx->fcnt.get()->overflow;
        p.skip_if_side = &ctx->fcnt_side.get()->overflow;
        p.n_in = n_act;
        p.batch = (uint32_t)nb;
        p.first = i == 0 ? 1u : 0u;
        p.pixels = (uint32_t)pixels;
        p.width = frame->width;
        p.height = frame->height;
        p.shard_rank = frame->shard_rank;
        p.shard_count = frame->shard_count;
        p.tiles_x = tiles_x;
        p.min_samples = (uint32_t)ad->min_samples;
        p.increment = (uint32_t)ad->increment;
        p.max_samples = (uint32_t)frame->samples;
        p.target = ad->target_variance;
        hipError_t e = (hipError_t)rtu_launch_adaptive_step(p, stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
        RTU_HIP(ctx, hipMemcpyAsync(sums.n_host, sums.n_dev + (cur ^ 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        return RTU_OK;
    };
    const uint4* no_list = nullptr;
    int rounds = 0;
    for (int i = i_begin; i < i_end; i += batch) {
        *reached = i;
        if (cancel_raised(ctx)) return fail(ctx, RTU_ERR_CANCELLED, "cancelled after %d of %d samples", i, frame->samples);  // StopRender(), main.cpp:70-72
        int nb = i_end - i < batch ? i_end - i : batch;
        while (!gi) {
            nb = i_end - i < batch ? i_end - i : batch;  // (i may have been reset below)
            int rc;
            if (ad && i == 0 && (rc = adaptive_start()) != RTU_OK) return rc;
            rc = launch(ctx, frame, ctx->sample_buf.get(), stream, zero_counters && i == 0, i, nb, nullptr, RTU_LAUNCH_ALL, 0, ad != nullptr, ad ? sums.list[cur] : no_list, n_act);
            if (rc != RTU_OK) return rc;
            if (ad && (rc = adaptive_step(i, nb)) != RTU_OK) return rc;
            RTU_HIP(ctx, hipStreamSynchronize(stream));
            bool overflow = false;
            if ((rc = check_overflow(ctx, &overflow)) != RTU_OK) return rc;
            if (!overflow) break;
            if (++rounds > 4 * RTU_MAX_LEVELS) return fail(ctx, RTU_ERR_CAPACITY, "recursion frames still exceed the capacity after %d rounds", rounds);
            if (frame->collect_stats) { i = 0; zero_counters = true; }  // the counters of the dropped pass are in the totals: start again
        }
        if (gi) {
            int rc;
            if (ad && i == 0 && (rc = adaptive_start()) != RTU_OK) return rc;
            // recipe P: the chain of gather rays first (depth 0 = the primary ray), then the Shade() trees from the
            // deepest hit up — each depth's AmbientLight needs the results of the depth below (k_gi_roots)
            // (adaptive: depth 0 walks the active tiles; the deeper depths run over every chain, a stopped one ends at once)
            for (int k = 0; k <= RTU_GI_BOUNCES; k++) {
                rc = launch(ctx, frame, ctx->sample_buf.get(), stream, zero_counters && i == 0 && k == 0, i, nb, nullptr, RTU_LAUNCH_CHAIN, k, ad != nullptr,
                            ad && k == 0 ? sums.list[cur] : no_list, ad ? n_act : 0u);
                if (rc != RTU_OK) return rc;
            }
            // the five shading steps are queued back to back; ONE host synchronisation per batch reads the (sticky) overflow
            // report of all of them. A batch that ran out of frame records is shaded again from the deepest depth with the
            // grown capacities: its chain records do not depend on them.
            for (;;) {
                for (int k = RTU_GI_BOUNCES; k >= 0; k--) {
                    rc = launch(ctx, frame, ctx->sample_buf.get(), stream, false, i, nb, nullptr, RTU_LAUNCH_SHADE, k, ad != nullptr, no_list, ad ? n_act : 0u);
                    if (rc != RTU_OK) return rc;
                }
                if (ad && (rc = adaptive_step(i, nb)) != RTU_OK) return rc;
                RTU_HIP(ctx, hipStreamSynchronize(stream));
                bool overflow = false;
                rc = check_overflow(ctx, &overflow);
                if (rc != RTU_OK) return rc;
                if (!overflow) break;
                if (frame->collect_stats) return fail(ctx, RTU_ERR_CAPACITY, "recipe P with counters: frame records ran out; render once without counters first");
                if (++rounds > 8 * RTU_MAX_LEVELS) return fail(ctx, RTU_ERR_CAPACITY, "recursion frames still exceed the capacity after %d rounds", rounds);
            }
        }
        if (ad) {
            cur ^= 1;
            n_act = *sums.n_host;  // (read in the batch's synchronisation)
            *reached = i + nb;
            if (n_act == 0) break;    // every pixel has stopped
            continue;
        }
        if (h_dump) {
            RTU_HIP(ctx, hipMemcpyAsync(h_dump + (size_t)(i - i_begin) * pixels * 4u, ctx->sample_buf.get(), (size_t)nb * pixels * sizeof(float4), hipMemcpyDeviceToHost, stream));
            RTU_HIP(ctx, hipStreamSynchronize(stream));
            *reached = i + nb;
            continue;
        }
        hipError_t e = (hipError_t)rtu_launch_accumulate(ctx->sample_buf.get(), (uint32_t)nb, sums.acc, sums.hits, (uint32_t)pixels, i == 0, stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
        *reached = i + nb;
    }
    *reached = i_end;
    return RTU_OK;
}

// Recipe S / P in one call: the batch loop on the context's own accumulators, then the mean to d_out.
int render_sampled(RtuContext* ctx, const RtuFrameDesc* frame, float4* d_out, hipStream_t stream, bool zero_counters, const SampledRun* run = nullptr) {
    const size_t pixels = (size_t)rtu_shard_rows(frame) * (size_t)frame->width;
    if (pixels == 0) return RTU_OK;
    const RtuAdaptiveDesc* ad = run ? run->ad : nullptr;
    float* const h_dump = run ? run->h_dump : nullptr;
    const int batch = sampled_batch(frame, ad, pixels);
    RTU_HIP(ctx, ctx->acc.grow(pixels));
    RTU_HIP(ctx, ctx->acc_hits.grow(pixels));
    RTU_HIP(ctx, ctx->sample_buf.grow(pixels * (size_t)batch));
    const uint32_t tiles_x = (uint32_t)((frame->width + 7) / 8);
    const uint32_t tiles = tiles_x * (uint32_t)shard_bands(frame->height, frame->shard_rank, frame->shard_count);
    SampleSums sums;
    sums.acc = ctx->acc.get();
    sums.hits = ctx->acc_hits.get();
    if (ad) {
        int rc = ensure_adaptive(ctx, pixels, tiles);
        if (rc != RTU_OK) return rc;
        sums.sq = ctx->ad_sq.get();
        sums.counts = ctx->ad_counts.get();
        sums.list[0] = ctx->ad_list[0].get();
        sums.list[1] = ctx->ad_list[1].get();
        sums.n_dev = ctx->ad_n.get();
        sums.n_host = ctx->ad_n_host.get();
    }
    int reached = 0;
    int rc = sample_batches(ctx, frame, stream, zero_counters, run, sums, h_dump ? run->first : 0, h_dump ? run->end : frame->samples, batch, &reached);
    if (rc != RTU_OK) return rc;
    if (h_dump) return RTU_OK;
    hipError_t e = ad ? (hipError_t)rtu_launch_resolve_counts(ctx->acc.get(), ctx->acc_hits.get(), ctx->ad_counts.get(), d_out, run->d_counts, (uint32_t)pixels, stream)
                      : (hipError_t)rtu_launch_resolve(ctx->acc.get(), ctx->acc_hits.get(), d_out, (uint32_t)pixels, (uint32_t)frame->samples, stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

}  // namespace

// The rules of RtuAdaptiveDesc for a maximum of `samples` per pixel (an adaptive frame, an adaptive sensor); ctx may be NULL
int check_adaptive_desc(RtuContext* ctx, const RtuAdaptiveDesc* ad, int samples) {
    if (!ad) return fail(ctx, RTU_ERR_ARG, "adaptive is NULL");
    if (ad->min_samples < 1 || ad->min_samples > samples) return fail(ctx, RTU_ERR_ARG, "min_samples is 1 .. frame.samples");
    if (ad->increment < 1) return fail(ctx, RTU_ERR_ARG, "increment is >= 1");
    if (!(ad->target_variance >= 0.0f)) return fail(ctx, RTU_ERR_ARG, "target_variance is >= 0 (or +inf)");
    if (ad->max_batch < 0 || ad->max_batch > RTU_MAX_BATCH) return fail(ctx, RTU_ERR_ARG, "max_batch is 0 .. %d", RTU_MAX_BATCH);
    return RTU_OK;
}

namespace {

// The arguments of an adaptive frame (rtu_render.h): a recipe S / P frame with 1 .. 255 samples and a valid RtuAdaptiveDesc.
int check_adaptive(RtuContext* ctx, const RtuFrameDesc* f, const RtuAdaptiveDesc* ad) {
    if (!f) return fail(ctx, RTU_ERR_ARG, "frame is NULL");
    if (f->samples < 1 || f->samples > 255) return fail(ctx, RTU_ERR_ARG, "an adaptive frame has 1 .. 255 samples per pixel at most (frame.samples)");
    int rc = check_frame(ctx, f);
    if (rc != RTU_OK) return rc;
    if ((rc = check_adaptive_desc(ctx, ad, f->samples)) != RTU_OK) return rc;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    return RTU_OK;
}

}  // namespace

// A progressive session (rtu_progressive_*): a recipe S / P frame whose running sums live from call to call. It owns them; the
// frame-record arrays and sample_buf it traces through are the context's scratch within one call.
struct RtuProgressive {
    RtuContext*     ctx = nullptr;    // nullptr once the context is destroyed
    RtuFrameDesc    frame{};
    bool            adaptive = false;
    RtuAdaptiveDesc ad{};
    uint64_t        scene_gen = 0;    // the context's scene generation at begin
    int32_t         done = 0;         // samples [0, done) are in the sums
    int             batch = 1;
    size_t          pixels = 0;
    uint32_t        tiles = 0;
    DevBuf<float4>   acc, sq;
    DevBuf<uint32_t> hits;
    DevBuf<uint8_t>  counts;
    DevBuf<uint4>    list[2];
    DevBuf<uint32_t> n_dev;
    PinnedBuf<uint32_t> n_host;
    SampleSums      sums;
    DevBuf<float4>   ft_hits, ft_albedo;  // rtu_progressive_snapshot_denoised: the first-hit features of the frame, made at the first such call
    bool            has_features = false;
};

static void progressive_release(RtuProgressive* p) {
    p->acc.reset();
    p->sq.reset();
    p->hits.reset();
    p->counts.reset();
    for (DevBuf<uint4>& l : p->list) l.reset();
    p->n_dev.reset();
    p->n_host.reset();
    p->ft_hits.reset();
    p->ft_albedo.reset();
    p->has_features = false;
    p->sums = SampleSums();
    p->ctx = nullptr;
}

extern "C" {

int rtu_device_info(int device_id, RtuDeviceInfo* out) {
    if (!out) return RTU_ERR_ARG;
    memset(out, 0, sizeof *out);
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device_id) != hipSuccess) return RTU_ERR_HIP;
    out->compute_units = p.multiProcessorCount;
    out->clock_khz = p.clockRate;
    out->memory_clock_khz = p.memoryClockRate;
    out->memory_bus_bits = p.memoryBusWidth;
    out->l2_bytes = (unsigned long long)p.l2CacheSize;
    out->hbm_bytes = (unsigned long long)p.totalGlobalMem;
    snprintf(out->name, sizeof out->name, "%s", p.name);
    snprintf(out->arch, sizeof out->arch, "%s", p.gcnArchName);
    return RTU_OK;
}

int rtu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* rtu_error_string(int err) {
    switch (err) {
        case RTU_OK: return "ok";
        case RTU_ERR_ARG: return "invalid argument";
        case RTU_ERR_HIP: return "HIP runtime error";
        case RTU_ERR_UNSUPPORTED: return "scene outside the device path's limits";
        case RTU_ERR_STOCHASTIC: return "scene uses a stochastic feature";
        case RTU_ERR_NO_SCENE: return "no scene uploaded";
        case RTU_ERR_NO_DEVICE: return "no such GPU";
        case RTU_ERR_CAPACITY: return "recursion frame capacity exceeded";
        case RTU_ERR_CANCELLED: return "cancelled";
        case RTU_ERR_SCENE_SHAPE: return "scene shape differs from the uploaded scene";
        case RTU_ERR_STALE: return "the session's context got a new scene";
    }
    return "unknown error";
}

RtuContext* rtu_create_context(int device_id, int* err_out) {
    int n = rtu_device_count();
    if (device_id < 0 || device_id >= n) {
        if (err_out) *err_out = RTU_ERR_NO_DEVICE;
        return nullptr;
    }
    RtuContext* ctx = new RtuContext;
    ctx->device = device_id;
    bool ok = hipSetDevice(device_id) == hipSuccess &&
              hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
              ctx->fcnt_side.grow(1) == hipSuccess && hipMemset(ctx->fcnt_side.get(), 0, sizeof(FrameCounters)) == hipSuccess &&
              hipEventCreate(&ctx->ev0) == hipSuccess && hipEventCreate(&ctx->ev1) == hipSuccess &&
              ctx->counters.grow(kCounterBytes / sizeof(unsigned long long)) == hipSuccess &&
              ctx->fcnt.grow(1) == hipSuccess &&
              hipMemset(ctx->fcnt.get(), 0, sizeof(FrameCounters)) == hipSuccess &&
              hipMemset(ctx->counters.get(), 0, kCounterBytes) == hipSuccess;
    if (!ok) {
        if (err_out) *err_out = RTU_ERR_HIP;
        rtu_destroy_context(ctx);
        return nullptr;
    }
    if (err_out) *err_out = RTU_OK;
    return ctx;
}

void rtu_destroy_context(RtuContext* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
    ll_builder_destroy(ctx->llb);
    rb_destroy(ctx->rb);
    for (RtuProgressive* p : ctx->sessions) progressive_release(p);  // the handles stay valid for rtu_progressive_free
    for (RtuTemporal* t : ctx->temporals) temporal_release(t);       // ... and for rtu_temporal_free
    // the buffers go with the context (DevBuf); its events and streams after them
    std::vector<hipEvent_t> events = {ctx->aux_ev0, ctx->aux_ev1, ctx->ev0, ctx->ev1};
    events.insert(events.end(), std::begin(ctx->cam_ev), std::end(ctx->cam_ev));
    events.insert(events.end(), std::begin(ctx->probe_ev), std::end(ctx->probe_ev));
    events.insert(events.end(), std::begin(ctx->mu_ev), std::end(ctx->mu_ev));
    events.insert(events.end(), std::begin(ctx->mud_ev), std::end(ctx->mud_ev));
    events.push_back(ctx->mud_wait);
    events.insert(events.end(), std::begin(ctx->sn_ev), std::end(ctx->sn_ev));
    const hipStream_t streams[] = {ctx->aux_stream, ctx->stream};
    delete ctx;
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : streams)
        if (s) (void)hipStreamDestroy(s);
}

const char* rtu_last_error(const RtuContext* ctx) { return ctx ? ctx->error.c_str() : "context is NULL"; }

int rtu_validate_scene(const RtuSceneDesc* s, char* err_buf, size_t err_len) {
    RtuContext tmp;  // plain host state: nothing here touches a GPU
    const int rc = validate(&tmp, s);
    if (err_buf && err_len) {
        snprintf(err_buf, err_len, "%s", tmp.error.c_str());
    }
    return rc;
}

}  // extern "C"

namespace {

// Everything that depends on where things are placed, on the lights or on the materials, into the placement buffers: nodes,
// node-level bounds, cover meshes, plane quads, occluder lists, materials, lights, and the host flags derived from them. Mesh and
// texture records of ctx->dscene stay. on_device: cover meshes and occluder lists from the meshes already in HBM
// (rtu_scene_update.hip; s->meshes is then read for its headers only); otherwise on the host from s->meshes.
int place_scene(RtuContext* ctx, const RtuSceneDesc* s, bool on_device) {
    int rc;
    // scene-graph nodes with their ancestor chains
    std::vector<DevNode> nodes(s->n_nodes);
    for (uint32_t i = 0; i < s->n_nodes; i++) {
        const RtuNode& n = s->nodes[i];
        DevNode& d = nodes[i];
        memset(&d, 0, sizeof d);
        memcpy(d.tm, n.tm, sizeof d.tm);
        memcpy(d.itm, n.itm, sizeof d.itm);
        memcpy(d.pos, n.pos, sizeof d.pos);
        d.parent = n.parent;
        d.obj_type = n.obj_type;
        d.mesh_id = n.mesh_id;
        d.material_id = n.material_id;
        d.depth = n.depth;
        int j = (int)i;
        for (int dd = n.depth; dd >= 0; dd--) {
            d.chain[dd] = j;
            j = s->nodes[j].parent;
        }
    }

    const float wscale = world_bounds(s, nodes);
    float sort_box[6];
    sort_box_of(nodes, wscale, sort_box);
    DevScene ds = ctx->dscene;
    if ((rc = place_upload(ctx, P_NODES, nodes.data(), nodes.size(), &ds.nodes)) != RTU_OK) return rc;
    if ((rc = place_upload(ctx, P_MATERIALS, s->materials, (size_t)s->n_materials, &ds.materials)) != RTU_OK) return rc;
    if ((rc = place_upload(ctx, P_LIGHTS, s->lights, (size_t)s->n_lights, &ds.lights)) != RTU_OK) return rc;
    // the world normals of the plane nodes (DevNode::plane_n), by the kernels' own code on the nodes just placed; a caller's stream
    // may read them next (ray queries)
    RTU_HIP(ctx, (hipError_t)rtu_launch_plane_normals(const_cast<DevNode*>(ds.nodes), s->n_nodes, ctx->stream));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ds.textured) {
        if (s->material_maps)
            if ((rc = place_upload(ctx, P_MATMAPS, s->material_maps, (size_t)s->n_materials * 4, &ds.mat_maps)) != RTU_OK) return rc;
        ds.bg_map = s->background_map;
        ds.env_map = s->environment_map;
    }
    ds.bg = s->background;
    ds.env = s->environment;
    ds.img_w = s->camera.img_width;
    ds.img_h = s->camera.img_height;
    ds.wscale = wscale;
    WorldFar far;
    world_far(s, wscale, far);
    ds.wnoise = far.wnoise;
    ds.wreach = far.wreach;
    ds.wsphere_k = far.sph_k;
    ds.wsphere_r = far.sph_r;
    ds.near_m0 = far.near_m0;
    ds.near_c1 = far.near_c1;
    ds.nol_ok = 1;
    for (uint32_t i = 0; i < s->n_lights; i++)
        for (int k = 0; k < 3; k++)
            if (!(std::fabs(s->lights[i].intensity[k]) < 1e15f)) ds.nol_ok = 0;
    ds.n_cover = 0;
    ctx->cover_faces = 0;
    std::vector<CoverMesh> cover_host;  // per masked mesh node: the world-space boxes and vertices of its triangles
    std::vector<LlCover> cover_dev;     // ... or where the device builder finds and puts them
    for (uint32_t i = 0; i < s->n_nodes && i < 64u; i++) {
        if (s->nodes[i].obj_type == RTU_OBJ_TRIMESH && ds.n_cover < RTU_MAX_COVER) {
            const uint32_t c = ds.n_cover++;
            const int mid = s->nodes[i].mesh_id;
            const uint32_t nf = s->meshes[mid].nf;
            ds.cover_node[c] = (int32_t)i;
            if (nf > ctx->cover_faces) ctx->cover_faces = nf;
            void* box = nullptr;
            if ((rc = ensure_place(ctx, P_COVER + (int)c, sizeof(float4) * 2 * (size_t)nf, &box)) != RTU_OK) return rc;
            ds.cover_box[c] = (const float4*)box;
            ds.cover_nf[c] = nf;
            if (on_device) {
                LlCover cv;
                cv.f = ctx->dmeshes[(size_t)mid].f;
                cv.v = ctx->dmeshes[(size_t)mid].v;
                cv.slot_of = ctx->slot_of[(size_t)mid];
                cv.nf = nf;
                cv.chain = node_chain(s, i);
                cv.boxes = (float4*)box;
                cover_dev.push_back(cv);
            } else {
                CoverMesh cm;
                make_cover_mesh(s, i, ctx->fast_elements[(size_t)mid], cm);
                RTU_HIP(ctx, hipMemcpy(box, cm.boxes.data(), sizeof(float4) * cm.boxes.size(), hipMemcpyHostToDevice));
                cover_host.push_back(std::move(cm));
            }
        }
    }
    std::vector<double> lohi(6 * (size_t)ds.n_cover + 6);
    if (on_device) RTU_HIP(ctx, ll_build_covers(ctx->llb, ctx->stream, cover_dev.data(), (int)cover_dev.size(), lohi.data()));
    // plane nodes with a coverage mask: the corners of the node's unit square in world space (k_plane_cover)
    ds.n_pcover = 0;
    for (uint32_t i = 0; i < s->n_nodes && i < 64u; i++) {
        if (s->nodes[i].obj_type != RTU_OBJ_PLANE || ds.n_pcover >= RTU_MAX_PCOVER) continue;
        static const double sq[4][2] = {{-1, -1}, {1, -1}, {1, 1}, {-1, 1}};
        float quad[4][3];
        bool finite = true;
        for (int c = 0; c < 4; c++) {
            double p[3] = {sq[c][0], sq[c][1], 0.0};
            for (int j = (int)i; j >= 0; j = s->nodes[j].parent) {
                const RtuNode& t = s->nodes[j];
                const double q[3] = {p[0] * t.tm[0] + p[1] * t.tm[3] + p[2] * t.tm[6] + t.pos[0], p[0] * t.tm[1] + p[1] * t.tm[4] + p[2] * t.tm[7] + t.pos[1],
                                     p[0] * t.tm[2] + p[1] * t.tm[5] + p[2] * t.tm[8] + t.pos[2]};
                p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
            }
            for (int k = 0; k < 3; k++) { quad[c][k] = (float)p[k]; finite = finite && std::isfinite(quad[c][k]); }
        }
        if (!finite) continue;  // NaN / infinite transformation: no mask (the node's rectangle is the whole image as well)
        ds.pcover_node[ds.n_pcover] = (int32_t)i;
        memcpy(ds.pcover_quad[ds.n_pcover], quad, sizeof quad);
        ds.n_pcover++;
    }
    ctx->light_list_info.clear();
    rc = on_device ? build_light_lists_device(ctx, s, cover_dev, lohi, far.wlist, ds) : build_light_lists(ctx, s, cover_host, far.wlist, ds);
    if (rc != RTU_OK) return rc;
    ds.obj_mask = 0;
    for (uint32_t i = 0; i < s->n_nodes && i < 64u; i++)
        if (s->nodes[i].obj_type != RTU_OBJ_NONE) ds.obj_mask |= 1ull << i;
    ds.n_lights = s->n_lights;
    env_value(s->background, ds.background);
    env_value(s->environment, ds.environment);
    ctx->dscene = ds;
    memcpy(ctx->sort_box, sort_box, sizeof sort_box);
    ctx->nsl = 0;
    for (uint32_t i = 0; i < s->n_lights; i++)
        if (s->lights[i].type != RTU_LIGHT_AMBIENT) {
            if (ctx->nsl < RTU_FI_NOL_LIGHTS) {
                for (int k = 0; k < 3; k++) ctx->nol_light[ctx->nsl][k] = s->lights[i].vec[k];
                ctx->nol_light[ctx->nsl][3] = s->lights[i].type == RTU_LIGHT_DIRECT ? 1.0f : 0.0f;
            }
            ctx->shadow_light[ctx->nsl++] = (int32_t)i;
        }
    memset(ctx->want_cap_s, 0, sizeof ctx->want_cap_s);
    ctx->want_defer_s = 0;
    ctx->tail_hint = 0;
    ctx->tail_hints.clear();
    ctx->list_hints.clear();
    ctx->mesh_hits_childless = true;
    for (uint32_t i = 0; i < s->n_nodes; i++) {
        const RtuNode& nd = s->nodes[i];
        if (nd.obj_type != RTU_OBJ_TRIMESH || nd.material_id < 0) continue;
        const RtuMaterial& mm = s->materials[nd.material_id];
        for (int k = 0; k < 3; k++)
            if (mm.reflection[k] != 0 || mm.refraction[k] != 0) ctx->mesh_hits_childless = false;
    }
    ctx->side_off.clear();
    ctx->side_frames.clear();
    ctx->occ_hints.clear();
    ctx->any_recursive_material = false;
    for (uint32_t i = 0; i < s->n_materials; i++) {
        const RtuMaterial& mm = s->materials[i];
        for (int k = 0; k < 3; k++)
            if (mm.reflection[k] != 0 || mm.refraction[k] != 0) ctx->any_recursive_material = true;
    }
    ctx->scene_stochastic = false;
    ctx->stochastic_what.clear();
    if (s->camera.dof != 0) { ctx->scene_stochastic = true; ctx->stochastic_what = "depth of field"; }
    for (uint32_t i = 0; i < s->n_lights && !ctx->scene_stochastic; i++)
        if (s->lights[i].type == RTU_LIGHT_POINT && s->lights[i].size > 0) { ctx->scene_stochastic = true; ctx->stochastic_what = "a soft shadow"; }
    for (uint32_t i = 0; i < s->n_materials && !ctx->scene_stochastic; i++)
        if (s->materials[i].reflection_glossiness > 0 || s->materials[i].refraction_glossiness > 0) { ctx->scene_stochastic = true; ctx->stochastic_what = "a glossy bounce"; }
    ctx->n_textures = s->n_textures;
    ctx->mat_maps_host.clear();
    if (s->n_textures > 0 && s->material_maps) ctx->mat_maps_host.assign(s->material_maps, s->material_maps + (size_t)s->n_materials * 4);
    return RTU_OK;
}

// what rtu_update_scene keeps fixed (rtu_render.h): "" or the first difference between the uploaded scene `a` and `b`
std::string shape_diff(const RtuSceneDesc* a, const RtuSceneDesc* b) {
    char buf[200];
    if (a->n_nodes != b->n_nodes) { snprintf(buf, sizeof buf, "n_nodes %u != %u", b->n_nodes, a->n_nodes); return buf; }
    for (uint32_t i = 0; i < a->n_nodes; i++) {
        const RtuNode &x = a->nodes[i], &y = b->nodes[i];
        const char* what = x.parent != y.parent ? "parent" : x.obj_type != y.obj_type ? "obj_type" : x.mesh_id != y.mesh_id ? "mesh_id"
                         : x.depth != y.depth ? "depth" : x.subtree_end != y.subtree_end ? "subtree_end" : nullptr;
        if (what) { snprintf(buf, sizeof buf, "node %u: %s differs", i, what); return buf; }
    }
    if (a->n_meshes != b->n_meshes) { snprintf(buf, sizeof buf, "n_meshes %u != %u", b->n_meshes, a->n_meshes); return buf; }
    for (uint32_t i = 0; i < a->n_meshes; i++) {
        const RtuMesh &x = a->meshes[i], &y = b->meshes[i];
        const char* what = x.nv != y.nv ? "nv" : x.nf != y.nf ? "nf" : x.nvn != y.nvn ? "nvn" : x.nvt != y.nvt ? "nvt"
                         : x.n_bvh_nodes != y.n_bvh_nodes ? "n_bvh_nodes" : nullptr;
        if (what) { snprintf(buf, sizeof buf, "mesh %u: %s differs", i, what); return buf; }
    }
    if (a->n_textures != b->n_textures) { snprintf(buf, sizeof buf, "n_textures %u != %u", b->n_textures, a->n_textures); return buf; }
    for (uint32_t i = 0; i < a->n_textures; i++) {
        const RtuTexture &x = a->textures[i], &y = b->textures[i];
        const char* what = x.type != y.type ? "type" : x.width != y.width ? "width" : x.height != y.height ? "height" : nullptr;
        if (what) { snprintf(buf, sizeof buf, "texture %u: %s differs", i, what); return buf; }
    }
    if (a->n_materials != b->n_materials) { snprintf(buf, sizeof buf, "n_materials %u != %u", b->n_materials, a->n_materials); return buf; }
    if ((a->material_maps != nullptr) != (b->material_maps != nullptr)) return "material_maps present in one scene only";
    return "";
}

// the arrays shape_diff reads must be there
int shape_args(RtuContext* ctx, const RtuSceneDesc* s) {
    if (!s || !s->nodes || s->n_nodes == 0) return fail(ctx, RTU_ERR_ARG, "scene has no nodes");
    if (s->n_meshes && !s->meshes) return fail(ctx, RTU_ERR_ARG, "meshes is NULL");
    if (s->n_textures && !s->textures) return fail(ctx, RTU_ERR_ARG, "textures is NULL");
    return RTU_OK;
}

// the uploaded scene's shape as a description (headers only)
RtuSceneDesc shape_desc(const RtuContext* ctx) {
    static const RtuTexMap present{};
    RtuSceneDesc d;
    memset(&d, 0, sizeof d);
    d.n_nodes = (uint32_t)ctx->shape_nodes.size();
    d.nodes = ctx->shape_nodes.data();
    d.n_meshes = (uint32_t)ctx->shape_meshes.size();
    d.meshes = ctx->shape_meshes.data();
    d.n_textures = (uint32_t)ctx->shape_textures.size();
    d.textures = ctx->shape_textures.data();
    d.n_materials = ctx->shape_materials;
    d.material_maps = ctx->shape_maps ? &present : nullptr;
    return d;
}

// The writing half of rtu_update_meshes, after every check has passed: for each listed mesh the new vertices, normals and `ref` tree
// go to HBM, and the kernels of rtu_mesh_update.hip rewrite what depends on the vertices — triangle records of both trees, the boxes
// of bvh4 / bvh8. Everything is enqueued on the context's stream and waited for at the end. new_shape: the headers the context
// remembers from now on.
int write_meshes(RtuContext* ctx, const RtuSceneDesc* s, const uint32_t* mesh_ids, int n_meshes, const std::vector<RtuMesh>& new_shape) {
    hipStream_t st = ctx->stream;
    const bool timing = ctx->mu_timing;
    if (timing && !ctx->mu_ev[0])
        for (hipEvent_t& e : ctx->mu_ev) RTU_HIP(ctx, hipEventCreate(&e));
    std::vector<std::vector<RtuBvhNode>> trees((size_t)n_meshes);  // host sources of asynchronous copies: alive until the wait below
    if (ctx->keep_prev) {
        // The replaced v and vn become the listed meshes' previous generation: the two grow-only buffers change places (the first such
        // update of a mesh allocates the second pair, later ones nothing), and the new arrays are written into what was the previous
        // one. For every other mesh "previous" is "current" again: previous means before THIS update only.
        ctx->prev_gen.resize(ctx->dmeshes.size());
        for (RtuContext::PrevGen& g : ctx->prev_gen) g.valid = false;
        for (int i = 0; i < n_meshes; i++) {
            const uint32_t id = mesh_ids[i];
            RtuContext::PrevGen& g = ctx->prev_gen[id];
            DevBuf<char>&v = ctx->scene_allocs[ctx->refit[id].v_alloc], &vn = ctx->scene_allocs[ctx->refit[id].vn_alloc];
            RTU_HIP(ctx, g.v.grow(v.size()));
            RTU_HIP(ctx, g.vn.grow(vn.size()));
            std::swap(g.v, v);
            std::swap(g.vn, vn);
            g.valid = true;
            ctx->dmeshes[id].v = reinterpret_cast<const float*>(v.get());
            ctx->dmeshes[id].vn = reinterpret_cast<const float*>(vn.get());
        }
    }
    ctx->df_dirty = true;
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->mu_ev[0], st));
    for (int i = 0; i < n_meshes; i++) {
        const uint32_t id = mesh_ids[i];
        const RtuMesh& m = s->meshes[id];
        DevMesh& d = ctx->dmeshes[id];
        renumber_bfs(m, trees[(size_t)i], d.any_empty_box);
        DevBuf<char>& tree_buf = ctx->scene_allocs[ctx->refit[id].ref_bvh_alloc];  // grow-only: a tree that fits makes no allocation
        RTU_HIP(ctx, tree_buf.grow(sizeof(RtuBvhNode) * (size_t)m.n_bvh_nodes));
        d.ref.bvh = reinterpret_cast<const float4*>(tree_buf.get());
        RTU_HIP(ctx, hipMemcpyAsync(tree_buf.get(), trees[(size_t)i].data(), sizeof(RtuBvhNode) * (size_t)m.n_bvh_nodes, hipMemcpyHostToDevice, st));
        RTU_HIP(ctx, hipMemcpyAsync(const_cast<uint32_t*>(d.ref.elements), m.elements, sizeof(uint32_t) * (size_t)m.n_elements, hipMemcpyHostToDevice, st));
        RTU_HIP(ctx, hipMemcpyAsync(const_cast<float*>(d.v), m.v, sizeof(float) * 3 * (size_t)m.nv, hipMemcpyHostToDevice, st));
        RTU_HIP(ctx, hipMemcpyAsync(const_cast<float*>(d.vn), m.vn, sizeof(float) * 3 * (size_t)m.nvn, hipMemcpyHostToDevice, st));
        d.scale = 0.0f;
        for (int k = 0; k < 3; k++) d.scale = fmaxf(d.scale, fmaxf(fabsf(m.bound_min[k]), fabsf(m.bound_max[k])));
        memcpy(d.bmin, m.bound_min, sizeof d.bmin);
        memcpy(d.bmax, m.bound_max, sizeof d.bmax);
        d.n_bvh_nodes = m.n_bvh_nodes;
        RTU_HIP(ctx, hipMemcpyAsync(const_cast<DevMesh*>(ctx->dscene.meshes) + id, &d, sizeof d, hipMemcpyHostToDevice, st));
    }
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->mu_ev[1], st));
    for (int i = 0; i < n_meshes; i++) {
        const DevMesh& d = ctx->dmeshes[mesh_ids[i]];
        RTU_HIP(ctx, mu_tri_records(st, d.f, d.v, d.ref.elements, d.n_elements, const_cast<float4*>(d.ref.tri)));
        RTU_HIP(ctx, mu_tri_records(st, d.f, d.v, d.fast.elements, d.n_elements, const_cast<float4*>(d.fast.tri)));
    }
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->mu_ev[2], st));
    for (int i = 0; i < n_meshes; i++) {
        const uint32_t id = mesh_ids[i];
        const DevMesh& d = ctx->dmeshes[id];
        const RtuContext::MeshRefit& r = ctx->refit[id];
        RTU_HIP(ctx, mu_refit(st, 4, const_cast<float4*>(d.bvh4), ctx->mesh_info[id].nodes4, r.lvl4.data(), (uint32_t)r.lvl4.size() - 1u, d.f, d.v,
                              d.fast.elements, d.n_elements));
        RTU_HIP(ctx, mu_refit(st, 8, const_cast<float4*>(d.bvh8), ctx->mesh_info[id].nodes8, r.lvl8.data(), (uint32_t)r.lvl8.size() - 1u, d.f, d.v,
                              d.fast.elements, d.n_elements));
    }
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->mu_ev[3], st));
    RTU_HIP(ctx, hipStreamSynchronize(st));
    // the `ref` trees' depths changed: the stack the walks need (what rtu_upload_scene computes, from the numbers it kept)
    ctx->shape_meshes = new_shape;
    uint32_t stack_needed = 1;
    for (size_t mi = 0; mi < ctx->shape_meshes.size(); mi++) {
        const RtuContext::MeshInfo& info = ctx->mesh_info[mi];
        stack_needed = std::max(stack_needed, std::min<uint32_t>(info.stack4, RTU_MAX_BVH_STACK));
        stack_needed = std::max(stack_needed, info.sah_depth);
        stack_needed = std::max(stack_needed, ctx->shape_meshes[mi].bvh_depth);
    }
    ctx->bvh_stack_needed = stack_needed;
    return RTU_OK;
}

}  // namespace

extern "C" {

int rtu_upload_scene(RtuContext* ctx, const RtuSceneDesc* s) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = validate(ctx, s);
    if (rc != RTU_OK) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->aux_stream) RTU_HIP(ctx, hipStreamSynchronize(ctx->aux_stream));
    free_scene(ctx);
    ctx->scene_gen++;
    ctx->slot_of.clear();

    // meshes
    std::vector<RtuContext::MeshInfo> mesh_info;
    std::vector<DevMesh> meshes(s->n_meshes);
    std::vector<uint32_t> fast_nodes(s->n_meshes, 0);
    std::vector<std::vector<uint32_t>> fast_elements(s->n_meshes);  // per mesh: slot of the fast tree's leaf order -> face
    std::vector<uint32_t> slot_of;
    std::vector<RtuContext::MeshRefit> refit(s->n_meshes);
    uint32_t stack_needed = 1;
    for (uint32_t mi = 0; mi < s->n_meshes; mi++) {
        const RtuMesh& m = s->meshes[mi];
        DevMesh& d = meshes[mi];
        memset(&d, 0, sizeof d);
        std::vector<float4> tri;
        build_tri_records(m, m.elements, m.n_elements, tri);
        static_assert(sizeof(RtuBvhNode) == 2 * sizeof(float4), "BVH node is two float4");
        // `ref` tree: the reference's, renumbered breadth-first
        std::vector<RtuBvhNode> bfs;
        renumber_bfs(m, bfs, d.any_empty_box);
        refit[mi].ref_bvh_alloc = ctx->scene_allocs.size();  // the allocation the next line makes
        if ((rc = upload(ctx, reinterpret_cast<const float4*>(bfs.data()), (size_t)m.n_bvh_nodes * 2, &d.ref.bvh)) != RTU_OK) return rc;
        if ((rc = upload(ctx, tri.data(), tri.size(), &d.ref.tri)) != RTU_OK) return rc;
        if ((rc = upload(ctx, m.elements, (size_t)m.n_elements, &d.ref.elements)) != RTU_OK) return rc;
        // `fast` tree: binned SAH over the same triangles
        SahTree sah;
        build_sah(m, sah);
        if (sah.depth > RTU_MAX_BVH_STACK) return fail(ctx, RTU_ERR_UNSUPPORTED, "mesh %u: SAH tree depth %u > %d", mi, sah.depth, RTU_MAX_BVH_STACK);
        std::vector<uint32_t> sub_first, sub_total;
        dfs_order(sah, sub_first, sub_total);
        build_tri_records(m, sah.elements.data(), (uint32_t)sah.elements.size(), tri);
        d.fast.bvh = nullptr;  // the kernels walk the collapsed forms (bvh4 / bvh8) of this tree
        if ((rc = upload(ctx, tri.data(), tri.size(), &d.fast.tri)) != RTU_OK) return rc;
        if ((rc = upload(ctx, sah.elements.data(), sah.elements.size(), &d.fast.elements)) != RTU_OK) return rc;
        fast_elements[mi] = sah.elements;
        slot_of.assign(m.nf, 0u);  // its inverse, for the device builder of rtu_update_scene
        for (uint32_t sl = 0; sl < (uint32_t)sah.elements.size(); sl++) slot_of[sah.elements[sl]] = sl;
        const uint32_t* d_slot_of = nullptr;
        if ((rc = upload(ctx, slot_of.data(), slot_of.size(), &d_slot_of)) != RTU_OK) return rc;
        ctx->slot_of.push_back(d_slot_of);
        std::vector<float4> wide8;
        build_wide8(sah, sub_first, sub_total, wide8);
        if ((rc = upload(ctx, wide8.data(), wide8.size(), &d.bvh8)) != RTU_OK) return rc;
        fast_nodes[mi] = (uint32_t)(wide8.size() / 16);
        wide_levels<8>(wide8, refit[mi].lvl8);
        std::vector<float4> wide4;
        uint32_t need4 = 1;
        build_wide4(sah, wide4, need4);
        wide_levels<4>(wide4, refit[mi].lvl4);
        if ((rc = upload(ctx, wide4.data(), wide4.size(), &d.bvh4)) != RTU_OK) return rc;
        mesh_info.push_back({m.nf, sah.depth, need4, (uint32_t)(wide4.size() / 8), (uint32_t)(wide8.size() / 16)});
        if (need4 > RTU_MAX_BVH_STACK) need4 = RTU_MAX_BVH_STACK;  // a walk that needs more finishes on the reference's tree
        if (need4 > stack_needed) stack_needed = need4;
        if (sah.depth > stack_needed) stack_needed = sah.depth;
        if ((rc = upload(ctx, m.f, (size_t)m.nf * 3, &d.f)) != RTU_OK) return rc;
        refit[mi].v_alloc = ctx->scene_allocs.size();  // the allocation the next line makes
        if ((rc = upload(ctx, m.v, (size_t)m.nv * 3, &d.v)) != RTU_OK) return rc;
        if ((rc = upload(ctx, m.fn, (size_t)m.nf * 3, &d.fn)) != RTU_OK) return rc;
        refit[mi].vn_alloc = ctx->scene_allocs.size();
        if ((rc = upload(ctx, m.vn, (size_t)m.nvn * 3, &d.vn)) != RTU_OK) return rc;
        d.vt = nullptr;
        d.ft = nullptr;
        if (s->n_textures > 0 && m.vt && m.ft && m.nvt) {  // texture coordinates only travel with textured scenes
            if ((rc = upload(ctx, m.vt, (size_t)m.nvt * 3, &d.vt)) != RTU_OK) return rc;
            if ((rc = upload(ctx, m.ft, (size_t)m.nf * 3, &d.ft)) != RTU_OK) return rc;
        }
        d.scale = 0.0f;
        for (int k = 0; k < 3; k++) d.scale = fmaxf(d.scale, fmaxf(fabsf(m.bound_min[k]), fabsf(m.bound_max[k])));
        memcpy(d.bmin, m.bound_min, sizeof d.bmin);
        memcpy(d.bmax, m.bound_max, sizeof d.bmax);
        d.n_bvh_nodes = m.n_bvh_nodes;
        d.n_elements = m.n_elements;
        if (m.bvh_depth > stack_needed) stack_needed = m.bvh_depth;
    }

    // LDS node area of the cooperative kernels, handed out in mesh order
    {
        uint32_t budget = (uint32_t)RTU_LDS_NODE_F4 / 16;  // node8
        uint32_t used = 0;
        for (uint32_t mi = 0; mi < s->n_meshes; mi++) {
            uint32_t take = fast_nodes[mi];
            if (take > budget - used) take = budget - used;
            meshes[mi].lds_nodes = take;
            meshes[mi].lds_off = used * 16;
            used += take;
        }
    }

    DevScene ds;
    memset(&ds, 0, sizeof ds);
    if ((rc = upload(ctx, meshes.data(), meshes.size(), &ds.meshes)) != RTU_OK) return rc;
    // textures
    ds.textured = (s->n_textures > 0) ? 1u : 0u;
    if (ds.textured) {
        std::vector<DevTexture> texs(s->n_textures);
        for (uint32_t i = 0; i < s->n_textures; i++) {
            const RtuTexture& t = s->textures[i];
            DevTexture& o = texs[i];
            memset(&o, 0, sizeof o);
            o.type = t.type; o.width = t.width; o.height = t.height;
            memcpy(o.color1, t.color1, sizeof o.color1);
            memcpy(o.color2, t.color2, sizeof o.color2);
            if (t.type == RTU_TEX_FILE && (size_t)t.width * t.height > 0)
                if ((rc = upload(ctx, t.rgb, (size_t)t.width * t.height * 3, &o.rgb)) != RTU_OK) return rc;
        }
        if ((rc = upload(ctx, texs.data(), texs.size(), &ds.textures)) != RTU_OK) return rc;
    }
    ctx->textured = ds.textured != 0;
    ds.n_nodes = s->n_nodes;
    ds.walk_stack_limit = 0xFFFFu;
    ds.node_bounds = 1;
    // screen rectangles of the node-level bounds, one set per frame in flight (written by k_node_rects on every launch)
    if ((rc = alloc_owned(ctx, ctx->scene_allocs, sizeof(int4) * (size_t)RTU_MAX_FRAME_BATCH * s->n_nodes, &ctx->node_rects)) != RTU_OK) return rc;
    ctx->n_meshes = s->n_meshes;
    ctx->mesh_info = mesh_info;
    ctx->bvh_stack_needed = stack_needed;
    // the shape (rtu_update_scene) and what an update builds from
    ctx->shape_nodes.assign(s->nodes, s->nodes + s->n_nodes);
    ctx->shape_meshes.assign(s->meshes, s->meshes + s->n_meshes);
    for (RtuMesh& m : ctx->shape_meshes) { m.v = nullptr; m.f = nullptr; m.vn = nullptr; m.fn = nullptr; m.vt = nullptr; m.ft = nullptr; m.bvh = nullptr; m.elements = nullptr; }
    ctx->shape_textures.assign(s->textures, s->textures + s->n_textures);
    for (RtuTexture& t : ctx->shape_textures) t.rgb = nullptr;
    ctx->shape_materials = s->n_materials;
    ctx->shape_maps = s->material_maps != nullptr;
    ctx->fast_elements = std::move(fast_elements);
    ctx->refit = std::move(refit);
    ctx->fn_is_f.assign(s->n_meshes, -1);
    rb_forget_meshes(ctx->rb);
    ctx->dmeshes = meshes;
    ctx->dscene = ds;
    if ((rc = place_scene(ctx, s, false)) != RTU_OK) return rc;
    ctx->has_scene = true;
    return RTU_OK;
}

int rtu_update_scene(RtuContext* ctx, const RtuSceneDesc* s) {
    if (!ctx) return RTU_ERR_ARG;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    // everything is checked before anything is written: a refused update leaves the context as it was
    int rc = shape_args(ctx, s);
    if (rc != RTU_OK) return rc;
    const RtuSceneDesc up = shape_desc(ctx);
    const std::string diff = shape_diff(&up, s);
    if (!diff.empty()) return fail(ctx, RTU_ERR_SCENE_SHAPE, "not the uploaded scene's shape: %s", diff.c_str());
    RtuSceneDesc placed = *s;  // the mesh and texture arrays are the uploaded ones: only their headers are read
    placed.meshes = ctx->shape_meshes.data();
    placed.textures = ctx->shape_textures.data();
    if ((rc = validate(ctx, &placed, true)) != RTU_OK) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight read the buffers rewritten below
    if (ctx->aux_stream) RTU_HIP(ctx, hipStreamSynchronize(ctx->aux_stream));
    if (!ctx->llb) ctx->llb = ll_builder_create();
    ctx->scene_gen++;
    if ((rc = place_scene(ctx, &placed, true)) != RTU_OK) {
        free_scene(ctx);  // half placed: nothing to render from
        return rc;
    }
    return RTU_OK;
}

int rtu_update_meshes(RtuContext* ctx, const RtuSceneDesc* s, const uint32_t* mesh_ids, int n_meshes) {
    if (!ctx) return RTU_ERR_ARG;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (n_meshes == 0) return rtu_update_scene(ctx, s);
    if (n_meshes < 0 || !mesh_ids) return fail(ctx, RTU_ERR_ARG, "mesh_ids is NULL or n_meshes negative");
    // everything is checked before anything is written: a refused update leaves the context as it was
    int rc = shape_args(ctx, s);
    if (rc != RTU_OK) return rc;
    const size_t nm = ctx->shape_meshes.size();
    std::vector<char> listed(nm, 0);
    for (int i = 0; i < n_meshes; i++) {
        const uint32_t id = mesh_ids[i];
        if (id >= nm) return fail(ctx, RTU_ERR_ARG, "mesh id %u out of range (%zu meshes)", id, nm);
        if (listed[id]) return fail(ctx, RTU_ERR_ARG, "mesh id %u listed twice", id);
        listed[id] = 1;
    }
    // the shape rule of rtu_update_scene, except that a LISTED mesh may bring a `ref` tree of another size
    std::vector<RtuMesh> want = ctx->shape_meshes;
    if (s->n_meshes == nm)
        for (size_t id = 0; id < nm; id++)
            if (listed[id]) want[id].n_bvh_nodes = s->meshes[id].n_bvh_nodes;
    RtuSceneDesc up = shape_desc(ctx);
    up.meshes = want.data();
    const std::string diff = shape_diff(&up, s);
    if (!diff.empty()) return fail(ctx, RTU_ERR_SCENE_SHAPE, "not the uploaded scene's shape: %s", diff.c_str());
    std::vector<RtuMesh> new_shape = ctx->shape_meshes;
    for (size_t id = 0; id < nm; id++) {
        if (!listed[id]) continue;
        const RtuMesh& m = s->meshes[id];
        const uint32_t mi = (uint32_t)id;
        if (m.n_elements != ctx->shape_meshes[id].n_elements)
            return fail(ctx, RTU_ERR_SCENE_SHAPE, "not the uploaded scene's shape: mesh %u: n_elements differs", mi);
        // what validate() asks of a mesh's vertices, normals and `ref` tree at upload, with its codes (connectivity is the uploaded one)
        if (!m.v || !m.vn || !m.bvh || !m.elements) return fail(ctx, RTU_ERR_ARG, "mesh %u: missing array (v, vn, bvh and elements are read)", mi);
        if (m.n_bvh_nodes < 2 || m.n_elements != m.nf || m.nf == 0) return fail(ctx, RTU_ERR_ARG, "mesh %u: empty", mi);
        if (m.n_bvh_nodes >= (1u << 28)) return fail(ctx, RTU_ERR_UNSUPPORTED, "mesh %u: more than 2^28 nodes/elements", mi);
        if (m.bvh_depth > RTU_MAX_BVH_STACK) return fail(ctx, RTU_ERR_UNSUPPORTED, "mesh %u: BVH depth %u > %d", mi, m.bvh_depth, RTU_MAX_BVH_STACK);
        if ((rc = validate_tree(ctx, m, mi)) != RTU_OK) return rc;
        RtuMesh& h = new_shape[id];
        h.n_bvh_nodes = m.n_bvh_nodes;
        h.bvh_depth = m.bvh_depth;
        memcpy(h.bound_min, m.bound_min, sizeof h.bound_min);
        memcpy(h.bound_max, m.bound_max, sizeof h.bound_max);
    }
    RtuSceneDesc placed = *s;  // headers as the context will remember them; the arrays stay NULL
    placed.meshes = new_shape.data();
    placed.textures = ctx->shape_textures.data();
    if ((rc = validate(ctx, &placed, true)) != RTU_OK) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight read the buffers rewritten below
    if (ctx->aux_stream) RTU_HIP(ctx, hipStreamSynchronize(ctx->aux_stream));
    if (!ctx->llb) ctx->llb = ll_builder_create();
    ctx->scene_gen++;
    // the meshes first (and the shape with them): the placement's node-level bounds read the mesh boxes from the remembered headers
    if ((rc = write_meshes(ctx, s, mesh_ids, n_meshes, new_shape)) == RTU_OK) {
        placed.meshes = ctx->shape_meshes.data();
        rc = place_scene(ctx, &placed, true);
    }
    if (rc != RTU_OK) {
        free_scene(ctx);  // half written: nothing to render from
        return rc;
    }
    if (ctx->mu_timing) {
        RTU_HIP(ctx, hipEventRecord(ctx->mu_ev[4], ctx->stream));
        RTU_HIP(ctx, hipEventSynchronize(ctx->mu_ev[4]));
        for (int k = 0; k < 4; k++) {
            float ms = 0;
            RTU_HIP(ctx, hipEventElapsedTime(&ms, ctx->mu_ev[k], ctx->mu_ev[k + 1]));
            ctx->mu_ms[k] += ms;
        }
    }
    return RTU_OK;
}

int rtu_debug_mesh_update_timing(RtuContext* ctx, int on, float* ms_out4) {
    if (!ctx) return RTU_ERR_ARG;
    if (ms_out4) memcpy(ms_out4, ctx->mu_ms, sizeof ctx->mu_ms);
    memset(ctx->mu_ms, 0, sizeof ctx->mu_ms);
    ctx->mu_timing = on != 0;
    return RTU_OK;
}

}  // extern "C"

namespace {

int dump_out(RtuContext* ctx, size_t bytes, void* out, size_t capacity, size_t* bytes_out);  // (below, with the mesh dumps)

// The writing half of rtu_update_meshes_device, after every check has passed and every tree is built and validated in the builder's
// scratch: what write_meshes does, with device-to-device copies in place of the uploads. res[i]: the header of edit i's build.
int write_meshes_device(RtuContext* ctx, const RtuMeshDeviceEdit* edits, int n_edits, const std::vector<RbResult>& res, const std::vector<RtuMesh>& new_shape) {
    hipStream_t st = ctx->stream;
    const bool timing = ctx->mu_timing;
    if (ctx->keep_prev) {  // as in write_meshes: the buffers change places before anything is copied
        ctx->prev_gen.resize(ctx->dmeshes.size());
        for (RtuContext::PrevGen& g : ctx->prev_gen) g.valid = false;
        for (int i = 0; i < n_edits; i++) {
            const uint32_t id = edits[i].mesh;
            RtuContext::PrevGen& g = ctx->prev_gen[id];
            DevBuf<char>&v = ctx->scene_allocs[ctx->refit[id].v_alloc], &vn = ctx->scene_allocs[ctx->refit[id].vn_alloc];
            RTU_HIP(ctx, g.v.grow(v.size()));
            RTU_HIP(ctx, g.vn.grow(vn.size()));
            std::swap(g.v, v);
            std::swap(g.vn, vn);
            g.valid = true;
            ctx->dmeshes[id].v = reinterpret_cast<const float*>(v.get());
            ctx->dmeshes[id].vn = reinterpret_cast<const float*>(vn.get());
        }
    }
    ctx->df_dirty = true;
    for (int i = 0; i < n_edits; i++) {
        const uint32_t id = edits[i].mesh;
        const RtuMesh& h = new_shape[id];
        const RbResult& r = res[(size_t)i];
        DevMesh& d = ctx->dmeshes[id];
        // the tree's buffer takes the largest tree these faces can have, once: later updates of the mesh allocate nothing
        DevBuf<char>& tree_buf = ctx->scene_allocs[ctx->refit[id].ref_bvh_alloc];
        RTU_HIP(ctx, tree_buf.grow(sizeof(RtuBvhNode) * 2 * (size_t)h.nf));
        d.ref.bvh = reinterpret_cast<const float4*>(tree_buf.get());
        RTU_HIP(ctx, hipMemcpyAsync(tree_buf.get(), rb_tree(ctx->rb, (uint32_t)i), sizeof(RtuBvhNode) * (size_t)r.n_bvh_nodes, hipMemcpyDeviceToDevice, st));
        RTU_HIP(ctx, hipMemcpyAsync(const_cast<uint32_t*>(d.ref.elements), rb_elements(ctx->rb, (uint32_t)i), sizeof(uint32_t) * (size_t)h.n_elements, hipMemcpyDeviceToDevice, st));
        RTU_HIP(ctx, hipMemcpyAsync(const_cast<float*>(d.v), edits[i].d_v, sizeof(float) * 3 * (size_t)h.nv, hipMemcpyDeviceToDevice, st));
        const void* vn = edits[i].d_vn;
        if (edits[i].flags & RTU_MESH_EDIT_RECOMPUTE_NORMALS) vn = rb_normals(ctx->rb, (uint32_t)i);
        else if (!vn && ctx->keep_prev) vn = ctx->prev_gen[id].vn.get();  // the normals stay: they are in the buffer that was swapped out
        if (vn) RTU_HIP(ctx, hipMemcpyAsync(const_cast<float*>(d.vn), vn, sizeof(float) * 3 * (size_t)h.nvn, hipMemcpyDeviceToDevice, st));
        d.scale = 0.0f;
        for (int k = 0; k < 3; k++) d.scale = fmaxf(d.scale, fmaxf(fabsf(h.bound_min[k]), fabsf(h.bound_max[k])));
        memcpy(d.bmin, h.bound_min, sizeof d.bmin);
        memcpy(d.bmax, h.bound_max, sizeof d.bmax);
        d.n_bvh_nodes = h.n_bvh_nodes;
        d.any_empty_box = r.any_empty_box;
        RTU_HIP(ctx, hipMemcpyAsync(const_cast<DevMesh*>(ctx->dscene.meshes) + id, &d, sizeof d, hipMemcpyHostToDevice, st));
    }
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->mud_ev[2], st));
    for (int i = 0; i < n_edits; i++) {
        const uint32_t id = edits[i].mesh;
        const DevMesh& d = ctx->dmeshes[id];
        const RtuContext::MeshRefit& r = ctx->refit[id];
        RTU_HIP(ctx, mu_tri_records(st, d.f, d.v, d.ref.elements, d.n_elements, const_cast<float4*>(d.ref.tri)));
        RTU_HIP(ctx, mu_tri_records(st, d.f, d.v, d.fast.elements, d.n_elements, const_cast<float4*>(d.fast.tri)));
        RTU_HIP(ctx, mu_refit(st, 4, const_cast<float4*>(d.bvh4), ctx->mesh_info[id].nodes4, r.lvl4.data(), (uint32_t)r.lvl4.size() - 1u, d.f, d.v,
                              d.fast.elements, d.n_elements));
        RTU_HIP(ctx, mu_refit(st, 8, const_cast<float4*>(d.bvh8), ctx->mesh_info[id].nodes8, r.lvl8.data(), (uint32_t)r.lvl8.size() - 1u, d.f, d.v,
                              d.fast.elements, d.n_elements));
    }
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->mud_ev[3], st));
    RTU_HIP(ctx, hipStreamSynchronize(st));
    ctx->shape_meshes = new_shape;
    uint32_t stack_needed = 1;  // as write_meshes computes it
    for (size_t mi = 0; mi < ctx->shape_meshes.size(); mi++) {
        const RtuContext::MeshInfo& info = ctx->mesh_info[mi];
        stack_needed = std::max(stack_needed, std::min<uint32_t>(info.stack4, RTU_MAX_BVH_STACK));
        stack_needed = std::max(stack_needed, info.sah_depth);
        stack_needed = std::max(stack_needed, ctx->shape_meshes[mi].bvh_depth);
    }
    ctx->bvh_stack_needed = stack_needed;
    return RTU_OK;
}

}  // namespace

extern "C" {

int rtu_update_meshes_device(RtuContext* ctx, const RtuSceneDesc* s, const RtuMeshDeviceEdit* edits, int n_edits, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (n_edits == 0) return rtu_update_scene(ctx, s);
    if (n_edits < 0 || !edits) return fail(ctx, RTU_ERR_ARG, "edits is NULL or n_edits negative");
    // everything that can be checked before the build is: a refused update leaves the context as it was
    int rc = shape_args(ctx, s);
    if (rc != RTU_OK) return rc;
    const size_t nm = ctx->shape_meshes.size();
    std::vector<char> listed(nm, 0);
    for (int i = 0; i < n_edits; i++) {
        const RtuMeshDeviceEdit& e = edits[i];
        if (e.mesh >= nm) return fail(ctx, RTU_ERR_ARG, "mesh id %u out of range (%zu meshes)", e.mesh, nm);
        if (listed[e.mesh]) return fail(ctx, RTU_ERR_ARG, "mesh id %u listed twice", e.mesh);
        listed[e.mesh] = 1;
        if (!e.d_v) return fail(ctx, RTU_ERR_ARG, "mesh %u: d_v is NULL", e.mesh);
        if (e.flags & ~RTU_MESH_EDIT_RECOMPUTE_NORMALS) return fail(ctx, RTU_ERR_ARG, "mesh %u: unknown flags 0x%x", e.mesh, e.flags);
        if ((e.flags & RTU_MESH_EDIT_RECOMPUTE_NORMALS) && e.d_vn) return fail(ctx, RTU_ERR_ARG, "mesh %u: d_vn given with RECOMPUTE_NORMALS", e.mesh);
    }
    // the shape rule of rtu_update_scene; of a LISTED mesh the tree's size is not compared (the host scene is stale by design)
    std::vector<RtuMesh> want = ctx->shape_meshes;
    if (s->n_meshes == nm)
        for (size_t id = 0; id < nm; id++)
            if (listed[id]) want[id].n_bvh_nodes = s->meshes[id].n_bvh_nodes;
    RtuSceneDesc up = shape_desc(ctx);
    up.meshes = want.data();
    const std::string diff = shape_diff(&up, s);
    if (!diff.empty()) return fail(ctx, RTU_ERR_SCENE_SHAPE, "not the uploaded scene's shape: %s", diff.c_str());
    for (int i = 0; i < n_edits; i++) {
        const uint32_t id = edits[i].mesh;
        const RtuMesh& h = ctx->shape_meshes[id];
        if (s->meshes[id].n_elements != h.n_elements)
            return fail(ctx, RTU_ERR_SCENE_SHAPE, "not the uploaded scene's shape: mesh %u: n_elements differs", id);
        if (h.nf == 0 || h.n_elements != h.nf) return fail(ctx, RTU_ERR_ARG, "mesh %u: empty", id);
        if (2 * (uint64_t)h.nf >= (1u << 28)) return fail(ctx, RTU_ERR_UNSUPPORTED, "mesh %u: more than 2^28 nodes/elements", id);
        if ((edits[i].flags & RTU_MESH_EDIT_RECOMPUTE_NORMALS) && h.nvn != h.nv)
            return fail(ctx, RTU_ERR_ARG, "mesh %u carries normals of its own (not one per vertex with fn == f)", id);
    }
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight read the buffers rewritten below
    if (ctx->aux_stream) RTU_HIP(ctx, hipStreamSynchronize(ctx->aux_stream));
    if (!ctx->rb) ctx->rb = rb_create();
    hipStream_t st = ctx->stream;
    for (int i = 0; i < n_edits; i++) {  // fn == f as uploaded: asked of the device copies once per upload
        const uint32_t id = edits[i].mesh;
        if (!(edits[i].flags & RTU_MESH_EDIT_RECOMPUTE_NORMALS)) continue;
        if (ctx->fn_is_f[id] < 0) {
            bool differ = true;
            RTU_HIP(ctx, rb_compare_device(ctx->rb, st, ctx->dmeshes[id].f, ctx->dmeshes[id].fn, 3 * ctx->shape_meshes[id].nf, differ));
            ctx->fn_is_f[id] = differ ? 0 : 1;
        }
        if (!ctx->fn_is_f[id]) return fail(ctx, RTU_ERR_ARG, "mesh %u carries normals of its own (not one per vertex with fn == f)", id);
    }
    // the caller's vertices: this call's reads wait for the work of the stream they were produced on, nothing else does
    if ((hipStream_t)hip_stream != st) {
        if (!ctx->mud_wait) RTU_HIP(ctx, hipEventCreateWithFlags(&ctx->mud_wait, hipEventDisableTiming));
        RTU_HIP(ctx, hipEventRecord(ctx->mud_wait, (hipStream_t)hip_stream));
        RTU_HIP(ctx, hipStreamWaitEvent(st, ctx->mud_wait, 0));
    }
    const bool timing = ctx->mu_timing;
    if (timing && !ctx->mud_ev[0])
        for (hipEvent_t& e : ctx->mud_ev) RTU_HIP(ctx, hipEventCreate(&e));
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->mud_ev[0], st));
    // the trees, into the builder's scratch (one output slot per edit); then their headers are validated
    std::vector<RbResult> res((size_t)n_edits);
    std::vector<RtuMesh> new_shape = ctx->shape_meshes;
    for (int i = 0; i < n_edits; i++) {
        const uint32_t id = edits[i].mesh;
        const DevMesh& d = ctx->dmeshes[id];
        RtuMesh& h = new_shape[id];
        const float* d_v = static_cast<const float*>(edits[i].d_v);
        if (edits[i].flags & RTU_MESH_EDIT_RECOMPUTE_NORMALS) RTU_HIP(ctx, rb_normals_device(ctx->rb, st, (uint32_t)i, id, d.f, d_v, h.nf, h.nv));
        RbResult& r = res[(size_t)i];
        RTU_HIP(ctx, rb_build_device(ctx->rb, st, (uint32_t)i, d.f, d_v, h.nf, h.nv, RTU_MAX_BVH_STACK, r));
        if (r.open || r.bvh_depth > RTU_MAX_BVH_STACK)
            return fail(ctx, RTU_ERR_UNSUPPORTED, "mesh %u: BVH depth > %d (%u nodes of level %u are inner)", id, RTU_MAX_BVH_STACK, r.open, r.bvh_depth);
        if (r.n_bvh_nodes >= (1u << 28)) return fail(ctx, RTU_ERR_UNSUPPORTED, "mesh %u: more than 2^28 nodes/elements", id);
        h.n_bvh_nodes = r.n_bvh_nodes;
        h.bvh_depth = r.bvh_depth;
        memcpy(h.bound_min, r.bmin, sizeof h.bound_min);
        memcpy(h.bound_max, r.bmax, sizeof h.bound_max);
    }
    RtuSceneDesc placed = *s;  // headers as the context will remember them; the arrays stay NULL
    placed.meshes = new_shape.data();
    placed.textures = ctx->shape_textures.data();
    if ((rc = validate(ctx, &placed, true)) != RTU_OK) return rc;
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->mud_ev[1], st));
    if (!ctx->llb) ctx->llb = ll_builder_create();
    ctx->scene_gen++;
    if ((rc = write_meshes_device(ctx, edits, n_edits, res, new_shape)) == RTU_OK) {
        placed.meshes = ctx->shape_meshes.data();
        rc = place_scene(ctx, &placed, true);
    }
    if (rc != RTU_OK) {
        free_scene(ctx);  // half written: nothing to render from
        return rc;
    }
    if (timing) {
        RTU_HIP(ctx, hipEventRecord(ctx->mud_ev[4], st));
        RTU_HIP(ctx, hipEventSynchronize(ctx->mud_ev[4]));
        for (int k = 0; k < 4; k++) {
            float ms = 0;
            RTU_HIP(ctx, hipEventElapsedTime(&ms, ctx->mud_ev[k], ctx->mud_ev[k + 1]));
            ctx->mud_ms[k] += ms;
        }
    }
    return RTU_OK;
}

int rtu_context_mesh_shape(RtuContext* ctx, uint32_t mesh, RtuMesh* header_out) {
    if (!ctx) return RTU_ERR_ARG;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (mesh >= ctx->shape_meshes.size()) return fail(ctx, RTU_ERR_ARG, "no mesh %u", mesh);
    if (!header_out) return fail(ctx, RTU_ERR_ARG, "header_out is NULL");
    *header_out = ctx->shape_meshes[mesh];
    return RTU_OK;
}

int rtu_debug_mesh_update_device_timing(RtuContext* ctx, float* ms_out4) {
    if (!ctx) return RTU_ERR_ARG;
    if (ms_out4) memcpy(ms_out4, ctx->mud_ms, sizeof ctx->mud_ms);
    memset(ctx->mud_ms, 0, sizeof ctx->mud_ms);
    return RTU_OK;
}

int rtu_debug_host_ref_build(const RtuMesh* m, const float* v, int which, void* out, size_t capacity_bytes, size_t* bytes_out) {
    if (bytes_out) *bytes_out = 0;
    if (!m || !m->f || !m->v || m->nf == 0 || m->nv == 0) return RTU_ERR_ARG;
    for (uint32_t i = 0; i < m->nf * 3; i++)
        if (m->f[i] >= m->nv) return RTU_ERR_ARG;
    if (!v) v = m->v;
    std::vector<RtuBvhNode> tree;
    std::vector<uint32_t> elements;
    std::vector<float> vn;
    RbResult r;
    RtuRefBuildHeader hd;
    const void* src = nullptr;
    size_t bytes = 0;
    if (which == RTU_MESH_VN) {
        if (m->nvn != m->nv) return RTU_ERR_ARG;
        rb_normals_host(m->f, v, m->nf, m->nv, vn);
        src = vn.data(); bytes = sizeof(float) * vn.size();
    } else if (which == RTU_MESH_REF_BVH || which == RTU_MESH_REF_ELEMENTS || which == RTU_MESH_HEADER) {
        rb_build_host(m->f, v, m->nf, m->nv, 0, tree, elements, r);
        if (which == RTU_MESH_REF_BVH) { src = tree.data(); bytes = sizeof(RtuBvhNode) * tree.size(); }
        else if (which == RTU_MESH_REF_ELEMENTS) { src = elements.data(); bytes = sizeof(uint32_t) * elements.size(); }
        else {
            memcpy(hd.bmin, r.bmin, sizeof hd.bmin); memcpy(hd.bmax, r.bmax, sizeof hd.bmax);
            hd.scale = 0.0f;
            for (int k = 0; k < 3; k++) hd.scale = fmaxf(hd.scale, fmaxf(fabsf(r.bmin[k]), fabsf(r.bmax[k])));
            hd.n_bvh_nodes = r.n_bvh_nodes; hd.any_empty_box = r.any_empty_box; hd.bvh_depth = r.bvh_depth;
            src = &hd; bytes = sizeof hd;
        }
    } else return RTU_ERR_ARG;
    int rc = dump_out(nullptr, bytes, out, capacity_bytes, bytes_out);
    if (rc == RTU_OK && bytes) memcpy(out, src, bytes);
    return rc;
}

int rtu_debug_partition_rule(const uint8_t* keep, uint32_t n, uint32_t* perm_out) {
    if (n && (!keep || !perm_out)) return RTU_ERR_ARG;
    rb_partition_host(keep, n, perm_out);
    return RTU_OK;
}

}  // extern "C"

namespace {

// one array of a mesh dump to the caller: *bytes_out is always set; RTU_ERR_ARG when `out` is too small for it
int dump_out(RtuContext* ctx, size_t bytes, void* out, size_t capacity, size_t* bytes_out) {
    if (bytes_out) *bytes_out = bytes;
    if (bytes > capacity || (bytes && !out)) return fail(ctx, RTU_ERR_ARG, "the array has %zu bytes, the buffer %zu", bytes, capacity);
    return RTU_OK;
}

}  // namespace

extern "C" {

int rtu_debug_context_mesh(RtuContext* ctx, uint32_t mesh, int which, void* out, size_t capacity_bytes, size_t* bytes_out) {
    if (!ctx) return RTU_ERR_ARG;
    if (bytes_out) *bytes_out = 0;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (mesh >= ctx->dmeshes.size()) return fail(ctx, RTU_ERR_ARG, "no mesh %u", mesh);
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    DevMesh d;  // the record the kernels read, not the host's copy of it
    RTU_HIP(ctx, hipMemcpy(&d, ctx->dscene.meshes + mesh, sizeof d, hipMemcpyDeviceToHost));
    const RtuMesh& h = ctx->shape_meshes[mesh];
    const RtuContext::MeshInfo& info = ctx->mesh_info[mesh];
    const void* src = nullptr;
    size_t bytes = 0;
    RtuMeshHeaderDump hd;
    switch (which) {
        case RTU_MESH_BVH4: src = d.bvh4; bytes = sizeof(float4) * 8 * (size_t)info.nodes4; break;
        case RTU_MESH_BVH8: src = d.bvh8; bytes = sizeof(float4) * 16 * (size_t)info.nodes8; break;
        case RTU_MESH_FAST_TRI: src = d.fast.tri; bytes = sizeof(float4) * 4 * (size_t)d.n_elements; break;
        case RTU_MESH_REF_TRI: src = d.ref.tri; bytes = sizeof(float4) * 4 * (size_t)d.n_elements; break;
        case RTU_MESH_REF_BVH: src = d.ref.bvh; bytes = sizeof(RtuBvhNode) * (size_t)d.n_bvh_nodes; break;
        case RTU_MESH_REF_ELEMENTS: src = d.ref.elements; bytes = sizeof(uint32_t) * (size_t)d.n_elements; break;
        case RTU_MESH_FAST_ELEMENTS: src = d.fast.elements; bytes = sizeof(uint32_t) * (size_t)d.n_elements; break;
        case RTU_MESH_V: src = d.v; bytes = sizeof(float) * 3 * (size_t)h.nv; break;
        case RTU_MESH_VN: src = d.vn; bytes = sizeof(float) * 3 * (size_t)h.nvn; break;
        case RTU_MESH_HEADER:
            memcpy(hd.bmin, d.bmin, sizeof hd.bmin); memcpy(hd.bmax, d.bmax, sizeof hd.bmax);
            hd.scale = d.scale; hd.n_bvh_nodes = d.n_bvh_nodes; hd.any_empty_box = d.any_empty_box;
            bytes = sizeof hd;
            break;
        default: return fail(ctx, RTU_ERR_ARG, "no mesh array %d", which);
    }
    int rc = dump_out(ctx, bytes, out, capacity_bytes, bytes_out);
    if (rc != RTU_OK) return rc;
    if (which == RTU_MESH_HEADER) memcpy(out, &hd, sizeof hd);
    else if (bytes) RTU_HIP(ctx, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return RTU_OK;
}

int rtu_debug_host_mesh(const RtuMesh* uploaded, const RtuMesh* now, int which, void* out, size_t capacity_bytes, size_t* bytes_out) {
    if (bytes_out) *bytes_out = 0;
    RtuContext tmp;  // plain host state: nothing here touches a GPU
    const RtuMesh* cur = now ? now : uploaded;
    for (const RtuMesh* m : {uploaded, cur}) {
        if (!m || !m->v || !m->f || !m->vn || !m->bvh || !m->elements || m->nf == 0 || m->n_elements != m->nf || m->n_bvh_nodes < 2) return RTU_ERR_ARG;
        if (m->bvh_depth > RTU_MAX_BVH_STACK) return RTU_ERR_UNSUPPORTED;
        for (uint32_t i = 0; i < m->nf * 3; i++)
            if (m->f[i] >= m->nv) return RTU_ERR_ARG;
        int rc = validate_tree(&tmp, *m, 0);
        if (rc != RTU_OK) return rc;
    }
    if (cur->nv != uploaded->nv || cur->nf != uploaded->nf || cur->nvn != uploaded->nvn) return RTU_ERR_SCENE_SHAPE;
    RtuMesh edited = *cur;  // the deformed vertices and `ref` tree on the UPLOADED connectivity
    edited.f = uploaded->f;
    std::vector<float4> f4;
    std::vector<RtuBvhNode> bfs;
    RtuMeshHeaderDump hd;
    const void* src = nullptr;
    size_t bytes = 0;
    SahTree sah;
    const bool fast = which == RTU_MESH_BVH4 || which == RTU_MESH_BVH8 || which == RTU_MESH_FAST_TRI || which == RTU_MESH_FAST_ELEMENTS;
    std::vector<uint32_t> sub_first, sub_total;
    if (fast) {  // the topology of the fast tree is the uploaded mesh's
        build_sah(*uploaded, sah);
        if (sah.depth > RTU_MAX_BVH_STACK) return RTU_ERR_UNSUPPORTED;
        dfs_order(sah, sub_first, sub_total);
    }
    switch (which) {
        case RTU_MESH_BVH4: {
            uint32_t need4 = 1;
            build_wide4(sah, f4, need4);
            if (now) refit_host<4>(f4, edited, sah.elements);
            src = f4.data(); bytes = sizeof(float4) * f4.size();
            break;
        }
        case RTU_MESH_BVH8:
            build_wide8(sah, sub_first, sub_total, f4);
            if (now) refit_host<8>(f4, edited, sah.elements);
            src = f4.data(); bytes = sizeof(float4) * f4.size();
            break;
        case RTU_MESH_FAST_TRI:
            build_tri_records(edited, sah.elements.data(), (uint32_t)sah.elements.size(), f4);
            src = f4.data(); bytes = sizeof(float4) * f4.size();
            break;
        case RTU_MESH_FAST_ELEMENTS: src = sah.elements.data(); bytes = sizeof(uint32_t) * sah.elements.size(); break;
        case RTU_MESH_REF_TRI:
            build_tri_records(edited, cur->elements, cur->n_elements, f4);
            src = f4.data(); bytes = sizeof(float4) * f4.size();
            break;
        case RTU_MESH_REF_BVH:
            renumber_bfs(*cur, bfs, hd.any_empty_box);
            src = bfs.data(); bytes = sizeof(RtuBvhNode) * bfs.size();
            break;
        case RTU_MESH_REF_ELEMENTS: src = cur->elements; bytes = sizeof(uint32_t) * (size_t)cur->n_elements; break;
        case RTU_MESH_V: src = cur->v; bytes = sizeof(float) * 3 * (size_t)cur->nv; break;
        case RTU_MESH_VN: src = cur->vn; bytes = sizeof(float) * 3 * (size_t)cur->nvn; break;
        case RTU_MESH_HEADER:
            renumber_bfs(*cur, bfs, hd.any_empty_box);
            memcpy(hd.bmin, cur->bound_min, sizeof hd.bmin); memcpy(hd.bmax, cur->bound_max, sizeof hd.bmax);
            hd.scale = 0.0f;
            for (int k = 0; k < 3; k++) hd.scale = fmaxf(hd.scale, fmaxf(fabsf(cur->bound_min[k]), fabsf(cur->bound_max[k])));
            hd.n_bvh_nodes = cur->n_bvh_nodes;
            src = &hd; bytes = sizeof hd;
            break;
        default: return RTU_ERR_ARG;
    }
    int rc = dump_out(nullptr, bytes, out, capacity_bytes, bytes_out);
    if (rc == RTU_OK && bytes) memcpy(out, src, bytes);
    return rc;
}

int rtu_scene_shape_diff(const RtuSceneDesc* a, const RtuSceneDesc* b, char* err_buf, size_t err_len) {
    RtuContext tmp;  // plain host state: nothing here touches a GPU
    int rc = shape_args(&tmp, a);
    if (rc == RTU_OK) rc = shape_args(&tmp, b);
    if (rc == RTU_OK) {
        const std::string d = shape_diff(a, b);
        if (!d.empty()) rc = fail(&tmp, RTU_ERR_SCENE_SHAPE, "%s", d.c_str());
    }
    if (err_buf && err_len) snprintf(err_buf, err_len, "%s", tmp.error.c_str());
    return rc;
}

}  // extern "C"

// The per-node maps of rtu_render.h "Temporal accumulation across scene updates", composed in binary64. Affine maps as {A row-major, b}.

namespace {

struct Affine64 { double A[9], b[3]; };

Affine64 affine_identity() { return Affine64{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}}; }

// x -> M (A x + b) + t with M column-major binary32 as RtuNode.tm: one level of FromNodeCoords
Affine64 affine_from_level(const Affine64& a, const float* M, const float* t) {
    Affine64 r;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) r.A[3 * i + j] = ((double)M[i] * a.A[j] + (double)M[i + 3] * a.A[3 + j]) + (double)M[i + 6] * a.A[6 + j];
        r.b[i] = (((double)M[i] * a.b[0] + (double)M[i + 3] * a.b[1]) + (double)M[i + 6] * a.b[2]) + (double)t[i];
    }
    return r;
}

// x -> M ((A x + b) - t): one level of ToNodeCoords with M = itm
Affine64 affine_to_level(const Affine64& a, const float* M, const float* t) {
    Affine64 r;
    const double c[3] = {a.b[0] - (double)t[0], a.b[1] - (double)t[1], a.b[2] - (double)t[2]};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) r.A[3 * i + j] = ((double)M[i] * a.A[j] + (double)M[i + 3] * a.A[3 + j]) + (double)M[i + 6] * a.A[6 + j];
        r.b[i] = ((double)M[i] * c[0] + (double)M[i + 3] * c[1]) + (double)M[i + 6] * c[2];
    }
    return r;
}

// a o b
Affine64 affine_compose(const Affine64& a, const Affine64& b) {
    Affine64 r;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) r.A[3 * i + j] = (a.A[3 * i] * b.A[j] + a.A[3 * i + 1] * b.A[3 + j]) + a.A[3 * i + 2] * b.A[6 + j];
        r.b[i] = ((a.A[3 * i] * b.b[0] + a.A[3 * i + 1] * b.b[1]) + a.A[3 * i + 2] * b.b[2]) + a.b[i];
    }
    return r;
}

// W (node -> world) and W^-1 of node i of scene s; false for a parent chain that does not lead to the root in RTU_MAX_NODE_DEPTH + 1 levels
bool node_chain(const RtuSceneDesc* s, uint32_t i, Affine64& W, Affine64& Winv) {
    uint32_t chain[RTU_MAX_NODE_DEPTH + 1];
    int n = 0;
    for (int32_t k = (int32_t)i; k >= 0; k = s->nodes[k].parent) {
        if (n > RTU_MAX_NODE_DEPTH || (uint32_t)k >= s->n_nodes) return false;
        chain[n++] = (uint32_t)k;
    }
    W = affine_identity();
    Winv = affine_identity();
    for (int l = 0; l < n; l++) W = affine_from_level(W, s->nodes[chain[l]].tm, s->nodes[chain[l]].pos);              // the node first
    for (int l = n - 1; l >= 0; l--) Winv = affine_to_level(Winv, s->nodes[chain[l]].itm, s->nodes[chain[l]].pos);   // the root first
    return true;
}

}  // namespace

extern "C" {

static int scene_motion(const RtuSceneDesc* prev, const RtuSceneDesc* cur, const uint32_t* deform_mesh_ids, int n_deform, const uint32_t* reset_mesh_ids,
                        int n_reset, RtuNodeMotion* out);

int rtu_scene_motion(const RtuSceneDesc* prev, const RtuSceneDesc* cur, const uint32_t* reset_mesh_ids, int n_reset, RtuNodeMotion* out) {
    return scene_motion(prev, cur, nullptr, 0, reset_mesh_ids, n_reset, out);
}

int rtu_scene_motion_deform(const RtuSceneDesc* prev, const RtuSceneDesc* cur, const uint32_t* deform_mesh_ids, int n_deform,
                            const uint32_t* reset_mesh_ids, int n_reset, RtuNodeMotion* out) {
    return scene_motion(prev, cur, deform_mesh_ids, n_deform, reset_mesh_ids, n_reset, out);
}

static int scene_motion(const RtuSceneDesc* prev, const RtuSceneDesc* cur, const uint32_t* deform_mesh_ids, int n_deform, const uint32_t* reset_mesh_ids,
                        int n_reset, RtuNodeMotion* out) {
    if (!prev || !cur || !out || n_reset < 0 || (n_reset > 0 && !reset_mesh_ids) || n_deform < 0 || (n_deform > 0 && !deform_mesh_ids)) return RTU_ERR_ARG;
    if ((prev->n_meshes && !prev->meshes) || (cur->n_meshes && !cur->meshes)) return RTU_ERR_ARG;
    for (int k = 0; k < n_reset; k++)
        if (reset_mesh_ids[k] >= cur->n_meshes) return RTU_ERR_ARG;
    for (int k = 0; k < n_deform; k++)
        if (deform_mesh_ids[k] >= cur->n_meshes) return RTU_ERR_ARG;
    // the shape rule of rtu_update_scene, except that a RESET mesh may have a reference tree of another size, as rtu_update_meshes allows
    RtuSceneDesc before = *prev;
    std::vector<RtuMesh> want;
    if (n_reset + n_deform > 0 && prev->n_meshes == cur->n_meshes) {  // (a DEFORM mesh went through rtu_update_meshes as well)
        want.assign(prev->meshes, prev->meshes + prev->n_meshes);
        for (int k = 0; k < n_reset; k++) want[reset_mesh_ids[k]].n_bvh_nodes = cur->meshes[reset_mesh_ids[k]].n_bvh_nodes;
        for (int k = 0; k < n_deform; k++) want[deform_mesh_ids[k]].n_bvh_nodes = cur->meshes[deform_mesh_ids[k]].n_bvh_nodes;
        before.meshes = want.data();
    }
    const int rc = rtu_scene_shape_diff(&before, cur, nullptr, 0);
    if (rc != RTU_OK) return rc;
    std::vector<uint8_t> same(cur->n_nodes);  // the node's own tm and pos are bit-identical, and so are its ancestors' (pre-order: a parent comes first)
    for (uint32_t i = 0; i < cur->n_nodes; i++) {
        const RtuNode &a = prev->nodes[i], &b = cur->nodes[i];
        if (a.parent >= (int32_t)i) return RTU_ERR_ARG;
        same[i] = memcmp(a.tm, b.tm, sizeof a.tm) == 0 && memcmp(a.pos, b.pos, sizeof a.pos) == 0 && (a.parent < 0 || same[a.parent]);
    }
    for (uint32_t i = 0; i < cur->n_nodes; i++) {
        RtuNodeMotion& o = out[i];
        memset(&o, 0, sizeof o);
        if (same[i]) {
            o.m[0] = o.m[5] = o.m[10] = 1.0f;
            o.g[0] = o.g[4] = o.g[8] = 1.0f;
            o.flags = RTU_MOTION_STATIC;
        } else {
            Affine64 Wp, Wpi, Wc, Wci;
            if (!node_chain(prev, i, Wp, Wpi) || !node_chain(cur, i, Wc, Wci)) return RTU_ERR_ARG;
            const Affine64 m = affine_compose(Wp, Wci), back = affine_compose(Wc, Wpi);
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) {
                    o.m[4 * r + c] = (float)m.A[3 * r + c];
                    o.g[3 * r + c] = (float)back.A[3 * c + r];
                }
                o.m[4 * r + 3] = (float)m.b[r];
            }
        }
        bool reset = false, deform = false;
        for (int k = 0; k < n_reset; k++)
            if (cur->nodes[i].mesh_id >= 0 && (uint32_t)cur->nodes[i].mesh_id == reset_mesh_ids[k]) reset = true;
        for (int k = 0; k < n_deform; k++)
            if (cur->nodes[i].mesh_id >= 0 && (uint32_t)cur->nodes[i].mesh_id == deform_mesh_ids[k]) deform = true;
        if (reset) {
            o.flags |= RTU_MOTION_RESET;  // (also a mesh in both lists)
        } else if (deform) {
            // a point of a deforming surface is given in the node's own coordinates (face, weights over the previous vertices):
            // m = W_prev, g = the transpose of the linear part of W_prev^-1
            Affine64 Wp, Wpi;
            if (!node_chain(prev, i, Wp, Wpi)) return RTU_ERR_ARG;
            memset(&o, 0, sizeof o);
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) {
                    o.m[4 * r + c] = (float)Wp.A[3 * r + c];
                    o.g[3 * r + c] = (float)Wpi.A[3 * c + r];
                }
                o.m[4 * r + 3] = (float)Wp.b[r];
            }
            o.flags = RTU_MOTION_DEFORM;
        }
    }
    return RTU_OK;
}

int rtu_keep_previous_vertices(RtuContext* ctx, int on) {
    if (!ctx) return RTU_ERR_ARG;
    if (ctx->keep_prev != (on != 0)) {
        RTU_HIP(ctx, hipSetDevice(ctx->device));
        RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (launches that read a previous generation)
        for (RtuContext::PrevGen& g : ctx->prev_gen) g.valid = false;  // previous is current until the next update
        ctx->df_dirty = true;
    }
    ctx->keep_prev = on != 0;
    return RTU_OK;
}

// CalculateImageOrigin + the u,v of CalculateCurrentPoint (RenderFunctions.cpp:243-269)
int rtu_frame_setup(const RtuCamera* cam, int width, int height, RtuFrameDesc* out) {
    if (!cam || !out || width <= 0 || height <= 0) return RTU_ERR_ARG;
    memset(out, 0, sizeof *out);
    out->width = width;
    out->height = height;
    out->shard_rank = 0;
    out->shard_count = 1;
    out->max_bounce = RTU_MAX_BOUNCE;
    out->collect_stats = 0;
    f3 pos = ld3(cam->pos), dir = ld3(cam->dir), up = ld3(cam->up);
    float distanceToImg = cam->focaldist;
    float actualHeight = (float)(tan((cam->fov / 2) * M_PI / 180.0) * 2 * distanceToImg);  // :247
    float actualWidth = ((float)width / (float)height) * actualHeight;                      // :248
    f3 dirN = norm3(dir), upN = norm3(up);
    f3 topCenterPoint = (pos + dirN * distanceToImg) + upN * (actualHeight / 2);            // :250
    f3 right = norm3(cross3(dirN, upN));
    f3 origin = topCenterPoint - right * (actualWidth / 2);                                 // :252
    f3 u = right * (actualWidth / (float)width);                                            // :263
    f3 v = (upN * -1.0f) * (actualHeight / (float)height);                                  // :264
    out->cam_pos[0] = pos.x; out->cam_pos[1] = pos.y; out->cam_pos[2] = pos.z;
    out->origin[0] = origin.x; out->origin[1] = origin.y; out->origin[2] = origin.z;
    out->u[0] = u.x; out->u[1] = u.y; out->u[2] = u.z;
    out->v[0] = v.x; out->v[1] = v.y; out->v[2] = v.z;
    // the lens disk of RenderFunctions.cpp:93: camera.up as given, normalize(dir x up)
    out->lens_up[0] = up.x; out->lens_up[1] = up.y; out->lens_up[2] = up.z;
    out->lens_right[0] = right.x; out->lens_right[1] = right.y; out->lens_right[2] = right.z;
    out->dof = cam->dof;
    return RTU_OK;
}

int rtu_shard_rows(const RtuFrameDesc* f) {
    if (!f || f->shard_count < 1 || f->shard_rank < 0 || f->shard_rank >= f->shard_count || f->height <= 0) return 0;
    int bands = shard_bands(f->height, f->shard_rank, f->shard_count);
    if (bands == 0) return 0;
    int last_global_band = (bands - 1) * f->shard_count + f->shard_rank;
    int rows = bands * RTU_BAND_ROWS;
    int over = (last_global_band + 1) * RTU_BAND_ROWS - f->height;
    if (over > 0) rows -= over;
    return rows;
}

int rtu_shard_max_rows(int height, int shard_count) {
    if (height <= 0 || shard_count < 1) return 0;
    return shard_bands(height, 0, shard_count) * RTU_BAND_ROWS;
}

int rtu_shard_global_row(const RtuFrameDesc* f, int local_row) {
    if (!f || local_row < 0) return -1;
    int lb = local_row / RTU_BAND_ROWS;
    return (lb * f->shard_count + f->shard_rank) * RTU_BAND_ROWS + local_row % RTU_BAND_ROWS;
}

int rtu_render_frame_device(RtuContext* ctx, const RtuFrameDesc* frame, void* d_rgbz, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = check_frame(ctx, frame);
    if (rc != RTU_OK) return rc;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (!d_rgbz && rtu_shard_rows(frame) > 0) return fail(ctx, RTU_ERR_ARG, "d_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;  // NULL is the device's default (null) stream
    if (frame->samples >= 1) return render_sampled(ctx, frame, (float4*)d_rgbz, st, true);
    return launch(ctx, frame, (float4*)d_rgbz, st, true);
}

int rtu_render_frames_device(RtuContext* ctx, const RtuFrameDesc* frames, int n_frames, void* d_rgbz, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (!frames || n_frames < 1 || n_frames > RTU_MAX_FRAMES_IN_FLIGHT) return fail(ctx, RTU_ERR_ARG, "1..%d frames per call", RTU_MAX_FRAMES_IN_FLIGHT);
    for (int i = 0; i < n_frames; i++) {
        int rc = check_frame(ctx, &frames[i]);
        if (rc != RTU_OK) return rc;
        const RtuFrameDesc &f = frames[i], &g = frames[0];
        if (f.samples != 0) return fail(ctx, RTU_ERR_ARG, "frames in flight are frames of recipe W (samples == 0)");
        if (f.width != g.width || f.height != g.height || f.shard_rank != g.shard_rank || f.shard_count != g.shard_count ||
            f.max_bounce != g.max_bounce || f.collect_stats != g.collect_stats || f.coop_threshold != g.coop_threshold)
            return fail(ctx, RTU_ERR_ARG, "frames in flight differ in more than their cameras");
    }
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    const size_t pixels = (size_t)rtu_shard_rows(&frames[0]) * (size_t)frames[0].width;
    if (pixels == 0) return RTU_OK;
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "d_rgbz is NULL");
    if (pixels * (size_t)n_frames > ((size_t)1 << 26)) return fail(ctx, RTU_ERR_ARG, "more than 2^26 pixels in flight");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    static_assert(RTU_MAX_FRAMES_IN_FLIGHT == RTU_MAX_FRAME_BATCH, "batch size");
    return launch(ctx, &frames[0], (float4*)d_rgbz, (hipStream_t)hip_stream, true, 0, n_frames, frames);
}

int rtu_pack_image_device(RtuContext* ctx, const void* d_rgbz, size_t n_pixels, void* d_z, void* d_rgb8, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (n_pixels == 0) return RTU_OK;
    if (!d_rgbz || !d_z || !d_rgb8) return fail(ctx, RTU_ERR_ARG, "NULL buffer");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = (hipError_t)rtu_launch_pack_image((const float4*)d_rgbz, (unsigned long long)n_pixels, (float*)d_z, (unsigned char*)d_rgb8, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_minmax_z_device(RtuContext* ctx, const void* d_rgbz, size_t pixels_per_frame, int n_frames, void* d_minmax, void* hip_stream) {
    if (!ctx || n_frames < 0 || pixels_per_frame > 0xFFFFFFFFull) return RTU_ERR_ARG;
    if (n_frames == 0) return RTU_OK;
    if (!d_minmax || (pixels_per_frame != 0 && !d_rgbz)) return fail(ctx, RTU_ERR_ARG, "NULL buffer");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    if (pixels_per_frame == 0) {
        // a shard without rows (fewer 8-row bands than ranks) still takes part in the all-reduce MIN of the keys: it must contribute
        // the "nothing yet" keys, not whatever the buffer held (zeros would win every MIN and turn the z-image of EVERY rank black)
        RTU_HIP(ctx, hipMemsetAsync(d_minmax, 0x7F, sizeof(long long) * 2 * (size_t)n_frames, (hipStream_t)hip_stream));
        return RTU_OK;
    }
    hipError_t e = (hipError_t)rtu_launch_minmax_z((const float4*)d_rgbz, (uint32_t)pixels_per_frame, (uint32_t)n_frames, (long long*)d_minmax, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_pack_output_device(RtuContext* ctx, const void* d_rgbz, size_t pixels_per_frame, int n_frames, const void* d_minmax, void* d_out4, void* hip_stream) {
    if (!ctx || n_frames < 0 || pixels_per_frame > 0xFFFFFFFFull) return RTU_ERR_ARG;
    if (pixels_per_frame == 0 || n_frames == 0) return RTU_OK;
    if (!d_rgbz || !d_minmax || !d_out4) return fail(ctx, RTU_ERR_ARG, "NULL buffer");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = (hipError_t)rtu_launch_pack_output((const float4*)d_rgbz, (uint32_t)pixels_per_frame, (uint32_t)n_frames, (const long long*)d_minmax,
                                                      (unsigned char*)d_out4, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_get_stats(RtuContext* ctx, RtuStats* stats) {
    if (!ctx || !stats) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipDeviceSynchronize());
    static_assert(sizeof(RtuStats) == 11 * sizeof(unsigned long long), "RtuStats layout");
    RTU_HIP(ctx, hipMemcpy(stats, ctx->counters.get(), sizeof(RtuStats), hipMemcpyDeviceToHost));
    std::unique_ptr<FrameCounters> hp(new FrameCounters);  // a quarter of a megabyte: not on the stack
    FrameCounters& h = *hp;
    RTU_HIP(ctx, hipMemcpy(&h, ctx->fcnt.get(), sizeof h, hipMemcpyDeviceToHost));
    if (!h.overflow) learn_tail(ctx, h, nullptr);  // (after a counting render: no side mode)
    return RTU_OK;
}

int rtu_get_touched(RtuContext* ctx, RtuTouched* per_slot, int n_slots) {
    if (!ctx || !per_slot || n_slots < 1) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipDeviceSynchronize());
    std::vector<unsigned long long> h((size_t)RTU_TL_KERNELS * RTU_TOUCH_STRIDE);
    RTU_HIP(ctx, hipMemcpy(h.data(), ctx->counters.get(), kCounterBytes, hipMemcpyDeviceToHost));
    static_assert(sizeof(RtuTouched) == RTU_TOUCH_FIELDS * sizeof(unsigned long long), "RtuTouched layout");
    static_assert(RTU_KERNEL_SLOTS == RTU_TL_KERNELS, "slot count");
    const int n = n_slots < RTU_TL_KERNELS ? n_slots : RTU_TL_KERNELS;
    for (int k = 0; k < n; k++) memcpy(&per_slot[k], &h[(size_t)k * RTU_TOUCH_STRIDE], sizeof(RtuTouched));
    return n;
}

int rtu_get_touched_launches(RtuContext* ctx, uint32_t* per_slot, int n_slots) {
    if (!ctx || !per_slot || n_slots < 0) return RTU_ERR_ARG;
    const int n = n_slots < RTU_TL_KERNELS ? n_slots : RTU_TL_KERNELS;
    for (int i = 0; i < n; i++) per_slot[i] = ctx->slot_launches[i];
    return n;
}

unsigned long long rtu_touched_bytes(const RtuTouched* t, int textured) {
    if (!t) return 0;
    return 24ull * t->bound_tests + 48ull * t->node_tests + 24ull * t->mesh_box_tests + 84ull * t->xform_levels + 112ull * t->inner4 + 256ull * t->inner8 +
           64ull * t->inner_ref + 64ull * t->tri_tests + (textured ? 148ull : 100ull) * t->winners + t->record_bytes;
}

const char* rtu_kernel_slot_name(int slot) {
    static const char* const level_kernels[4] = {"k_trace", "k_trace2c", "k_trace2", "k_consume"};
    static char buf[RTU_TL_KERNELS][24];
    if (slot < 0 || slot >= RTU_TL_KERNELS) return "";
    if (slot == 0) return "k_primary";
    if (slot == 1) return "k_primary2c";
    if (slot == 2) return "k_primary2";
    if (slot < 3 + 4 * RTU_MAX_LEVELS) snprintf(buf[slot], sizeof buf[slot], "%s(L%d)", level_kernels[(slot - 3) % 4], (slot - 3) / 4);
    else if (slot < 3 + 5 * RTU_MAX_LEVELS) snprintf(buf[slot], sizeof buf[slot], "k_combine(L%d)", slot - (3 + 4 * RTU_MAX_LEVELS));
    else if (slot == 3 + 5 * RTU_MAX_LEVELS) return "k_gi_roots";
    else if (slot == 4 + 5 * RTU_MAX_LEVELS) return "k_tail(side)";
    else return "";
    return buf[slot];
}

int rtu_probe_kernel(RtuContext* ctx, int slot) {
    if (!ctx || slot >= RTU_TL_KERNELS) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    if (slot >= 0 && !ctx->probe_ev[0])
        for (hipEvent_t& e : ctx->probe_ev) RTU_HIP(ctx, hipEventCreate(&e));
    ctx->probe_slot = slot < 0 ? -1 : slot;
    if (slot >= 0) ctx->probe_used = 0;  // stopping keeps what was measured until it is read
    return RTU_OK;
}

int rtu_probe_read(RtuContext* ctx, float* total_ms_out, int* launches_out) {
    if (!ctx || !total_ms_out || !launches_out) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipDeviceSynchronize());
    float total = 0;
    for (int i = 0; i < ctx->probe_used; i++) {
        float ms = 0;
        RTU_HIP(ctx, hipEventElapsedTime(&ms, ctx->probe_ev[2 * i], ctx->probe_ev[2 * i + 1]));
        total += ms;
    }
    *total_ms_out = total;
    *launches_out = ctx->probe_used;
    ctx->probe_used = 0;
    return RTU_OK;
}

int rtu_render_frame(RtuContext* ctx, const RtuFrameDesc* frame, float* h_rgbz, RtuStats* stats) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = check_frame(ctx, frame);
    if (rc != RTU_OK) return rc;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (!h_rgbz) return fail(ctx, RTU_ERR_ARG, "h_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    size_t rows = (size_t)rtu_shard_rows(frame);
    size_t bytes = rows * (size_t)frame->width * sizeof(float4);
    RTU_HIP(ctx, ctx->fb.grow(rows * (size_t)frame->width));
    RtuFrameDesc f = *frame;
    if (stats) f.collect_stats = 1;
    for (int attempt = 0;; attempt++) {
        if (f.samples >= 1) {  // recipe S settles its capacities pass by pass
            if ((rc = render_sampled(ctx, &f, ctx->fb.get(), ctx->stream, true)) != RTU_OK) return rc;
            RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
            break;
        }
        rc = launch(ctx, &f, ctx->fb.get(), ctx->stream, true);
        if (rc != RTU_OK) return rc;
        RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
        bool overflow = false;
        if ((rc = check_overflow(ctx, &overflow)) != RTU_OK) return rc;
        if (!overflow) break;
        // more frames than provisioned: check_overflow has raised the wanted capacities; render again
        // (every round settles at least one more recursion level)
        if (attempt >= 2 * RTU_MAX_LEVELS) return fail(ctx, RTU_ERR_CAPACITY, "recursion frames still exceed the capacity after %d rounds", attempt);
    }
    if (bytes) RTU_HIP(ctx, hipMemcpy(h_rgbz, ctx->fb.get(), bytes, hipMemcpyDeviceToHost));
    if (stats) return rtu_get_stats(ctx, stats);
    return RTU_OK;
}

int rtu_adaptive_defaults(RtuAdaptiveDesc* out) {
    if (!out) return RTU_ERR_ARG;
    out->min_samples = 8;           // minSampleSize, RenderFunctions.cpp:27
    out->increment = 1;             // sampleIncrement, :29
    out->target_variance = 0.005f;  // targetVariance, :28
    out->max_batch = 0;
    return RTU_OK;
}

int rtu_render_frame_adaptive_device(RtuContext* ctx, const RtuFrameDesc* frame, const RtuAdaptiveDesc* adaptive, void* d_rgbz, void* d_counts,
                                     void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = check_adaptive(ctx, frame, adaptive);
    if (rc != RTU_OK) return rc;
    if (!d_rgbz && rtu_shard_rows(frame) > 0) return fail(ctx, RTU_ERR_ARG, "d_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    SampledRun run;
    run.ad = adaptive;
    run.d_counts = (uint8_t*)d_counts;
    return render_sampled(ctx, frame, (float4*)d_rgbz, (hipStream_t)hip_stream, true, &run);
}

int rtu_render_frame_adaptive(RtuContext* ctx, const RtuFrameDesc* frame, const RtuAdaptiveDesc* adaptive, float* h_rgbz, uint8_t* h_counts,
                              RtuStats* stats) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = check_adaptive(ctx, frame, adaptive);
    if (rc != RTU_OK) return rc;
    if (!h_rgbz) return fail(ctx, RTU_ERR_ARG, "h_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pixels = (size_t)rtu_shard_rows(frame) * (size_t)frame->width;
    RTU_HIP(ctx, ctx->fb.grow(pixels));
    RtuFrameDesc f = *frame;
    if (stats) f.collect_stats = 1;
    SampledRun run;
    run.ad = adaptive;
    if ((rc = render_sampled(ctx, &f, ctx->fb.get(), ctx->stream, true, &run)) != RTU_OK) return rc;
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (pixels) {
        RTU_HIP(ctx, hipMemcpy(h_rgbz, ctx->fb.get(), pixels * sizeof(float4), hipMemcpyDeviceToHost));
        if (h_counts) RTU_HIP(ctx, hipMemcpy(h_counts, ctx->ad_counts.get(), pixels, hipMemcpyDeviceToHost));
    }
    if (stats) return rtu_get_stats(ctx, stats);
    return RTU_OK;
}

int rtu_debug_sample_images(RtuContext* ctx, const RtuFrameDesc* frame, int first, int n, float* h_out) {
    if (!ctx) return RTU_ERR_ARG;
    if (frame && frame->samples < 1) return fail(ctx, RTU_ERR_ARG, "a recipe S / P frame (samples >= 1)");
    int rc = check_frame(ctx, frame);
    if (rc != RTU_OK) return rc;
    if (first < 0 || n < 1 || first > frame->samples - n) return fail(ctx, RTU_ERR_ARG, "samples [first, first + n) must lie in [0, frame.samples)");
    if (!h_out) return fail(ctx, RTU_ERR_ARG, "h_out is NULL");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RtuFrameDesc f = *frame;
    f.collect_stats = 0;
    SampledRun run;
    run.h_dump = h_out;
    run.first = first;
    run.end = first + n;
    return render_sampled(ctx, &f, nullptr, ctx->stream, true, &run);
}

RtuProgressive* rtu_progressive_begin(RtuContext* ctx, const RtuFrameDesc* frame, const RtuAdaptiveDesc* adaptive, int* err_out) {
    auto refuse = [&](int rc) -> RtuProgressive* {
        if (err_out) *err_out = rc;
        return nullptr;
    };
    if (!ctx) return refuse(RTU_ERR_ARG);
    if (!frame) return refuse(fail(ctx, RTU_ERR_ARG, "frame is NULL"));
    if (frame->samples < 1) return refuse(fail(ctx, RTU_ERR_ARG, "a progressive frame is a recipe S / P frame (samples >= 1)"));
    if (frame->collect_stats != 0)
        return refuse(fail(ctx, RTU_ERR_ARG, "a progressive frame has no counters (collect_stats == 0): the counting variant restarts from sample 0"));
    int rc = adaptive ? check_adaptive(ctx, frame, adaptive) : check_frame(ctx, frame);
    if (rc != RTU_OK) return refuse(rc);
    if (!ctx->has_scene) return refuse(fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded"));
    if (hipSetDevice(ctx->device) != hipSuccess) return refuse(fail(ctx, RTU_ERR_HIP, "hipSetDevice failed"));
    std::unique_ptr<RtuProgressive> p(new RtuProgressive);
    p->frame = *frame;
    p->adaptive = adaptive != nullptr;
    if (adaptive) p->ad = *adaptive;
    p->scene_gen = ctx->scene_gen;
    p->pixels = (size_t)rtu_shard_rows(frame) * (size_t)frame->width;
    p->tiles = (uint32_t)((frame->width + 7) / 8) * (uint32_t)shard_bands(frame->height, frame->shard_rank, frame->shard_count);
    p->batch = p->pixels ? sampled_batch(frame, adaptive, p->pixels) : 1;
    hipError_t e = p->acc.grow(p->pixels);
    if (e == hipSuccess) e = p->hits.grow(p->pixels);
    if (e == hipSuccess && adaptive) {
        e = p->sq.grow(p->pixels);
        if (e == hipSuccess) e = p->counts.grow(p->pixels);
        for (DevBuf<uint4>& l : p->list)
            if (e == hipSuccess) e = l.grow(p->tiles);
        if (e == hipSuccess) e = p->n_dev.grow(2);
        if (e == hipSuccess) e = p->n_host.grow(1);
    }
    if (e != hipSuccess) return refuse(fail(ctx, RTU_ERR_HIP, "session buffers: %s", hipGetErrorString(e)));
    p->sums.acc = p->acc.get();
    p->sums.hits = p->hits.get();
    p->sums.sq = p->sq.get();
    p->sums.counts = p->counts.get();
    p->sums.list[0] = p->list[0].get();
    p->sums.list[1] = p->list[1].get();
    p->sums.n_dev = p->n_dev.get();
    p->sums.n_host = p->n_host.get();
    p->sums.n_act = p->tiles;
    p->ctx = ctx;
    ctx->sessions.push_back(p.get());
    if (err_out) *err_out = RTU_OK;
    return p.release();
}

int rtu_progressive_advance(RtuProgressive* p, int n_samples, void* hip_stream) {
    if (!p || !p->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = p->ctx;
    const int S = p->frame.samples;
    if (n_samples < 1 || n_samples > S - p->done) return fail(ctx, RTU_ERR_ARG, "samples [%d, %d + %d) do not lie in [0, %d)", p->done, p->done, n_samples, S);
    if (p->scene_gen != ctx->scene_gen) return fail(ctx, RTU_ERR_STALE, "the context got a new scene after this session began");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const int end = p->done + n_samples;
    if (p->pixels == 0 || (p->adaptive && p->done > 0 && p->sums.n_act == 0)) {  // nothing to trace: no rows, or every pixel has stopped
        p->done = end;
        return RTU_OK;
    }
    RTU_HIP(ctx, ctx->sample_buf.grow(p->pixels * (size_t)p->batch));
    SampledRun run;
    run.ad = p->adaptive ? &p->ad : nullptr;
    const hipStream_t stream = (hipStream_t)hip_stream;
    int reached = p->done;
    const int rc = sample_batches(ctx, &p->frame, stream, p->done == 0, &run, p->sums, p->done, end, p->batch, &reached);
    // the sums hold every batch added so far, whatever ended the call; the last one may still be queued
    const hipError_t e = hipStreamSynchronize(stream);
    p->done = reached;
    if (rc != RTU_OK) return rc;
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_progressive_status(const RtuProgressive* p, int32_t* samples_done, uint32_t* live_tiles) {
    if (!p || !p->ctx) return RTU_ERR_ARG;
    if (samples_done) *samples_done = p->done;
    if (live_tiles) {
        if (p->adaptive) *live_tiles = p->done == 0 ? p->tiles : p->sums.n_act;
        else *live_tiles = p->done < p->frame.samples ? p->tiles : 0u;
    }
    return RTU_OK;
}

int rtu_progressive_snapshot_device(RtuProgressive* p, void* d_rgbz, void* d_counts, void* hip_stream) {
    if (!p || !p->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = p->ctx;
    if (p->done == 0) return fail(ctx, RTU_ERR_ARG, "no samples yet: advance the session first");
    if (d_counts && p->frame.samples > 255) return fail(ctx, RTU_ERR_ARG, "counts are bytes: a session with more than 255 samples has none");
    if (p->pixels == 0) return RTU_OK;
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "d_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = (hipError_t)rtu_launch_progressive_snapshot(p->acc.get(), p->hits.get(), p->adaptive ? p->counts.get() : nullptr, (uint32_t)p->done,
                                                               (float4*)d_rgbz, (uint8_t*)d_counts, (uint32_t)p->pixels, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_progressive_snapshot(RtuProgressive* p, float* h_rgbz, uint8_t* h_counts) {
    if (!p || !p->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = p->ctx;
    if (p->done == 0) return fail(ctx, RTU_ERR_ARG, "no samples yet: advance the session first");
    if (h_counts && p->frame.samples > 255) return fail(ctx, RTU_ERR_ARG, "counts are bytes: a session with more than 255 samples has none");
    if (p->pixels == 0) return RTU_OK;
    if (!h_rgbz) return fail(ctx, RTU_ERR_ARG, "h_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->fb.grow(p->pixels));
    int rc = rtu_progressive_snapshot_device(p, ctx->fb.get(), nullptr, ctx->stream);
    if (rc != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpyAsync(h_rgbz, ctx->fb.get(), p->pixels * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    if (h_counts && p->adaptive) RTU_HIP(ctx, hipMemcpyAsync(h_counts, p->counts.get(), p->pixels, hipMemcpyDeviceToHost, ctx->stream));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_counts && !p->adaptive) memset(h_counts, p->done, p->pixels);  // what k_progressive_snapshot writes for a fixed session
    return RTU_OK;
}

void rtu_progressive_free(RtuProgressive* p) {
    if (!p) return;
    if (RtuContext* ctx = p->ctx) {
        (void)hipSetDevice(ctx->device);
        ctx->sessions.erase(std::remove(ctx->sessions.begin(), ctx->sessions.end(), p), ctx->sessions.end());
    }
    delete p;
}

int rtu_frame_status(RtuContext* ctx) {
    if (!ctx) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipDeviceSynchronize());
    bool overflow = false;
    int rc = check_overflow(ctx, &overflow);
    if (rc != RTU_OK) return rc;
    if (overflow) {
        return fail(ctx, RTU_ERR_CAPACITY, "recursion frames exceeded the provisioned capacity (or the tail kernel refused its cut level); render the frame again");
    }
    return RTU_OK;
}

int rtu_time_render(RtuContext* ctx, const RtuFrameDesc* frame, void* d_rgbz, void* hip_stream, int iters, float* avg_ms_out) {
    if (!ctx || !avg_ms_out || iters < 1) return RTU_ERR_ARG;
    int rc = check_frame(ctx, frame);
    if (rc != RTU_OK) return rc;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "d_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    RTU_HIP(ctx, hipEventRecord(ctx->ev0, st));
    for (int i = 0; i < iters; i++) {
        rc = frame->samples >= 1 ? render_sampled(ctx, frame, (float4*)d_rgbz, st, i == 0) : launch(ctx, frame, (float4*)d_rgbz, st, i == 0);
        if (rc != RTU_OK) return rc;
    }
    RTU_HIP(ctx, hipEventRecord(ctx->ev1, st));
    RTU_HIP(ctx, hipEventSynchronize(ctx->ev1));
    {
        bool overflow = false;
        if ((rc = check_overflow(ctx, &overflow)) != RTU_OK) return rc;
        if (overflow) return fail(ctx, RTU_ERR_CAPACITY, "recursion frames exceeded the provisioned capacity; time the frame again");
    }
    float ms = 0;
    RTU_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *avg_ms_out = ms / (float)iters;
    return RTU_OK;
}

int rtu_render_timeline(RtuContext* ctx, const RtuFrameDesc* frame, void* d_rgbz, int max_entries, int* slot_out, double* start_us_out,
                        double* end_us_out) {
    if (!ctx || !slot_out || !start_us_out || !end_us_out || max_entries < 1) return RTU_ERR_ARG;
    int rc = check_frame(ctx, frame);
    if (rc != RTU_OK) return rc;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "d_rgbz is NULL");
    if (frame->samples != 0) return fail(ctx, RTU_ERR_ARG, "the timeline is of one launch sequence of recipe W (samples == 0)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)RTU_TL_KERNELS * RTU_TL_STRIDE;
    RTU_HIP(ctx, ctx->tl.grow(n));
    RTU_HIP(ctx, hipMemsetAsync(ctx->tl.get(), 0, n * sizeof(unsigned long long), ctx->stream));
    ctx->stamp_next = true;
    rc = launch(ctx, frame, (float4*)d_rgbz, ctx->stream, true);
    ctx->stamp_next = false;
    if (rc != RTU_OK) return rc;
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    {
        bool overflow = false;
        if ((rc = check_overflow(ctx, &overflow)) != RTU_OK) return rc;  // also learns where the tail kernel may take over
        if (overflow) return fail(ctx, RTU_ERR_CAPACITY, "recursion frames exceeded the provisioned capacity; render the frame again");
    }
    std::vector<unsigned long long> h(n);
    RTU_HIP(ctx, hipMemcpy(h.data(), ctx->tl.get(), n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    int khz = 0;
    RTU_HIP(ctx, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    if (khz <= 0) khz = 100000;
    unsigned long long lo[RTU_TL_KERNELS], hi[RTU_TL_KERNELS], t0 = ~0ull;
    for (int k = 0; k < RTU_TL_KERNELS; k++) {
        lo[k] = ~0ull; hi[k] = 0;
        const unsigned long long* row = h.data() + (size_t)k * RTU_TL_STRIDE;
        for (uint32_t j = 0; j < 64; j++) if (row[j] && row[j] < lo[k]) lo[k] = row[j];
        for (uint32_t j = 64; j < RTU_TL_STRIDE; j++) if (row[j] > hi[k]) hi[k] = row[j];
        if (hi[k] && lo[k] < t0) t0 = lo[k];
    }
    int cnt = 0;
    for (int k = 0; k < RTU_TL_KERNELS && cnt < max_entries; k++) {
        if (hi[k] == 0 || lo[k] == ~0ull) continue;  // not launched
        slot_out[cnt] = k;
        start_us_out[cnt] = (double)(lo[k] - t0) * 1e3 / (double)khz;
        end_us_out[cnt] = (double)(hi[k] - t0) * 1e3 / (double)khz;
        cnt++;
    }
    return cnt;
}

int rtu_timeline_exits(RtuContext* ctx, int slot, int max_values, double* exit_us_out) {
    if (!ctx || !exit_us_out || slot < 0 || slot >= RTU_TL_KERNELS || max_values < 1) return RTU_ERR_ARG;
    if (!ctx->tl.get()) return fail(ctx, RTU_ERR_ARG, "no timeline recorded yet (rtu_render_timeline)");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned long long> h(RTU_TL_STRIDE);
    RTU_HIP(ctx, hipMemcpy(h.data(), ctx->tl.get() + (size_t)slot * RTU_TL_STRIDE, RTU_TL_STRIDE * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    int khz = 0;
    RTU_HIP(ctx, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    if (khz <= 0) khz = 100000;
    unsigned long long t0 = ~0ull;
    for (uint32_t j = 0; j < 64; j++) if (h[j] && h[j] < t0) t0 = h[j];
    if (t0 == ~0ull) return 0;
    int n = 0;
    for (uint32_t j = 64; j < RTU_TL_STRIDE && n < max_values; j++)
        if (h[j]) exit_us_out[n++] = (double)(h[j] - t0) * 1e3 / (double)khz;
    return n;
}

int rtu_set_cancel_flag(RtuContext* ctx, const volatile int* flag) {
    if (!ctx) return RTU_ERR_ARG;
    ctx->cancel = flag;
    return RTU_OK;
}

int rtu_debug_tail_from(RtuContext* ctx, int level) {
    if (!ctx || level < 1 || level > RTU_MAX_LEVELS) return RTU_ERR_ARG;
    ctx->tail_hint = level;
    return RTU_OK;
}

int rtu_debug_last_tail_from(RtuContext* ctx) {
    if (!ctx) return RTU_ERR_ARG;
    return ctx->last_tail_from;
}

int rtu_set_sequences_in_flight(RtuContext* ctx, int n) {
    if (!ctx || n < 1) return RTU_ERR_ARG;
    ctx->sequences_in_flight = n;
    return RTU_OK;
}

int rtu_debug_flags(RtuContext* ctx, uint32_t bits) {
    if (!ctx) return RTU_ERR_ARG;
    ctx->dbg = bits;
    return RTU_OK;
}

int rtu_debug_node_bounds(RtuContext* ctx, int on) {
    if (!ctx) return RTU_ERR_ARG;
    ctx->dscene.node_bounds = on ? 1u : 0u;
    return RTU_OK;
}

int rtu_debug_walk_stack_limit(RtuContext* ctx, uint32_t entries) {
    if (!ctx || entries < 1) return RTU_ERR_ARG;
    ctx->dscene.walk_stack_limit = entries;
    return RTU_OK;
}

int rtu_mesh_info(const RtuContext* ctx, uint32_t mesh, uint32_t* out5) {
    if (!ctx || !out5 || mesh >= ctx->mesh_info.size()) return RTU_ERR_ARG;
    const RtuContext::MeshInfo& i = ctx->mesh_info[mesh];
    out5[0] = i.faces; out5[1] = i.sah_depth; out5[2] = i.stack4; out5[3] = i.nodes4; out5[4] = i.nodes8;
    return RTU_OK;
}

int rtu_debug_light_list(const RtuSceneDesc* s, uint32_t light_slot, uint32_t cover_slot, RtuLightListDump* out) {
    if (!out) return RTU_ERR_ARG;
    memset(out, 0, sizeof *out);
    RtuContext tmp;  // plain host state: nothing here touches a GPU
    int rc = validate(&tmp, s);
    if (rc != RTU_OK) return rc;
    int li = -1, node = -1;
    uint32_t seen = 0;
    for (uint32_t i = 0; i < s->n_lights; i++)
        if (s->lights[i].type != RTU_LIGHT_AMBIENT && seen++ == light_slot) { li = (int)i; break; }
    seen = 0;
    for (uint32_t i = 0; i < s->n_nodes && i < 64u; i++)
        if (s->nodes[i].obj_type == RTU_OBJ_TRIMESH && seen++ == cover_slot) { node = (int)i; break; }
    if (li < 0 || node < 0) return RTU_ERR_ARG;
    std::vector<DevNode> nodes(s->n_nodes);
    const float wbound = world_bounds(s, nodes);
    WorldFar far;
    world_far(s, wbound, far);
    const float wscale = far.wlist;  // (the lists carry the margin of the shadow rays that look them up)
    SahTree sah;
    build_sah(s->meshes[s->nodes[node].mesh_id], sah);
    CoverMesh cm;
    make_cover_mesh(s, (uint32_t)node, sah.elements, cm);
    HostLightList hl;
    out->node = node;
    out->light = li;
    if (!compute_light_list(s->lights[li], cm, wscale, hl)) return RTU_OK;  // usable == 0
    out->usable = 1;
    out->G = hl.m.G;
    out->point = hl.m.point;
    memcpy(out->X, hl.m.X, sizeof out->X); memcpy(out->Y, hl.m.Y, sizeof out->Y); memcpy(out->Z, hl.m.Z, sizeof out->Z); memcpy(out->L, hl.m.L, sizeof out->L);
    out->u0 = hl.m.u0; out->v0 = hl.m.v0; out->su = hl.m.su; out->sv = hl.m.sv;
    out->n_entries = (uint32_t)(hl.ent.size() / 2);
    out->cell_off = (uint32_t*)malloc(hl.off.size() * sizeof(uint32_t));
    out->entry_face = (uint32_t*)malloc((hl.ent.size() / 2 + 1) * sizeof(uint32_t));
    out->entry_zmin = (float*)malloc((hl.ent.size() / 2 + 1) * sizeof(float));
    if (!out->cell_off || !out->entry_face || !out->entry_zmin) { rtu_debug_light_list_free(out); return RTU_ERR_ARG; }
    memcpy(out->cell_off, hl.off.data(), hl.off.size() * sizeof(uint32_t));
    for (size_t e = 0; e < hl.ent.size() / 2; e++) {
        out->entry_face[e] = sah.elements[hl.ent[2 * e]];  // slot of the fast tree -> face of the mesh
        memcpy(&out->entry_zmin[e], &hl.ent[2 * e + 1], 4);
    }
    return RTU_OK;
}

void rtu_debug_light_list_free(RtuLightListDump* d) {
    if (!d) return;
    free(d->cell_off); free(d->entry_face); free(d->entry_zmin);
    d->cell_off = nullptr; d->entry_face = nullptr; d->entry_zmin = nullptr;
}

int rtu_debug_context_light_list(RtuContext* ctx, uint32_t index, RtuLightListDump* out) {
    if (!ctx || !out) return RTU_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (index >= ctx->light_list_info.size()) return fail(ctx, RTU_ERR_ARG, "no list %u", index);
    const RtuContext::LightListInfo& li = ctx->light_list_info[index];
    const uint32_t nc = ctx->dscene.n_cover;
    const DevLightMask& m = ctx->lmask_host[(size_t)li.light * nc + li.cover];
    const int node = ctx->dscene.cover_node[li.cover];
    const std::vector<uint32_t>& elements = ctx->fast_elements[(size_t)ctx->shape_nodes[(size_t)node].mesh_id];
    out->node = node;
    out->light = ctx->shadow_light[li.light];
    out->usable = 1;
    out->G = m.G;
    out->point = m.point;
    memcpy(out->X, m.X, sizeof out->X); memcpy(out->Y, m.Y, sizeof out->Y); memcpy(out->Z, m.Z, sizeof out->Z); memcpy(out->L, m.L, sizeof out->L);
    out->u0 = m.u0; out->v0 = m.v0; out->su = m.su; out->sv = m.sv;
    out->n_entries = li.entries;
    const size_t n_off = (size_t)m.G * m.G + 1;
    std::vector<uint32_t> ent(2 * (size_t)li.entries);
    out->cell_off = (uint32_t*)malloc(n_off * sizeof(uint32_t));
    out->entry_face = (uint32_t*)malloc(((size_t)li.entries + 1) * sizeof(uint32_t));
    out->entry_zmin = (float*)malloc(((size_t)li.entries + 1) * sizeof(float));
    if (!out->cell_off || !out->entry_face || !out->entry_zmin) { rtu_debug_light_list_free(out); return RTU_ERR_ARG; }
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipMemcpy(out->cell_off, m.cell_off, n_off * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (!ent.empty()) RTU_HIP(ctx, hipMemcpy(ent.data(), m.cell_tri, ent.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < li.entries; e++) {
        const uint32_t slot = ent[2 * e];
        out->entry_face[e] = slot < elements.size() ? elements[slot] : 0xFFFFFFFFu;  // slot of the fast tree -> face of the mesh
        memcpy(&out->entry_zmin[e], &ent[2 * e + 1], 4);
    }
    return RTU_OK;
}

int rtu_debug_update_timing(RtuContext* ctx, int on, float* ms_out5) {
    if (!ctx) return RTU_ERR_ARG;
    if (!ctx->llb) ctx->llb = ll_builder_create();
    LlTimes t;
    ll_get_times(ctx->llb, &t, true);
    if (ms_out5) { ms_out5[0] = t.cover_ms; ms_out5[1] = t.extent_ms; ms_out5[2] = t.count_ms; ms_out5[3] = t.fill_ms; ms_out5[4] = t.sort_ms; }
    (void)hipSetDevice(ctx->device);
    ll_set_timing(ctx->llb, on != 0);
    return RTU_OK;
}

int rtu_light_list_info(const RtuContext* ctx, uint32_t index, uint32_t* out5) {
    if (!ctx || !out5) return RTU_ERR_ARG;
    if (index >= ctx->light_list_info.size()) return RTU_ERR_ARG;
    const RtuContext::LightListInfo& i = ctx->light_list_info[index];
    out5[0] = i.light; out5[1] = i.cover; out5[2] = i.G; out5[3] = i.entries; out5[4] = i.longest;
    return RTU_OK;
}

int rtu_frame_counts(RtuContext* ctx, uint32_t* frames_out, uint32_t* deferred_out) {
    if (!ctx || !frames_out || !deferred_out) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipDeviceSynchronize());
    std::unique_ptr<FrameCounters> hp(new FrameCounters);  // a quarter of a megabyte: not on the stack
    FrameCounters& h = *hp;
    RTU_HIP(ctx, hipMemcpy(&h, ctx->fcnt.get(), sizeof h, hipMemcpyDeviceToHost));
    for (int L = 0; L < RTU_MAX_LEVELS; L++) {
        frames_out[L] = 0;
        for (int s = 0; s < RTU_SHARDS; s++) frames_out[L] += h.n_frames[L][(s) * RTU_CSTRIDE];
    }
    for (int p = 0; p <= RTU_MAX_LEVELS; p++) {
        deferred_out[p] = 0;
        for (int s = 0; s < RTU_SHARDS; s++) deferred_out[p] += h.n_defer[p][(s) * RTU_CSTRIDE];
    }
    if (ctx->last_side) {  // side mode: the primary phase's defer list and the frames its stage 2 made are counted apart (KernelArgs::fcnt0)
        RTU_HIP(ctx, hipMemcpy(&h, ctx->fcnt_side.get(), sizeof h, hipMemcpyDeviceToHost));
        for (int L = 0; L < RTU_MAX_LEVELS; L++)
            for (int s = 0; s < RTU_SHARDS; s++) frames_out[L] += h.n_frames[L][(s) * RTU_CSTRIDE];
        for (int s = 0; s < RTU_SHARDS; s++) deferred_out[0] += h.n_defer[0][(s) * RTU_CSTRIDE];
    }
    return RTU_OK;
}

int rtu_selftest_division(RtuContext* ctx, unsigned long long n_pairs, unsigned long long seed, unsigned long long* mismatches_out) {
    if (!ctx || !mismatches_out) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipMemsetAsync(ctx->counters.get(), 0, sizeof(unsigned long long), ctx->stream));
    hipError_t e = (hipError_t)rtu_launch_selftest_fdiv(n_pairs, seed, ctx->counters.get(), ctx->stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "selftest launch: %s", hipGetErrorString(e));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RTU_HIP(ctx, hipMemcpy(mismatches_out, ctx->counters.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RTU_OK;
}

int rtu_selftest_primitives(RtuContext* ctx, unsigned long long n_rays, unsigned long long seed, unsigned long long* mismatches_out) {
    if (!ctx || !mismatches_out) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipMemsetAsync(ctx->counters.get(), 0, sizeof(unsigned long long), ctx->stream));
    hipError_t e = (hipError_t)rtu_launch_selftest_prims(n_rays, seed, ctx->counters.get(), ctx->stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "selftest launch: %s", hipGetErrorString(e));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RTU_HIP(ctx, hipMemcpy(mismatches_out, ctx->counters.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RTU_OK;
}

int rtu_debug_texcoords(RtuContext* ctx, int op, int index, const float* h_in, unsigned long long n, float* h_out) {
    if (!ctx) return RTU_ERR_ARG;
    if (op < RTU_TEXOP_ATAN2F || op > RTU_TEXOP_MAP) return fail(ctx, RTU_ERR_ARG, "unknown texcoords op %d", op);
    if (n && (!h_in || !h_out)) return fail(ctx, RTU_ERR_ARG, "h_in / h_out is NULL");
    const DevTexture* tex = nullptr;
    RtuTexMap map;  // checked here, on the host: the kernel samples it as map_sample does, without looking at `present`
    const DevScene& s = ctx->dscene;
    if (op == RTU_TEXOP_TEXTURE || op == RTU_TEXOP_MAP) {
        if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
        if (ctx->n_textures == 0) return fail(ctx, RTU_ERR_ARG, "the uploaded scene has no textures");
        if (op == RTU_TEXOP_TEXTURE) {
            if (index < 0 || (uint32_t)index >= ctx->n_textures) return fail(ctx, RTU_ERR_ARG, "texture %d: the scene has %u", index, ctx->n_textures);
            tex = s.textures + index;
        } else {
            if (index == -1 || index == -2) map = index == -1 ? s.bg_map : s.env_map;
            else if (index >= 0 && (size_t)index < ctx->mat_maps_host.size()) map = ctx->mat_maps_host[index];
            else return fail(ctx, RTU_ERR_ARG, "no material map %d", index);
            if (!map.present || map.texture >= (int32_t)ctx->n_textures) return fail(ctx, RTU_ERR_ARG, "map %d is not present", index);
        }
    }
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned long long chunk = 1ull << 22;
    const int nin = RTU_TEXOP_IN(op), nout = RTU_TEXOP_OUT(op);
    DevBuf<float> d_in, d_out;
    DevBuf<RtuTexMap> d_map;  // the kernel reads the map from device memory
    hipError_t e = d_in.grow(nin * chunk);
    if (e == hipSuccess) e = d_out.grow(nout * chunk);
    if (e == hipSuccess && op == RTU_TEXOP_MAP) e = d_map.grow(1);
    if (e == hipSuccess && op == RTU_TEXOP_MAP) e = hipMemcpy(d_map.get(), &map, sizeof map, hipMemcpyHostToDevice);
    for (unsigned long long done = 0; e == hipSuccess && done < n; done += chunk) {
        const unsigned long long m = n - done < chunk ? n - done : chunk;
        e = hipMemcpyAsync(d_in.get(), h_in + nin * done, sizeof(float) * nin * m, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = (hipError_t)rtu_launch_debug_texcoords(s, op, tex, d_map.get(), d_in.get(), d_out.get(), m, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_out + nout * done, d_out.get(), sizeof(float) * nout * m, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "texcoords: %s", hipGetErrorString(e));
    return RTU_OK;
}

}  // extern "C"

// ---- ray queries (rtu_query.hip) ----------------------------------------------------------------------------------------------

namespace {

const size_t kQueryChunk = (size_t)1 << 20;  // rays per launch of the host forms: 32 MB of rays, 48 MB of hits

int query_args(RtuContext* ctx, const void* rays, const void* out, size_t n, uint32_t flags, bool device) {
    if (flags & ~RTU_QUERY_REFERENCE_WALK) return fail(ctx, RTU_ERR_ARG, "unknown ray-query flag bits 0x%x", flags & ~RTU_QUERY_REFERENCE_WALK);
    if (n && (!rays || !out)) return fail(ctx, RTU_ERR_ARG, "rays / result pointer is NULL");
    if (device && n && (((uintptr_t)rays & 15u) || ((uintptr_t)out & 15u)))
        return fail(ctx, RTU_ERR_ARG, "device ray / result buffers must be 16-byte aligned");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    return RTU_OK;
}

// the scene as the renders see it now, without the experiment switches of rtu_debug_flags (they exist to render wrong images)
DevScene query_scene(const RtuContext* ctx) {
    DevScene s = ctx->dscene;
    s.dbg = 0;
    return s;
}

int query_host(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t flags, RtuRayHit* h_hits, uint8_t* h_occ) {
    const size_t chunk = n < kQueryChunk ? n : kQueryChunk;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->q_rays.grow(2 * chunk));
    if (h_hits) RTU_HIP(ctx, ctx->q_hits.grow(3 * chunk));
    else RTU_HIP(ctx, ctx->q_occ.grow((chunk + 15u) & ~(size_t)15u));
    const DevScene s = query_scene(ctx);
    const bool ref = (flags & RTU_QUERY_REFERENCE_WALK) != 0;
    for (size_t done = 0; done < n; done += chunk) {
        const size_t m = n - done < chunk ? n - done : chunk;
        RTU_HIP(ctx, hipMemcpyAsync(ctx->q_rays.get(), h_rays + done, sizeof(RtuRay) * m, hipMemcpyHostToDevice, ctx->stream));
        hipError_t e;
        if (h_hits) {
            e = (hipError_t)rtu_launch_query_closest(s, ctx->q_rays.get(), ctx->q_hits.get(), m, ref, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(h_hits + done, ctx->q_hits.get(), sizeof(RtuRayHit) * m, hipMemcpyDeviceToHost, ctx->stream);
        } else {
            e = (hipError_t)rtu_launch_query_any(s, ctx->q_rays.get(), ctx->q_occ.get(), m, ref, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(h_occ + done, ctx->q_occ.get(), m, hipMemcpyDeviceToHost, ctx->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "ray query: %s", hipGetErrorString(e));
    }
    return RTU_OK;
}

static_assert(sizeof(RtuRay) == 32 && sizeof(RtuRayHit) == 48, "ray query records are two / three float4");

}  // namespace

extern "C" {

int rtu_trace_rays_device(RtuContext* ctx, const void* d_rays, size_t n, uint32_t flags, void* d_hits, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    const int rc = query_args(ctx, d_rays, d_hits, n, flags, true);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_query_closest(query_scene(ctx), (const float4*)d_rays, (float4*)d_hits, n,
                                                              (flags & RTU_QUERY_REFERENCE_WALK) != 0, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "ray query launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_occluded_rays_device(RtuContext* ctx, const void* d_rays, size_t n, uint32_t flags, void* d_occluded, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (n && d_rays && ((uintptr_t)d_rays & 15u)) return fail(ctx, RTU_ERR_ARG, "device ray buffer must be 16-byte aligned");
    const int rc = query_args(ctx, d_rays, d_occluded, n, flags, false);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_query_any(query_scene(ctx), (const float4*)d_rays, (uint8_t*)d_occluded, n,
                                                          (flags & RTU_QUERY_REFERENCE_WALK) != 0, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "ray query launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_trace_rays(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t flags, RtuRayHit* h_hits) {
    if (!ctx) return RTU_ERR_ARG;
    const int rc = query_args(ctx, h_rays, h_hits, n, flags, false);
    if (rc != RTU_OK || n == 0) return rc;
    return query_host(ctx, h_rays, n, flags, h_hits, nullptr);
}

int rtu_occluded_rays(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t flags, uint8_t* h_occluded) {
    if (!ctx) return RTU_ERR_ARG;
    const int rc = query_args(ctx, h_rays, h_occluded, n, flags, false);
    if (rc != RTU_OK || n == 0) return rc;
    return query_host(ctx, h_rays, n, flags, nullptr, h_occluded);
}

}  // extern "C"

// ---- first-hit features (rtu_features.hip) and the denoising filter (rtu_denoise.hip) -----------------------------------------------

namespace {

static int feature_cam(RtuContext* ctx, const RtuFrameDesc* f, FeatureCam& cam) {
    if (!f) return fail(ctx, RTU_ERR_ARG, "frame is NULL");
    if (f->width <= 0 || f->height <= 0 || f->width > 65536 || f->height > 65536) return fail(ctx, RTU_ERR_ARG, "bad resolution");
    if (f->shard_count != 1 || f->shard_rank != 0) return fail(ctx, RTU_ERR_ARG, "the features of a frame are those of the whole image: shard_count must be 1");
    for (int k = 0; k < 3; k++) { cam.pos[k] = f->cam_pos[k]; cam.origin[k] = f->origin[k]; cam.u[k] = f->u[k]; cam.v[k] = f->v[k]; }
    cam.width = f->width;
    cam.height = f->height;
    return RTU_OK;
}

// chunks of rays (h_rays) or of a frame's pixels in image order (cam) through q_rays / q_hits / ft_albedo; h_surface (the surface
// entries): the kernels with one more output, through ft_surface
static int features_host(RtuContext* ctx, const RtuRay* h_rays, const FeatureCam* cam, size_t n, uint32_t flags, RtuRayHit* h_hits, float* h_albedo,
                         RtuRaySurface* h_surface = nullptr) {
    const size_t chunk = n < kQueryChunk ? n : kQueryChunk;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    if (h_rays) RTU_HIP(ctx, ctx->q_rays.grow(2 * chunk));
    RTU_HIP(ctx, ctx->q_hits.grow(3 * chunk));
    RTU_HIP(ctx, ctx->ft_albedo.grow(chunk));
    if (h_surface) RTU_HIP(ctx, ctx->ft_surface.grow(2 * chunk));
    const DevScene s = query_scene(ctx);
    const bool ref = (flags & RTU_QUERY_REFERENCE_WALK) != 0;
    for (size_t done = 0; done < n; done += chunk) {
        const size_t m = n - done < chunk ? n - done : chunk;
        hipError_t e = hipSuccess;
        if (h_rays) {
            e = hipMemcpyAsync(ctx->q_rays.get(), h_rays + done, sizeof(RtuRay) * m, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess && h_surface)
                e = (hipError_t)rtu_launch_ray_surface(s, ctx->q_rays.get(), ctx->q_hits.get(), ctx->ft_albedo.get(), ctx->ft_surface.get(), m, ref, ctx->stream);
            else if (e == hipSuccess)
                e = (hipError_t)rtu_launch_ray_features(s, ctx->q_rays.get(), ctx->q_hits.get(), ctx->ft_albedo.get(), m, ref, ctx->stream);
        } else if (h_surface) {
            e = (hipError_t)rtu_launch_frame_surface(s, *cam, done, m, ctx->q_hits.get(), ctx->ft_albedo.get(), ctx->ft_surface.get(), ctx->stream);
        } else {
            e = (hipError_t)rtu_launch_frame_features(s, *cam, done, m, ctx->q_hits.get(), ctx->ft_albedo.get(), ctx->stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(h_hits + done, ctx->q_hits.get(), sizeof(RtuRayHit) * m, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_albedo + 4 * done, ctx->ft_albedo.get(), sizeof(float4) * m, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && h_surface)
            e = hipMemcpyAsync(h_surface + done, ctx->ft_surface.get(), sizeof(RtuRaySurface) * m, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "first-hit features: %s", hipGetErrorString(e));
    }
    return RTU_OK;
}

}  // namespace

extern "C" {

int rtu_ray_features_device(RtuContext* ctx, const void* d_rays, size_t n, uint32_t flags, void* d_hits, void* d_albedo, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (n && !d_albedo) return fail(ctx, RTU_ERR_ARG, "albedo pointer is NULL");
    if (n && misaligned(d_albedo)) return fail(ctx, RTU_ERR_ARG, "device albedo buffer must be 16-byte aligned");
    const int rc = query_args(ctx, d_rays, d_hits, n, flags, true);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_ray_features(query_scene(ctx), (const float4*)d_rays, (float4*)d_hits, (float4*)d_albedo, n,
                                                             (flags & RTU_QUERY_REFERENCE_WALK) != 0, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "first-hit features launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_ray_features(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t flags, RtuRayHit* h_hits, float* h_albedo) {
    if (!ctx) return RTU_ERR_ARG;
    if (n && !h_albedo) return fail(ctx, RTU_ERR_ARG, "albedo pointer is NULL");
    const int rc = query_args(ctx, h_rays, h_hits, n, flags, false);
    if (rc != RTU_OK || n == 0) return rc;
    return features_host(ctx, h_rays, nullptr, n, flags, h_hits, h_albedo);
}

int rtu_frame_features_device(RtuContext* ctx, const RtuFrameDesc* frame, void* d_hits, void* d_albedo, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    FeatureCam cam;
    const int rc = feature_cam(ctx, frame, cam);
    if (rc != RTU_OK) return rc;
    if (!d_hits || !d_albedo) return fail(ctx, RTU_ERR_ARG, "hits / albedo pointer is NULL");
    if (misaligned(d_hits) || misaligned(d_albedo)) return fail(ctx, RTU_ERR_ARG, "device hits / albedo buffers must be 16-byte aligned");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_frame_features(query_scene(ctx), cam, 0, (unsigned long long)cam.width * (unsigned long long)cam.height,
                                                               (float4*)d_hits, (float4*)d_albedo, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "first-hit features launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_frame_features(RtuContext* ctx, const RtuFrameDesc* frame, RtuRayHit* h_hits, float* h_albedo) {
    if (!ctx) return RTU_ERR_ARG;
    FeatureCam cam;
    const int rc = feature_cam(ctx, frame, cam);
    if (rc != RTU_OK) return rc;
    if (!h_hits || !h_albedo) return fail(ctx, RTU_ERR_ARG, "hits / albedo pointer is NULL");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    return features_host(ctx, nullptr, &cam, (size_t)cam.width * (size_t)cam.height, 0, h_hits, h_albedo);
}

// ---- surface records: the features with the winning triangle and the texture coordinate (k_features_surface, rtu_features.hip) ----
static_assert(sizeof(RtuRaySurface) == 32, "a surface record is two float4");

int rtu_ray_surface_device(RtuContext* ctx, const void* d_rays, size_t n, uint32_t flags, void* d_hits, void* d_albedo, void* d_surface,
                           void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (n && (!d_albedo || !d_surface)) return fail(ctx, RTU_ERR_ARG, "albedo / surface pointer is NULL");
    if (n && (misaligned(d_albedo) || misaligned(d_surface))) return fail(ctx, RTU_ERR_ARG, "device albedo / surface buffers must be 16-byte aligned");
    const int rc = query_args(ctx, d_rays, d_hits, n, flags, true);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_ray_surface(query_scene(ctx), (const float4*)d_rays, (float4*)d_hits, (float4*)d_albedo, (float4*)d_surface, n,
                                                            (flags & RTU_QUERY_REFERENCE_WALK) != 0, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "surface records launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_ray_surface(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t flags, RtuRayHit* h_hits, float* h_albedo, RtuRaySurface* h_surface) {
    if (!ctx) return RTU_ERR_ARG;
    if (n && (!h_albedo || !h_surface)) return fail(ctx, RTU_ERR_ARG, "albedo / surface pointer is NULL");
    const int rc = query_args(ctx, h_rays, h_hits, n, flags, false);
    if (rc != RTU_OK || n == 0) return rc;
    return features_host(ctx, h_rays, nullptr, n, flags, h_hits, h_albedo, h_surface);
}

int rtu_frame_surface_device(RtuContext* ctx, const RtuFrameDesc* frame, void* d_hits, void* d_albedo, void* d_surface, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    FeatureCam cam;
    const int rc = feature_cam(ctx, frame, cam);
    if (rc != RTU_OK) return rc;
    if (!d_hits || !d_albedo || !d_surface) return fail(ctx, RTU_ERR_ARG, "hits / albedo / surface pointer is NULL");
    if (misaligned(d_hits) || misaligned(d_albedo) || misaligned(d_surface))
        return fail(ctx, RTU_ERR_ARG, "device hits / albedo / surface buffers must be 16-byte aligned");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_frame_surface(query_scene(ctx), cam, 0, (unsigned long long)cam.width * (unsigned long long)cam.height,
                                                              (float4*)d_hits, (float4*)d_albedo, (float4*)d_surface, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "surface records launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_frame_surface(RtuContext* ctx, const RtuFrameDesc* frame, RtuRayHit* h_hits, float* h_albedo, RtuRaySurface* h_surface) {
    if (!ctx) return RTU_ERR_ARG;
    FeatureCam cam;
    const int rc = feature_cam(ctx, frame, cam);
    if (rc != RTU_OK) return rc;
    if (!h_hits || !h_albedo || !h_surface) return fail(ctx, RTU_ERR_ARG, "hits / albedo / surface pointer is NULL");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    return features_host(ctx, nullptr, &cam, (size_t)cam.width * (size_t)cam.height, 0, h_hits, h_albedo, h_surface);
}

int rtu_denoise_device(RtuContext* ctx, const RtuDenoiseDesc* desc, const void* d_in, const void* d_hits, const void* d_albedo, void* d_out,
                       void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (rtu_denoise_check_desc(desc) != RTU_OK)
        return fail(ctx, RTU_ERR_ARG, "denoise: width, height 1 .. 65536, n_passes 1 .. 8, normal_log2_power 0 .. 7, sigmas > 0, reserved words 0");
    if (!d_in || !d_hits || !d_albedo || !d_out) return fail(ctx, RTU_ERR_ARG, "denoise: a device pointer is NULL");
    if (misaligned(d_in) || misaligned(d_hits) || misaligned(d_albedo) || misaligned(d_out))
        return fail(ctx, RTU_ERR_ARG, "denoise: device buffers must be 16-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->dn_planes.grow(4 * (size_t)desc->width * (size_t)desc->height));
    const hipError_t e = (hipError_t)rtu_launch_denoise(*desc, (const float4*)d_in, (const float4*)d_hits, (const float4*)d_albedo, (float4*)d_out,
                                                        ctx->dn_planes.get(), (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "denoise launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_progressive_snapshot_denoised_device(RtuProgressive* p, const RtuDenoiseDesc* desc_or_NULL, void* d_rgbz, void* hip_stream) {
    if (!p || !p->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = p->ctx;
    FeatureCam cam;
    int rc = feature_cam(ctx, &p->frame, cam);  // refuses a sharded session
    if (rc != RTU_OK) return rc;
    RtuDenoiseDesc d;
    if (desc_or_NULL) d = *desc_or_NULL;
    else rtu_denoise_defaults(&d);
    d.width = cam.width;
    d.height = cam.height;
    if (rtu_denoise_check_desc(&d) != RTU_OK)
        return fail(ctx, RTU_ERR_ARG, "denoise: n_passes 1 .. 8, normal_log2_power 0 .. 7, sigmas > 0, reserved words 0");
    if (p->done == 0) return fail(ctx, RTU_ERR_ARG, "no samples yet: advance the session first");
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "d_rgbz is NULL");
    if (misaligned(d_rgbz)) return fail(ctx, RTU_ERR_ARG, "d_rgbz must be 16-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    if (!p->has_features) {
        // the session's frame as its scene was when it began: a newer scene would guide the filter with surfaces the sums never saw
        if (p->scene_gen != ctx->scene_gen) return fail(ctx, RTU_ERR_STALE, "the context got a new scene before this session made its features");
        if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
        RTU_HIP(ctx, p->ft_hits.grow(3 * p->pixels));
        RTU_HIP(ctx, p->ft_albedo.grow(p->pixels));
        const hipError_t e = (hipError_t)rtu_launch_frame_features(query_scene(ctx), cam, 0, p->pixels, p->ft_hits.get(), p->ft_albedo.get(),
                                                                   (hipStream_t)hip_stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "first-hit features launch: %s", hipGetErrorString(e));
        p->has_features = true;
    }
    rc = rtu_progressive_snapshot_device(p, d_rgbz, nullptr, hip_stream);
    if (rc != RTU_OK) return rc;
    return rtu_denoise_device(ctx, &d, d_rgbz, p->ft_hits.get(), p->ft_albedo.get(), d_rgbz, hip_stream);  // in place
}

int rtu_progressive_snapshot_denoised(RtuProgressive* p, const RtuDenoiseDesc* desc_or_NULL, float* h_rgbz) {
    if (!p || !p->ctx) return RTU_ERR_ARG;
    RtuContext* ctx = p->ctx;
    if (!h_rgbz) return fail(ctx, RTU_ERR_ARG, "h_rgbz is NULL");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->fb.grow(p->pixels ? p->pixels : 1));
    const int rc = rtu_progressive_snapshot_denoised_device(p, desc_or_NULL, ctx->fb.get(), ctx->stream);
    if (rc != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpyAsync(h_rgbz, ctx->fb.get(), p->pixels * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTU_OK;
}

}  // extern "C"

// ---- ray batches: Shade() along caller-supplied rays (render_rays_impl.h) -------------------------------------------------------

namespace {

// chains per launch sequence of recipe P: what sampled_batch allows a frame's batch of samples by default (2^25 pixels; its tuning
// knob RTU_GI_BATCH_LOG2 moves the frame path's figure, not this one), and so a path-traced ray batch's _device form
const size_t kPathChains = (size_t)1 << 25;

}  // namespace

// the checks both forms share, then the frame descriptor launch() takes for a ray batch: no camera, the eye in cam_pos
// keys: the sampled forms (rtu_shade_rays_sampled*) — n uint32, one per ray; the frame is then a recipe-S frame of one sample
// paths: rtu_shade_rays_paths* — sampled, and every ray is a chain of recipe P (352 bytes of chain records and results each)
int shade_args(RtuContext* ctx, const void* rays, const void* out, size_t n, const RtuShadeDesc* d, bool device, RtuFrameDesc* f, bool sampled,
               const void* keys, bool paths) {
    if (!d) return fail(ctx, RTU_ERR_ARG, "shade descriptor is NULL");
    if (d->flags & ~RTU_QUERY_REFERENCE_WALK) return fail(ctx, RTU_ERR_ARG, "unknown shade flag bits 0x%x", d->flags & ~RTU_QUERY_REFERENCE_WALK);
    if (d->reserved[0] | d->reserved[1] | d->reserved[2]) return fail(ctx, RTU_ERR_ARG, "RtuShadeDesc.reserved must be 0");
    if (d->max_bounce < 0 || d->max_bounce > RTU_MAX_BOUNCE) return fail(ctx, RTU_ERR_ARG, "max_bounce out of range");
    if (!std::isfinite(d->eye[0]) || !std::isfinite(d->eye[1]) || !std::isfinite(d->eye[2])) return fail(ctx, RTU_ERR_ARG, "eye is not finite");
    if (n && (!rays || !out)) return fail(ctx, RTU_ERR_ARG, "rays / result pointer is NULL");
    if (device && n && (((uintptr_t)rays & 15u) || ((uintptr_t)out & 15u)))
        return fail(ctx, RTU_ERR_ARG, "device ray / result buffers must be 16-byte aligned");
    if (device && n > ((size_t)1 << 26)) return fail(ctx, RTU_ERR_ARG, "more than 2^26 rays in one call");
    if (device && paths && n > kPathChains) return fail(ctx, RTU_ERR_ARG, "more than 2^25 rays (chains of recipe P) in one call");
    if (sampled && n && !keys) return fail(ctx, RTU_ERR_ARG, "key pointer is NULL");
    if (sampled && n && ((uintptr_t)keys & 3u)) return fail(ctx, RTU_ERR_ARG, "the key buffer must be 4-byte aligned");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    if (ctx->scene_stochastic && !sampled)
        return fail(ctx, RTU_ERR_STOCHASTIC, "the scene has %s: rtu_shade_rays is recipe W (rtu_shade_rays_sampled shades rays by recipe S)", ctx->stochastic_what.c_str());
    memset(f, 0, sizeof *f);
    f->width = 64;  // (launch() sizes a ray batch from n; these only have to be a valid frame)
    f->height = 1;
    f->shard_count = 1;
    f->max_bounce = d->max_bounce;
    f->collect_stats = (d->flags & RTU_QUERY_REFERENCE_WALK) ? 1 : 0;
    f->samples = sampled ? 1 : 0;  // one Shade() call of recipe S per ray: launch() sets the sampled feature set from it
    f->gather_bounces = paths ? RTU_GI_BOUNCES : 0;
    memcpy(f->cam_pos, d->eye, sizeof f->cam_pos);
    return RTU_OK;
}

// ---- a path-traced ray batch (rtu_shade_rays_paths): the launch sequence of recipe P with chain i = ray i ----
// the chain of a batch: the roots, then the four gather rays; chain records do not depend on the frame capacities.
// A cut level set by rtu_debug_tail_from is for the "next launch", which launch() takes to be its own next call: a chain step has no
// recursion levels, so the level is kept from it and handed on to the shading steps.
int paths_chain(RtuContext* ctx, const RtuFrameDesc& f, float4* d_out, hipStream_t stream, const float4* d_rays, const uint32_t* d_keys, uint32_t n) {
    const int forced = ctx->tail_hint;
    int rc = RTU_OK;
    for (int k = 0; k <= RTU_GI_BOUNCES && rc == RTU_OK; k++) {
        ctx->tail_hint = 0;
        rc = launch(ctx, &f, d_out, stream, k == 0, 0, 1, nullptr, RTU_LAUNCH_CHAIN, k, false, nullptr, 0, d_rays, n, d_keys);
    }
    ctx->tail_hint = forced;
    return rc;
}

namespace {

// the five shading steps from the deepest depth up (k_gi_roots needs the results of the depth below); depth 0 ends with k_gi_final.
// Each of them is a whole launch of the recursion levels: a forced cut level applies to all five, then it is spent.
int paths_shade(RtuContext* ctx, const RtuFrameDesc& f, float4* d_out, hipStream_t stream, const float4* d_rays, const uint32_t* d_keys, uint32_t n) {
    const int forced = ctx->tail_hint;
    int rc = RTU_OK;
    for (int k = RTU_GI_BOUNCES; k >= 0 && rc == RTU_OK; k--) {
        ctx->tail_hint = forced;
        rc = launch(ctx, &f, d_out, stream, false, 0, 1, nullptr, RTU_LAUNCH_SHADE, k, false, nullptr, 0, d_rays, n, d_keys);
    }
    ctx->tail_hint = 0;
    return rc;
}

}  // namespace

// Shade a ray batch whose rays (and keys) are in device memory until its frame records suffice: launch() — with paths the five steps
// of paths_shade, the chain having been traced by the caller —, wait, check_overflow, and again with the capacities that raised.
// counters_refusal: what to say where a path-traced batch with counters would have to be shaded again (its counters of the dropped
// steps are already in the totals), or nullptr where the caller has no counters.
// behind (may be nullptr): queued behind every attempt and ahead of its synchronisation — kernels that read the batch and leave it alone
// where the overflow flags say it is incomplete (adaptive sensors: k_sa_step and the length of the next list, read in this synchronisation).
int shade_until_fits(RtuContext* ctx, const RtuFrameDesc& f, float4* d_out, hipStream_t stream, const float4* d_rays, const uint32_t* d_keys, uint32_t n,
                     bool paths, const char* counters_refusal, int (*behind)(void*), void* behind_arg) {
    for (int attempt = 0;; attempt++) {
        int rc = paths ? paths_shade(ctx, f, d_out, stream, d_rays, d_keys, n)
                       : launch(ctx, &f, d_out, stream, true, 0, 1, nullptr, RTU_LAUNCH_ALL, 0, false, nullptr, 0, d_rays, n, d_keys);
        if (rc != RTU_OK) return rc;
        if (behind && (rc = behind(behind_arg)) != RTU_OK) return rc;
        RTU_HIP(ctx, hipStreamSynchronize(stream));
        bool overflow = false;
        if ((rc = check_overflow(ctx, &overflow)) != RTU_OK) return rc;
        if (!overflow) return RTU_OK;
        if (paths && f.collect_stats && counters_refusal) return fail(ctx, RTU_ERR_CAPACITY, "%s", counters_refusal);
        if (attempt >= (paths ? 8 : 2) * RTU_MAX_LEVELS) return fail(ctx, RTU_ERR_CAPACITY, "recursion frames still exceed the capacity after %d rounds", attempt);
    }
}

namespace {

// the host forms of all three recipes: chunks of at most kQueryChunk rays (and keys) through the context's buffers, each checked for
// capacity and shaded again if need be. paths: the chain of a chunk is traced once, its shading steps are what is repeated
int shade_host(RtuContext* ctx, RtuFrameDesc& f, const RtuRay* h_rays, const uint32_t* h_keys, size_t n, float* h_rgbt, RtuStats* stats, bool paths = false) {
    int rc = RTU_OK;
    if (stats) { memset(stats, 0, sizeof *stats); f.collect_stats = 1; }
    if (n == 0) return RTU_OK;
    const size_t chunk = n < kQueryChunk ? n : kQueryChunk;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->sh_rays.grow(2 * chunk));
    RTU_HIP(ctx, ctx->sh_out.grow(chunk));
    if (h_keys) RTU_HIP(ctx, ctx->sh_keys.grow(chunk));
    for (size_t done = 0; done < n; done += chunk) {
        const size_t m = n - done < chunk ? n - done : chunk;
        RTU_HIP(ctx, hipMemcpyAsync(ctx->sh_rays.get(), h_rays + done, sizeof(RtuRay) * m, hipMemcpyHostToDevice, ctx->stream));
        if (h_keys) RTU_HIP(ctx, hipMemcpyAsync(ctx->sh_keys.get(), h_keys + done, sizeof(uint32_t) * m, hipMemcpyHostToDevice, ctx->stream));
        if (paths && (rc = paths_chain(ctx, f, ctx->sh_out.get(), ctx->stream, ctx->sh_rays.get(), ctx->sh_keys.get(), (uint32_t)m)) != RTU_OK) return rc;
        // as rtu_render_frame: a chunk that ran out of frame capacity is shaded again
        if ((rc = shade_until_fits(ctx, f, ctx->sh_out.get(), ctx->stream, ctx->sh_rays.get(), h_keys ? ctx->sh_keys.get() : nullptr, (uint32_t)m, paths,
                                   "recipe P with counters: frame records ran out; shade the batch once without counters first")) != RTU_OK)
            return rc;
        RTU_HIP(ctx, hipMemcpy(h_rgbt + 4 * done, ctx->sh_out.get(), sizeof(float4) * m, hipMemcpyDeviceToHost));
        if (stats) {  // the counters are zeroed per launch: the batch's are the sum over its chunks
            RtuStats part;
            if ((rc = rtu_get_stats(ctx, &part)) != RTU_OK) return rc;
            unsigned long long* to = reinterpret_cast<unsigned long long*>(stats);
            const unsigned long long* from = reinterpret_cast<const unsigned long long*>(&part);
            for (size_t k = 0; k < sizeof(RtuStats) / sizeof(unsigned long long); k++) to[k] += from[k];
        }
    }
    return RTU_OK;
}

// ---- the sample streams on the host (include/rtu_render.h "Sample streams of recipe S"; rtu_intersect.h states them for the device) ----
uint32_t h_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}

}  // namespace

// portable_sincos of rtu_intersect.h restated for the host: binary64, IEEE operations only (this file is compiled with -ffp-contract=off),
// the same sequence, so the same floats
void h_portable_sincos(float t, float& sn, float& cs) {
    const double x = (double)t;
    const double kd = floor(x * 6.36619772367581382433e-01 + 0.5);
    const int k = (int)kd;
    const double y = (x - kd * 1.57079632673412561417e+00) - kd * 6.07710050650619224932e-11;
    const double y2 = y * y;
    const double ps = -1.66666666666666324348e-01 + y2 * (8.33333333332248946124e-03 + y2 * (-1.98412698298579493134e-04 +
                      y2 * (2.75573137070700676789e-06 + y2 * (-2.50507602534068634195e-08 + y2 * 1.58969099521155010221e-10))));
    const double pc = 4.16666666666666019037e-02 + y2 * (-1.38888888888741095749e-03 + y2 * (2.48015872894767294178e-05 +
                      y2 * (-2.75573143513906633035e-07 + y2 * (2.08757232129817482790e-09 + y2 * -1.13596475577881948265e-11))));
    const double s = y + (y * y2) * ps;
    const double c = 1.0 - (0.5 * y2 - (y2 * y2) * pc);
    const double so = (k & 1) ? c : s, co = (k & 1) ? s : c;
    sn = (float)((k & 2) ? -so : so);
    cs = (float)((((k + 1) & 2) != 0) ? -co : co);
}

// what camera_sample_ray (rtu_camrays.h) takes of sample `sample` of `frame`: the camera, and the pixel offsets by launch()'s expressions
CamSample cam_sample(const RtuFrameDesc* frame, int sample) {
    CamSample c;
    memset(&c, 0, sizeof c);
    for (int k = 0; k < 3; k++) {
        c.cam_pos[k] = frame->cam_pos[k]; c.origin[k] = frame->origin[k]; c.u[k] = frame->u[k]; c.v[k] = frame->v[k];
        c.lens_up[k] = frame->lens_up[k]; c.lens_right[k] = frame->lens_right[k];
    }
    c.dof = frame->dof;
    const float pixelIncrement = (float)(1.0 / frame->samples);  // RenderFunctions.cpp:68 (launch())
    const float currentOffset = (float)sample * pixelIncrement;  // :80
    c.ox = currentOffset + halton(sample, 4);                    // :84, :85, :96
    c.oy = currentOffset + halton(sample, 5);
    c.width = frame->width;
    c.height = frame->height;
    c.sample = (uint32_t)sample;
    return c;
}

static_assert(sizeof(RtuShadeDesc) == 32, "RtuShadeDesc is 32 bytes");

extern "C" {

int rtu_shade_defaults(RtuShadeDesc* out) {
    if (!out) return RTU_ERR_ARG;
    memset(out, 0, sizeof *out);
    out->max_bounce = RTU_MAX_BOUNCE;
    return RTU_OK;
}

int rtu_shade_rays_device(RtuContext* ctx, const void* d_rays, size_t n, const RtuShadeDesc* desc, void* d_rgbt, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    RtuFrameDesc f;
    const int rc = shade_args(ctx, d_rays, d_rgbt, n, desc, true, &f);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    return launch(ctx, &f, (float4*)d_rgbt, (hipStream_t)hip_stream, true, 0, 1, nullptr, RTU_LAUNCH_ALL, 0, false, nullptr, 0, (const float4*)d_rays, (uint32_t)n);
}

int rtu_shade_rays(RtuContext* ctx, const RtuRay* h_rays, size_t n, const RtuShadeDesc* desc, float* h_rgbt, RtuStats* stats) {
    if (!ctx) return RTU_ERR_ARG;
    RtuFrameDesc f;
    const int rc = shade_args(ctx, h_rays, h_rgbt, n, desc, false, &f);
    if (rc != RTU_OK) return rc;
    return shade_host(ctx, f, h_rays, nullptr, n, h_rgbt, stats);
}

// ---- sampled ray batches: one Shade() call of recipe S per ray, its sample streams keyed by the caller (render_rays2.hip / render_rays3.hip) ----
int rtu_shade_rays_sampled_device(RtuContext* ctx, const void* d_rays, const void* d_keys, size_t n, const RtuShadeDesc* desc, void* d_rgbt, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    RtuFrameDesc f;
    const int rc = shade_args(ctx, d_rays, d_rgbt, n, desc, true, &f, true, d_keys);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    return launch(ctx, &f, (float4*)d_rgbt, (hipStream_t)hip_stream, true, 0, 1, nullptr, RTU_LAUNCH_ALL, 0, false, nullptr, 0, (const float4*)d_rays, (uint32_t)n,
                  (const uint32_t*)d_keys);
}

int rtu_shade_rays_sampled(RtuContext* ctx, const RtuRay* h_rays, const uint32_t* h_keys, size_t n, const RtuShadeDesc* desc, float* h_rgbt, RtuStats* stats) {
    if (!ctx) return RTU_ERR_ARG;
    RtuFrameDesc f;
    const int rc = shade_args(ctx, h_rays, h_rgbt, n, desc, false, &f, true, h_keys);
    if (rc != RTU_OK) return rc;
    return shade_host(ctx, f, h_rays, h_keys, n, h_rgbt, stats);
}

// ---- path-traced ray batches: recipe P per ray (render_rays4.hip / render_rays5.hip for the chain, render_feat10/11.hip behind it) ----
int rtu_shade_rays_paths_device(RtuContext* ctx, const void* d_rays, const void* d_keys, size_t n, const RtuShadeDesc* desc, void* d_rgbt, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    RtuFrameDesc f;
    int rc = shade_args(ctx, d_rays, d_rgbt, n, desc, true, &f, true, d_keys, true);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = paths_chain(ctx, f, (float4*)d_rgbt, (hipStream_t)hip_stream, (const float4*)d_rays, (const uint32_t*)d_keys, (uint32_t)n)) != RTU_OK) return rc;
    return paths_shade(ctx, f, (float4*)d_rgbt, (hipStream_t)hip_stream, (const float4*)d_rays, (const uint32_t*)d_keys, (uint32_t)n);
}

int rtu_shade_rays_paths(RtuContext* ctx, const RtuRay* h_rays, const uint32_t* h_keys, size_t n, const RtuShadeDesc* desc, float* h_rgbt, RtuStats* stats) {
    if (!ctx) return RTU_ERR_ARG;
    RtuFrameDesc f;
    const int rc = shade_args(ctx, h_rays, h_rgbt, n, desc, false, &f, true, h_keys, true);
    if (rc != RTU_OK) return rc;
    return shade_host(ctx, f, h_rays, h_keys, n, h_rgbt, stats, true);
}

}  // extern "C"

// ---- the two halves of a recipe-P sample (render_gather_impl.h; render_rays6.hip / render_rays7.hip) ----

namespace {

enum { HALF_GATHER = 1, HALF_AMBIENT = 2 };

DevScene half_scene(const RtuContext* ctx) {
    DevScene s = ctx->dscene;
    s.dbg = ctx->dbg;
    return s;
}

// What is traced once per batch. A gather: the whole chain of a path-traced batch. An ambient batch: the roots alone.
int half_chain(RtuContext* ctx, const RtuFrameDesc& f, float4* d_out, hipStream_t stream, const float4* d_rays, const uint32_t* d_keys, uint32_t n, int kind) {
    if (kind == HALF_GATHER) return paths_chain(ctx, f, d_out, stream, d_rays, d_keys, n);
    const int forced = ctx->tail_hint;  // (as paths_chain: a chain step has no recursion levels)
    ctx->tail_hint = 0;
    const int rc = launch(ctx, &f, d_out, stream, true, 0, 1, nullptr, RTU_LAUNCH_CHAIN, 0, false, nullptr, 0, d_rays, n, d_keys);
    ctx->tail_hint = forced;
    return rc;
}

// One attempt at what depends on the frame capacities. A gather: the shading steps of depth 4 .. 1, then k_gather_amb writes the sum
// of depth 0 out. An ambient batch: k_amb_seed plants amb as the results of depth 1 (the shading step overwrites them, so every
// attempt plants them again), then the shading step of depth 0 with k_gi_final, as compiled.
int half_shade(RtuContext* ctx, const RtuFrameDesc& f, float4* d_out, hipStream_t stream, const float4* d_rays, const uint32_t* d_keys, uint32_t n, int kind,
               const float4* d_amb) {
    const int forced = ctx->tail_hint;
    int rc = RTU_OK;
    if (kind == HALF_AMBIENT) {
        const hipError_t e = (hipError_t)rtu_launch_amb_seed(ctx->gi_h.get(), ctx->gi_res.get(), d_amb, n, stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "ambient seed launch: %s", hipGetErrorString(e));
        rc = launch(ctx, &f, d_out, stream, false, 0, 1, nullptr, RTU_LAUNCH_SHADE, 0, false, nullptr, 0, d_rays, n, d_keys);
    } else {
        for (int k = RTU_GI_BOUNCES; k >= 1 && rc == RTU_OK; k--) {
            ctx->tail_hint = forced;
            rc = launch(ctx, &f, d_out, stream, false, 0, 1, nullptr, RTU_LAUNCH_SHADE, k, false, nullptr, 0, d_rays, n, d_keys);
        }
        if (rc == RTU_OK) {
            const hipError_t e = (hipError_t)rtu_launch_gather_amb(half_scene(ctx), ctx->gi_h.get(), ctx->gi_res.get(), n, d_out, stream);
            if (e != hipSuccess) rc = fail(ctx, RTU_ERR_HIP, "gather sum launch: %s", hipGetErrorString(e));
        }
    }
    ctx->tail_hint = 0;
    return rc;
}

// shade_until_fits for a half: attempt, wait, check_overflow, and again with the capacities that raised
int half_until_fits(RtuContext* ctx, const RtuFrameDesc& f, float4* d_out, hipStream_t stream, const float4* d_rays, const uint32_t* d_keys, uint32_t n, int kind,
                    const float4* d_amb, const char* counters_refusal) {
    for (int attempt = 0;; attempt++) {
        int rc = half_shade(ctx, f, d_out, stream, d_rays, d_keys, n, kind, d_amb);
        if (rc != RTU_OK) return rc;
        RTU_HIP(ctx, hipStreamSynchronize(stream));
        bool overflow = false;
        if ((rc = check_overflow(ctx, &overflow)) != RTU_OK) return rc;
        if (!overflow) return RTU_OK;
        if (f.collect_stats && counters_refusal) return fail(ctx, RTU_ERR_CAPACITY, "%s", counters_refusal);
        if (attempt >= 8 * RTU_MAX_LEVELS) return fail(ctx, RTU_ERR_CAPACITY, "recursion frames still exceed the capacity after %d rounds", attempt);
    }
}

int half_check_amb(RtuContext* ctx, const void* amb, size_t n, bool device) {
    if (n && !amb) return fail(ctx, RTU_ERR_ARG, "amb pointer is NULL");
    if (n && ((uintptr_t)amb & (device ? 15u : 3u))) return fail(ctx, RTU_ERR_ARG, device ? "the device amb buffer must be 16-byte aligned" : "amb must be 4-byte aligned");
    return RTU_OK;
}

int half_device(RtuContext* ctx, const void* d_rays, const void* d_keys, const void* d_amb, size_t n, const RtuShadeDesc* desc, void* d_out, void* hip_stream, int kind) {
    if (!ctx) return RTU_ERR_ARG;
    RtuFrameDesc f;
    int rc = shade_args(ctx, d_rays, d_out, n, desc, true, &f, true, d_keys, true);
    if (rc == RTU_OK && kind == HALF_AMBIENT) rc = half_check_amb(ctx, d_amb, n, true);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = half_chain(ctx, f, (float4*)d_out, (hipStream_t)hip_stream, (const float4*)d_rays, (const uint32_t*)d_keys, (uint32_t)n, kind)) != RTU_OK) return rc;
    return half_shade(ctx, f, (float4*)d_out, (hipStream_t)hip_stream, (const float4*)d_rays, (const uint32_t*)d_keys, (uint32_t)n, kind, (const float4*)d_amb);
}

// shade_host for a half: chunks through the context's buffers, the chain of a chunk traced once, its shading repeated if need be
int half_host(RtuContext* ctx, const RtuRay* h_rays, const uint32_t* h_keys, const float* h_amb, size_t n, const RtuShadeDesc* desc, float* h_out, RtuStats* stats,
              int kind) {
    if (!ctx) return RTU_ERR_ARG;
    RtuFrameDesc f;
    int rc = shade_args(ctx, h_rays, h_out, n, desc, false, &f, true, h_keys, true);
    if (rc == RTU_OK && kind == HALF_AMBIENT) rc = half_check_amb(ctx, h_amb, n, false);
    if (rc != RTU_OK) return rc;
    if (stats) { memset(stats, 0, sizeof *stats); f.collect_stats = 1; }
    if (n == 0) return RTU_OK;
    const size_t chunk = n < kQueryChunk ? n : kQueryChunk;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->sh_rays.grow(2 * chunk));
    RTU_HIP(ctx, ctx->sh_out.grow(chunk));
    RTU_HIP(ctx, ctx->sh_keys.grow(chunk));
    if (kind == HALF_AMBIENT) RTU_HIP(ctx, ctx->sh_amb.grow(chunk));
    for (size_t done = 0; done < n; done += chunk) {
        const size_t m = n - done < chunk ? n - done : chunk;
        RTU_HIP(ctx, hipMemcpyAsync(ctx->sh_rays.get(), h_rays + done, sizeof(RtuRay) * m, hipMemcpyHostToDevice, ctx->stream));
        RTU_HIP(ctx, hipMemcpyAsync(ctx->sh_keys.get(), h_keys + done, sizeof(uint32_t) * m, hipMemcpyHostToDevice, ctx->stream));
        if (kind == HALF_AMBIENT) RTU_HIP(ctx, hipMemcpyAsync(ctx->sh_amb.get(), h_amb + 4 * done, sizeof(float4) * m, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = half_chain(ctx, f, ctx->sh_out.get(), ctx->stream, ctx->sh_rays.get(), ctx->sh_keys.get(), (uint32_t)m, kind)) != RTU_OK) return rc;
        if ((rc = half_until_fits(ctx, f, ctx->sh_out.get(), ctx->stream, ctx->sh_rays.get(), ctx->sh_keys.get(), (uint32_t)m, kind, ctx->sh_amb.get(),
                                  "recipe P with counters: frame records ran out; shade the batch once without counters first")) != RTU_OK)
            return rc;
        RTU_HIP(ctx, hipMemcpy(h_out + 4 * done, ctx->sh_out.get(), sizeof(float4) * m, hipMemcpyDeviceToHost));
        if (stats) {  // the counters are zeroed per launch: the batch's are the sum over its chunks
            RtuStats part;
            if ((rc = rtu_get_stats(ctx, &part)) != RTU_OK) return rc;
            unsigned long long* to = reinterpret_cast<unsigned long long*>(stats);
            const unsigned long long* from = reinterpret_cast<const unsigned long long*>(&part);
            for (size_t k = 0; k < sizeof(RtuStats) / sizeof(unsigned long long); k++) to[k] += from[k];
        }
    }
    return RTU_OK;
}

}  // namespace

extern "C" {

int rtu_gather_rays_device(RtuContext* ctx, const void* d_rays, const void* d_keys, size_t n, const RtuShadeDesc* desc, void* d_ct, void* hip_stream) {
    return half_device(ctx, d_rays, d_keys, nullptr, n, desc, d_ct, hip_stream, HALF_GATHER);
}
int rtu_gather_rays(RtuContext* ctx, const RtuRay* h_rays, const uint32_t* h_keys, size_t n, const RtuShadeDesc* desc, float* h_ct, RtuStats* stats) {
    return half_host(ctx, h_rays, h_keys, nullptr, n, desc, h_ct, stats, HALF_GATHER);
}
int rtu_shade_rays_ambient_device(RtuContext* ctx, const void* d_rays, const void* d_keys, const void* d_amb, size_t n, const RtuShadeDesc* desc,
                                  void* d_rgbt, void* hip_stream) {
    return half_device(ctx, d_rays, d_keys, d_amb, n, desc, d_rgbt, hip_stream, HALF_AMBIENT);
}
int rtu_shade_rays_ambient(RtuContext* ctx, const RtuRay* h_rays, const uint32_t* h_keys, const float* h_amb, size_t n, const RtuShadeDesc* desc,
                           float* h_rgbt, RtuStats* stats) {
    return half_host(ctx, h_rays, h_keys, h_amb, n, desc, h_rgbt, stats, HALF_AMBIENT);
}

}  // extern "C"

// ---- the irradiance map (rtu_irradiance.h, rtu_irradiance.hip) ----

namespace {

const size_t kIrrChunkChains = (size_t)1 << 22;  // chains per chunk of a pass's list: 1.4 GB of chain records and results

int irr_check_frame(RtuContext* ctx, const RtuFrameDesc* frame) {
    if (!frame || frame->width <= 0 || frame->height <= 0) return fail(ctx, RTU_ERR_ARG, "frame is NULL or empty");
    if (frame->shard_count > 1 || frame->shard_rank != 0) return fail(ctx, RTU_ERR_UNSUPPORTED, "the irradiance map has no sharded form");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(frame->cam_pos[k]) || !std::isfinite(frame->origin[k]) || !std::isfinite(frame->u[k]) || !std::isfinite(frame->v[k]))
            return fail(ctx, RTU_ERR_ARG, "the frame's camera is not finite");
    return RTU_OK;
}

int irr_check_map(RtuContext* ctx, const RtuIrradianceMap* map, bool device, IrrGrid* g) {
    if (!map || map->reserved || map->reserved_ptr) return fail(ctx, RTU_ERR_ARG, "map is NULL, or its reserved fields are not 0");
    if (map->max_subdiv < -15) return fail(ctx, RTU_ERR_ARG, "map.max_subdiv out of range");
    RtuIrradianceDesc d;
    rtu_irradiance_defaults(&d);
    d.min_subdiv = map->max_subdiv < 0 ? map->max_subdiv : 0;
    d.max_subdiv = map->max_subdiv;
    const int rc = rtu_irradiance_check(&d, map->width, map->height, g);
    if (rc != RTU_OK) return fail(ctx, rc, rc == RTU_ERR_UNSUPPORTED ? "max_subdiv > 0 (several points per pixel) is not supported" : "the image is no multiple of the map's spacing, or too large");
    if (!map->records) return fail(ctx, RTU_ERR_ARG, "map.records is NULL");
    if (device && ((uintptr_t)map->records & 15u)) return fail(ctx, RTU_ERR_ARG, "device records must be 16-byte aligned");
    return RTU_OK;
}

}  // namespace

extern "C" {

int rtu_irradiance_sample_device(RtuContext* ctx, const RtuIrradianceMap* map, const void* d_xy, size_t n, void* d_out, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    IrrGrid g;
    const int rc = irr_check_map(ctx, map, true, &g);
    if (rc != RTU_OK || n == 0) return rc;
    if (!d_xy || !d_out) return fail(ctx, RTU_ERR_ARG, "position / result pointer is NULL");
    if (((uintptr_t)d_xy & 3u) || ((uintptr_t)d_out & 15u)) return fail(ctx, RTU_ERR_ARG, "positions must be 4-byte, results 16-byte aligned");
    if (n > ((size_t)1 << 26)) return fail(ctx, RTU_ERR_ARG, "more than 2^26 positions in one call");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_irr_sample((const float4*)map->records, g, (const float*)d_xy, n, (float4*)d_out, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "irradiance lookup launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_irradiance_build_device(RtuContext* ctx, const RtuFrameDesc* frame, const RtuIrradianceDesc* desc, void* d_records, void* d_computed,
                                uint32_t* n_computed, uint32_t* per_pass, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = irr_check_frame(ctx, frame);
    if (rc != RTU_OK) return rc;
    IrrGrid g;
    if ((rc = rtu_irradiance_check(desc, frame->width, frame->height, &g)) != RTU_OK)
        return fail(ctx, rc, rc == RTU_ERR_UNSUPPORTED ? "max_subdiv > 0 (several points per pixel) is not supported"
                                                       : "irradiance: min_subdiv -15 .. max_subdiv <= 0, width and height multiples of 2^-max_subdiv, samples 1 .. 4096, "
                                                         "first_sample >= 0, thresholds no NaN, max_bounce 0 .. 5, reserved 0, at most 2^26 points");
    if (!d_records || !d_computed) return fail(ctx, RTU_ERR_ARG, "records / computed pointer is NULL");
    if ((uintptr_t)d_records & 15u) return fail(ctx, RTU_ERR_ARG, "device records must be 16-byte aligned");
    RtuShadeDesc sd;
    rtu_shade_defaults(&sd);
    memcpy(sd.eye, frame->cam_pos, sizeof sd.eye);
    sd.max_bounce = desc->max_bounce;
    RtuFrameDesc f;  // what launch() takes for a path-traced ray batch (RTU_ERR_NO_SCENE here)
    if ((rc = shade_args(ctx, nullptr, nullptr, 0, &sd, true, &f, true, nullptr, true)) != RTU_OK) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const size_t points = (size_t)g.gw * g.gh;
    const uint32_t M = (uint32_t)desc->samples;
    const size_t chunk_points = kIrrChunkChains / M ? kIrrChunkChains / M : 1;
    const size_t max_chains = (points < chunk_points ? points : chunk_points) * M;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const size_t scratch_words = rtu_irr_scratch_words(points);
    RTU_HIP(ctx, ctx->ir_scratch.grow(scratch_words + 4));  // (+ the list's length)
    RTU_HIP(ctx, ctx->ir_list.grow(points));
    RTU_HIP(ctx, ctx->ir_keys.grow(max_chains));
    RTU_HIP(ctx, ctx->ir_c.grow(max_chains));
    uint32_t* const d_total = ctx->ir_scratch.get() + scratch_words;
    float4* const rec = (float4*)d_records;
    uint8_t* const bytes = (uint8_t*)d_computed;
    float4* const c = ctx->ir_c.get();
    IrrThresholds t;
    memcpy(t.color, desc->threshold_color, sizeof t.color);
    t.z = desc->threshold_z;
    t.n = desc->threshold_n;
    IrrRoots roots;
    memcpy(roots.cam.cam_pos, frame->cam_pos, sizeof roots.cam.cam_pos);
    memcpy(roots.cam.origin, frame->origin, sizeof roots.cam.origin);
    memcpy(roots.cam.u, frame->u, sizeof roots.cam.u);
    memcpy(roots.cam.v, frame->v, sizeof roots.cam.v);
    roots.cam.scale = (float)g.scale;
    roots.cam.gw = g.gw;
    roots.samples = M;
    roots.first_sample = (uint32_t)desc->first_sample;
    uint32_t computed_all = 0;
    for (uint32_t p = 0; p <= 2u * g.levels; p++) {
        const IrrPass q = irr_pass(g, p);
        hipError_t e = (hipError_t)rtu_launch_irr_classify(q, t, rec, bytes, ctx->ir_list.get(), d_total, ctx->ir_scratch.get(), stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "irradiance classify launch: %s", hipGetErrorString(e));
        uint32_t total = 0;
        RTU_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, stream));
        RTU_HIP(ctx, hipStreamSynchronize(stream));
        if (total > q.count) return fail(ctx, RTU_ERR_HIP, "irradiance pass %u listed %u of %u points", p, total, q.count);
        for (size_t base = 0; base < total; base += chunk_points) {
            if (cancel_raised(ctx)) return fail(ctx, RTU_ERR_CANCELLED, "cancelled in pass %u of the irradiance map", p);
            const uint32_t m = (uint32_t)(total - base < chunk_points ? total - base : chunk_points), n = m * M;
            RTU_HIP(ctx, ctx->gi_h.grow((size_t)n * (RTU_GI_BOUNCES + 1) * 4));  // (what launch() grows them to for n chains)
            RTU_HIP(ctx, ctx->gi_res.grow((size_t)n * 2));
            roots.list = ctx->ir_list.get() + base;
            roots.n_points = m;
            e = (hipError_t)rtu_launch_irr_roots(half_scene(ctx), roots, ctx->bvh_stack_needed, ctx->gi_h.get(), c, stream);
            if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "irradiance roots launch: %s", hipGetErrorString(e));
            // the chain steps of a path-traced batch of n rays: they read chain records, no ray and no key (the pointers only say "a ray batch")
            const int forced = ctx->tail_hint;
            for (int k = 1; k <= RTU_GI_BOUNCES; k++) {
                ctx->tail_hint = 0;
                if ((rc = launch(ctx, &f, c, stream, k == 1, 0, 1, nullptr, RTU_LAUNCH_CHAIN, k, false, nullptr, 0, c, n, ctx->ir_keys.get())) != RTU_OK) return rc;
            }
            ctx->tail_hint = forced;
            if ((rc = half_until_fits(ctx, f, c, stream, c, ctx->ir_keys.get(), n, HALF_GATHER, nullptr, nullptr)) != RTU_OK) return rc;
            e = (hipError_t)rtu_launch_irr_store(roots.list, m, M, c, ctx->gi_h.get(), rec, bytes, stream);
            if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "irradiance store launch: %s", hipGetErrorString(e));
        }
        if (per_pass) { per_pass[2 * p] = q.count; per_pass[2 * p + 1] = total; }
        computed_all += total;
    }
    RTU_HIP(ctx, hipStreamSynchronize(stream));
    if (n_computed) *n_computed = computed_all;
    return RTU_OK;
}

int rtu_irradiance_build(RtuContext* ctx, const RtuFrameDesc* frame, const RtuIrradianceDesc* desc, float* h_records, uint8_t* h_computed,
                         uint32_t* n_computed, uint32_t* per_pass) {
    if (!ctx) return RTU_ERR_ARG;
    if (!h_records || !h_computed) return fail(ctx, RTU_ERR_ARG, "records / computed pointer is NULL");
    int rc = irr_check_frame(ctx, frame);
    if (rc != RTU_OK) return rc;
    IrrGrid g;
    size_t points = 1;
    if (rtu_irradiance_check(desc, frame->width, frame->height, &g) == RTU_OK) points = (size_t)g.gw * g.gh;  // (else the _device form refuses)
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->ir_rec.grow(2 * points));
    RTU_HIP(ctx, ctx->ir_bytes.grow(points));
    if ((rc = rtu_irradiance_build_device(ctx, frame, desc, ctx->ir_rec.get(), ctx->ir_bytes.get(), n_computed, per_pass, ctx->stream)) != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpy(h_records, ctx->ir_rec.get(), sizeof(float4) * 2 * points, hipMemcpyDeviceToHost));
    RTU_HIP(ctx, hipMemcpy(h_computed, ctx->ir_bytes.get(), points, hipMemcpyDeviceToHost));
    return RTU_OK;
}

int rtu_render_frame_irradiance_device(RtuContext* ctx, const RtuFrameDesc* frame, const RtuIrradianceMap* map, void* d_rgbz, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = irr_check_frame(ctx, frame);
    if (rc != RTU_OK) return rc;
    if (frame->samples < 1) return fail(ctx, RTU_ERR_ARG, "the irradiance frame is a recipe-S frame: samples >= 1");
    if (frame->gather_bounces != 0) return fail(ctx, RTU_ERR_ARG, "the map replaces the gather: gather_bounces must be 0");
    IrrGrid g;
    if ((rc = irr_check_map(ctx, map, true, &g)) != RTU_OK) return rc;
    if (map->width != frame->width || map->height != frame->height) return fail(ctx, RTU_ERR_ARG, "the map was built for another image size");
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "image pointer is NULL");
    if ((uintptr_t)d_rgbz & 15u) return fail(ctx, RTU_ERR_ARG, "the device image must be 16-byte aligned");
    const size_t pixels = (size_t)frame->width * (size_t)frame->height;
    if (pixels > kPathChains) return fail(ctx, RTU_ERR_ARG, "more than 2^25 pixels");
    RtuShadeDesc sd;
    rtu_shade_defaults(&sd);
    memcpy(sd.eye, frame->cam_pos, sizeof sd.eye);
    sd.max_bounce = frame->max_bounce;
    sd.flags = frame->collect_stats == 1 ? RTU_QUERY_REFERENCE_WALK : 0u;
    RtuFrameDesc f;
    if ((rc = shade_args(ctx, nullptr, nullptr, 0, &sd, true, &f, true, nullptr, true)) != RTU_OK) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->ir_rays.grow(2 * pixels));
    RTU_HIP(ctx, ctx->ir_keys.grow(pixels));
    RTU_HIP(ctx, ctx->ir_c.grow(pixels));
    RTU_HIP(ctx, ctx->ir_amb.grow(pixels));
    RTU_HIP(ctx, ctx->ir_acc.grow(pixels));
    RTU_HIP(ctx, ctx->ir_hits.grow(pixels));
    float4* const rays = ctx->ir_rays.get();
    float4* const out = ctx->ir_c.get();
    uint32_t* const keys = ctx->ir_keys.get();
    hipError_t e = (hipError_t)rtu_launch_irr_lookup_centres((const float4*)map->records, g, (uint32_t)frame->width, (uint32_t)frame->height, ctx->ir_amb.get(), stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "irradiance lookup launch: %s", hipGetErrorString(e));
    for (int k = 0; k < frame->samples; k++) {
        if (cancel_raised(ctx)) return fail(ctx, RTU_ERR_CANCELLED, "cancelled after %d of %d samples", k, frame->samples);
        e = (hipError_t)rtu_launch_camera_sample_rays(cam_sample(frame, k), rays, keys, stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "camera ray launch: %s", hipGetErrorString(e));
        if ((rc = half_chain(ctx, f, out, stream, rays, keys, (uint32_t)pixels, HALF_AMBIENT)) != RTU_OK) return rc;
        if ((rc = half_until_fits(ctx, f, out, stream, rays, keys, (uint32_t)pixels, HALF_AMBIENT, ctx->ir_amb.get(),
                                  "the irradiance frame with counters: frame records ran out; render it once without counters first")) != RTU_OK)
            return rc;
        e = (hipError_t)rtu_launch_accumulate(out, 1u, ctx->ir_acc.get(), ctx->ir_hits.get(), (uint32_t)pixels, k == 0, stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "accumulate launch: %s", hipGetErrorString(e));
    }
    e = (hipError_t)rtu_launch_resolve(ctx->ir_acc.get(), ctx->ir_hits.get(), (float4*)d_rgbz, (uint32_t)pixels, (uint32_t)frame->samples, stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "resolve launch: %s", hipGetErrorString(e));
    RTU_HIP(ctx, hipStreamSynchronize(stream));
    return RTU_OK;
}

int rtu_render_frame_irradiance(RtuContext* ctx, const RtuFrameDesc* frame, const RtuIrradianceMap* map, float* h_rgbz) {
    if (!ctx) return RTU_ERR_ARG;
    if (!h_rgbz) return fail(ctx, RTU_ERR_ARG, "image pointer is NULL");
    int rc = irr_check_frame(ctx, frame);
    if (rc != RTU_OK) return rc;
    IrrGrid g;
    if ((rc = irr_check_map(ctx, map, false, &g)) != RTU_OK) return rc;
    const size_t points = (size_t)g.gw * g.gh, pixels = (size_t)frame->width * (size_t)frame->height;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->ir_rec.grow(2 * points));
    RTU_HIP(ctx, ctx->ir_img.grow(pixels));
    RTU_HIP(ctx, hipMemcpy(ctx->ir_rec.get(), map->records, sizeof(float4) * 2 * points, hipMemcpyHostToDevice));
    RtuIrradianceMap dm = *map;
    dm.records = ctx->ir_rec.get();
    if ((rc = rtu_render_frame_irradiance_device(ctx, frame, &dm, ctx->ir_img.get(), ctx->stream)) != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpy(h_rgbz, ctx->ir_img.get(), sizeof(float4) * pixels, hipMemcpyDeviceToHost));
    return RTU_OK;
}

uint32_t rtu_sample_key(uint32_t pixel, uint32_t sample) { return h_mix32(h_mix32(pixel + 0x68bc21ebU) ^ (sample * 0x9e3779b9U + 1U)); }
uint32_t rtu_child_key(uint32_t key, uint32_t slot) { return h_mix32(key + (slot + 1U) * 0x632be5abU); }

// the rays and keys of sample `sample` of a recipe-S frame: primary_pixel's recipe-S branch (render_impl.h; RenderFunctions.cpp:80-97,
// :258-268) and launch()'s pixel offsets, the same binary32 expressions in the same order, so the same bits
int rtu_camera_sample_rays(const RtuFrameDesc* frame, int sample, int row0, int nrows, RtuRay* rays_out, uint32_t* keys_out) {
    if (!frame || frame->width <= 0 || frame->height <= 0 || row0 < 0 || nrows < 0 || row0 > frame->height || nrows > frame->height - row0)
        return RTU_ERR_ARG;
    if (frame->samples < 1 || sample < 0 || sample >= frame->samples) return RTU_ERR_ARG;
    if (nrows && (!rays_out || !keys_out)) return RTU_ERR_ARG;
    const CamSample c = cam_sample(frame, sample);
    for (int y = row0; y < row0 + nrows; y++)
        for (int x = 0; x < frame->width; x++) {
            f3 org, dir;
            uint32_t key;
            camera_sample_ray(c, x, y, HostSinCos(), org, dir, key);
            const size_t i = (size_t)(y - row0) * (size_t)frame->width + (size_t)x;
            RtuRay& r = rays_out[i];
            r.org[0] = org.x; r.org[1] = org.y; r.org[2] = org.z;
            r.tmax = RTU_BIGFLOAT;
            r.dir[0] = dir.x; r.dir[1] = dir.y; r.dir[2] = dir.z;
            r.reserved = 0;
            keys_out[i] = key;
        }
    return RTU_OK;
}

// the same on the device (rtu_camrays.hip): camera_sample_ray per lane, so the same bits
int rtu_camera_sample_rays_device(RtuContext* ctx, const RtuFrameDesc* frame, int sample, void* d_rays, void* d_keys, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (!frame || frame->width <= 0 || frame->height <= 0) return fail(ctx, RTU_ERR_ARG, "frame is NULL or empty");
    if (frame->samples < 1 || sample < 0 || sample >= frame->samples) return fail(ctx, RTU_ERR_ARG, "not a recipe S frame, or sample outside [0, samples)");
    if ((size_t)frame->width * (size_t)frame->height > ((size_t)1 << 26)) return fail(ctx, RTU_ERR_ARG, "more than 2^26 pixels in one call");
    if (!d_rays || !d_keys) return fail(ctx, RTU_ERR_ARG, "ray / key pointer is NULL");
    if (((uintptr_t)d_rays & 15u) || ((uintptr_t)d_keys & 3u)) return fail(ctx, RTU_ERR_ARG, "the ray buffer must be 16-byte, the key buffer 4-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_camera_sample_rays(cam_sample(frame, sample), (float4*)d_rays, (uint32_t*)d_keys, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "camera ray launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

// the primary rays of primary_pixel (render_impl.h; RenderFunctions.cpp:258-268, :97) for the pixel centres of rows [row0, row0 + nrows):
// the same binary32 expressions in the same order (rtu_vec.h, this file is compiled with -ffp-contract=off), so the same bits
int rtu_camera_rays(const RtuFrameDesc* frame, int row0, int nrows, RtuRay* rays_out) {
    if (!frame || frame->width <= 0 || frame->height <= 0 || row0 < 0 || nrows < 0 || row0 > frame->height || nrows > frame->height - row0)
        return RTU_ERR_ARG;
    if (nrows && !rays_out) return RTU_ERR_ARG;
    const f3 cam_pos = ld3(frame->cam_pos), cam_origin = ld3(frame->origin), cam_u = ld3(frame->u), cam_v = ld3(frame->v);
    for (int y = row0; y < row0 + nrows; y++)
        for (int x = 0; x < frame->width; x++) {
            const f3 cp = (cam_origin + cam_u * ((float)x + 0.5f)) + cam_v * ((float)y + 0.5f);
            const f3 dir = norm3(cp - cam_pos);
            RtuRay& r = rays_out[(size_t)(y - row0) * (size_t)frame->width + (size_t)x];
            r.org[0] = cam_pos.x; r.org[1] = cam_pos.y; r.org[2] = cam_pos.z;
            r.tmax = RTU_BIGFLOAT;
            r.dir[0] = dir.x; r.dir[1] = dir.y; r.dir[2] = dir.z;
            r.reserved = 0;
        }
    return RTU_OK;
}

}  // extern "C"

extern "C" {

// ---- ray sorting (rtu_raysort.hip): the order, and the kernels that apply it ----------------------------------------------------
int rtu_ray_sort_box(const RtuContext* ctx, float box_out[6]) {
    if (!ctx || !box_out) return RTU_ERR_ARG;
    if (!ctx->has_scene) return RTU_ERR_NO_SCENE;
    memcpy(box_out, ctx->sort_box, sizeof ctx->sort_box);
    return RTU_OK;
}

// what rtu_ray_sort_box answers after rtu_upload_scene(scene), without a GPU
int rtu_scene_sort_box(const RtuSceneDesc* s, float box_out[6]) {
    if (!box_out) return RTU_ERR_ARG;
    RtuContext tmp;  // plain host state: nothing here touches a GPU
    const int rc = validate(&tmp, s);
    if (rc != RTU_OK) return rc;
    std::vector<DevNode> nodes(s->n_nodes);
    const float wscale = world_bounds(s, nodes);
    sort_box_of(nodes, wscale, box_out);
    return RTU_OK;
}

}  // extern "C"

namespace {

const size_t kSortMaxRays = (size_t)1 << 26;

int order_args(RtuContext* ctx, const void* rays, const void* order, size_t n, bool device) {
    if (n > kSortMaxRays) return fail(ctx, RTU_ERR_ARG, "more than 2^26 rays in one call");
    if (n && (!rays || !order)) return fail(ctx, RTU_ERR_ARG, "rays / order pointer is NULL");
    if (device && n && ((uintptr_t)rays & 15u)) return fail(ctx, RTU_ERR_ARG, "the device ray buffer must be 16-byte aligned");
    if (device && n && ((uintptr_t)order & 3u)) return fail(ctx, RTU_ERR_ARG, "the order buffer must be 4-byte aligned");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    return RTU_OK;
}

}  // namespace

extern "C" {

int rtu_ray_order_device(RtuContext* ctx, const void* d_rays, size_t n, void* d_order, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    const int rc = order_args(ctx, d_rays, d_order, n, true);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->so_scratch.grow(rtu_ray_order_scratch_words(n)));
    const hipError_t e = (hipError_t)rtu_launch_ray_order(make_sortbox(ctx->sort_box), (const float4*)d_rays, n, (uint32_t*)d_order,
                                                          ctx->so_scratch.get(), (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "ray sort launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_ray_order(RtuContext* ctx, const RtuRay* h_rays, size_t n, uint32_t* h_order) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = order_args(ctx, h_rays, h_order, n, false);
    if (rc != RTU_OK || n == 0) return rc;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->so_rays.grow(2 * n));
    RTU_HIP(ctx, ctx->so_order.grow(n));
    RTU_HIP(ctx, hipMemcpyAsync(ctx->so_rays.get(), h_rays, sizeof(RtuRay) * n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = rtu_ray_order_device(ctx, ctx->so_rays.get(), n, ctx->so_order.get(), ctx->stream)) != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpyAsync(h_order, ctx->so_order.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTU_OK;
}

int rtu_permute_device(RtuContext* ctx, const void* d_src, void* d_dst, const void* d_order, size_t n, uint32_t elem_bytes, int scatter,
                       void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    if (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 16 && elem_bytes != 32 && elem_bytes != 48)
        return fail(ctx, RTU_ERR_ARG, "elem_bytes must be 1, 4, 16, 32 or 48");
    if (scatter != 0 && scatter != 1) return fail(ctx, RTU_ERR_ARG, "scatter must be 0 or 1");
    if (n > kSortMaxRays) return fail(ctx, RTU_ERR_ARG, "more than 2^26 elements in one call");
    if (n == 0) return RTU_OK;
    if (!d_src || !d_dst || !d_order) return fail(ctx, RTU_ERR_ARG, "source / destination / order pointer is NULL");
    if (d_src == d_dst) return fail(ctx, RTU_ERR_ARG, "a permutation cannot be applied in place");
    const uintptr_t align = elem_bytes >= 16 ? 15u : elem_bytes - 1;
    if (((uintptr_t)d_src & align) || ((uintptr_t)d_dst & align) || ((uintptr_t)d_order & 3u))
        return fail(ctx, RTU_ERR_ARG, "source and destination must be aligned to min(elem_bytes, 16), the order to 4 bytes");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = (hipError_t)rtu_launch_permute(d_src, d_dst, (const uint32_t*)d_order, n, elem_bytes, scatter, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "permute launch: %s", hipGetErrorString(e));
    return RTU_OK;
}

int rtu_copy_to_device(RtuContext* ctx, void* d_dst, const void* h_src, size_t bytes) {
    if (!ctx || !d_dst || !h_src) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return RTU_OK;
}

unsigned long long rtu_debug_device_allocations(void) { return g_devbuf_allocations.load(); }
unsigned long long rtu_debug_device_bytes(void) { return g_devbuf_bytes.load(); }

void* rtu_device_alloc(RtuContext* ctx, size_t bytes) {
    if (!ctx || bytes == 0) return nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}

void rtu_device_free(RtuContext* ctx, void* d_ptr) {
    if (!ctx || !d_ptr) return;
    (void)hipSetDevice(ctx->device);
    (void)hipFree(d_ptr);
}

void* rtu_context_stream(RtuContext* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int rtu_context_device(const RtuContext* ctx) { return ctx ? ctx->device : -1; }

int rtu_context_sync(RtuContext* ctx) {
    if (!ctx) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTU_OK;
}

void* rtu_host_alloc_pinned(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void rtu_host_free_pinned(void* p) {
    if (p) (void)hipHostFree(p);
}

int rtu_copy_to_host_async(RtuContext* ctx, void* h_dst, const void* d_src, size_t bytes, void* hip_stream) {
    if (!ctx || !h_dst || !d_src) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    return RTU_OK;
}

int rtu_copy_to_host(RtuContext* ctx, void* h_dst, const void* d_src, size_t bytes) {
    if (!ctx || !h_dst || !d_src) return RTU_ERR_ARG;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, hipDeviceSynchronize());
    RTU_HIP(ctx, hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return RTU_OK;
}

}  // extern "C"
