/*
 * rtu_oracle.h — C interface of the CPU restatement (oracle/rtu_oracle.cpp).
 * TEST INFRASTRUCTURE: see the header of rtu_oracle.cpp. Loaded only by tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg.
 * Besides the renders of whole images there are two ray-level entries on caller-supplied rays: rtu_oracle_rays (closest hit, occlusion
 * and the radiance of recipe W) and rtu_oracle_rays_keyed (recipes S and P, the gathered light alone and a given ambient term, under
 * caller-supplied keys), with rtu_oracle_rays_keyed_info to tell what such rays meet.
 */
#ifndef RTU_ORACLE_H_INCLUDED
#define RTU_ORACLE_H_INCLUDED

#include "rtu_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTU_ORACLE_ERR_ARG         (-1)
#define RTU_ORACLE_ERR_STOCHASTIC  (-2) /* soft shadows / glossy / dof: reference is non-deterministic */
#define RTU_ORACLE_ERR_UNSUPPORTED (-3) /* outside the restated scope */

/* Same fields, same meaning as RtuStats in rtu_render.h, so CPU and GPU ray and
 * traversal counters can be compared exactly. */
typedef struct RtuOracleStats {
    uint64_t primary_rays, primary_hits;
    uint64_t secondary_rays;  /* root-level Trace calls issued by Shade */
    uint64_t shadow_rays;     /* root-level ShadowTrace calls issued by Shadow */
    uint64_t node_tests;      /* ray x object-node intersection calls */
    uint64_t mesh_entries;    /* rays that passed a mesh's bounding box */
    uint64_t inner_visits, leaf_visits, leaf_elems;
    uint64_t tri_tests, tri_accepts;
} RtuOracleStats;

/* Recipe W over rows [row0,row0+nrows): rgbz_out holds nrows*width float4
 * {linear r,g,b, z}; z = hInfo.z of the primary hit (RTU_BIGFLOAT on a miss). */
int  rtu_oracle_render_rows(const RtuSceneDesc* scene, int width, int height, int row0, int nrows,
                            float* rgbz_out, RtuOracleStats* stats, int threads);
int  rtu_oracle_render(const RtuSceneDesc* scene, int width, int height, float* rgbz_out,
                       RtuOracleStats* stats, int threads);
/* The whole frame with the work distribution chosen: 0 = chunks of four rows per fetch (what the other entry points do),
 * 1 = the reference's PixelIterator (PixelIterator.h:25-38): one shared atomic counter, one pixel per fetch. Same image. */
int  rtu_oracle_render_scheduled(const RtuSceneDesc* scene, int width, int height, float* rgbz_out,
                                 RtuOracleStats* stats, int threads, int per_pixel_schedule);
/* Recipe S (row f1): spp samples per pixel as in the sample loop of Render() (RenderFunctions.cpp:73-152:
 * Halton pixel offsets, depth of field, soft shadows, glossy bounces), direct lighting only; rgb = mean
 * of the samples, z = mean hInfo.z of the samples that hit. stream: where the integers that replace
 * rand() come from (see rtu_oracle.cpp "Sample streams"); trig: sinf/cosf of libm (as the reference
 * calls them) or the portable evaluation the device uses. */
#define RTU_ORACLE_STREAM_KEYED      0
#define RTU_ORACLE_STREAM_SEQUENTIAL 1
#define RTU_ORACLE_TRIG_PORTABLE     0
#define RTU_ORACLE_TRIG_LIBM         1
int  rtu_oracle_render_samples(const RtuSceneDesc* scene, int width, int height, int row0, int nrows, int spp,
                               int stream, int trig, float* rgbz_out, RtuOracleStats* stats, int threads);
/* Recipe P (config 5): recipe S plus the Monte-Carlo gather of Render() (RenderFunctions.cpp:129-135: MonteCarlo
 * with 4 bounces and 1 sample, :549-590; cosine-weighted hemisphere sampling, :320-337). */
int  rtu_oracle_render_paths(const RtuSceneDesc* scene, int width, int height, int row0, int nrows, int spp,
                             int stream, int trig, float* rgbz_out, RtuOracleStats* stats, int threads);
/* The samples [first, first + n) of the fixed spp-sample frame of recipe S (gi 0) or P (gi 1), keyed stream and portable trig:
 * out holds n x nrows x width float4 {r, g, b, z}, z = RTU_BIGFLOAT for a miss — what the device's rtu_debug_sample_images returns. */
int  rtu_oracle_render_sample_images(const RtuSceneDesc* scene, int width, int height, int row0, int nrows, int spp, int gi, int first,
                                     int n, float* out, int threads);
/* Adaptive sampling of recipe S / P as include/rtu_render.h states it (keyed stream, portable trig): binary32 sums s, q in sample
 * order; at each checkpoint n = min_samples + k * increment < spp the pixel stops when (q - s * (s / n)) / (n - 1) <= target for r,
 * g and b (n == 1: +inf). counts_out: the rule's count per pixel. rgbz_out: the mean of the first counts_in[p] samples (counts_in
 * NULL: of the rule's count), z the mean over the hits among them. margin_out (may be NULL): per pixel, the smallest
 * |max(var_r, var_g, var_b) - target| over the checkpoints the rule evaluated up to its stop, divided by target when
 * 0 < target < inf; +inf when no checkpoint could go either way. trace_batch B: a pixel that stops at n is traced and shaded on,
 * for the counters only, to min(spp, B * ceil(n / B)) — what the device traces with batches of B samples; with counts_in NULL
 * the stats then equal the device's counting variant (with counts_in they count the samples traced for the larger of the two counts). */
int  rtu_oracle_render_adaptive(const RtuSceneDesc* scene, int width, int height, int row0, int nrows, int spp, int gi, int min_samples,
                                int increment, float target, int trace_batch, const uint8_t* counts_in, float* rgbz_out,
                                uint8_t* counts_out, float* margin_out, RtuOracleStats* stats, int threads);
/* Test hook: 1 = test every triangle of a mesh whatever its boxes say (NOT the reference's algorithm; see rtu_oracle.cpp). */
void rtu_oracle_debug_all_triangles(int on);
/* Test hook: the bounceCount the root Shade() calls of every later render receive (0..RTU_MAX_BOUNCE; the reference's 5 until set;
 * a value outside the range changes nothing). Returns the previous value. Not to be called while a render runs. */
int  rtu_oracle_debug_max_bounce(int max_bounce);
void rtu_oracle_portable_sincos(const float* t, int n, float* sin_out, float* cos_out);
void rtu_oracle_portable_acos(const float* x, int n, float* out);
uint32_t rtu_oracle_rand31(uint32_t key, uint32_t idx);
uint32_t rtu_oracle_sample_key(uint32_t pixel, uint32_t sample);
uint32_t rtu_oracle_child_key(uint32_t key, uint32_t slot);
/* The texture arithmetic recipe W uses, on n inputs: the counterpart of the device's rtu_debug_texcoords (same op codes,
 * same layouts; see include/rtu_render.h). ATAN2F / ASINF / SPHERE_UV / ENV_UVW call the host libm's atan2f and asinf, as
 * the reference does. TEXTURE / MAP need a textured `scene`: texture `index`, or material map `index` (-1 background,
 * -2 environment), which must be present (RTU_ORACLE_ERR_ARG otherwise, as the device's RTU_ERR_ARG). */
#define RTU_ORACLE_TEXOP_ATAN2F     0
#define RTU_ORACLE_TEXOP_ASINF      1
#define RTU_ORACLE_TEXOP_SPHERE_UV  2
#define RTU_ORACLE_TEXOP_ENV_UVW    3
#define RTU_ORACLE_TEXOP_TILE_CLAMP 4
#define RTU_ORACLE_TEXOP_TEXTURE    5
#define RTU_ORACLE_TEXOP_MAP        6
int  rtu_oracle_texcoords(const RtuSceneDesc* scene, int op, int index, const float* in, long long n, float* out, int threads);
/* The restatements of glibc's asinf / atanf / atan2f that the device uses (rtu_oracle.cpp), and the host libm's own
 * functions, on n inputs (atan2f: n pairs {y, x}). */
#define RTU_ORACLE_FN_ASINF  0
#define RTU_ORACLE_FN_ATANF  1
#define RTU_ORACLE_FN_ATAN2F 2
void rtu_oracle_portable_libm(int fn, const float* in, long long n, float* out);
void rtu_oracle_host_libm(int fn, const float* in, long long n, float* out);
/* Restatement against the host libm on `count` inputs: for ASINF / ATANF the floats with bit patterns first .. first +
 * count - 1, for ATAN2F the pairs first .. first + count - 1 of a seeded generator (rtu_oracle.cpp atan2f_pair). Counts
 * results that differ (NaN equals NaN); first_bad[2] gets the lowest failing input (bits of x, or of y and x). */
long long rtu_oracle_check_portable(int fn, uint64_t first, uint64_t count, uint64_t seed, int threads, uint32_t* first_bad);
/* The ray-level entry: Trace / ShadowTrace / Shade on n caller-supplied rays, the counterpart of the device's rtu_trace_rays,
 * rtu_occluded_rays and rtu_shade_rays (include/rtu_render.h; RtuOracleRay and RtuOracleRayHit have the layouts of RtuRay and
 * RtuRayHit). Per ray HitInfo::Init's z is replaced by tmax and dir is used as given; NO ray is filtered: pass valid rays only.
 * out: CLOSEST n RtuOracleRayHit (a miss: t = tmax, flags 0, node = material = -1, p = N = 0); OCCLUDED n bytes (`hit && hInfo.z > 0`);
 * SHADE n float4 {r, g, b, hInfo.z} — a hit is Shade() at the depth of rtu_oracle_debug_max_bounce with `eye` (three floats, SHADE
 * only) as camera.pos, a miss is environment.SampleEnvironment(dir) with z = tmax — and the counters in `stats` (may be NULL).
 * Stochastic scenes are refused as by rtu_oracle_render_rows. */
typedef struct RtuOracleRay    { float org[3]; float tmax; float dir[3]; uint32_t reserved; } RtuOracleRay;       /* 32 B */
typedef struct RtuOracleRayHit { float t; int32_t node; uint32_t flags; int32_t material;
                                 float p[3]; float pad0; float N[3]; float pad1; } RtuOracleRayHit;                /* 48 B */
#define RTU_ORACLE_RAY_HIT       1u
#define RTU_ORACLE_RAY_FRONT     2u
#define RTU_ORACLE_RAYS_CLOSEST  0
#define RTU_ORACLE_RAYS_OCCLUDED 1
#define RTU_ORACLE_RAYS_SHADE    2
int  rtu_oracle_rays(const RtuSceneDesc* scene, const RtuOracleRay* rays, long long n, const float* eye, int mode, void* out,
                     RtuOracleStats* stats, int threads);
/* The keyed ray-level entry: recipes S and P on n caller-supplied rays with one key each, the counterpart of the device's
 * rtu_shade_rays_sampled, rtu_shade_rays_paths, rtu_gather_rays and rtu_shade_rays_ambient (include/rtu_render.h). Keyed stream, portable
 * trig, the depth of rtu_oracle_debug_max_bounce, `eye` (three floats) as camera.pos. As for rtu_oracle_rays, HitInfo::Init's z is replaced
 * by tmax, dir is used as given and NO ray is filtered: pass valid rays only. out: n float4 in every mode.
 *   SAMPLED  {r, g, b, hInfo.z}: a hit is Shade(hit, max_bounce, lights) on the streams of keys[i] (a node without material: white), a miss
 *            is environment.SampleEnvironment(dir) with t = tmax — one sample of rtu_oracle_render_samples after it has its ray.
 *   PATHS    a hit with a material: c = MonteCarlo(hit, 4) drawn from keys[i], then Shade(hit, {AmbientLight(c)}) on child_key(keys[i], 4)
 *            + Shade(hit, lights) on keys[i], in that order (RenderFunctions.cpp:129-135); otherwise as SAMPLED.
 *   GATHER   {c.r, c.g, c.b, hInfo.z}; c = 0 on a miss (t = tmax) and at a node without material.
 *   AMBIENT  PATHS with (0 + amb[i]) + 0 in place of c (a negative zero becomes +0); amb: n float4 {r, g, b, ignored}, this mode only.
 * stats (may be NULL): the counters of a render; gather rays are in no ray counter (their traversal counters are counted), as in
 * rtu_oracle_render_paths. Scenes without stochastic features are accepted. keys == NULL, or amb == NULL in AMBIENT, with n > 0, eye ==
 * NULL and an unknown mode are RTU_ORACLE_ERR_ARG. Threads take contiguous chunks of rays. */
#define RTU_ORACLE_KEYED_SAMPLED 0
#define RTU_ORACLE_KEYED_PATHS   1
#define RTU_ORACLE_KEYED_GATHER  2
#define RTU_ORACLE_KEYED_AMBIENT 3
int  rtu_oracle_rays_keyed(const RtuSceneDesc* scene, const RtuOracleRay* rays, const uint32_t* keys, const float* amb, long long n,
                           const float* eye, int mode, float* out, RtuOracleStats* stats, int threads);
/* What keyed rays meet, for the tests that assert the contents of a ray family: four words per ray. [0]: 1 hit | 2 front | 4 the node
 * has a material | 8 that material is glossy; [1]: how many gather rays of MonteCarlo(hit, 4)'s chain under keys[i] hit (4: the chain
 * reaches depth 4; d < 4: it leaves the scene at depth d + 1; 0 where nothing is gathered); [2], [3]: the shadow rays the root Shade()
 * fires towards lights of size > 0 under keys[i], and how many of them are occluded. */
#define RTU_ORACLE_INFO_HIT      1u
#define RTU_ORACLE_INFO_FRONT    2u
#define RTU_ORACLE_INFO_MATERIAL 4u
#define RTU_ORACLE_INFO_GLOSSY   8u
int  rtu_oracle_rays_keyed_info(const RtuSceneDesc* scene, const RtuOracleRay* rays, const uint32_t* keys, long long n, uint32_t* info,
                                int threads);
/* pos, origin, u, v of the image plane (RenderFunctions.cpp:243-269). */
int  rtu_oracle_camera_frame(const RtuCamera* cam, int width, int height, float out12[12]);
/* gamma + Color24 + z-image; any output pointer may be NULL. */
void rtu_oracle_postprocess(const float* rgbz, int width, int height, unsigned char* rgb_out,
                            float* z_out, unsigned char* zimg_out);

#ifdef __cplusplus
}
#endif
#endif
