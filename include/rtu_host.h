/*
 * rtu_host.h — C entry points of librtu_host.so, the host side of the drop-in
 * boundary (pure C++/g++, no GPU code). It is the input and output side of the
 * render path:
 *
 *   scene files  --rtu_scene_load_xml-->  RtuScene (owned, flattened)
 *   RtuScene     --rtu_scene_desc------>  RtuSceneDesc  --> rtu_upload_scene (rtu_render.h)
 *   float4 rgbz  --rtu_image_*---------->  Color24 / z-image / Result.png / ZBuffer.png
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   rtu_scene_load_xml      <- int LoadScene(const char*)        ExternalLibrary/xmlload.cpp:64-131
 *                              TriObj::Load                      ExternalLibrary/objects.h:52-60
 *   rtu_image_from_rgbz     <- gamma + Color24 store             RenderFunctions.cpp:152-160
 *   rtu_image_compute_zimg  <- RenderImage::ComputeZBufferImage  ExternalLibrary/scene.h:590-612
 *   rtu_image_save_png      <- RenderImage::SaveImage/SaveZImage ExternalLibrary/scene.h:633-654
 *   rtu_image_compute_sample_count_img / rtu_image_save_sample_count_png
 *                           <- ComputeSampleCountImage / SaveSampleCountImage  scene.h:614-640
 *   rtu_begin_render / rtu_stop_render / rtu_render_wait
 *                           <- BeginRender()/StopRender()        main.cpp:66-72, viewport.cpp:36-37
 *   rtu_begin_render_progressive
 *                           <- the viewport showing renderImage fill in  viewport.cpp:390-449
 */
#ifndef RTU_HOST_H_INCLUDED
#define RTU_HOST_H_INCLUDED

#include "rtu_scene.h"
#include "rtu_render.h"  /* RtuAdaptiveDesc */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- owned scenes ------------------------------------------------------- */
typedef struct RtuScene RtuScene; /* opaque; owns every array its desc points to */

/* Load a scene XML (+ the OBJ files it names). Every occurrence of the prefix
 * `remap_from` at the start of a file name inside the XML is replaced by
 * `remap_to` (the reference's scenes carry the author's absolute paths);
 * either may be NULL. Returns NULL on failure (message via rtu_host_last_error),
 * mirroring LoadScene()'s 0 return. */
RtuScene* rtu_scene_load_xml(const char* xml_path, const char* remap_from, const char* remap_to);

/* Deep-copy an existing description (e.g. one assembled by a caller). */
RtuScene* rtu_scene_clone(const RtuSceneDesc* desc);

/* Blob round trip (little endian, position independent) — the format of the
 * fixtures in tests/golden/. */
RtuScene* rtu_scene_load_blob(const void* blob, size_t size);
RtuScene* rtu_scene_load_blob_file(const char* path);
void*     rtu_scene_to_blob(const RtuSceneDesc* desc, size_t* size_out); /* malloc'ed */
int       rtu_scene_save_blob_file(const RtuSceneDesc* desc, const char* path);
void      rtu_blob_free(void* blob);

const RtuSceneDesc* rtu_scene_desc(const RtuScene* scene);
/* Override the render resolution after loading (set camera.imgWidth /
 * imgHeight after LoadScene, then re-Init the RenderImage). */
void      rtu_scene_set_resolution(RtuScene* scene, int width, int height);
void      rtu_scene_free(RtuScene* scene);

/* Move things in a loaded scene (then rtu_update_scene, rtu_render.h). Each appends one more operation to node `node`'s
 * transformation with the loader's own arithmetic (Transformation::Scale / Rotate / Translate, scene.h:244-247): the node's
 * tm / itm / pos equal a load of the XML with that operation appended to the node's transform. rotate normalises the axis as
 * LoadTransform does (xmlload.cpp:274); the angle is in degrees. set_light replaces light `index`, normalising a direct light's
 * direction as DirectLight::SetDirection does. 0, or -1 for a bad index / NULL. */
int       rtu_scene_node_scale(RtuScene* scene, uint32_t node, float sx, float sy, float sz);
int       rtu_scene_node_rotate(RtuScene* scene, uint32_t node, float ax, float ay, float az, float degrees);
int       rtu_scene_node_translate(RtuScene* scene, uint32_t node, float x, float y, float z);
int       rtu_scene_set_light(RtuScene* scene, uint32_t index, const RtuLight* light);

/* Deform a mesh of a loaded scene (then rtu_update_meshes, rtu_render.h). set_mesh_vertices: v is nv * 3 floats replacing the
 * mesh's positions; vn is nvn * 3 floats or NULL (the normals stay). Connectivity (f, fn, ft, vt) stays. Then exactly what
 * TriObj::Load does after reading the file (objects.h:57-58): ComputeBoundingBox and the reference's BVH build — the scene is,
 * byte for byte as a blob, the scene a load of an .obj with those vertices gives; n_bvh_nodes and bvh_depth may change.
 * recompute_normals: ComputeNormals (area-weighted, cyTriMesh.h:248-261) from the current positions, only for a mesh whose normals
 * have that form (nvn == nv and fn equal to f, what the loader makes for a file without vn lines); otherwise -1 and nothing
 * changes. Pointers from an earlier rtu_scene_desc stay valid (the arrays keep their sizes; bvh may move: read the desc again).
 * 0, or -1 for a bad index / NULL (rtu_host_last_error). */
int       rtu_scene_set_mesh_vertices(RtuScene* scene, uint32_t mesh, const float* v, const float* vn);
int       rtu_scene_recompute_normals(RtuScene* scene, uint32_t mesh);

const char* rtu_host_last_error(void);

/* ---- output side: RenderImage mirror ------------------------------------ */
typedef struct RtuImage RtuImage; /* Color24 img[], float zbuffer[], uchar zimg[] */

RtuImage* rtu_image_create(int width, int height);            /* RenderImage::Init, scene.h:552-572 */
void      rtu_image_free(RtuImage* img);
int       rtu_image_width(const RtuImage* img);
int       rtu_image_height(const RtuImage* img);
uint8_t*  rtu_image_pixels(RtuImage* img);                    /* W*H*3, GetPixels() */
float*    rtu_image_zbuffer(RtuImage* img);                   /* W*H,   GetZBuffer() */
uint8_t*  rtu_image_zimage(RtuImage* img);                    /* W*H or NULL before compute */
int       rtu_image_num_rendered(const RtuImage* img);        /* GetNumRenderedPixels() */
int       rtu_image_is_done(const RtuImage* img);             /* IsRenderDone() */

/* Fill rows [row0,row0+nrows) from linear float4 {r,g,b,z}: gamma
 * pow(double(c),1/2.2) -> float, Color24 truncation, z copy; bumps the rendered
 * pixel counter by nrows*W. */
void      rtu_image_from_rgbz(RtuImage* img, const float* rgbz, int row0, int nrows);
void      rtu_image_compute_zimg(RtuImage* img);
int       rtu_image_save_png(const RtuImage* img, const char* path);   /* 8-bit RGB */
int       rtu_image_save_zpng(const RtuImage* img, const char* path);  /* 8-bit grey */
/* uchar sampleCount[] (scene.h:545): the samples each pixel took, W*H, zero after create; fill rows from a count image
 * (rtu_render_frame_adaptive). ComputeSampleCountImage (scene.h:614-635): 255 * (c - smin) / (smax - smin) in integers, all 0 when
 * smax == smin; returns smax. The sample-count image is NULL before it is computed; the PNG is 8-bit grey (SaveSampleCountImage). */
uint8_t*  rtu_image_sample_count(RtuImage* img);
void      rtu_image_fill_sample_count(RtuImage* img, const uint8_t* counts, int row0, int nrows);
int       rtu_image_compute_sample_count_img(RtuImage* img);
uint8_t*  rtu_image_sample_count_image(RtuImage* img);
int       rtu_image_save_sample_count_png(const RtuImage* img, const char* path);
/* Generic 8-bit PNG writer (comp = 1 or 3). */
int       rtu_write_png(const char* path, const uint8_t* data, int width, int height, int comp);

/* ---- BeginRender()/StopRender() drop-in ---------------------------------- */
typedef struct RtuRenderJob RtuRenderJob;

/* Start rendering `scene` into `img` on the given GPUs (device ordinals) and
 * return immediately; a single host thread drives the C-ABI in rtu_render.h,
 * then writes result_png / zbuffer_png (either may be NULL to skip), exactly
 * the sequence of main.cpp:29-64. */
RtuRenderJob* rtu_begin_render(const RtuScene* scene, RtuImage* img,
                               const int* device_ids, int n_devices,
                               const char* result_png, const char* zbuffer_png);
/* The same with `samples` per pixel (RtuFrameDesc.samples in rtu_render.h): 0 is rtu_begin_render; S >= 1
 * renders recipe S, which scenes with soft shadows, glossy bounces or depth of field need (the reference's
 * Render() hard-codes 1024 samples, RenderFunctions.cpp:27). */
RtuRenderJob* rtu_begin_render_sampled(const RtuScene* scene, RtuImage* img,
                                       const int* device_ids, int n_devices, int samples,
                                       const char* result_png, const char* zbuffer_png);
/* HEAD's path-traced mode (config 5): the same plus the 4-bounce Monte-Carlo gather (RtuFrameDesc.gather_bounces = 4). */
RtuRenderJob* rtu_begin_render_paths(const RtuScene* scene, RtuImage* img,
                                     const int* device_ids, int n_devices, int samples,
                                     const char* result_png, const char* zbuffer_png);
/* Adaptive sampling (rtu_render_frame_adaptive): `samples` is the maximum per pixel (1 .. 255), gather_bounces 0 (recipe S) or 4
 * (recipe P), adaptive NULL = rtu_adaptive_defaults. One context per listed device (ids may repeat), each rendering its shard;
 * rows and sample counts are assembled into img. Then main.cpp:59-63: Result.png, ZBuffer.png and — the lines the reference leaves
 * commented out — ComputeSampleCountImage + SampleCount.png (any path may be NULL to skip). rtu_stop_render cancels between batches. */
RtuRenderJob* rtu_begin_render_adaptive(const RtuScene* scene, RtuImage* img, const int* device_ids, int n_devices, int samples,
                                        int gather_bounces, const RtuAdaptiveDesc* adaptive, const char* result_png,
                                        const char* zbuffer_png, const char* samplecount_png);
/* Progressive display (rtu_progressive_begin, rtu_render.h): the frame refined pass by pass behind BeginRender(), as the reference's
 * viewport shows renderImage filling in (viewport.cpp:390-449). A recipe S (gather_bounces 0) or P (4) frame of `samples` per pixel
 * (adaptive NULL), or adaptive with `samples` the maximum (1 .. 255). pass_samples[n_passes] are the samples of each pass: every
 * one >= 1, adding up to `samples` (NULL: 1, 1, 2, 4, 8, ... — each pass doubles what is shown, the last one up to `samples`);
 * anything else is refused (NULL, rtu_host_last_error) before any GPU is touched. One context and one session per listed device (ids
 * may repeat), each rendering its shard; the passes advance in lockstep. After every pass the shards' snapshots are assembled into
 * img — Color24 pixels, z-buffer, and sample counts when adaptive — and on_pass(user, samples_done, pass) is called from the job's
 * thread (pass: 1 for the first); the next pass starts when it returns, so img does not change while it runs (copy img there); the rendered-pixel counter reaches W * H with the first pass and stays there. At the end:
 * Result.png, ZBuffer.png and, adaptive only, SampleCount.png (any path may be NULL). rtu_stop_render ends the job after the current
 * batch: img then holds the last complete pass, which is VALID — the mean of each pixel's first samples_done samples (its count, if
 * adaptive) — and its PNGs are written; rtu_render_wait returns RTU_ERR_CANCELLED (no PNG if no pass had completed). */
typedef void (*RtuPassDone)(void* user, int samples_done, int pass);
RtuRenderJob* rtu_begin_render_progressive(const RtuScene* scene, RtuImage* img, const int* device_ids, int n_devices,
                                           int samples, int gather_bounces, const RtuAdaptiveDesc* adaptive,
                                           const int* pass_samples, int n_passes,
                                           RtuPassDone on_pass, void* user,
                                           const char* result_png, const char* zbuffer_png, const char* samplecount_png);
void      rtu_stop_render(RtuRenderJob* job);      /* cooperative cancel between bands (a relaxed atomic store: any thread) */
int       rtu_render_wait(RtuRenderJob* job);      /* join; 0 or negative error code */
/* After the job (joins): how the shards reached the host — 1 one context; 2 several contexts, asynchronous copies into one
 * pinned buffer, all in flight together; 3 RCCL (grouped ncclSend / ncclRecv to the root GPU, then one copy). */
int       rtu_render_gather_kind(RtuRenderJob* job);
void      rtu_render_job_free(RtuRenderJob* job);

#ifdef __cplusplus
}
#endif
#endif /* RTU_HOST_H_INCLUDED */
