// rtu_features.h — launch interface of the first-hit feature kernels (rtu_features.hip), called by rtu_capi.hip.
#ifndef RTU_FEATURES_H_INCLUDED
#define RTU_FEATURES_H_INCLUDED

#include "rtu_device.h"
#include "rtu_vec.h"

// the camera of a frame as rtu_camera_rays reads it (RtuFrameDesc: cam_pos, origin, u, v, width, height)
struct FeatureCam {
    float pos[3], origin[3], u[3], v[3];
    int   width, height;
};

// The pixel-centre ray of pixel (x, y): primary_pixel's expressions (render_impl.h; RenderFunctions.cpp:258-268, :97), the ones
// rtu_camera_rays states on the host, in the same order: the same bits. a = {org, tmax}, b = {dir, 0}: the two float4 of an RtuRay.
RTU_HD void feature_cam_ray(const FeatureCam& c, int x, int y, float4& a, float4& b) {
    const f3 cam_pos = ld3(c.pos);
    const f3 cp = (ld3(c.origin) + ld3(c.u) * ((float)x + 0.5f)) + ld3(c.v) * ((float)y + 0.5f);
    const f3 dir = norm3(cp - cam_pos);
    a = make_float4(cam_pos.x, cam_pos.y, cam_pos.z, RTU_BIGFLOAT);
    b = make_float4(dir.x, dir.y, dir.z, 0.0f);
}

// rays: n RtuRay (two float4 each), hits: n RtuRayHit (three float4 each), albedo: n float4 {r, g, b, 0}. All pointers 16-byte
// aligned (checked by the caller). n == 0 launches nothing. Returns a hipError_t as int. Asynchronous on `stream`.
int rtu_launch_ray_features(const DevScene& s, const float4* rays, float4* hits, float4* albedo, unsigned long long n, bool reference_walk,
                            hipStream_t stream);
// ... the same for the pixel-centre rays of pixels [first, first + n) of `cam` in image order, generated in the kernel: answer i
// belongs to pixel first + i. The caller keeps first + n <= width * height.
int rtu_launch_frame_features(const DevScene& s, const FeatureCam& cam, unsigned long long first, unsigned long long n, float4* hits, float4* albedo,
                              hipStream_t stream);
// ... both with one more output, surface: n RtuRaySurface (two float4 each: {mesh, face, bc0, bc1}, {bc2, uvw}), 16-byte aligned. hits and
// albedo get the bytes of the two entries above.
int rtu_launch_ray_surface(const DevScene& s, const float4* rays, float4* hits, float4* albedo, float4* surface, unsigned long long n, bool reference_walk,
                           hipStream_t stream);
int rtu_launch_frame_surface(const DevScene& s, const FeatureCam& cam, unsigned long long first, unsigned long long n, float4* hits, float4* albedo,
                             float4* surface, hipStream_t stream);

#endif
