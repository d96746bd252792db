// rtu_camrays.h — the ray and key of one sample of one pixel of a recipe-S frame (include/rtu_render.h, rtu_camera_sample_rays) for
// host and device, and the launch interface of its kernel (rtu_camrays.hip), called by rtu_capi.hip.
#ifndef RTU_CAMRAYS_H_INCLUDED
#define RTU_CAMRAYS_H_INCLUDED

#include "rtu_render.h"
#include "rtu_vec.h"

#include <stddef.h>
#include <stdint.h>

// the sample streams (rtu_intersect.h mix32 / rand31 / sample_key) for host and device: integer arithmetic, the same words
RTU_HD uint32_t cs_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
RTU_HD uint32_t cs_rand31(uint32_t key, uint32_t purpose) { return cs_mix32(key ^ cs_mix32(purpose * 0x9e3779b9U + 0x85ebca6bU)) >> 1; }
RTU_HD uint32_t cs_sample_key(uint32_t pixel, uint32_t sample) { return cs_mix32(cs_mix32(pixel + 0x68bc21ebU) ^ (sample * 0x9e3779b9U + 1U)); }

// what a sample of a frame needs of its RtuFrameDesc, and the pixel offsets of the sample (made on the host: launch()'s expressions)
struct CamSample {
    float    cam_pos[3], origin[3], u[3], v[3], lens_up[3], lens_right[3];
    float    dof, ox, oy;
    int32_t  width, height;
    uint32_t sample;
};

// The ray and key of pixel (x, y): primary_pixel's recipe-S branch (render_impl.h; RenderFunctions.cpp:80-97, :258-268), the same
// binary32 expressions in the same order. sc(t, sn, cs) is portable_sincos (rtu_intersect.h) on the device and its host restatement in
// rtu_capi.hip, as for sensor_ray (rtu_sensor.h). The translation units that include this are compiled with -ffp-contract=off and IEEE
// divide / sqrt.
template <class SinCos>
RTU_HD void camera_sample_ray(const CamSample& c, int x, int y, SinCos sc, f3& org, f3& dir, uint32_t& key) {
    key = cs_sample_key((uint32_t)x + (uint32_t)c.width * (uint32_t)y, c.sample);
    const float sampleX = (float)cs_rand31(key, 0u) / 2147483648.0f;                                              // :88 (RTU_RAND_MAX_F)
    const float sampleTheta = (float)cs_rand31(key, 1u) / ((float)(2147483647 / (2 * 3.14159265358979323846)));  // :89 (RTU_THETA_DIV)
    float sn, cs;
    sc(sampleTheta, sn, cs);
    const float rad = sqrtf((sampleX * c.dof) * c.dof);
    const float camOffsetX = rad * cs, camOffsetY = rad * sn;                                                     // :90-91
    org = (ld3(c.cam_pos) + ld3(c.lens_up) * camOffsetY) + ld3(c.lens_right) * camOffsetX;                        // :93
    const f3 cp = (ld3(c.origin) + ld3(c.u) * ((float)x + c.ox)) + ld3(c.v) * ((float)y + c.oy);
    dir = norm3(cp - org);
}

// rays[2 * p ..] and keys[p] for every pixel p of the frame, image order: the bits of rtu_camera_sample_rays. rays 16-byte aligned.
// Asynchronous on `stream`; returns a hipError_t as int.
int rtu_launch_camera_sample_rays(const CamSample& c, float4* rays, uint32_t* keys, hipStream_t stream);

#endif
