// rtu_sensor.h — the ray of a sensor pixel (include/rtu_render.h, "Sensors") for host and device, and the launch interface of the
// generator and accumulator kernels (rtu_sensor.hip), called by rtu_capi.hip.
#ifndef RTU_SENSOR_H_INCLUDED
#define RTU_SENSOR_H_INCLUDED

#include "rtu_render.h"
#include "rtu_vec.h"

#include <stddef.h>
#include <stdint.h>

// The ray of pixel (x, y) at offsets (ox, oy) of sensor `d` (validated by the caller), model MODEL. binary32, one rounding per
// operation, in the order rtu_render.h states; sc(t, sn, cs) is portable_sincos (rtu_intersect.h) on the device and its host
// restatement in rtu_capi.hip: IEEE binary64 operations in the same sequence, so the same floats. The translation units that include
// this are compiled with -ffp-contract=off and IEEE divide / sqrt. A fisheye sample outside the image circle gets dir = 0.
template <int MODEL, class SinCos>
RTU_HD void sensor_ray(const RtuSensorDesc& d, int x, int y, float ox, float oy, SinCos sc, f3& org, f3& dir) {
    const f3 pos = ld3(d.pos), right = ld3(d.right), up = ld3(d.up), forward = ld3(d.forward);
    org = pos;
    if (MODEL == RTU_SENSOR_FISHEYE) {
        const float R = 0.5f * (float)(d.width < d.height ? d.width : d.height);
        const float dx = (((float)x + ox) - 0.5f * (float)d.width) / R, dy = (((float)y + oy) - 0.5f * (float)d.height) / R;
        const float r = sqrtf(dx * dx + dy * dy);
        if (r > 1.0f) {
            dir = mk3(0.0f, 0.0f, 0.0f);
        } else if (r == 0.0f) {
            dir = forward;
        } else {
            const float a = r * (d.fov_deg * 0.008726646f);
            float sa, ca;
            sc(a, sa, ca);
            dir = norm3(forward * ca + (right * (dx / r) + up * (-(dy / r))) * sa);
        }
        return;
    }
    float u = ((float)x + ox) / (float)d.width, v = ((float)y + oy) / (float)d.height;
    if (MODEL == RTU_SENSOR_EQUIRECT) {
        if (u >= 1.0f) u -= 1.0f;
        if (v > 1.0f) v = 1.0f;
        const float lon = u * 6.2831855f, pol = v * 3.1415927f;
        float sl, cl, sp, cp;
        sc(lon, sl, cl);
        sc(pol, sp, cp);
        const f3 h = forward * (-cl) + right * (-sl);
        dir = norm3(up * cp + h * sp);
    } else {
        org = (pos + right * ((u - 0.5f) * d.extent[0])) + up * ((0.5f - v) * d.extent[1]);
        dir = forward;
    }
}

// ---- launch interface (rtu_sensor.hip). Every function is asynchronous on `stream` and returns a hipError_t as int. ----
#define RTU_SENSOR_LAUNCH_SAMPLES 16  // samples per launch of k_sensor_rays: their pixel offsets travel in the kernel arguments
struct SensorOffsets {
    float    ox[RTU_SENSOR_LAUNCH_SAMPLES], oy[RTU_SENSOR_LAUNCH_SAMPLES];
    uint32_t sample[RTU_SENSOR_LAUNCH_SAMPLES];  // the sample index the keys are made of
};
// rays[(s * pixels + p) * 2 ..] and keys[s * pixels + p] (keys may be nullptr) for s < n_samples <= RTU_SENSOR_LAUNCH_SAMPLES and every
// pixel p of the sensor: the bits of rtu_sensor_rays. rays 16-byte aligned; d validated.
int rtu_launch_sensor_rays(const RtuSensorDesc& d, const SensorOffsets& off, uint32_t n_samples, float4* rays, uint32_t* keys, hipStream_t stream);
// Per pixel: the samples[b * pixels + p], b < batch, added in that order to acc / hits (first: the sums start at zero): rgb always, t
// and the hit count where the sample hit (t is neither RTU_BIGFLOAT nor 0). out != nullptr (the last batch): out[p] = the mean over n.
int rtu_launch_sensor_accumulate(const float4* samples, uint32_t batch, float4* acc, uint32_t* hits, uint32_t pixels, bool first, float4* out,
                                 uint32_t n, hipStream_t stream);

#endif
