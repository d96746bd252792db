// rtu_sensor.h — the ray of a sensor pixel (include/rtu_render.h, "Sensors") for host and device, and the launch interface of the
// generator and accumulator kernels (rtu_sensor.hip), called by rtu_capi_sensor.hip.
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

// ---- the projection of a sensor (include/rtu_render.h, "Temporal accumulation for sensors"): the counterpart of sensor_ray ----------
// acos of a float in [-1, 1]: binary64 IEEE operations in fdlibm's e_acos sequence, rounded to float — the sequence of portable_acos
// (rtu_intersect.h, device only: the render kernels' copy stays where it is) and of the oracle, for host and device.
RTU_HD double sensor_acos_poly(double z) {
    const double p = z * (1.66666666666666657415e-01 + z * (-3.25565818622400915405e-01 + z * (2.01212532134862925881e-01 +
                     z * (-4.00555345006794114027e-02 + z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))));
    const double q = 1.0 + z * (-2.40339491173441421878e+00 + z * (2.02094576023350569471e+00 + z * (-6.88283971605453293030e-01 + z * 7.70381505559019352791e-02)));
    return p / q;
}
RTU_HD float sensor_acos(float xf) {
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    const double x = (double)xf;
    const double ax = fabs(x);
    double r;
    if (ax >= 1.0) r = x > 0 ? 0.0 : pi;
    else if (ax < 0.5) r = pio2_hi - (x - (pio2_lo - x * sensor_acos_poly(x * x)));
    else if (x < 0) {
        const double z = (1.0 + x) * 0.5, s = sqrt(z);
        r = pi - 2.0 * (s + (sensor_acos_poly(z) * s - pio2_lo));
    } else {
        const double z = (1.0 - x) * 0.5, s = sqrt(z);
        r = 2.0 * (s + sensor_acos_poly(z) * s);
    }
    return (float)r;
}

// The angle in [0, pi] between the direction (s, k), s >= 0, and the axis k: false unless its length is finite and > 0. acos gets the
// smaller of the two ratios — at most about 0.71 —, where it is well conditioned in binary32.
RTU_HD bool sensor_angle(float s, float k, float& ang) {
    const float L = sqrtf(s * s + k * k);
    if (!((L - L) == 0.0f && L > 0.0f)) return false;
    if (fabsf(k) <= s) {
        ang = sensor_acos(k / L);
    } else {
        const float q = sensor_acos(s / L);
        ang = k > 0.0f ? 1.5707964f - q : 1.5707964f + q;
    }
    return true;
}

// The image coordinates (fx, fy) of world point Pm in sensor `d` (validated by the caller), model MODEL — pixel (x, y) has its centre
// at (x, y) — or false: the point has none. binary32, one rounding per operation, in the order rtu_render.h states.
template <int MODEL>
RTU_HD bool sensor_project(const RtuSensorDesc& d, const f3& Pm, float& fx, float& fy) {
    const f3 Q = Pm - ld3(d.pos);
    const float a = dot3(Q, ld3(d.forward)), b = dot3(Q, ld3(d.right)), c = dot3(Q, ld3(d.up));
    const float W = (float)d.width, H = (float)d.height;
    if (MODEL == RTU_SENSOR_EQUIRECT) {
        const float h = sqrtf(a * a + b * b);
        if (h == 0.0f) return false;  // a pole
        float pol, th;
        if (!sensor_angle(h, c, pol) || !sensor_angle(fabsf(b), -a, th)) return false;
        const float lon = b <= 0.0f ? th : 6.2831855f - th;
        fx = lon / 6.2831855f * W - 0.5f;
        fy = pol / 3.1415927f * H - 0.5f;
        return true;
    }
    if (MODEL == RTU_SENSOR_FISHEYE) {
        const float p = sqrtf(b * b + c * c);
        if (p == 0.0f) {
            fx = 0.5f * W - 0.5f;
            fy = 0.5f * H - 0.5f;
            return a > 0.0f;
        }
        float ang;
        if (!sensor_angle(p, a, ang)) return false;
        const float r = ang / (d.fov_deg * 0.008726646f);
        if (!(r <= 1.0f)) return false;
        const float R = 0.5f * (float)(d.width < d.height ? d.width : d.height);
        fx = ((r * (b / p)) * R + 0.5f * W) - 0.5f;
        fy = ((-(r * (c / p))) * R + 0.5f * H) - 0.5f;
        return true;
    }
    if (!(a > 0.0f)) return false;
    fx = (b / d.extent[0] + 0.5f) * W - 0.5f;
    fy = (0.5f - c / d.extent[1]) * H - 0.5f;
    return true;
}

// RTU_OK or RTU_ERR_ARG: the rules of RtuSensorDesc (rtu_capi_sensor.hip), without a context
extern "C" int rtu_sensor_check_desc(const RtuSensorDesc* d);

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
