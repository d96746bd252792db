// rtu_sensor.hip — sensors (include/rtu_render.h, "Sensors"): the rays and keys of a panoramic, fisheye or orthographic
// sensor written where the shading kernels read them, and the sums and the mean of the samples that come back.
//
//   k_sensor_rays<MODEL>  one lane per (sample, pixel): the ray of rtu_sensor.h's sensor_ray (the bits of rtu_sensor_rays) as two float4
//                         stores, and the key as one dword store. blockIdx.y is the sample of the launch, so its offsets and index are
//                         wave-uniform (scalar loads from the kernel arguments); the model is a template parameter: no lane branches on it.
//   k_sensor_accumulate   one lane per pixel: the samples of a batch added in sample order, no atomics; the resolve of the frame
//                         path (render_kernel.hip resolve_mean, restated here) fused into the last batch.
//
// Every store is a vector store; there is no inline assembly.
#include "rtu_sensor.h"

#include "rtu_intersect.h"

namespace {

struct DevSinCos {
    __device__ __forceinline__ void operator()(float t, float& sn, float& cs) const { portable_sincos(t, sn, cs); }
};

template <int MODEL>
__global__ void __launch_bounds__(256) k_sensor_rays(RtuSensorDesc d, SensorOffsets off, float4* __restrict__ rays, uint32_t* __restrict__ keys) {
    const uint32_t pixels = (uint32_t)d.width * (uint32_t)d.height;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= pixels) return;
    const uint32_t s = blockIdx.y;
    const uint32_t y = p / (uint32_t)d.width, x = p - y * (uint32_t)d.width;
    f3 org, dir;
    sensor_ray<MODEL>(d, (int)x, (int)y, off.ox[s], off.oy[s], DevSinCos(), org, dir);
    const size_t i = (size_t)s * pixels + p;
    rays[2 * i] = make_float4(org.x, org.y, org.z, RTU_BIGFLOAT);
    rays[2 * i + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(0u));
    if (keys) keys[i] = sample_key(p, off.sample[s]);
}

// the mean of a pixel's sums over n samples of which `hits` hit: resolve_mean of render_kernel.hip, the same binary32 divisions
__device__ __forceinline__ float4 sensor_mean(const float4& s, uint32_t hits, float n) {
    return make_float4(s.x / n, s.y / n, s.z / n, hits ? s.w / (float)hits : RTU_BIGFLOAT);
}

__global__ void __launch_bounds__(256) k_sensor_accumulate(const float4* __restrict__ samples, uint32_t batch, float4* __restrict__ acc,
                                                           uint32_t* __restrict__ hits, uint32_t pixels, int first, float4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t h = 0;
    if (!first) { s = acc[i]; h = hits[i]; }
    for (uint32_t b = 0; b < batch; b++) {  // the samples of the batch in their order
        const float4 v = samples[(size_t)b * pixels + i];
        s.x += v.x; s.y += v.y; s.z += v.z;
        if (v.w != RTU_BIGFLOAT && v.w != 0.0f) { s.w += v.w; h++; }  // a miss answers tmax, a sample outside the fisheye circle 0
    }
    if (out) {
        out[i] = sensor_mean(s, h, (float)n);
    } else {
        acc[i] = s;
        hits[i] = h;
    }
}

}  // namespace

int rtu_launch_sensor_rays(const RtuSensorDesc& d, const SensorOffsets& off, uint32_t n_samples, float4* rays, uint32_t* keys, hipStream_t stream) {
    const uint32_t pixels = (uint32_t)d.width * (uint32_t)d.height;
    if (pixels == 0 || n_samples == 0) return (int)hipSuccess;
    const dim3 grid((pixels + 255u) / 256u, n_samples), block(256);
    switch (d.model) {
    case RTU_SENSOR_EQUIRECT: hipLaunchKernelGGL(k_sensor_rays<RTU_SENSOR_EQUIRECT>, grid, block, 0, stream, d, off, rays, keys); break;
    case RTU_SENSOR_FISHEYE: hipLaunchKernelGGL(k_sensor_rays<RTU_SENSOR_FISHEYE>, grid, block, 0, stream, d, off, rays, keys); break;
    default: hipLaunchKernelGGL(k_sensor_rays<RTU_SENSOR_ORTHO>, grid, block, 0, stream, d, off, rays, keys); break;
    }
    return (int)hipGetLastError();
}

int rtu_launch_sensor_accumulate(const float4* samples, uint32_t batch, float4* acc, uint32_t* hits, uint32_t pixels, bool first, float4* out,
                                 uint32_t n, hipStream_t stream) {
    if (pixels == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_sensor_accumulate, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, samples, batch, acc, hits, pixels, first ? 1 : 0, out, n);
    return (int)hipGetLastError();
}
