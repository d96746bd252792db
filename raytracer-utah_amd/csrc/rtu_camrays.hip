// rtu_camrays.hip — the rays and keys of one sample of a recipe-S pinhole / thin-lens frame, written where the shading kernels read
// them (rtu_camera_sample_rays_device, include/rtu_render.h): a new sample of a frame costs no upload.
//
//   k_camera_sample_rays  one lane per pixel: camera_sample_ray of rtu_camrays.h (the bits of rtu_camera_sample_rays) as two float4
//                         stores, and the key as one dword store. The camera and the offsets of the sample are kernel arguments.
//
// Every store is a vector store; there is no inline assembly.
#include "rtu_camrays.h"

#include "rtu_intersect.h"

namespace {

struct DevSinCos {
    __device__ __forceinline__ void operator()(float t, float& sn, float& cs) const { portable_sincos(t, sn, cs); }
};

__global__ void __launch_bounds__(256) k_camera_sample_rays(CamSample c, float4* __restrict__ rays, uint32_t* __restrict__ keys) {
    const uint32_t pixels = (uint32_t)c.width * (uint32_t)c.height;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= pixels) return;
    const uint32_t y = p / (uint32_t)c.width, x = p - y * (uint32_t)c.width;
    f3 org, dir;
    uint32_t key;
    camera_sample_ray(c, (int)x, (int)y, DevSinCos(), org, dir, key);
    rays[2 * (size_t)p] = make_float4(org.x, org.y, org.z, RTU_BIGFLOAT);
    rays[2 * (size_t)p + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(0u));
    keys[p] = key;
}

}  // namespace

int rtu_launch_camera_sample_rays(const CamSample& c, float4* rays, uint32_t* keys, hipStream_t stream) {
    const uint32_t pixels = (uint32_t)c.width * (uint32_t)c.height;
    if (pixels == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_camera_sample_rays, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, c, rays, keys);
    return (int)hipGetLastError();
}
