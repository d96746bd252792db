// rtu_features.hip — first-hit features (rtu_ray_features / rtu_frame_features, include/rtu_render.h): what a feature-guided filter
// needs of every pixel — the closest hit of rtu_trace_rays and the ALBEDO of the surface there.
//
//   k_features<REFWALK, CAM>   the query kernel's shape (rtu_query.hip: one ray per lane, 64-thread workgroups, the traversal stack in
//                              LDS, chunks of 64 rays strided over the grid), with trace<> instantiated with TEX so the hit carries
//                              hInfo.uvw, then TexturedColor::Sample of the hit material's diffuse colour (mtl_color<true>).
//                              CAM: ray i is the pixel-centre ray of pixel first + i of a frame, generated here (feature_cam_ray) — no ray
//                              buffer, no upload.
//
// ALBEDO is what MtlBlinn::Shade returns for the hit under one AmbientLight of intensity (1, 1, 1) with bounceCount 0
// (mtlFunctions.cpp:125-133): on a front face Color(0, 0, 0) + diffuse.Sample(hInfo.uvw) * intensity — the light loop's own two
// operations (direct_light, render_impl.h), so the bits of a recipe-W render of the all-ambient scene —, on a back face Color(0, 0, 0),
// white for a node without a material. A miss or an invalid ray: four zeros. The RtuRayHit is k_query_closest's, byte for
// byte: TEX only adds uvw to the sphere and plane tests.
//
//   k_features_surface<REFWALK, CAM>   the same statements with SURF: trace<> hands out the winning triangle (TriSurf, rtu_intersect.h), and a
//                              third output gets one RtuRaySurface per ray (two float4: {mesh, face, bc0, bc1}, {bc2, uvw}) —
//                              rtu_ray_surface / rtu_frame_surface. hits and albedo: the bytes of k_features (the walk and every
//                              expression that feeds them are the same; SURF only copies the winner out at the finish of a mesh walk).
// Reads the scene only; no frame state, no allocation, any stream.
#include "rtu_intersect.h"
#include "rtu_features.h"
#include "rtu_query.h"

namespace {

// three wavefronts per SIMD, as the queries (RTU_OCC_QUERY, rtu_query.hip): the 12 KB LDS stack allows 13 workgroups per CU
#define RTU_OCC_FEATURES __attribute__((amdgpu_waves_per_eu(3, 3)))

template <bool REFWALK, bool SURF>
__device__ __forceinline__ bool features_trace(const DevScene& s, const float4& a, const float4& b, Hit& h, uint32_t* stk, TriSurf* surf) {
    Ray ray;
    ray.p = mk3(a.x, a.y, a.z);
    ray.dir = mk3(b.x, b.y, b.z);  // as given: not renormalised
    fresh_hit(h, a.w);
    h.uvw = mk3(0, 0, 0);
    Counters cnt = {};
    bool deferred;
    if (REFWALK)
        return trace<RTU_MAX_BVH_STACK, true, false, false, false, true, false, false, false, false, SURF>(s, ray, false, h, stk, cnt, deferred, 64, nullptr, 0,
                                                                                                            false, -1, surf);
    return trace<RTU_MAX_BVH_STACK, false, true, false, false, true, false, false, false, true, SURF>(s, ray, false, h, stk, cnt, deferred, 64, nullptr, 0, false,
                                                                                                       -1, surf);  // FAR: any origin
}

// k_features with the surface record: the same statements in the same order, and what SURF adds. (k_features keeps its own text: as a
// shared function with SURF off the body compiled to two SGPR spills fewer / more than before in two of its instantiations, and the
// rule for this kernel's neighbours is that their code does not move.)
template <bool REFWALK, bool CAM>
__device__ __forceinline__ void surface_body(const DevScene& s, const FeatureCam& cam, const float4* __restrict__ rays, float4* __restrict__ hits,
                                              float4* __restrict__ albedo, float4* __restrict__ surface, unsigned long long first, unsigned long long n,
                                              uint32_t* s_stack) {
    const uint32_t lane = threadIdx.x;
    const unsigned long long chunks = (n + 63ull) / 64ull;
    for (unsigned long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const unsigned long long i = c * 64ull + lane;
        if (i >= n) continue;
        float4 a, b;
        if (CAM) feature_cam_ray(cam, (int)((first + i) % (unsigned long long)cam.width), (int)((first + i) / (unsigned long long)cam.width), a, b);
        else { a = rays[2 * i]; b = rays[2 * i + 1]; }
        Hit h;
        fresh_hit(h, a.w);
        uint32_t flags = RTU_RAY_INVALID;
        int material = -1;
        f3 alb = mk3(0, 0, 0);
        TriSurf win;
        win.face = 0;
        win.bc = mk3(0, 0, 0);
        int mesh = -1;
        f3 uvw = mk3(0, 0, 0);
        if (ray_valid(a, b)) {
            const bool hit = features_trace<REFWALK, true>(s, a, b, h, s_stack + lane, &win);
            flags = (hit ? RTU_RAY_HIT : 0u) | (hit && h.front ? RTU_RAY_FRONT : 0u);
            if (hit) {
                material = s.nodes[h.node].material_id;  // per-lane node: an ordinary load
                if (material < 0) alb = mk3(1.0f, 1.0f, 1.0f);  // null material => white, whatever the face
                else if (h.front)  // result += diffuse.Sample(uvw) * intensity, mtlFunctions.cpp:132
                    alb = mk3(0, 0, 0) + mtl_color<true>(s, material, RTU_MAP_DIFFUSE, ld3(s.materials[material].diffuse), h.uvw) * mk3(1.0f, 1.0f, 1.0f);
                uvw = h.uvw;
                if (s.nodes[h.node].obj_type == RTU_OBJ_TRIMESH) mesh = s.nodes[h.node].mesh_id;  // else `win` is of a mesh hit that lost
            } else { h.node = -1; h.p = mk3(0, 0, 0); h.N = mk3(0, 0, 0); }
        }
        hits[3 * i] = make_float4(h.z, __int_as_float(h.node), __uint_as_float(flags), __int_as_float(material));
        hits[3 * i + 1] = make_float4(h.p.x, h.p.y, h.p.z, 0.0f);
        hits[3 * i + 2] = make_float4(h.N.x, h.N.y, h.N.z, 0.0f);
        albedo[i] = make_float4(alb.x, alb.y, alb.z, 0.0f);
        const bool tri = mesh >= 0;
        surface[2 * i] = make_float4(__int_as_float(mesh), __int_as_float(tri ? (int)win.face : -1), tri ? win.bc.x : 0.0f, tri ? win.bc.y : 0.0f);
        surface[2 * i + 1] = make_float4(tri ? win.bc.z : 0.0f, uvw.x, uvw.y, uvw.z);
    }
}

template <bool REFWALK, bool CAM>
__global__ void __launch_bounds__(64) RTU_OCC_FEATURES k_features(DevScene s, FeatureCam cam, const float4* __restrict__ rays, float4* __restrict__ hits,
                                                                  float4* __restrict__ albedo, unsigned long long first, unsigned long long n) {
    __shared__ uint32_t s_stack[RTU_MAX_BVH_STACK * 64];
    const uint32_t lane = threadIdx.x;
    const unsigned long long chunks = (n + 63ull) / 64ull;
    for (unsigned long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const unsigned long long i = c * 64ull + lane;
        if (i >= n) continue;
        float4 a, b;
        if (CAM) feature_cam_ray(cam, (int)((first + i) % (unsigned long long)cam.width), (int)((first + i) / (unsigned long long)cam.width), a, b);
        else { a = rays[2 * i]; b = rays[2 * i + 1]; }
        Hit h;
        fresh_hit(h, a.w);
        uint32_t flags = RTU_RAY_INVALID;
        int material = -1;
        f3 alb = mk3(0, 0, 0);
        if (ray_valid(a, b)) {
            const bool hit = features_trace<REFWALK, false>(s, a, b, h, s_stack + lane, nullptr);
            flags = (hit ? RTU_RAY_HIT : 0u) | (hit && h.front ? RTU_RAY_FRONT : 0u);
            if (hit) {
                material = s.nodes[h.node].material_id;  // per-lane node: an ordinary load
                if (material < 0) alb = mk3(1.0f, 1.0f, 1.0f);  // null material => white, whatever the face
                else if (h.front)  // result += diffuse.Sample(uvw) * intensity, mtlFunctions.cpp:132
                    alb = mk3(0, 0, 0) + mtl_color<true>(s, material, RTU_MAP_DIFFUSE, ld3(s.materials[material].diffuse), h.uvw) * mk3(1.0f, 1.0f, 1.0f);
            } else { h.node = -1; h.p = mk3(0, 0, 0); h.N = mk3(0, 0, 0); }
        }
        hits[3 * i] = make_float4(h.z, __int_as_float(h.node), __uint_as_float(flags), __int_as_float(material));
        hits[3 * i + 1] = make_float4(h.p.x, h.p.y, h.p.z, 0.0f);
        hits[3 * i + 2] = make_float4(h.N.x, h.N.y, h.N.z, 0.0f);
        albedo[i] = make_float4(alb.x, alb.y, alb.z, 0.0f);
    }
}

template <bool REFWALK, bool CAM>
__global__ void __launch_bounds__(64) RTU_OCC_FEATURES k_features_surface(DevScene s, FeatureCam cam, const float4* __restrict__ rays,
                                                                          float4* __restrict__ hits, float4* __restrict__ albedo,
                                                                          float4* __restrict__ surface, unsigned long long first, unsigned long long n) {
    __shared__ uint32_t s_stack[RTU_MAX_BVH_STACK * 64];
    surface_body<REFWALK, CAM>(s, cam, rays, hits, albedo, surface, first, n, s_stack);
}

// enough workgroups to fill every CU several times over (13 fit per CU); longer batches stride (query_grid, rtu_query.hip)
uint32_t features_grid(unsigned long long n) {
    const unsigned long long chunks = (n + 63ull) / 64ull;
    return (uint32_t)(chunks < 8192ull ? chunks : 8192ull);
}

}  // namespace

int rtu_launch_ray_features(const DevScene& s, const float4* rays, float4* hits, float4* albedo, unsigned long long n, bool reference_walk,
                            hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    const FeatureCam none = {};
    if (reference_walk) hipLaunchKernelGGL((k_features<true, false>), dim3(features_grid(n)), dim3(64), 0, stream, s, none, rays, hits, albedo, 0ull, n);
    else hipLaunchKernelGGL((k_features<false, false>), dim3(features_grid(n)), dim3(64), 0, stream, s, none, rays, hits, albedo, 0ull, n);
    return (int)hipGetLastError();
}

int rtu_launch_frame_features(const DevScene& s, const FeatureCam& cam, unsigned long long first, unsigned long long n, float4* hits, float4* albedo,
                              hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    hipLaunchKernelGGL((k_features<false, true>), dim3(features_grid(n)), dim3(64), 0, stream, s, cam, (const float4*)nullptr, hits, albedo, first, n);
    return (int)hipGetLastError();
}

int rtu_launch_ray_surface(const DevScene& s, const float4* rays, float4* hits, float4* albedo, float4* surface, unsigned long long n, bool reference_walk,
                           hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    const FeatureCam none = {};
    if (reference_walk)
        hipLaunchKernelGGL((k_features_surface<true, false>), dim3(features_grid(n)), dim3(64), 0, stream, s, none, rays, hits, albedo, surface, 0ull, n);
    else hipLaunchKernelGGL((k_features_surface<false, false>), dim3(features_grid(n)), dim3(64), 0, stream, s, none, rays, hits, albedo, surface, 0ull, n);
    return (int)hipGetLastError();
}

int rtu_launch_frame_surface(const DevScene& s, const FeatureCam& cam, unsigned long long first, unsigned long long n, float4* hits, float4* albedo,
                             float4* surface, hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    hipLaunchKernelGGL((k_features_surface<false, true>), dim3(features_grid(n)), dim3(64), 0, stream, s, cam, (const float4*)nullptr, hits, albedo, surface,
                       first, n);
    return (int)hipGetLastError();
}
