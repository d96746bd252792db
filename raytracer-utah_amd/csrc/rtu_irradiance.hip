// rtu_irradiance.hip — the irradiance map of include/rtu_render.h ("Irradiance map"): the pure host forms rtu_irradiance_grid,
// rtu_irradiance_rays, rtu_irradiance_classify and rtu_irradiance_sample, which are the executable statement of the rules, and the
// kernels of the build and the lookup. Both call the same functions of rtu_irradiance.h.
//
//   k_irr_classify        a lane per point the pass visits: the point can be estimated — its record becomes the average, its byte 0 — or
//                         it is flagged: weight 1 in the scratch of the allocation scan (rtu_steer.h), whose Wsum lane 0 sets to 1, so
//                         that k_steer_counts' count of a point IS its flag and the scan's offsets are list positions in visiting order.
//                         A pass reads earlier passes' points only and writes its own, so no lane reads what another writes.
//   k_irr_list            a lane per visited point: a flagged one writes its grid index at its offset
//   k_irr_store           a lane per listed point: its M values of c summed in order, divided by (float)M; z, N from its chain records
//   k_irr_sample          a lane per position: the lookup
//   k_irr_lookup_centres  a lane per pixel: E at the pixel's centre, the AmbientLight of the frame's root calls
//
// Every store is a vector store; there are no atomics and no inline assembly. Nothing is read or written beyond the grid, the list
// or n.
#include "rtu_irradiance.h"

#include "rtu_steer.h"

#include <string.h>
#include <vector>

namespace {

__global__ void __launch_bounds__(256) k_irr_classify(IrrPass q, IrrThresholds t, float4* __restrict__ rec, uint8_t* __restrict__ computed,
                                                      uint32_t* __restrict__ w_out, unsigned long long* __restrict__ wsum) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k == 0u) *wsum = 1ull;
    if (k >= q.count) return;
    uint32_t x, y, idx[4];
    irr_pass_point(q, k, x, y);
    float4 A, B;
    bool estimated = false;
    if (irr_neighbours(q, x, y, idx)) estimated = irr_estimate(t, rec, idx, A, B);
    if (estimated) {
        const size_t i = (size_t)y * q.gw + x;
        rec[2 * i] = A;
        rec[2 * i + 1] = B;
        computed[i] = 0;
    }
    w_out[k] = estimated ? 0u : 1u;
}

__global__ void __launch_bounds__(256) k_irr_list(IrrPass q, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                  uint32_t* __restrict__ list) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= q.count || counts[k] == 0u) return;
    uint32_t x, y;
    irr_pass_point(q, k, x, y);
    const uint32_t o = offsets[k];
    if (o < q.count) list[o] = y * q.gw + x;  // (an offset is below the number of flagged points: the test only guards the store)
}

__global__ void __launch_bounds__(256) k_irr_store(const uint32_t* __restrict__ list, uint32_t n_points, uint32_t samples, const float4* __restrict__ c,
                                                   const float4* __restrict__ gi_h, float4* __restrict__ rec, uint8_t* __restrict__ computed) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_points) return;
    const size_t n = (size_t)n_points * samples, i0 = (size_t)j * samples;
    float4 s = c[i0];
    for (uint32_t m = 1; m < samples; m++) {
        const float4 v = c[i0 + m];
        s.x += v.x; s.y += v.y; s.z += v.z;
    }
    const float fm = (float)samples;
    const float4 hA = gi_h[i0], hB = gi_h[n + i0];
    const size_t i = list[j];
    rec[2 * i] = make_float4(s.x / fm, s.y / fm, s.z / fm, hA.w);
    rec[2 * i + 1] = make_float4(hB.x, hB.y, hB.z, 0.0f);
    computed[i] = 1;
}

__global__ void __launch_bounds__(256) k_irr_sample(const float4* __restrict__ rec, IrrGrid g, const float* __restrict__ xy, size_t n, float4* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 A, B;
    irr_sample(rec, g.gw, g.gh, g.scale, xy[2 * i], xy[2 * i + 1], A, B);
    out[2 * i] = A;
    out[2 * i + 1] = B;
}

__global__ void __launch_bounds__(256) k_irr_lookup_centres(const float4* __restrict__ rec, IrrGrid g, uint32_t width, uint32_t height, float4* __restrict__ amb) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= width * height) return;
    const uint32_t y = p / width, x = p - y * width;
    float4 A, B;
    irr_sample(rec, g.gw, g.gh, g.scale, (float)x + 0.5f, (float)y + 0.5f, A, B);
    amb[p] = make_float4(A.x, A.y, A.z, 0.0f);
}

// what the allocation scan reads of its descriptor for a pass of `count` points with weights 0 / 1 and Wsum 1: the count of a point
// is min((budget * w + 0) / 1, max_extra) = w, the cut at budget = count never cuts
RtuSteerDesc irr_scan_desc(uint32_t count) {
    RtuSteerDesc d{};
    d.width = (int32_t)count;
    d.height = 1;
    d.budget = count;
    d.max_extra = 1;
    return d;
}

inline float4 ld4(const float* p, size_t i) { return make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]); }

}  // namespace

// the scratch of a pass: the allocation scan's own, then counts and offsets
size_t rtu_irr_scratch_words(size_t points) { return ((rtu_steer_scratch_words(points) + 3) / 4) * 4 + 2 * (((points + 3) / 4) * 4); }

int rtu_launch_irr_classify(const IrrPass& q, const IrrThresholds& t, float4* rec, uint8_t* computed, uint32_t* list, uint32_t* total, uint32_t* scratch,
                            hipStream_t stream) {
    if (q.count == 0u) return (int)hipMemsetAsync(total, 0, sizeof(uint32_t), stream);
    const StScratch s = st_scratch(scratch, q.count);
    const size_t base = ((rtu_steer_scratch_words(q.count) + 3) / 4) * 4, padded = (((size_t)q.count + 3) / 4) * 4;
    uint32_t* counts = scratch + base;
    uint32_t* offsets = counts + padded;
    const hipError_t e = hipMemsetAsync(scratch, 0, 16, stream);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((q.count + 255u) / 256u);
    hipLaunchKernelGGL(k_irr_classify, grid, dim3(256), 0, stream, q, t, rec, computed, s.w, s.wsum);
    const int rc = rtu_launch_allocation_scan(irr_scan_desc(q.count), s, counts, offsets, total, stream);
    if (rc != (int)hipSuccess) return rc;
    hipLaunchKernelGGL(k_irr_list, grid, dim3(256), 0, stream, q, counts, offsets, list);
    return (int)hipGetLastError();
}

int rtu_launch_irr_store(const uint32_t* list, uint32_t n_points, uint32_t samples, const float4* c, const float4* gi_h, float4* rec, uint8_t* computed,
                         hipStream_t stream) {
    if (n_points == 0u || samples == 0u) return (int)hipSuccess;
    hipLaunchKernelGGL(k_irr_store, dim3((n_points + 255u) / 256u), dim3(256), 0, stream, list, n_points, samples, c, gi_h, rec, computed);
    return (int)hipGetLastError();
}

int rtu_launch_irr_sample(const float4* rec, const IrrGrid& g, const float* xy, size_t n, float4* out, hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_irr_sample, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, rec, g, xy, n, out);
    return (int)hipGetLastError();
}

int rtu_launch_irr_lookup_centres(const float4* rec, const IrrGrid& g, uint32_t width, uint32_t height, float4* amb, hipStream_t stream) {
    if (width == 0u || height == 0u) return (int)hipSuccess;
    hipLaunchKernelGGL(k_irr_lookup_centres, dim3((width * height + 255u) / 256u), dim3(256), 0, stream, rec, g, width, height, amb);
    return (int)hipGetLastError();
}

int rtu_irradiance_check(const RtuIrradianceDesc* d, int width, int height, IrrGrid* g) {
    if (!d || width < 1 || height < 1 || width > 65536 || height > 65536) return RTU_ERR_ARG;
    if (d->min_subdiv > d->max_subdiv || d->min_subdiv < -15) return RTU_ERR_ARG;
    if (d->max_subdiv > 0) return RTU_ERR_UNSUPPORTED;  // several points per pixel
    if (d->samples < 1 || d->samples > 4096 || d->first_sample < 0) return RTU_ERR_ARG;
    if (d->max_bounce < 0 || d->max_bounce > RTU_MAX_BOUNCE) return RTU_ERR_ARG;
    const float th[5] = {d->threshold_color[0], d->threshold_color[1], d->threshold_color[2], d->threshold_z, d->threshold_n};
    for (float v : th)
        if (v != v) return RTU_ERR_ARG;
    for (uint32_t r : d->reserved)
        if (r) return RTU_ERR_ARG;
    const uint32_t s = 1u << (uint32_t)(-d->max_subdiv);
    if (((uint32_t)width & (s - 1u)) || ((uint32_t)height & (s - 1u))) return RTU_ERR_ARG;
    IrrGrid r;
    r.gw = (uint32_t)width / s + 1u;
    r.gh = (uint32_t)height / s + 1u;
    r.scale = s;
    r.levels = (uint32_t)(d->max_subdiv - d->min_subdiv);
    if ((unsigned long long)r.gw * r.gh > (1ull << 26)) return RTU_ERR_ARG;
    if (g) *g = r;
    return RTU_OK;
}

extern "C" {

static_assert(sizeof(RtuIrradianceDesc) == 64, "RtuIrradianceDesc is 64 bytes");
static_assert(sizeof(RtuIrradianceMap) == 32, "RtuIrradianceMap is 32 bytes");

int rtu_irradiance_defaults(RtuIrradianceDesc* out) {
    if (!out) return RTU_ERR_ARG;
    *out = RtuIrradianceDesc{};
    out->min_subdiv = -5;
    out->max_subdiv = 0;
    out->samples = 64;
    out->threshold_color[0] = out->threshold_color[1] = out->threshold_color[2] = 1.0e30f;
    out->threshold_z = 1.0e30f;
    out->threshold_n = 0.7f;
    out->max_bounce = RTU_MAX_BOUNCE;
    return RTU_OK;
}

int rtu_irradiance_grid(const RtuIrradianceDesc* desc, int width, int height, int* grid_w, int* grid_h, int* passes) {
    IrrGrid g;
    const int rc = rtu_irradiance_check(desc, width, height, &g);
    if (rc != RTU_OK) return rc;
    if (grid_w) *grid_w = (int)g.gw;
    if (grid_h) *grid_h = (int)g.gh;
    if (passes) *passes = 1 + 2 * (int)g.levels;
    return RTU_OK;
}

int rtu_irradiance_rays(const RtuFrameDesc* frame, const RtuIrradianceDesc* desc, RtuRay* rays_out) {
    if (!frame || !rays_out) return RTU_ERR_ARG;
    IrrGrid g;
    const int rc = rtu_irradiance_check(desc, frame->width, frame->height, &g);
    if (rc != RTU_OK) return rc;
    IrrCam c;
    memcpy(c.cam_pos, frame->cam_pos, sizeof c.cam_pos);
    memcpy(c.origin, frame->origin, sizeof c.origin);
    memcpy(c.u, frame->u, sizeof c.u);
    memcpy(c.v, frame->v, sizeof c.v);
    c.scale = (float)g.scale;
    c.gw = g.gw;
    for (uint32_t i = 0; i < g.gw * g.gh; i++) {
        f3 org, dir;
        irr_point_ray(c, i, org, dir);
        RtuRay& r = rays_out[i];
        r.org[0] = org.x; r.org[1] = org.y; r.org[2] = org.z;
        r.tmax = RTU_BIGFLOAT;
        r.dir[0] = dir.x; r.dir[1] = dir.y; r.dir[2] = dir.z;
        r.reserved = 0;
    }
    return RTU_OK;
}

int rtu_irradiance_classify(const RtuIrradianceDesc* desc, int width, int height, int pass, float* records, uint8_t* computed, uint32_t* visit_out,
                            uint8_t* compute_out, uint32_t* n_visit) {
    IrrGrid g;
    const int rc = rtu_irradiance_check(desc, width, height, &g);
    if (rc != RTU_OK) return rc;
    if (pass < 0 || pass > 2 * (int)g.levels || !records || !computed || !visit_out || !compute_out || !n_visit) return RTU_ERR_ARG;
    const IrrPass q = irr_pass(g, (uint32_t)pass);
    IrrThresholds t;
    memcpy(t.color, desc->threshold_color, sizeof t.color);
    t.z = desc->threshold_z;
    t.n = desc->threshold_n;
    // (a pass reads earlier passes' points only, so estimating in place reads nothing this pass wrote)
    std::vector<float4> rec((size_t)g.gw * g.gh * 2);
    for (size_t i = 0; i < rec.size(); i++) rec[i] = ld4(records, i);
    for (uint32_t k = 0; k < q.count; k++) {
        uint32_t x, y, idx[4];
        irr_pass_point(q, k, x, y);
        const size_t i = (size_t)y * g.gw + x;
        float4 A, B;
        bool estimated = false;
        if (irr_neighbours(q, x, y, idx)) estimated = irr_estimate(t, rec.data(), idx, A, B);
        if (estimated) {
            const float v[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
            memcpy(records + 8 * i, v, sizeof v);
            computed[i] = 0;
        }
        visit_out[k] = (uint32_t)i;
        compute_out[k] = estimated ? 0 : 1;
    }
    *n_visit = q.count;
    return RTU_OK;
}

int rtu_irradiance_sample(const RtuIrradianceMap* map, const float* xy, size_t n, float* out) {
    if (!map || map->reserved || map->reserved_ptr || map->max_subdiv > 0 || map->max_subdiv < -15) return RTU_ERR_ARG;
    RtuIrradianceDesc d;
    rtu_irradiance_defaults(&d);
    d.min_subdiv = d.max_subdiv = map->max_subdiv;
    IrrGrid g;
    const int rc = rtu_irradiance_check(&d, map->width, map->height, &g);
    if (rc != RTU_OK) return rc;
    if (n == 0) return RTU_OK;
    if (!map->records || !xy || !out) return RTU_ERR_ARG;
    const float* r = static_cast<const float*>(map->records);
    std::vector<float4> rec((size_t)g.gw * g.gh * 2);
    for (size_t i = 0; i < rec.size(); i++) rec[i] = ld4(r, i);
    for (size_t i = 0; i < n; i++) {
        float4 A, B;
        irr_sample(rec.data(), g.gw, g.gh, g.scale, xy[2 * i], xy[2 * i + 1], A, B);
        const float v[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
        memcpy(out + 8 * i, v, sizeof v);
    }
    return RTU_OK;
}

}  // extern "C"
