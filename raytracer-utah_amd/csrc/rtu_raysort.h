// rtu_raysort.h — the sort key of a ray (include/rtu_render.h, "Ray sorting") for host and device, and the launch interface of the
// sorter and the permutation kernels (rtu_raysort.hip), called by rtu_capi.hip.
#ifndef RTU_RAYSORT_H_INCLUDED
#define RTU_RAYSORT_H_INCLUDED

#include "rtu_vec.h"

#include <stddef.h>
#include <stdint.h>

#define RTU_SORTKEY_INVALID 0xFFFFFFFFu  // a ray the queries do not trace (ray_valid)
#define RTU_SORTKEY_MISS    0x40000000u  // a valid ray whose segment [0, tmax] misses the box: this bit | the 18 direction bits

// the box of the keys: lo[3], hi[3], and whether cells can be told apart in it — every bound finite, hi >= lo and hi - lo finite on
// every axis. In a degenerate box every spatial cell is 0 and no ray misses.
struct SortBox {
    float lo[3], hi[3];
    int   ok;
};

RTU_HD bool sortbox_fin(float x) { return x - x == 0.0f; }  // false for NaN and the infinities
RTU_HD SortBox make_sortbox(const float* b) {
    SortBox s;
    s.ok = 1;
    for (int k = 0; k < 3; k++) {
        s.lo[k] = b[k];
        s.hi[k] = b[3 + k];
        if (!(sortbox_fin(b[k]) && sortbox_fin(b[3 + k]) && b[3 + k] >= b[k] && sortbox_fin(b[3 + k] - b[k]))) s.ok = 0;
    }
    return s;
}

// bits 0..3 of v to bits 0, 3, 6, 9; bits 0..8 of v to bits 0, 2, .. 16
RTU_HD uint32_t sort_spread3(uint32_t v) { return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6); }
RTU_HD uint32_t sort_spread2(uint32_t v) {
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

// The key of a VALID ray (the caller has applied ray_valid's rule: finite components, tmax > 0, |dir| = 1 within 2e-3). binary32, one
// rounding per operation, in the order written (rtu_render.h states the same expressions); + - * /, fabsf, floorf and comparisons only.
RTU_HD uint32_t ray_sort_key(const SortBox& bx, const float* org, float tmax, const float* dir) {
    uint32_t spatial = 0;
    bool miss = false;
    if (bx.ok) {
        float p[3] = {org[0], org[1], org[2]};
        const bool inside = org[0] >= bx.lo[0] && org[0] <= bx.hi[0] && org[1] >= bx.lo[1] && org[1] <= bx.hi[1] && org[2] >= bx.lo[2] &&
                            org[2] <= bx.hi[2];
        if (!inside) {
            float t0 = 0.0f, t1 = tmax;
            for (int k = 0; k < 3; k++) {
                if (dir[k] == 0.0f) {
                    if (org[k] < bx.lo[k] || org[k] > bx.hi[k]) miss = true;
                    continue;
                }
                const float ta = (bx.lo[k] - org[k]) / dir[k], tb = (bx.hi[k] - org[k]) / dir[k];
                const float tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
                if (tn > t0) t0 = tn;
                if (tf < t1) t1 = tf;
            }
            if (t0 > t1) miss = true;
            for (int k = 0; k < 3 && !miss; k++) {
                float q = org[k] + t0 * dir[k];
                if (!(q >= bx.lo[k])) q = bx.lo[k];  // (also a NaN, which inf * 0 cannot give here: dir[k] == 0 adds nothing to t0)
                if (q > bx.hi[k]) q = bx.hi[k];
                p[k] = q;
            }
        }
        uint32_t c[3] = {0, 0, 0};
        for (int k = 0; k < 3 && !miss; k++) {
            const float ext = bx.hi[k] - bx.lo[k];
            int cell = 0;
            if (ext > 0.0f) {
                cell = (int)floorf((p[k] - bx.lo[k]) / ext * 16.0f);
                if (cell > 15) cell = 15;
                if (cell < 0) cell = 0;
            }
            c[k] = (uint32_t)cell;
        }
        spatial = sort_spread3(c[0]) | (sort_spread3(c[1]) << 1) | (sort_spread3(c[2]) << 2);
    }
    // the octahedral map of dir: (u, v) in [0, 1]^2
    const float ax = fabsf(dir[0]), ay = fabsf(dir[1]), az = fabsf(dir[2]);
    const float s = (ax + ay) + az;
    float px = dir[0] / s, py = dir[1] / s;
    if (dir[2] < 0.0f) {
        const float fx = (1.0f - fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f);
        const float fy = (1.0f - fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
        px = fx;
        py = fy;
    }
    int qu = (int)floorf((px * 0.5f + 0.5f) * 512.0f), qv = (int)floorf((py * 0.5f + 0.5f) * 512.0f);
    if (qu > 511) qu = 511;
    if (qu < 0) qu = 0;
    if (qv > 511) qv = 511;
    if (qv < 0) qv = 0;
    const uint32_t directional = sort_spread2((uint32_t)qu) | (sort_spread2((uint32_t)qv) << 1);
    return miss ? RTU_SORTKEY_MISS | directional : (spatial << 18) | directional;
}

// ---- launch interface (rtu_raysort.hip). Every function is asynchronous on `stream` and returns a hipError_t as int. ----
// (both can be set from the command line, RTU_EXTRA of the Makefile: DESIGN.md 20 has the six geometries that were measured)
#ifndef RTU_SORT_BLOCK
#define RTU_SORT_BLOCK 1024u     // threads per workgroup of the histogram and scatter kernels, and
#endif
#ifndef RTU_SORT_ITEMS
#define RTU_SORT_ITEMS 4u        // pairs per thread: a workgroup takes a tile of
#endif
#define RTU_SORT_TILE (RTU_SORT_BLOCK * RTU_SORT_ITEMS)  // consecutive pairs
#define RTU_SORT_BINS 256u       // 8-bit digits: four passes over the 32-bit key
// uint32 words of scratch rtu_launch_ray_order needs for n rays: keys and indices double-buffered, the digit histograms
size_t rtu_ray_order_scratch_words(size_t n);
// order[0 .. n) = the stable argsort of the keys of rays[0 .. n) in `box`. rays 16-byte aligned, n >= 1.
int rtu_launch_ray_order(const SortBox& box, const float4* rays, size_t n, uint32_t* order, uint32_t* scratch, hipStream_t stream);
// scatter == 0: dst[i] = src[order[i]]; 1: dst[order[i]] = src[i]. elem_bytes 1, 4, 16, 32 or 48 (the caller has checked alignment).
int rtu_launch_permute(const void* src, void* dst, const uint32_t* order, size_t n, uint32_t elem_bytes, int scatter, hipStream_t stream);

#endif
