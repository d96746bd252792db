// rtu_meshrec.h — what a mesh's device structures take from its VERTICES, shared by the host builders (rtu_capi_build.hip: build_tri_records
// at upload, the host restatement behind rtu_debug_host_mesh) and the device kernels of rtu_update_meshes (rtu_mesh_update.hip):
//   * the 64-byte triangle record of one face (TriRec, rtu_intersect.h);
//   * the box of one child slot of the collapsed fast trees (DevMesh::bvh4 / ::bvh8): of a leaf slot from the vertices of its
//     element slots, of an inner slot from the boxes of the node it refers to.
// Both sides run the same expressions with -ffp-contract=off and IEEE divide / sqrt, so both write the same bits. The boxes are
// comparisons only: the exact min / max of vertex coordinates, as build_sah stores them. Not included by the render kernels.
#pragma once
#include "rtu_vec.h"

#include <stdint.h>

#define RTU_MU_REF_EMPTY 0x0FFFFFFFu  // == RTU_REF8_EMPTY (rtu_device.h): an unused child slot

// The ray-independent part of TriObj::IntersectTriangle (objFunctions.cpp:259-300) for the triangle A, B, C, evaluated with the
// same float ops: four float4 of a TriRec.
RTU_HD void mu_tri_record(f3 A, f3 B, f3 C, float4* out) {
    f3 N = norm3(cross3(B - A, C - A));                                        // :263
    float anx = fabsf(N.x), any = fabsf(N.y), anz = fabsf(N.z);
    float maxNormalAxis = smax(smax(anx, any), anz);                           // :274
    uint32_t axis = (maxNormalAxis == anx) ? 0u : (maxNormalAxis == any) ? 1u : 2u;  // :278-296
    float ax = axis == 0 ? A.y : A.x, ay = axis == 2 ? A.y : A.z;
    float bx = axis == 0 ? B.y : B.x, by = axis == 2 ? B.y : B.z;
    float cx = axis == 0 ? C.y : C.x, cy = axis == 2 ? C.y : C.z;
    float e1x = cx - ax, e1y = cy - ay, e2x = bx - ax, e2y = by - ay;
    float TriABCArea = (float)((double)((-e1y) * e2x + e1x * e2y) / 2.0);      // :298, Point2::Cross
    double rcp = 1.0 / (double)TriABCArea;
    uint64_t bits;
    __builtin_memcpy(&bits, &rcp, 8);
    uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
    float flo, fhi, faxis;
    __builtin_memcpy(&flo, &lo, 4); __builtin_memcpy(&fhi, &hi, 4); __builtin_memcpy(&faxis, &axis, 4);
    out[0] = make_float4(A.x, A.y, A.z, N.x);
    out[1] = make_float4(N.y, N.z, ax, ay);
    out[2] = make_float4(e1x, e1y, e2x, e2y);
    out[3] = make_float4(flo, fhi, faxis, 0.0f);
}

// the record of element slot e: elements[e] names the face
RTU_HD void mu_slot_record(const uint32_t* f, const float* v, const uint32_t* elements, uint32_t e, float4* out) {
    const uint32_t* fv = f + 3 * (size_t)elements[e];
    mu_tri_record(ld3(v + 3 * (size_t)fv[0]), ld3(v + 3 * (size_t)fv[1]), ld3(v + 3 * (size_t)fv[2]), out);
}

// Where a child slot keeps its six box floats and its ref word, in floats from the start of its node.
//   4-wide: {min.x[4]} {min.y[4]} {min.z[4]} {max.x[4]} {max.y[4]} {max.z[4]} {ref[4]} {-}
//   8-wide: child c = {bmin.xyz, ref} {bmax.xyz, -}
template <int W> struct MuWide;
template <> struct MuWide<4> {
    static constexpr uint32_t kNodeFloats = 32;
    static RTU_HD uint32_t lo(uint32_t c, uint32_t k) { return 4 * k + c; }
    static RTU_HD uint32_t hi(uint32_t c, uint32_t k) { return 4 * (3 + k) + c; }
    static RTU_HD uint32_t ref(uint32_t c) { return 24 + c; }
};
template <> struct MuWide<8> {
    static constexpr uint32_t kNodeFloats = 64;
    static RTU_HD uint32_t lo(uint32_t c, uint32_t k) { return 8 * c + k; }
    static RTU_HD uint32_t hi(uint32_t c, uint32_t k) { return 8 * c + 4 + k; }
    static RTU_HD uint32_t ref(uint32_t c) { return 8 * c + 3; }
};

template <int W> RTU_HD uint32_t mu_ref(const float* tree, uint32_t node, uint32_t c) {
    uint32_t r;
    __builtin_memcpy(&r, tree + (size_t)node * MuWide<W>::kNodeFloats + MuWide<W>::ref(c), 4);
    return r;
}
RTU_HD bool mu_is_leaf(uint32_t ref) { return (ref >> 28) != 0u; }
RTU_HD bool mu_is_inner(uint32_t ref) { return (ref >> 28) == 0u && ref != RTU_MU_REF_EMPTY; }

// A leaf slot (ref = index | count << 28): min / max over the vertices of element slots [index, index + count) — per face the
// expressions of build_sah, then its strict comparisons from the same start values.
template <int W>
RTU_HD void mu_leaf_slot(float* tree, uint32_t node, uint32_t c, const uint32_t* f, const float* v, const uint32_t* elements, uint32_t n_elements) {
    const uint32_t ref = mu_ref<W>(tree, node, c);
    if (!mu_is_leaf(ref)) return;
    const uint32_t first = ref & 0x0FFFFFFFu, count = ref >> 28;
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    for (uint32_t s = first; s < first + count && s < n_elements; s++) {
        const uint32_t* fv = f + 3 * (size_t)elements[s];
        for (uint32_t k = 0; k < 3; k++) {
            const float a = v[3 * (size_t)fv[0] + k], b = v[3 * (size_t)fv[1] + k], cc = v[3 * (size_t)fv[2] + k];
            const float l = a < b ? (a < cc ? a : cc) : (b < cc ? b : cc);
            const float h = a > b ? (a > cc ? a : cc) : (b > cc ? b : cc);
            if (l < lo[k]) lo[k] = l;
            if (h > hi[k]) hi[k] = h;
        }
    }
    float* n = tree + (size_t)node * MuWide<W>::kNodeFloats;
    for (uint32_t k = 0; k < 3; k++) { n[MuWide<W>::lo(c, k)] = lo[k]; n[MuWide<W>::hi(c, k)] = hi[k]; }
}

// An inner slot (ref = the node it stands for): the union of that node's child boxes, which must be final (children come after
// their parents in the breadth-first order: deepest level first). Unused slots hold +-infinity and drop out.
template <int W>
RTU_HD void mu_inner_slot(float* tree, uint32_t n_nodes, uint32_t node, uint32_t c) {
    const uint32_t ref = mu_ref<W>(tree, node, c);
    if (!mu_is_inner(ref) || ref >= n_nodes) return;
    const float* ch = tree + (size_t)ref * MuWide<W>::kNodeFloats;
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    for (uint32_t cc = 0; cc < (uint32_t)W; cc++)
        for (uint32_t k = 0; k < 3; k++) {
            const float l = ch[MuWide<W>::lo(cc, k)], h = ch[MuWide<W>::hi(cc, k)];
            if (l < lo[k]) lo[k] = l;
            if (h > hi[k]) hi[k] = h;
        }
    float* n = tree + (size_t)node * MuWide<W>::kNodeFloats;
    for (uint32_t k = 0; k < 3; k++) { n[MuWide<W>::lo(c, k)] = lo[k]; n[MuWide<W>::hi(c, k)] = hi[k]; }
}

// ---- the device side (rtu_mesh_update.hip); every pointer is device memory, every call enqueues on `st` and returns ----
// records of element slots [0, n) into tri [4 n]
hipError_t mu_tri_records(hipStream_t st, const uint32_t* f, const float* v, const uint32_t* elements, uint32_t n, float4* tri);
// the boxes of every child slot of a collapsed tree of `width` 4 or 8 and n_nodes nodes, rewritten from f / v through the fast tree's
// `elements`; level_start [n_levels + 1] (host): node ranges of the tree's levels, root first
hipError_t mu_refit(hipStream_t st, int width, float4* tree, uint32_t n_nodes, const uint32_t* level_start, uint32_t n_levels, const uint32_t* f,
                    const float* v, const uint32_t* elements, uint32_t n_elements);
