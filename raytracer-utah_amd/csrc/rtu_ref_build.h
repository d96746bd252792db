// rtu_ref_build.h — the reference's mean-split tree (BuildBVH / TreeWriter of host/mesh.cpp) restated LEVEL BY LEVEL, so that a GPU
// can build it (rtu_update_meshes_device). One set of __host__ __device__ passes: the kernels of rtu_ref_build.hip run a pass with
// one lane per index, the host form (rb_build_host, behind rtu_debug_host_ref_build) runs the same pass in a loop. Both sides are
// compiled with -ffp-contract=off and IEEE divide / sqrt, and the tree holds comparisons, one addition chain and one divide per
// centre: both write the same bits as host/mesh.cpp.
//
// A level is a list of segments [first, first + count) of the element order, in the queue order of renumber_bfs: node ids of a
// level are consecutive, and the children of its inner nodes take the next ids pair by pair (an exclusive scan of the inner flags),
// so the tree is born in the breadth-first numbering the device walks.
//
// The passes of one level, S segments over n element positions:
//   RbFlag      position: does its element keep left in this attempt of its segment (centre <= mid on the attempt's axis)
//   (scan)      exclusive sum of the flags
//   RbKeepers   position: a keeper at or behind L (the segment's number of keepers) notes itself by its rank from the back
//   RbScatter   position: where partition_from_back leaves its element (the closed form below), into the other element buffer
//   RbResolve   segment: split found / next attempt / after three: leaf (count <= 8) or halved
//   (scan)      exclusive sum of the inner flags
//   RbEmit      segment: its node; the two child segments of an inner one
//   RbAssign    position: the child segment of its element; the element's triangle box into that child's box
//   RbSegment   child segment: its box from the reduction; leaf (count <= 4) or open, and the axis order of its attempts
//
// partition_from_back in closed form. n the segment's count, L its number of keepers, q_0 > q_1 > ... the positions >= L that hold
// keepers: a keeper at p < L stays; the j-th failing position p <= L (from the front) receives the keeper of q_j if p < L and sends
// its own element to q_(j-1) - 1 (q_(-1) = n); every other failing element, at q > L, moves to q - 1.
//
// Boxes. The host folds `if (lo > x) lo = x` over triangle boxes in element order from +-1e30: the result is the smallest value
// below 1e30, and among equal values (-0 against +0) the FIRST in element order; a NaN never enters. Here each value becomes a
// 64-bit key {ordered float bits with -0 read as +0, position, was it -0} and the fold is a min / max of keys, which any order of
// evaluation (atomics, a wave's butterfly) answers the same. Not included by the render kernels.
#pragma once
#include "rtu_scene.h"
#include "rtu_vec.h"

#include <stdint.h>

#define RB_NONE 0xFFFFFFFFu
enum { RB_LEAF = 0, RB_OPEN = 1, RB_SPLIT = 2 };
#define RB_MAX_PER_NODE 4u   // BuildBVH(data, 4), objects.h:58
#define RB_HARD_LEAF    8u   // CY_BVH_MAX_ELEMENT_COUNT

struct RbSeg {
    uint32_t first, count, left, state;
    uint32_t axes, pad;  // the axis of attempt a: (axes >> 2a) & 3
    float    lo[3], hi[3];
};

struct RbCounters {
    uint32_t open[3];    // segments still open after attempt a of the level
    uint32_t split;      // inner nodes of the level so far
    uint32_t any_empty;  // some node's box has min > max
    uint32_t differs;    // rb_compare: the two index arrays differ
};

// the arrays of one build; the driver swaps el_in / el_out after every attempt and seg / next after every level
struct RbWork {
    const uint32_t* f;
    const float*    v;
    uint32_t        n;         // faces = element positions
    uint32_t *el_in, *el_out;  // [n] the element order, double-buffered
    uint32_t*       seg_of;    // [n] the segment (of the current level) position p lies in, RB_NONE below a leaf
    uint32_t *flag, *scan;     // [n + 1]
    uint32_t*       kq;        // [n] per segment from its first: the positions >= L that hold keepers, from the back
    RbSeg *seg, *next;         // [n] each: the current level's segments and the next one's
    uint32_t *inner, *inner_scan;  // [n + 1]
    unsigned long long* keys;  // [6 n] per next-level segment: min keys of x, y, z, then max keys
    RtuBvhNode* tree;          // [2 n]
    RbCounters* cnt;
    uint32_t S, base, attempt; // segments of the level, the node id of its first, the attempt
};

// ---- keys -------------------------------------------------------------------------------------------------------------------------
RTU_HD uint32_t rb_bits(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
RTU_HD float rb_float(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
RTU_HD uint32_t rb_ord(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }   // unsigned order = float order
RTU_HD uint32_t rb_unord(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }
#define RB_MIN_IDENTITY 0xFFFFFFFFFFFFFFFFull
#define RB_MAX_IDENTITY 0ull
// x is no NaN; pos < 2^31. The smaller key: the smaller value, then the earlier position.
RTU_HD unsigned long long rb_min_key(float x, uint32_t pos) {
    uint32_t u = rb_bits(x);
    const uint32_t nz = u == 0x80000000u ? 1u : 0u;
    if (nz) u = 0;
    return ((unsigned long long)rb_ord(u) << 32) | ((unsigned long long)pos << 1) | nz;
}
// The larger key: the larger value, then the earlier position.
RTU_HD unsigned long long rb_max_key(float x, uint32_t pos) {
    uint32_t u = rb_bits(x);
    const uint32_t nz = u == 0x80000000u ? 1u : 0u;
    if (nz) u = 0;
    return ((unsigned long long)rb_ord(u) << 32) | ((unsigned long long)(0x7FFFFFFFu - pos) << 1) | nz;
}
RTU_HD float rb_key_value(unsigned long long key) {
    return (key & 1ull) ? rb_float(0x80000000u) : rb_float(rb_unord((uint32_t)(key >> 32)));
}

// the six keys of a triangle box at element position pos, as Bounds::include would fold it from +-1e30
RTU_HD void rb_box_keys(const float lo[3], const float hi[3], uint32_t pos, unsigned long long k[6]) {
    for (int a = 0; a < 3; a++) {
        k[a] = rb_min_key((1e30f > lo[a]) ? lo[a] : 1e30f, pos);        // (a NaN and anything >= 1e30 never replace the 1e30)
        k[3 + a] = rb_max_key((-1e30f < hi[a]) ? hi[a] : -1e30f, pos);
    }
}

// dst[0..2] = min(dst, k), dst[3..5] = max(dst, k). On the device with atomics; a full wave whose lanes all feed the same six
// (same != 0, wave-uniform) reduces them by a butterfly first and lane 0 writes.
RTU_HD void rb_fold_keys(unsigned long long* dst, unsigned long long k[6], bool same) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (same) {
        for (int i = 0; i < 6; i++)
            for (int m = 32; m >= 1; m >>= 1) {
                const unsigned long long o = __shfl_xor(k[i], m, 64);
                k[i] = i < 3 ? (o < k[i] ? o : k[i]) : (o > k[i] ? o : k[i]);
            }
        if ((threadIdx.x & 63u) != 0) return;
    }
    for (int i = 0; i < 3; i++) atomicMin(dst + i, k[i]);
    for (int i = 3; i < 6; i++) atomicMax(dst + i, k[i]);
#else
    (void)same;
    for (int i = 0; i < 3; i++) if (k[i] < dst[i]) dst[i] = k[i];
    for (int i = 3; i < 6; i++) if (k[i] > dst[i]) dst[i] = k[i];
#endif
}

// do all lanes of this (full) wave hold the same c? Host: no waves.
RTU_HD bool rb_wave_same(uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (__ballot(1) != 0xFFFFFFFFFFFFFFFFull) return false;
    const uint32_t c0 = (uint32_t)__shfl((int)c, 0, 64);
    return __all(c == c0) != 0;
#else
    (void)c;
    return false;
#endif
}

RTU_HD void rb_count(uint32_t* counter) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(counter, 1u);
#else
    (*counter)++;
#endif
}

// ---- per element ------------------------------------------------------------------------------------------------------------------
// GetElementBounds (cyBVH.h:356-367): corner 0 is assigned, the others compared
RTU_HD void rb_tri_bounds(const uint32_t* f, const float* v, uint32_t face, float lo[3], float hi[3]) {
    for (int c = 0; c < 3; c++) {
        const float* p = v + 3 * (size_t)f[3 * (size_t)face + c];
        for (int k = 0; k < 3; k++) {
            if (c == 0 || lo[k] > p[k]) lo[k] = p[k];
            if (c == 0 || hi[k] < p[k]) hi[k] = p[k];
        }
    }
}
// GetElementCenter (:370-374)
RTU_HD float rb_centre(const uint32_t* f, const float* v, uint32_t face, uint32_t axis) {
    const uint32_t* fv = f + 3 * (size_t)face;
    return (v[3 * (size_t)fv[0] + axis] + v[3 * (size_t)fv[1] + axis] + v[3 * (size_t)fv[2] + axis]) / 3.0f;
}

// ---- per segment ------------------------------------------------------------------------------------------------------------------
// MeanSplit's axis order (:290-326): widest first (x before y before z among equals), then the two others in cyclic order unless
// the second of them is strictly wider
RTU_HD uint32_t rb_axes(const float lo[3], const float hi[3]) {
    const float ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const uint32_t first = ext[0] >= ext[1] ? (ext[0] >= ext[2] ? 0u : 2u) : (ext[1] >= ext[2] ? 1u : 2u);
    uint32_t a1 = (first + 1u) % 3u, a2 = (first + 2u) % 3u;
    if (ext[a1] < ext[a2]) { const uint32_t t = a1; a1 = a2; a2 = t; }
    return first | (a1 << 2) | (a2 << 4);
}

// Where partition_from_back leaves things, for the element at local position p of a segment of n with L keepers. kb: keepers
// before p; kq[j]: the j-th position >= L that holds a keeper, from the back. src: the local position whose element ends at p
// (RB_NONE: none from this rule); dst: where p's own element goes (RB_NONE: nowhere from this rule, it is pulled).
RTU_HD void rb_partition_rule(uint32_t p, uint32_t n, uint32_t L, bool keep, uint32_t kb, const uint32_t* kq, uint32_t& src, uint32_t& dst) {
    src = dst = RB_NONE;
    if (keep) {
        if (p < L) dst = p;
        return;
    }
    if (p <= L) {
        const uint32_t j = p - kb;  // failing positions before p
        if (p < L) src = kq[j];
        dst = (j > 0 ? kq[j - 1] : n) - 1u;
    } else {
        dst = p - 1u;
    }
}

// ---- the passes -------------------------------------------------------------------------------------------------------------------
struct RbBegin {  // one lane
    static RTU_HD void run(const RbWork& w, uint32_t) {
        RbCounters c = {};
        *w.cnt = c;
        RtuBvhNode z = {};
        w.tree[0] = z;  // node 0 is unused, the root is node 1
        for (int i = 0; i < 3; i++) { w.keys[i] = RB_MIN_IDENTITY; w.keys[3 + i] = RB_MAX_IDENTITY; }
        w.next[0].first = 0;
        w.next[0].count = w.n;
    }
};

struct RbInit {  // position: the identity order, all of it the root's
    static RTU_HD void run(const RbWork& w, uint32_t p) {
        w.el_in[p] = p;
        w.seg_of[p] = 0;
        float lo[3], hi[3];
        rb_tri_bounds(w.f, w.v, p, lo, hi);
        unsigned long long k[6];
        rb_box_keys(lo, hi, p, k);
        rb_fold_keys(w.keys, k, rb_wave_same(0));
    }
};

struct RbSegment {  // segment of the NEXT level (w.next): its box, and split()'s first decision
    static RTU_HD void run(const RbWork& w, uint32_t c) {
        RbSeg& s = w.next[c];
        const unsigned long long* k = w.keys + 6 * (size_t)c;
        for (int a = 0; a < 3; a++) {
            s.lo[a] = k[a] == RB_MIN_IDENTITY ? 1e30f : rb_key_value(k[a]);
            s.hi[a] = k[3 + a] == RB_MAX_IDENTITY ? -1e30f : rb_key_value(k[3 + a]);
        }
        s.left = 0;
        s.pad = 0;
        s.axes = rb_axes(s.lo, s.hi);
        s.state = s.count <= RB_MAX_PER_NODE ? RB_LEAF : RB_OPEN;
    }
};

struct RbFlag {  // n + 1 lanes
    static RTU_HD void run(const RbWork& w, uint32_t p) {
        uint32_t keep = 0;
        const uint32_t si = p < w.n ? w.seg_of[p] : RB_NONE;
        if (si != RB_NONE) {
            const RbSeg& s = w.seg[si];
            if (s.state == RB_OPEN) {
                const uint32_t axis = (s.axes >> (2u * w.attempt)) & 3u;
                const float mid = 0.5f * (s.lo[axis] + s.hi[axis]);
                keep = rb_centre(w.f, w.v, w.el_in[p], axis) <= mid ? 1u : 0u;
            }
        }
        w.flag[p] = keep;
    }
};

struct RbKeepers {
    static RTU_HD void run(const RbWork& w, uint32_t p) {
        const uint32_t si = w.seg_of[p];
        if (si == RB_NONE || !w.flag[p]) return;
        const RbSeg& s = w.seg[si];
        if (s.state != RB_OPEN) return;
        const uint32_t L = w.scan[s.first + s.count] - w.scan[s.first], kb = w.scan[p] - w.scan[s.first], q = p - s.first;
        if (q >= L) w.kq[s.first + (L - 1u - kb)] = q;
    }
};

struct RbScatter {
    static RTU_HD void run(const RbWork& w, uint32_t p) {
        const uint32_t si = w.seg_of[p];
        const RbSeg* s = si == RB_NONE ? nullptr : &w.seg[si];
        if (!s || s->state != RB_OPEN) {
            w.el_out[p] = w.el_in[p];
            return;
        }
        const uint32_t L = w.scan[s->first + s->count] - w.scan[s->first], kb = w.scan[p] - w.scan[s->first];
        uint32_t src, dst;
        rb_partition_rule(p - s->first, s->count, L, w.flag[p] != 0, kb, w.kq + s->first, src, dst);
        if (src != RB_NONE) w.el_out[p] = w.el_in[s->first + src];
        if (dst != RB_NONE) w.el_out[s->first + dst] = w.el_in[p];
    }
};

struct RbResolve {  // S + 1 lanes
    static RTU_HD void run(const RbWork& w, uint32_t si) {
        if (si == w.S) { w.inner[si] = 0; return; }
        RbSeg& s = w.seg[si];
        if (s.state == RB_OPEN) {
            const uint32_t L = w.scan[s.first + s.count] - w.scan[s.first];
            if (L > 0 && L < s.count) { s.state = RB_SPLIT; s.left = L; }
            else if (w.attempt == 2) {
                if (s.count <= RB_HARD_LEAF) s.state = RB_LEAF;
                else { s.state = RB_SPLIT; s.left = s.count / 2; }  // nothing separates them: halve the list as it stands
            } else rb_count(&w.cnt->open[w.attempt]);
            if (s.state == RB_SPLIT) rb_count(&w.cnt->split);
        }
        w.inner[si] = s.state == RB_SPLIT ? 1u : 0u;
    }
};

struct RbEmit {
    static RTU_HD void run(const RbWork& w, uint32_t si) {
        const RbSeg& s = w.seg[si];
        RtuBvhNode nd;
        for (int k = 0; k < 3; k++) { nd.bmin[k] = s.lo[k]; nd.bmax[k] = s.hi[k]; }
        if (s.lo[0] > s.hi[0] || s.lo[1] > s.hi[1] || s.lo[2] > s.hi[2]) w.cnt->any_empty = 1;
        if (s.state == RB_SPLIT) {
            const uint32_t c = 2u * w.inner_scan[si];
            nd.index = w.base + w.S + c;
            nd.count = 0;
            w.next[c].first = s.first;
            w.next[c].count = s.left;
            w.next[c + 1].first = s.first + s.left;
            w.next[c + 1].count = s.count - s.left;
            for (uint32_t h = 0; h < 2; h++)
                for (int i = 0; i < 3; i++) {
                    w.keys[6 * (size_t)(c + h) + i] = RB_MIN_IDENTITY;
                    w.keys[6 * (size_t)(c + h) + 3 + i] = RB_MAX_IDENTITY;
                }
        } else {
            nd.index = s.first;
            nd.count = s.count;
        }
        w.tree[w.base + si] = nd;
        if (si == 0) { w.cnt->open[0] = w.cnt->open[1] = w.cnt->open[2] = 0; w.cnt->split = 0; }  // (the host has read them)
    }
};

struct RbAssign {
    static RTU_HD void run(const RbWork& w, uint32_t p) {
        const uint32_t si = w.seg_of[p];
        uint32_t c = RB_NONE;
        if (si != RB_NONE) {
            const RbSeg& s = w.seg[si];
            if (s.state == RB_SPLIT) c = 2u * w.inner_scan[si] + (p - s.first >= s.left ? 1u : 0u);
        }
        w.seg_of[p] = c;
        const bool same = rb_wave_same(c);  // (every lane of the wave asks, whatever its c)
        if (c == RB_NONE) return;
        float lo[3], hi[3];
        rb_tri_bounds(w.f, w.v, w.el_in[p], lo, hi);
        unsigned long long k[6];
        rb_box_keys(lo, hi, p, k);
        rb_fold_keys(w.keys + 6 * (size_t)c, k, same);
    }
};

// ---- the mesh box: ComputeBoundingBox over all vertices (cyTriMesh.h:226-246) -------------------------------------------------------
// Vertex 0 is assigned, the others compared: a NaN coordinate of vertex 0 sticks, any other NaN drops out.
struct RbVertexBox {
    const float* v;
    uint32_t nv;
    unsigned long long* keys;  // [6], identities before the pass
    float* out;                // [6] bmin, bmax
};
RTU_HD void rb_vertex_box_fold(const RbVertexBox& b, uint32_t i) {
    unsigned long long k[6];
    for (int a = 0; a < 3; a++) {
        const float c = b.v[3 * (size_t)i + a];
        const bool nan = c != c;
        k[a] = rb_min_key(nan ? rb_float(0x7F800000u) : c, i);
        k[3 + a] = rb_max_key(nan ? rb_float(0xFF800000u) : c, i);
    }
    rb_fold_keys(b.keys, k, rb_wave_same(0));
}
RTU_HD void rb_vertex_box_finish(const RbVertexBox& b) {
    for (int a = 0; a < 3; a++) {
        const float c = b.v[a];
        const bool nan = c != c;
        b.out[a] = nan ? c : rb_key_value(b.keys[a]);
        b.out[3 + a] = nan ? c : rb_key_value(b.keys[3 + a]);
    }
}

// ---- normals: ComputeNormals (cyTriMesh.h:248-261) by vertex ----------------------------------------------------------------------
// corners: the ids 3 face + corner of all corners, sorted by the vertex they name, stably (so in (face, corner) order per vertex);
// [lo, hi) those of this vertex. A face that names the vertex twice adds its cross product twice, as the host's loop does.
RTU_HD void rb_vertex_normal(const uint32_t* f, const float* v, const uint32_t* corners, uint32_t lo, uint32_t hi, float* out3) {
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t* fv = f + 3 * (size_t)(corners[j] / 3u);
        const f3 A = ld3(v + 3 * (size_t)fv[0]);
        const f3 N = cross3(ld3(v + 3 * (size_t)fv[1]) - A, ld3(v + 3 * (size_t)fv[2]) - A);
        sx += N.x; sy += N.y; sz += N.z;
    }
    const f3 n = norm3(mk3(sx, sy, sz));
    out3[0] = n.x; out3[1] = n.y; out3[2] = n.z;
}
// the range of `vertex` in the sorted keys (keys[j] = the vertex corner corners[j] names)
RTU_HD void rb_vertex_range(const uint32_t* keys, uint32_t n, uint32_t vertex, uint32_t& lo, uint32_t& hi) {
    uint32_t a = 0, b = n;
    while (a < b) { const uint32_t m = a + (b - a) / 2; if (keys[m] < vertex) a = m + 1; else b = m; }
    lo = a;
    b = n;
    while (a < b) { const uint32_t m = a + (b - a) / 2; if (keys[m] <= vertex) a = m + 1; else b = m; }
    hi = a;
}

// ---- host interface ---------------------------------------------------------------------------------------------------------------
#include <vector>

#pragma GCC visibility push(hidden)

struct RbResult {
    uint32_t n_bvh_nodes = 0, bvh_depth = 0, any_empty_box = 0;
    uint32_t open = 0;  // inner nodes of level max_levels whose children the build did not make: the tree is deeper than that
    float    bmin[3] = {}, bmax[3] = {};
};

// The host form: the same passes in loops. tree [n_bvh_nodes] breadth-first, elements [nf]. max_levels 0: no bound.
void rb_build_host(const uint32_t* f, const float* v, uint32_t nf, uint32_t nv, uint32_t max_levels, std::vector<RtuBvhNode>& tree,
                   std::vector<uint32_t>& elements, RbResult& out);
void rb_normals_host(const uint32_t* f, const float* v, uint32_t nf, uint32_t nv, std::vector<float>& vn);
void rb_partition_host(const uint8_t* keep, uint32_t n, uint32_t* perm_out);  // perm_out[i]: the position whose element ends at i

// The device form. A RefBuilder owns every scratch buffer (grow-only) and the adjacency of the meshes it computed normals for.
struct RefBuilder;
RefBuilder* rb_create();
void rb_destroy(RefBuilder* b);
void rb_forget_meshes(RefBuilder* b);  // a new upload: the cached adjacencies are another scene's
// Builds the tree of (d_f, d_v) into output slot `slot` of the builder and waits: out is filled, rb_tree / rb_elements are valid
// until the next build into the same slot. Plain launches on st.
hipError_t rb_build_device(RefBuilder* b, hipStream_t st, uint32_t slot, const uint32_t* d_f, const float* d_v, uint32_t nf, uint32_t nv,
                           uint32_t max_levels, RbResult& out);
const RtuBvhNode* rb_tree(const RefBuilder* b, uint32_t slot);
const uint32_t* rb_elements(const RefBuilder* b, uint32_t slot);
// ComputeNormals of (d_f, d_v) into the builder's vn of `slot` (rb_normals), enqueued on st. mesh: the key of the cached adjacency.
hipError_t rb_normals_device(RefBuilder* b, hipStream_t st, uint32_t slot, uint32_t mesh, const uint32_t* d_f, const float* d_v, uint32_t nf,
                             uint32_t nv);
const float* rb_normals(const RefBuilder* b, uint32_t slot);
// do the index arrays a and b [n] differ? (synchronous)
hipError_t rb_compare_device(RefBuilder* b, hipStream_t st, const uint32_t* d_a, const uint32_t* d_b, uint32_t n, bool& differ);
#pragma GCC visibility pop
