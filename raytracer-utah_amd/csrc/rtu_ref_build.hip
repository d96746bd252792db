// rtu_ref_build.hip — the drivers of rtu_ref_build.h's passes: one level loop, instantiated for the host (loops; rb_build_host) and
// for the device (plain launches on the caller's stream; rb_build_device), and the normals by vertex adjacency.
//   k_rb<Pass>          a lane per index of the pass (element position or segment); 256-lane blocks, no LDS. RbInit and RbAssign
//                       fold 64-bit box keys with atomicMin / atomicMax, one per wave where a wave feeds one segment
//   k_rb_vertex_box*    the mesh box over all vertices, the same keys
//   k_rb_corner_keys    {vertex, corner id} pairs for the stable sort that makes the adjacency
//   k_rb_normals        a lane per vertex: its faces' cross products in (face, corner) order
//   k_rb_compare        do two index arrays differ
// The device loop reads 24 bytes of counters back through pinned memory after every attempt of a level (how many segments are still
// open, how many split): there is no grid barrier and no lane waits for another. Every index a lane follows is an element id below
// n, a position below n, or a face / vertex id that was range-checked at upload.
#include "rtu_ref_build.h"

#include "rtu_devbuf.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <map>
#include <numeric>

#define RB_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

namespace {

const uint32_t kBlock = 256;

template <class Pass>
__global__ void k_rb(RbWork w, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) Pass::run(w, i);
}

__global__ void k_rb_vertex_box_begin(RbVertexBox b) {
    if (blockIdx.x * blockDim.x + threadIdx.x != 0) return;
    for (int i = 0; i < 3; i++) { b.keys[i] = RB_MIN_IDENTITY; b.keys[3 + i] = RB_MAX_IDENTITY; }
}
__global__ void k_rb_vertex_box(RbVertexBox b) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b.nv) rb_vertex_box_fold(b, i);
}
__global__ void k_rb_vertex_box_finish(RbVertexBox b) {
    if (blockIdx.x * blockDim.x + threadIdx.x == 0) rb_vertex_box_finish(b);
}

__global__ void k_rb_corner_keys(const uint32_t* __restrict__ f, uint32_t n3, uint32_t* __restrict__ keys, uint32_t* __restrict__ corners) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    keys[i] = f[i];
    corners[i] = i;
}

__global__ void k_rb_normals(const uint32_t* __restrict__ f, const float* __restrict__ v, const uint32_t* __restrict__ keys,
                             const uint32_t* __restrict__ corners, uint32_t n3, uint32_t nv, float* __restrict__ vn) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    uint32_t lo, hi;
    rb_vertex_range(keys, n3, i, lo, hi);
    rb_vertex_normal(f, v, corners, lo, hi, vn + 3 * (size_t)i);
}

__global__ void k_rb_compare(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n, uint32_t* __restrict__ differ) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && a[i] != b[i]) *differ = 1u;
}

uint32_t blocks(uint32_t count) { return (count + kBlock - 1) / kBlock; }

// The level loop. Exec: run<Pass>(w, count), scan(in, out, n1) — exclusive sum of n1 values —, counters(w, c) — the counters as
// they are once everything enqueued has run. w comes back with el_in the final element order.
template <class Exec>
hipError_t rb_levels(Exec& ex, RbWork& w, uint32_t max_levels, RbResult& out) {
    RB_TRY(ex.template run<RbBegin>(w, 1));
    RB_TRY(ex.template run<RbInit>(w, w.n));
    RB_TRY(ex.template run<RbSegment>(w, 1));
    std::swap(w.seg, w.next);
    w.S = 1;
    w.base = 1;
    RbCounters c = {};
    for (uint32_t level = 1;; level++) {
        for (w.attempt = 0; w.attempt < 3; w.attempt++) {  // a failed attempt has permuted its segment: the next one works on that order
            RB_TRY(ex.template run<RbFlag>(w, w.n + 1));
            RB_TRY(ex.scan(w.flag, w.scan, w.n + 1));
            RB_TRY(ex.template run<RbKeepers>(w, w.n));
            RB_TRY(ex.template run<RbScatter>(w, w.n));
            RB_TRY(ex.template run<RbResolve>(w, w.S + 1));
            std::swap(w.el_in, w.el_out);
            RB_TRY(ex.counters(w, c));
            if (c.open[w.attempt] == 0) break;  // (never open after the third)
        }
        RB_TRY(ex.scan(w.inner, w.inner_scan, w.S + 1));
        RB_TRY(ex.template run<RbEmit>(w, w.S));
        out.bvh_depth = level;
        out.n_bvh_nodes = w.base + w.S;
        out.open = 0;
        if (c.split == 0) break;
        if (max_levels && level == max_levels) { out.open = c.split; break; }
        RB_TRY(ex.template run<RbAssign>(w, w.n));
        RB_TRY(ex.template run<RbSegment>(w, 2 * c.split));
        std::swap(w.seg, w.next);
        w.base += w.S;
        w.S = 2 * c.split;
    }
    RB_TRY(ex.counters(w, c));
    out.any_empty_box = c.any_empty;
    return hipSuccess;
}

struct HostExec {
    template <class Pass> hipError_t run(const RbWork& w, uint32_t count) {
        for (uint32_t i = 0; i < count; i++) Pass::run(w, i);
        return hipSuccess;
    }
    hipError_t scan(const uint32_t* in, uint32_t* out, uint32_t n1) {
        uint32_t sum = 0;
        for (uint32_t i = 0; i < n1; i++) { const uint32_t x = in[i]; out[i] = sum; sum += x; }
        return hipSuccess;
    }
    hipError_t counters(const RbWork& w, RbCounters& c) { c = *w.cnt; return hipSuccess; }
};

}  // namespace

struct RefBuilder {
    struct Slot {
        DevBuf<RtuBvhNode> tree;
        DevBuf<uint32_t>   el[2];
        DevBuf<float>      vn;
        const uint32_t*    elements = nullptr;  // the one of el[] the last build left the order in
    };
    std::vector<Slot> slots;
    DevBuf<uint32_t> seg_of, flag, scan, kq, inner, inner_scan;
    DevBuf<RbSeg> seg[2];
    DevBuf<unsigned long long> keys, vkeys;
    DevBuf<RbCounters> cnt;
    DevBuf<float> vbox;
    DevBuf<uint32_t> differ;
    PinnedBuf<RbCounters> h_cnt;
    PinnedBuf<float> h_box;
    PinnedBuf<uint32_t> h_differ;
    DevBuf<char> tmp;                       // hipcub's temporary storage
    DevBuf<uint32_t> sort_keys, sort_vals;  // the unsorted corner pairs
    struct Adj { DevBuf<uint32_t> keys, corners; };
    std::map<uint32_t, Adj> adj;            // per mesh: its corners sorted by vertex (built on first use)
};

namespace {

struct DeviceExec {
    RefBuilder* b;
    hipStream_t st;
    template <class Pass> hipError_t run(const RbWork& w, uint32_t count) {
        if (count == 0) return hipSuccess;
        k_rb<Pass><<<blocks(count), kBlock, 0, st>>>(w, count);
        return hipGetLastError();
    }
    hipError_t scan(const uint32_t* in, uint32_t* out, uint32_t n1) {
        size_t bytes = 0;
        RB_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)n1, st));
        RB_TRY(b->tmp.grow(bytes ? bytes : 16));
        bytes = b->tmp.size();
        return hipcub::DeviceScan::ExclusiveSum(b->tmp.get(), bytes, in, out, (int)n1, st);
    }
    hipError_t counters(const RbWork& w, RbCounters& c) {
        RB_TRY(hipMemcpyAsync(b->h_cnt.get(), w.cnt, sizeof c, hipMemcpyDeviceToHost, st));
        RB_TRY(hipStreamSynchronize(st));
        c = *b->h_cnt.get();
        return hipSuccess;
    }
};

RefBuilder::Slot& slot_of(RefBuilder* b, uint32_t slot) {
    if (b->slots.size() <= slot) b->slots.resize((size_t)slot + 1);
    return b->slots[slot];
}

}  // namespace

RefBuilder* rb_create() { return new RefBuilder; }
void rb_destroy(RefBuilder* b) { delete b; }
void rb_forget_meshes(RefBuilder* b) { if (b) b->adj.clear(); }

hipError_t rb_build_device(RefBuilder* b, hipStream_t st, uint32_t slot, const uint32_t* d_f, const float* d_v, uint32_t nf, uint32_t nv,
                           uint32_t max_levels, RbResult& out) {
    RefBuilder::Slot& s = slot_of(b, slot);
    const size_t n = nf;
    RB_TRY(s.tree.grow(2 * n));
    RB_TRY(s.el[0].grow(n));
    RB_TRY(s.el[1].grow(n));
    RB_TRY(b->seg_of.grow(n));
    RB_TRY(b->flag.grow(n + 1));
    RB_TRY(b->scan.grow(n + 1));
    RB_TRY(b->kq.grow(n));
    RB_TRY(b->inner.grow(n + 1));
    RB_TRY(b->inner_scan.grow(n + 1));
    RB_TRY(b->seg[0].grow(n));
    RB_TRY(b->seg[1].grow(n));
    RB_TRY(b->keys.grow(6 * n));
    RB_TRY(b->vkeys.grow(6));
    RB_TRY(b->vbox.grow(6));
    RB_TRY(b->cnt.grow(1));
    RB_TRY(b->h_cnt.grow(1));
    RB_TRY(b->h_box.grow(6));
    // the mesh box first: its read-back rides on the level loop's
    RbVertexBox vb = {d_v, nv, b->vkeys.get(), b->vbox.get()};
    k_rb_vertex_box_begin<<<1, 64, 0, st>>>(vb);
    k_rb_vertex_box<<<blocks(nv), kBlock, 0, st>>>(vb);
    k_rb_vertex_box_finish<<<1, 64, 0, st>>>(vb);
    RB_TRY(hipGetLastError());
    RB_TRY(hipMemcpyAsync(b->h_box.get(), b->vbox.get(), 6 * sizeof(float), hipMemcpyDeviceToHost, st));
    RbWork w = {};
    w.f = d_f; w.v = d_v; w.n = nf;
    w.el_in = s.el[0].get(); w.el_out = s.el[1].get();
    w.seg_of = b->seg_of.get(); w.flag = b->flag.get(); w.scan = b->scan.get(); w.kq = b->kq.get();
    w.seg = b->seg[0].get(); w.next = b->seg[1].get();
    w.inner = b->inner.get(); w.inner_scan = b->inner_scan.get();
    w.keys = b->keys.get(); w.tree = s.tree.get(); w.cnt = b->cnt.get();
    DeviceExec ex = {b, st};
    RB_TRY(rb_levels(ex, w, max_levels, out));
    s.elements = w.el_in;
    memcpy(out.bmin, b->h_box.get(), sizeof out.bmin);
    memcpy(out.bmax, b->h_box.get() + 3, sizeof out.bmax);
    return hipSuccess;
}

const RtuBvhNode* rb_tree(const RefBuilder* b, uint32_t slot) { return b->slots[slot].tree.get(); }
const uint32_t* rb_elements(const RefBuilder* b, uint32_t slot) { return b->slots[slot].elements; }
const float* rb_normals(const RefBuilder* b, uint32_t slot) { return b->slots[slot].vn.get(); }

hipError_t rb_normals_device(RefBuilder* b, hipStream_t st, uint32_t slot, uint32_t mesh, const uint32_t* d_f, const float* d_v, uint32_t nf,
                             uint32_t nv) {
    RefBuilder::Slot& s = slot_of(b, slot);
    RB_TRY(s.vn.grow(3 * (size_t)nv));
    const uint32_t n3 = 3 * nf;
    auto it = b->adj.find(mesh);
    if (it == b->adj.end()) {  // once per uploaded topology
        RefBuilder::Adj a;
        RB_TRY(a.keys.grow(n3));
        RB_TRY(a.corners.grow(n3));
        RB_TRY(b->sort_keys.grow(n3));
        RB_TRY(b->sort_vals.grow(n3));
        k_rb_corner_keys<<<blocks(n3), kBlock, 0, st>>>(d_f, n3, b->sort_keys.get(), b->sort_vals.get());
        RB_TRY(hipGetLastError());
        size_t bytes = 0;
        RB_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, b->sort_keys.get(), a.keys.get(), b->sort_vals.get(), a.corners.get(), (int)n3, 0, 32, st));
        RB_TRY(b->tmp.grow(bytes ? bytes : 16));
        bytes = b->tmp.size();
        RB_TRY(hipcub::DeviceRadixSort::SortPairs(b->tmp.get(), bytes, b->sort_keys.get(), a.keys.get(), b->sort_vals.get(), a.corners.get(), (int)n3, 0, 32, st));
        it = b->adj.emplace(mesh, std::move(a)).first;
    }
    k_rb_normals<<<blocks(nv), kBlock, 0, st>>>(d_f, d_v, it->second.keys.get(), it->second.corners.get(), n3, nv, s.vn.get());
    return hipGetLastError();
}

hipError_t rb_compare_device(RefBuilder* b, hipStream_t st, const uint32_t* d_a, const uint32_t* d_b, uint32_t n, bool& differ) {
    RB_TRY(b->differ.grow(1));
    RB_TRY(b->h_differ.grow(1));
    RB_TRY(hipMemsetAsync(b->differ.get(), 0, sizeof(uint32_t), st));
    if (n) k_rb_compare<<<blocks(n), kBlock, 0, st>>>(d_a, d_b, n, b->differ.get());
    RB_TRY(hipGetLastError());
    RB_TRY(hipMemcpyAsync(b->h_differ.get(), b->differ.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RB_TRY(hipStreamSynchronize(st));
    differ = *b->h_differ.get() != 0;
    return hipSuccess;
}

// ---- the host form ----------------------------------------------------------------------------------------------------------------

void rb_build_host(const uint32_t* f, const float* v, uint32_t nf, uint32_t nv, uint32_t max_levels, std::vector<RtuBvhNode>& tree,
                   std::vector<uint32_t>& elements, RbResult& out) {
    const size_t n = nf;
    std::vector<uint32_t> el[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
    std::vector<uint32_t> seg_of(n), flag(n + 1), scan(n + 1), kq(n), inner(n + 1), inner_scan(n + 1);
    std::vector<RbSeg> seg[2] = {std::vector<RbSeg>(n), std::vector<RbSeg>(n)};
    std::vector<unsigned long long> keys(6 * n);
    RbCounters cnt = {};
    tree.assign(2 * n, RtuBvhNode{});
    RbWork w = {};
    w.f = f; w.v = v; w.n = nf;
    w.el_in = el[0].data(); w.el_out = el[1].data();
    w.seg_of = seg_of.data(); w.flag = flag.data(); w.scan = scan.data(); w.kq = kq.data();
    w.seg = seg[0].data(); w.next = seg[1].data();
    w.inner = inner.data(); w.inner_scan = inner_scan.data();
    w.keys = keys.data(); w.tree = tree.data(); w.cnt = &cnt;
    HostExec ex;
    (void)rb_levels(ex, w, max_levels, out);
    tree.resize(out.n_bvh_nodes);
    elements.assign(w.el_in, w.el_in + n);
    unsigned long long vkeys[6];
    for (int i = 0; i < 3; i++) { vkeys[i] = RB_MIN_IDENTITY; vkeys[3 + i] = RB_MAX_IDENTITY; }
    float box[6];
    RbVertexBox vb = {v, nv, vkeys, box};
    for (uint32_t i = 0; i < nv; i++) rb_vertex_box_fold(vb, i);
    rb_vertex_box_finish(vb);
    memcpy(out.bmin, box, sizeof out.bmin);
    memcpy(out.bmax, box + 3, sizeof out.bmax);
}

void rb_normals_host(const uint32_t* f, const float* v, uint32_t nf, uint32_t nv, std::vector<float>& vn) {
    const uint32_t n3 = 3 * nf;
    std::vector<uint32_t> corners(n3), keys(n3);
    std::iota(corners.begin(), corners.end(), 0u);
    std::stable_sort(corners.begin(), corners.end(), [&](uint32_t a, uint32_t b) { return f[a] < f[b]; });
    for (uint32_t i = 0; i < n3; i++) keys[i] = f[corners[i]];
    vn.assign(3 * (size_t)nv, 0.0f);
    for (uint32_t i = 0; i < nv; i++) {
        uint32_t lo, hi;
        rb_vertex_range(keys.data(), n3, i, lo, hi);
        rb_vertex_normal(f, v, corners.data(), lo, hi, &vn[3 * (size_t)i]);
    }
}

void rb_partition_host(const uint8_t* keep, uint32_t n, uint32_t* perm_out) {
    std::vector<uint32_t> scan((size_t)n + 1), kq(n);
    uint32_t L = 0;
    for (uint32_t p = 0; p < n; p++) { scan[p] = L; L += keep[p] ? 1u : 0u; }
    scan[n] = L;
    for (uint32_t q = L; q < n; q++)
        if (keep[q]) kq[L - 1u - scan[q]] = q;
    for (uint32_t p = 0; p < n; p++) {
        uint32_t src, dst;
        rb_partition_rule(p, n, L, keep[p] != 0, scan[p], kq.data(), src, dst);
        if (src != RB_NONE) perm_out[p] = src;
        if (dst != RB_NONE) perm_out[dst] = p;
    }
}
