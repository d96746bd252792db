// rtu_scene_update.hip — the device builder of rtu_update_scene: the cover meshes (world-space faces of the masked mesh nodes) and
// the occluder lists of shadow rays, from the meshes already in HBM. The per-face arithmetic is rtu_lightlist.h, the same code the
// host builder (rtu_capi_build.hip compute_light_list) runs, so a list built here equals the host's entry for entry and bit for bit;
// the scalar decisions between the passes (frame, G, slack) run on the host on a few read-back doubles.
//
// One list on a G x G grid:
//   k_face_setup   one lane per face: its cells record (LlFaceCells) and the number of grid rows its rectangle spans
//   scan           rows -> the first (face, row) pair of every face
//   k_row_count    one lane per (face, row): the cells of that row the face enters (a big triangle is many lanes, not one long loop)
//   scan           -> where each (face, row)'s entries go; the total is read back (the 32 M cap halves G)
//   k_row_fill     the entries {key = cell << 32 | zmin as an ordered key, face}, in face order
//   radix sort     stable, by key: per cell ascending zmin, ties in face order — std::stable_sort of the host's face-order cells
//   k_cell_off     cell -> first entry (binary search), and the longest cell
//   k_entries      {slot of the fast tree, zmin bits} per entry
#include "rtu_devbuf.h"
#include "rtu_lightlist.h"

#include <hipcub/hipcub.hpp>

#include <cstring>
#include <vector>

namespace {

const int kBlock = 256;

// at least n elements, with slack: a buffer that grows gets n + n / 4 + 64
template <class T>
hipError_t grow(DevBuf<T>& b, size_t n) {
    if (n <= b.size() && b.get()) return hipSuccess;
    return b.grow(n + n / 4 + 64);
}

// a float's bits as an unsigned key in the order of float comparison: -0 and +0 are one key (they compare equal, so the face
// index decides, as in the host's stable sort). zmin is never NaN: NaN vertex coordinates drop out of its min, and a list whose
// boxes are not finite has no usable extent; -inf / +inf order as floats do.
__device__ __forceinline__ uint32_t zkey(uint32_t b) {
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ void k_cover_faces(const uint32_t* __restrict__ f, const float* __restrict__ v, uint32_t nf, LlChain chain, double* __restrict__ verts,
                              float4* __restrict__ boxes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const uint32_t a = f[3 * (size_t)i], b = f[3 * (size_t)i + 1], c = f[3 * (size_t)i + 2];
    double w[9];
    float4 lo, hi;
    ll_cover_face(chain, v + 3 * (size_t)a, v + 3 * (size_t)b, v + 3 * (size_t)c, w, lo, hi);
    for (int k = 0; k < 9; k++) verts[9 * (size_t)i + k] = w[k];
    boxes[2 * (size_t)i] = lo;
    boxes[2 * (size_t)i + 1] = hi;
}

struct CoverSet {
    const float4* boxes[RTU_MAX_COVER];
    uint32_t nf[RTU_MAX_COVER];
};

// per cover node (one block each): lo / hi of its face boxes, as the host's sequential std::min / std::max makes them — of values that
// compare equal the first face's (the sign of a zero)
__global__ void __launch_bounds__(kBlock) k_box_extent(CoverSet cs, double* __restrict__ out) {
    __shared__ double sv[6][kBlock];
    __shared__ int32_t si[6][kBlock];
    const int c = blockIdx.x, t = threadIdx.x;
    double v[6] = {1e300, 1e300, 1e300, -1e300, -1e300, -1e300};
    int32_t id[6] = {-1, -1, -1, -1, -1, -1};
    for (uint32_t f = t; f < cs.nf[c]; f += kBlock) {
        const float4 a = cs.boxes[c][2 * (size_t)f], b = cs.boxes[c][2 * (size_t)f + 1];
        const double al[3] = {a.x, a.y, a.z}, bh[3] = {b.x, b.y, b.z};
        for (int k = 0; k < 3; k++) {
            if (al[k] < v[k]) { v[k] = al[k]; id[k] = (int32_t)f; }
            if (v[3 + k] < bh[k]) { v[3 + k] = bh[k]; id[3 + k] = (int32_t)f; }
        }
    }
    for (int k = 0; k < 6; k++) { sv[k][t] = v[k]; si[k][t] = id[k]; }
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < 6; k++) {
                const double a = sv[k][t], b = sv[k][t + s];
                const int32_t ia = si[k][t], ib = si[k][t + s];
                const bool take = (k < 3 ? b < a : a < b) || (a == b && ib < ia);
                if (take) { sv[k][t] = b; si[k][t] = ib; }
            }
        __syncthreads();
    }
    if (t < 6) out[6 * c + t] = sv[t][0];
}

// per (light, cover node) pair (one block each): U0, U1, V0, V1, ratio, ok of the corner pass (the signs of zeros in U / V do not
// reach the list: only differences and magnitudes of them do)
__global__ void __launch_bounds__(kBlock) k_corner_extent(CoverSet cs, const int* __restrict__ pair_cover, const LlFrame* __restrict__ frames, float wscale,
                                                          double* __restrict__ out) {
    __shared__ double sv[5][kBlock];
    __shared__ int sok[kBlock];
    const int p = blockIdx.x, t = threadIdx.x;
    const int c = pair_cover[p];
    const LlFrame F = frames[p];
    double U0 = 1e300, U1 = -1e300, V0 = 1e300, V1 = -1e300, ratio = 1.0;
    bool ok = true;
    for (uint32_t f = t; f < cs.nf[c] && ok; f += kBlock) {
        const float4 a = cs.boxes[c][2 * (size_t)f], b = cs.boxes[c][2 * (size_t)f + 1];
        ok = ll_face_corners(a, b, ll_face_wid(a, b, wscale), F, U0, U1, V0, V1, ratio);
    }
    sv[0][t] = U0; sv[1][t] = U1; sv[2][t] = V0; sv[3][t] = V1; sv[4][t] = ratio; sok[t] = ok ? 1 : 0;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) {
            sv[0][t] = ll_min(sv[0][t], sv[0][t + s]); sv[1][t] = ll_max(sv[1][t], sv[1][t + s]);
            sv[2][t] = ll_min(sv[2][t], sv[2][t + s]); sv[3][t] = ll_max(sv[3][t], sv[3][t + s]);
            sv[4][t] = ll_max(sv[4][t], sv[4][t + s]); sok[t] = sok[t] & sok[t + s];
        }
        __syncthreads();
    }
    if (t < 5) out[6 * p + t] = sv[t][0];
    if (t == 5) out[6 * p + 5] = sok[0] ? 1.0 : 0.0;
}

__global__ void k_face_setup(const double* __restrict__ verts, const float4* __restrict__ boxes, uint32_t nf, LlFrame F, LlGrid g, float wscale,
                             LlFaceCells* __restrict__ cells, unsigned long long* __restrict__ rows) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) rows[nf] = 0;
    if (i >= nf) return;
    LlFaceCells c;
    ll_face_cells(verts + 9 * (size_t)i, ll_face_wid(boxes[2 * (size_t)i], boxes[2 * (size_t)i + 1], wscale), F, g, wscale, c);
    cells[i] = c;
    rows[i] = (c.x1 >= c.x0 && c.y1 >= c.y0) ? (unsigned long long)(c.y1 - c.y0 + 1) : 0ull;
}

// the face of (face, row) pair r: the last face whose first pair is <= r
__device__ __forceinline__ uint32_t face_of(const unsigned long long* __restrict__ start, uint32_t nf, unsigned long long r) {
    uint32_t lo = 0, hi = nf;  // start[lo] <= r < start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (start[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void k_row_count(const unsigned long long* __restrict__ row_start, uint32_t nf, unsigned long long R, const LlFaceCells* __restrict__ cells,
                            unsigned long long* __restrict__ cnt) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long r = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; r < R; r += stride) {
        const uint32_t f = face_of(row_start, nf, r);
        const LlFaceCells& c = cells[f];
        const int y = c.y0 + (int)(r - row_start[f]);
        unsigned long long n = 0;
        for (int x = c.x0; x <= c.x1; x++) n += ll_cell_in(c, x, y) ? 1u : 0u;
        cnt[r] = n;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[R] = 0;
}

__global__ void k_row_fill(const unsigned long long* __restrict__ row_start, uint32_t nf, unsigned long long R, const LlFaceCells* __restrict__ cells,
                           uint32_t G, const unsigned long long* __restrict__ ent_start, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long r = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; r < R; r += stride) {
        const uint32_t f = face_of(row_start, nf, r);
        const LlFaceCells& c = cells[f];
        const int y = c.y0 + (int)(r - row_start[f]);
        const unsigned long long zk = zkey(c.zbits);
        unsigned long long at = ent_start[r];
        for (int x = c.x0; x <= c.x1; x++)
            if (ll_cell_in(c, x, y)) {
                keys[at] = ((unsigned long long)((uint32_t)y * G + (uint32_t)x) << 32) | zk;
                vals[at] = f;
                at++;
            }
    }
}

__device__ __forceinline__ uint32_t first_of_cell(const unsigned long long* __restrict__ keys, uint32_t E, uint32_t cell) {
    const unsigned long long k = (unsigned long long)cell << 32;
    uint32_t lo = 0, hi = E;  // first entry with key >= k
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_cell_off(const unsigned long long* __restrict__ keys, uint32_t E, uint32_t cells, uint32_t* __restrict__ cell_off, uint32_t* __restrict__ longest) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > cells) return;
    const uint32_t b = first_of_cell(keys, E, c);
    cell_off[c] = b;
    if (c < cells) {
        const uint32_t e = first_of_cell(keys, E, c + 1);
        if (e - b > 0) atomicMax(longest, e - b);
    }
}

__global__ void k_entries(const uint32_t* __restrict__ faces, uint32_t E, const uint32_t* __restrict__ slot_of, const LlFaceCells* __restrict__ cells,
                          uint32_t* __restrict__ cell_tri) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    const uint32_t f = faces[i];
    cell_tri[2 * (size_t)i] = slot_of[f];
    cell_tri[2 * (size_t)i + 1] = cells[f].zbits;
}

uint32_t blocks_for(size_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }
uint32_t blocks_capped(unsigned long long n) { const unsigned long long b = (n + kBlock - 1) / kBlock; return (uint32_t)(b < 65536ull ? (b ? b : 1) : 65536ull); }

}  // namespace

struct LlBuilder {
    DevBuf<double> verts[RTU_MAX_COVER];  // per cover node: 9 doubles per face (world-space vertices)
    DevBuf<double> red;                   // reductions (6 doubles per cover node / pair)
    DevBuf<LlFrame> frames;
    DevBuf<int> pair_cover;
    DevBuf<LlFaceCells> cells;            // of the list being built
    DevBuf<unsigned long long> rows;      // [nf + 1] rows per face, then its first (face, row) pair
    DevBuf<unsigned long long> row_start;
    DevBuf<unsigned long long> cnt;       // [R + 1] entries per (face, row), then where they go
    DevBuf<unsigned long long> ent_start;
    DevBuf<unsigned long long> keys[2];
    DevBuf<uint32_t> vals[2];
    DevBuf<char> tmp;                     // hipcub's temporary storage
    DevBuf<uint32_t> longest;
    // the list counted last
    uint32_t cur_nf = 0, cur_E = 0;
    int      cur_cover = -1;
    unsigned long long cur_R = 0;
    bool timing = false;
    hipEvent_t ev[2] = {};
    LlTimes t{};
};

namespace {

hipError_t tick(LlBuilder* b, hipStream_t st) { return b->timing ? hipEventRecord(b->ev[0], st) : hipSuccess; }
hipError_t tock(LlBuilder* b, hipStream_t st, float* acc) {
    if (!b->timing) return hipSuccess;
    hipError_t e;
    if ((e = hipEventRecord(b->ev[1], st)) != hipSuccess) return e;
    if ((e = hipEventSynchronize(b->ev[1])) != hipSuccess) return e;
    float ms = 0;
    if ((e = hipEventElapsedTime(&ms, b->ev[0], b->ev[1])) != hipSuccess) return e;
    *acc += ms;
    return hipSuccess;
}

// exclusive sum of n + 1 values (the last one 0): out[n] is the total
hipError_t scan(LlBuilder* b, hipStream_t st, const unsigned long long* in, unsigned long long* out, size_t n1) {
    size_t bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, n1, st);
    if (e != hipSuccess) return e;
    if ((e = grow(b->tmp, bytes)) != hipSuccess) return e;
    bytes = b->tmp.size();
    return hipcub::DeviceScan::ExclusiveSum(b->tmp.get(), bytes, in, out, n1, st);
}

CoverSet cover_set(const LlCover* covers, int n) {
    CoverSet cs;
    memset(&cs, 0, sizeof cs);
    for (int c = 0; c < n && c < RTU_MAX_COVER; c++) { cs.boxes[c] = covers[c].boxes; cs.nf[c] = covers[c].nf; }
    return cs;
}

}  // namespace

#define LL_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

LlBuilder* ll_builder_create() { return new LlBuilder; }

void ll_builder_destroy(LlBuilder* b) {
    if (!b) return;
    for (hipEvent_t e : b->ev) if (e) (void)hipEventDestroy(e);
    delete b;
}

void ll_set_timing(LlBuilder* b, bool on) {
    if (on && !b->ev[0]) {
        if (hipEventCreate(&b->ev[0]) != hipSuccess || hipEventCreate(&b->ev[1]) != hipSuccess) return;
    }
    b->timing = on;
}

void ll_get_times(LlBuilder* b, LlTimes* out, bool reset) {
    if (out) *out = b->t;
    if (reset) memset(&b->t, 0, sizeof b->t);
}

hipError_t ll_build_covers(LlBuilder* b, hipStream_t st, const LlCover* covers, int n_cover, double* lohi_out) {
    if (n_cover <= 0) return hipSuccess;
    LL_TRY(tick(b, st));
    for (int c = 0; c < n_cover; c++) {
        const LlCover& cv = covers[c];
        LL_TRY(grow(b->verts[c], (size_t)cv.nf * 9));
        k_cover_faces<<<blocks_for(cv.nf), kBlock, 0, st>>>(cv.f, cv.v, cv.nf, cv.chain, b->verts[c].get(), cv.boxes);
        LL_TRY(hipGetLastError());
    }
    LL_TRY(grow(b->red, (size_t)6 * RTU_LMASK_LIGHTS * RTU_MAX_COVER));
    k_box_extent<<<n_cover, kBlock, 0, st>>>(cover_set(covers, n_cover), b->red.get());
    LL_TRY(hipGetLastError());
    LL_TRY(hipMemcpyAsync(lohi_out, b->red.get(), sizeof(double) * 6 * n_cover, hipMemcpyDeviceToHost, st));
    LL_TRY(hipStreamSynchronize(st));
    return tock(b, st, &b->t.cover_ms);
}

hipError_t ll_build_extents(LlBuilder* b, hipStream_t st, const LlCover* covers, const int* pair_cover, const LlFrame* frames, int n_pairs, float wscale,
                            double* out6) {
    if (n_pairs <= 0) return hipSuccess;
    LL_TRY(tick(b, st));
    int n_cover = 0;
    for (int p = 0; p < n_pairs; p++) n_cover = pair_cover[p] + 1 > n_cover ? pair_cover[p] + 1 : n_cover;
    LL_TRY(grow(b->frames, (size_t)n_pairs));
    LL_TRY(grow(b->pair_cover, (size_t)n_pairs));
    LL_TRY(grow(b->red, (size_t)6 * n_pairs));
    LL_TRY(hipMemcpyAsync(b->frames.get(), frames, sizeof(LlFrame) * n_pairs, hipMemcpyHostToDevice, st));
    LL_TRY(hipMemcpyAsync(b->pair_cover.get(), pair_cover, sizeof(int) * n_pairs, hipMemcpyHostToDevice, st));
    k_corner_extent<<<n_pairs, kBlock, 0, st>>>(cover_set(covers, n_cover), b->pair_cover.get(), b->frames.get(), wscale, b->red.get());
    LL_TRY(hipGetLastError());
    LL_TRY(hipMemcpyAsync(out6, b->red.get(), sizeof(double) * 6 * n_pairs, hipMemcpyDeviceToHost, st));
    LL_TRY(hipStreamSynchronize(st));
    return tock(b, st, &b->t.extent_ms);
}

hipError_t ll_count(LlBuilder* b, hipStream_t st, const LlCover& cv, int cover_index, const LlFrame& F, const LlGrid& g, float wscale, size_t* entries_out) {
    LL_TRY(tick(b, st));
    const uint32_t nf = cv.nf;
    LL_TRY(grow(b->cells, (size_t)nf));
    LL_TRY(grow(b->rows, (size_t)nf + 1));
    LL_TRY(grow(b->row_start, (size_t)nf + 1));
    k_face_setup<<<blocks_for(nf), kBlock, 0, st>>>(b->verts[cover_index].get(), cv.boxes, nf, F, g, wscale, b->cells.get(), b->rows.get());
    LL_TRY(hipGetLastError());
    LL_TRY(scan(b, st, b->rows.get(), b->row_start.get(), (size_t)nf + 1));
    unsigned long long R = 0;
    LL_TRY(hipMemcpyAsync(&R, b->row_start.get() + nf, sizeof R, hipMemcpyDeviceToHost, st));
    LL_TRY(hipStreamSynchronize(st));
    LL_TRY(grow(b->cnt, (size_t)R + 1));
    LL_TRY(grow(b->ent_start, (size_t)R + 1));
    k_row_count<<<blocks_capped(R), kBlock, 0, st>>>(b->row_start.get(), nf, R, b->cells.get(), b->cnt.get());
    LL_TRY(hipGetLastError());
    LL_TRY(scan(b, st, b->cnt.get(), b->ent_start.get(), (size_t)R + 1));
    unsigned long long E = 0;
    LL_TRY(hipMemcpyAsync(&E, b->ent_start.get() + R, sizeof E, hipMemcpyDeviceToHost, st));
    LL_TRY(hipStreamSynchronize(st));
    b->cur_nf = nf;
    b->cur_R = R;
    b->cur_E = E > RTU_LLIST_MAX_ENTRIES ? 0u : (uint32_t)E;
    b->cur_cover = cover_index;
    b->t.passes++;
    *entries_out = (size_t)E;
    return tock(b, st, &b->t.count_ms);
}

hipError_t ll_fill(LlBuilder* b, hipStream_t st, const LlCover& cv, const LlGrid& g, uint32_t* cell_off, uint32_t* cell_tri, uint32_t* longest_out) {
    LL_TRY(tick(b, st));
    const uint32_t E = b->cur_E, cells = g.G * g.G;
    for (int k = 0; k < 2; k++) {
        LL_TRY(grow(b->keys[k], (size_t)E + 1));
        LL_TRY(grow(b->vals[k], (size_t)E + 1));
    }
    LL_TRY(grow(b->longest, 1));
    LL_TRY(hipMemsetAsync(b->longest.get(), 0, sizeof(uint32_t), st));
    if (b->cur_R)
        k_row_fill<<<blocks_capped(b->cur_R), kBlock, 0, st>>>(b->row_start.get(), b->cur_nf, b->cur_R, b->cells.get(), g.G, b->ent_start.get(), b->keys[0].get(), b->vals[0].get());
    LL_TRY(hipGetLastError());
    LL_TRY(tock(b, st, &b->t.fill_ms));
    LL_TRY(tick(b, st));
    int end_bit = 32;
    while ((1u << (end_bit - 32)) < cells) end_bit++;
    hipcub::DoubleBuffer<unsigned long long> kb(b->keys[0].get(), b->keys[1].get());
    hipcub::DoubleBuffer<uint32_t> vb(b->vals[0].get(), b->vals[1].get());
    if (E > 1) {
        size_t bytes = 0;
        LL_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, kb, vb, (int)E, 0, end_bit, st));
        LL_TRY(grow(b->tmp, bytes));
        bytes = b->tmp.size();
        LL_TRY(hipcub::DeviceRadixSort::SortPairs(b->tmp.get(), bytes, kb, vb, (int)E, 0, end_bit, st));
    }
    LL_TRY(tock(b, st, &b->t.sort_ms));
    LL_TRY(tick(b, st));
    k_cell_off<<<blocks_for((size_t)cells + 1), kBlock, 0, st>>>(kb.Current(), E, cells, cell_off, b->longest.get());
    LL_TRY(hipGetLastError());
    if (E) k_entries<<<blocks_for(E), kBlock, 0, st>>>(vb.Current(), E, cv.slot_of, b->cells.get(), cell_tri);
    LL_TRY(hipGetLastError());
    LL_TRY(hipMemcpyAsync(longest_out, b->longest.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LL_TRY(hipStreamSynchronize(st));
    b->t.lists++;
    return tock(b, st, &b->t.fill_ms);
}
