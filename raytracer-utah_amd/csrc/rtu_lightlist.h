// rtu_lightlist.h — the arithmetic of the occluder lists of shadow rays (rtu_device.h DevLightMask), shared by the host builder
// (rtu_capi_build.hip compute_light_list, used by rtu_upload_scene) and the device builder (rtu_scene_update.hip, used by
// rtu_update_scene). Both run the same expressions in binary64 with -ffp-contract=off, so both build the same lists bit for bit.
//   * per-face pieces (RTU_HD): the cover mesh of a face, its widened box in the light's (u, v), its cells and its zmin;
//   * scalar decisions (host): the light's frame, the grid size G and the slack S0.
// Not included by the render kernels.
#pragma once
#include "rtu_device.h"

#include <climits>
#include <cmath>

// std::min / std::max exactly: the first argument wins a tie (signed zeros) and a NaN second argument is dropped
RTU_HD double ll_min(double a, double b) { return (b < a) ? b : a; }
RTU_HD double ll_max(double a, double b) { return (a < b) ? b : a; }
// (int)std::floor(x) as x86-64 converts it (cvttsd2si): INT_MIN for NaN and for anything outside int's range
RTU_HD int ll_floor_int(double x) {
    const double f = ::floor(x);
    if (!(f >= -2147483648.0 && f <= 2147483647.0)) return INT_MIN;
    return (int)f;
}

// the chain of transformations of a node, self first, root last (make_cover_mesh: p -> tm p + pos in binary64)
struct LlChain {
    int32_t n;
    float   tm[RTU_MAX_NODE_DEPTH][9];
    float   pos[RTU_MAX_NODE_DEPTH][3];
};

// one face of a cover mesh: its three world-space vertices and its box rounded outwards
RTU_HD void ll_cover_face(const LlChain& c, const float* v0, const float* v1, const float* v2, double* w9, float4& lo4, float4& hi4) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    const float* vs[3] = {v0, v1, v2};
    for (int v = 0; v < 3; v++) {
        double p[3] = {vs[v][0], vs[v][1], vs[v][2]};
        for (int j = 0; j < c.n; j++) {
            const float* tm = c.tm[j];
            const float* pos = c.pos[j];
            const double q[3] = {p[0] * tm[0] + p[1] * tm[3] + p[2] * tm[6] + pos[0], p[0] * tm[1] + p[1] * tm[4] + p[2] * tm[7] + pos[1],
                                 p[0] * tm[2] + p[1] * tm[5] + p[2] * tm[8] + pos[2]};
            p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
        }
        for (int k = 0; k < 3; k++) { lo[k] = ll_min(lo[k], p[k]); hi[k] = ll_max(hi[k], p[k]); w9[3 * v + k] = p[k]; }
    }
    lo4 = make_float4(::nextafterf((float)lo[0], -INFINITY), ::nextafterf((float)lo[1], -INFINITY), ::nextafterf((float)lo[2], -INFINITY), 0.0f);
    hi4 = make_float4(::nextafterf((float)hi[0], INFINITY), ::nextafterf((float)hi[1], INFINITY), ::nextafterf((float)hi[2], INFINITY), 0.0f);
}

// the light's frame: L its position (point) or 0, Z towards the mesh (point) or its direction, X and Y across
struct LlFrame {
    double L[3], X[3], Y[3], Z[3];
    int32_t point, pad;
};

// the cull margin of a face (a displacement of wid on every axis covers the ray's rounding)
RTU_HD double ll_face_wid(const float4& a, const float4& b, float wscale) {
    const double al[3] = {a.x, a.y, a.z}, bh[3] = {b.x, b.y, b.z};
    double big = 0;
    for (int k = 0; k < 3; k++) big = ll_max(big, ll_max(::fabs(al[k]), ::fabs(bh[k])));
    return 1e-4 * (double)wscale + 1e-5 * big;
}

// the corners of a face's widened box in the light's (u, v), folded into U0..V1 and ratio; false: a corner is not in front of
// the pinhole (the list is unusable)
RTU_HD bool ll_face_corners(const float4& a, const float4& b, double wid, const LlFrame& F, double& U0, double& U1, double& V0, double& V1, double& ratio) {
    const double al[3] = {a.x, a.y, a.z}, bh[3] = {b.x, b.y, b.z};
    const double* L = F.L;
    const double* X = F.X;
    const double* Y = F.Y;
    const double* Z = F.Z;
    for (int cn = 0; cn < 8; cn++) {
        const double q[3] = {((cn & 1) ? bh[0] + wid : al[0] - wid) - L[0], ((cn & 2) ? bh[1] + wid : al[1] - wid) - L[1],
                             ((cn & 4) ? bh[2] + wid : al[2] - wid) - L[2]};
        double u = q[0] * X[0] + q[1] * X[1] + q[2] * X[2], v = q[0] * Y[0] + q[1] * Y[1] + q[2] * Y[2];
        if (F.point) {
            const double depth = q[0] * Z[0] + q[1] * Z[1] + q[2] * Z[2];
            const double len = ::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
            if (!(depth > 1e-3 * len)) return false;  // (within 89.94 degrees of the axis: tan stays below 1000)
            ratio = ll_max(ratio, len / depth);
            u /= depth; v /= depth;
        }
        U0 = ll_min(U0, u); U1 = ll_max(U1, u); V0 = ll_min(V0, v); V1 = ll_max(V1, v);
    }
    return true;
}

// the grid: G x G cells spanning the extent plus two cells on every side, and the slack S0 every face gets
struct LlGrid {
    double du, dv, gu0, gv0, S0;
    uint32_t G, pad;
};

// one face on the grid: its vertices in cells, the rectangle of cells its widened projection may touch, its edges as separating
// lines and the depth zmin (float bits) in front of which an origin cannot see it
struct LlFaceCells {
    double pu[3], pv[3], nx[3], ny[3], nd[3];
    int32_t x0, x1, y0, y1;
    uint32_t edges, zbits;
};

RTU_HD void ll_face_cells(const double* w, double wid, const LlFrame& F, const LlGrid& g, float wscale, LlFaceCells& c) {
    const double r3 = 1.7320508075688772;
    const double* L = F.L;
    const double* X = F.X;
    const double* Y = F.Y;
    const double* Z = F.Z;
    double dmin = 1e300, umax = 0, vmax = 0;
    for (int k = 0; k < 3; k++) {
        const double q[3] = {w[3 * k] - L[0], w[3 * k + 1] - L[1], w[3 * k + 2] - L[2]};
        double u = q[0] * X[0] + q[1] * X[1] + q[2] * X[2], v = q[0] * Y[0] + q[1] * Y[1] + q[2] * Y[2];
        if (F.point) {
            const double depth = q[0] * Z[0] + q[1] * Z[1] + q[2] * Z[2];
            dmin = ll_min(dmin, depth);
            u /= depth; v /= depth;
        }
        c.pu[k] = (u - g.gu0) / g.du; c.pv[k] = (v - g.gv0) / g.dv;  // in cells
        umax = ll_max(umax, ::fabs(u)); vmax = ll_max(vmax, ::fabs(v));
    }
    const double wd = wid * r3;
    double Su, Sv;
    if (F.point) { Su = wd * (1.0 + umax) / (dmin - wd) / g.du; Sv = wd * (1.0 + vmax) / (dmin - wd) / g.dv; }  // (dmin > wd: the box corners passed)
    else { Su = wd / g.du; Sv = wd / g.dv; }
    const double S = g.S0 + ll_max(Su, Sv);
    const double* pu = c.pu;
    const double* pv = c.pv;
    const double bu0 = ll_min(pu[0], ll_min(pu[1], pu[2])) - S, bu1 = ll_max(pu[0], ll_max(pu[1], pu[2])) + S;
    const double bv0 = ll_min(pv[0], ll_min(pv[1], pv[2])) - S, bv1 = ll_max(pv[0], ll_max(pv[1], pv[2])) + S;
    int x0 = ll_floor_int(bu0), x1 = ll_floor_int(bu1), y0 = ll_floor_int(bv0), y1 = ll_floor_int(bv1);
    x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
    x1 = x1 < (int)g.G - 1 ? x1 : (int)g.G - 1; y1 = y1 < (int)g.G - 1 ? y1 : (int)g.G - 1;
    c.x0 = x0; c.x1 = x1; c.y0 = y0; c.y1 = y1;
    // the triangle's edges as separating lines: a cell (a square of half-width 0.5 + S about its centre) lies beyond edge i when
    // n_i . (centre - v_i) > (|n_i.x| + |n_i.y|) (0.5 + S), n_i the outward normal
    const double area2 = (pu[1] - pu[0]) * (pv[2] - pv[0]) - (pu[2] - pu[0]) * (pv[1] - pv[0]);
    c.edges = ::fabs(area2) > 1e-9 ? 1u : 0u;  // (an edge-on triangle has no inside: its bounding box is all there is)
    for (int i = 0; i < 3; i++) {
        const int k = (i + 1) % 3;
        const double ex = pu[k] - pu[i], ey = pv[k] - pv[i];
        const double sg = area2 > 0 ? 1.0 : -1.0;
        c.nx[i] = sg * ey; c.ny[i] = -sg * ex;  // outward for a counter-clockwise triangle (area2 > 0)
        c.nd[i] = (::fabs(c.nx[i]) + ::fabs(c.ny[i])) * (0.5 + S);
    }
    // every point of the triangle, the cull margin and the rounding of the device's own depth included, lies beyond zmin
    double zmin = 1e300;
    for (int k = 0; k < 3; k++) zmin = ll_min(zmin, (w[3 * k] - L[0]) * Z[0] + (w[3 * k + 1] - L[1]) * Z[1] + (w[3 * k + 2] - L[2]) * Z[2]);
    zmin -= wd + 8e-6 * (r3 * (double)wscale + ::fabs(L[0]) + ::fabs(L[1]) + ::fabs(L[2]));
    float zf = (float)zmin;
    if ((double)zf > zmin) zf = ::nextafterf(zf, -INFINITY);
    uint32_t zb;
    __builtin_memcpy(&zb, &zf, 4);
    c.zbits = zb;
}

RTU_HD bool ll_cell_in(const LlFaceCells& c, int x, int y) {
    if (c.edges)
        for (int i = 0; i < 3; i++)
            if (c.nx[i] * ((double)x + 0.5 - c.pu[i]) + c.ny[i] * ((double)y + 0.5 - c.pv[i]) > c.nd[i]) return false;
    return true;
}

// ---- scalar decisions (host) ---------------------------------------------------------------------------------------------
#define RTU_LLIST_MAX_ENTRIES ((size_t)32 << 20)  // G is halved while the lists would hold more

// the frame of light l looking at a mesh whose face boxes span [lo, hi]; false: no usable direction
bool ll_frame(const RtuLight& l, const double lo[3], const double hi[3], LlFrame& F);
// the largest G to try for a mesh of nf faces (RTU_LGRID_SPAN: tuning knob, any value renders the same image)
uint32_t ll_first_grid(size_t nf);
// the extent check after the corner pass: false: no extent a float lookup could resolve
bool ll_extent_ok(double U0, double U1, double V0, double V1, double& mag);
// the grid of size G for that extent; false: the binary32 cell coordinate is not good to a quarter of a cell at this G
bool ll_grid_at(uint32_t G, double U0, double U1, double V0, double V1, double ratio, double mag, LlGrid& g);
// the list's device header from frame and grid (cell_off / cell_tri stay null)
void ll_mask(const LlFrame& F, const LlGrid& g, DevLightMask& m);

// the device builder (rtu_scene_update.hip): per cover node its world-space faces, per (light, cover node) its list
struct LlBuilder;
struct LlCover {                   // one cover node
    const uint32_t* f;             // device: the mesh's faces and vertices (DevMesh::f / ::v)
    const float*    v;
    const uint32_t* slot_of;       // device: face -> slot of the fast tree's leaf order
    uint32_t nf;
    LlChain chain;
    float4* boxes;                 // device, [2 nf]: written (the DevScene::cover_box buffer)
};
struct LlTimes { float cover_ms, extent_ms, count_ms, fill_ms, sort_ms; int lists, passes; };
LlBuilder* ll_builder_create();
void ll_builder_destroy(LlBuilder* b);
// world-space faces of every cover node and the box extents of each (lo[3], hi[3] per node, read back); hipSuccess or the error
hipError_t ll_build_covers(LlBuilder* b, hipStream_t st, const LlCover* covers, int n_cover, double* lohi_out);
// U0, U1, V0, V1, ratio, ok of every (frame, cover node) pair of `pairs` (cover index per pair), read back
hipError_t ll_build_extents(LlBuilder* b, hipStream_t st, const LlCover* covers, const int* pair_cover, const LlFrame* frames, int n_pairs,
                            float wscale, double* out6);
// count the entries of one list on grid g: *entries_out (read back)
hipError_t ll_count(LlBuilder* b, hipStream_t st, const LlCover& cv, int cover_index, const LlFrame& F, const LlGrid& g, float wscale, size_t* entries_out);
// fill the list counted last into cell_off [G G + 1] and cell_tri [2 entries] (device buffers of the caller); *longest_out: entries
// of the longest cell (read back)
hipError_t ll_fill(LlBuilder* b, hipStream_t st, const LlCover& cv, const LlGrid& g, uint32_t* cell_off, uint32_t* cell_tri, uint32_t* longest_out);
// phase times of the builder's work since the last reset (HIP events; only when timing is on)
void ll_set_timing(LlBuilder* b, bool on);
void ll_get_times(LlBuilder* b, LlTimes* out, bool reset);
