// rtu_capi_build.hip — what an upload builds on the host, without a GPU: the binned-SAH tree of a mesh and its wide-4 / wide-8
// collapses, the world bounds and the margins that grow with a scene's extent, and the occluder lists of shadow rays (with the
// scalar decisions of rtu_lightlist.h that the device builder shares). Pure host code, called by the upload and update entries of
// rtu_capi.hip; compiled like it with -ffp-contract=off.
#include "rtu_capi.h"
#include "rtu_meshrec.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

// ---- binned-SAH BVH over a mesh's triangles (the `fast` tree of DevMesh) -------------------
// Breadth-first node numbering with adjacent sibling pairs, root = node 1, node 0 unused —
// the layout the kernels expect. Leaves hold <= 4 triangles. Box bounds are the exact
// min/max of the vertex coordinates (no arithmetic), like cy::BVH's.
void build_sah(const RtuMesh& m, SahTree& out) {
    const uint32_t nf = m.nf;
    const uint32_t max_leaf = 4;  // leaves of the one-lane-per-ray walk; the cooperative walk merges subtrees of <= 8 (build_wide8)
    std::vector<float> bmin(3 * (size_t)nf), bmax(3 * (size_t)nf), cen(3 * (size_t)nf);
    for (uint32_t i = 0; i < nf; i++) {
        const uint32_t* fv = m.f + 3 * i;
        for (int k = 0; k < 3; k++) {
            float a = m.v[3 * fv[0] + k], b = m.v[3 * fv[1] + k], c = m.v[3 * fv[2] + k];
            float lo = a < b ? (a < c ? a : c) : (b < c ? b : c);
            float hi = a > b ? (a > c ? a : c) : (b > c ? b : c);
            bmin[3 * i + k] = lo; bmax[3 * i + k] = hi; cen[3 * i + k] = 0.5f * (lo + hi);
        }
    }
    std::vector<uint32_t> idx(nf);
    for (uint32_t i = 0; i < nf; i++) idx[i] = i;
    struct Job { uint32_t begin, end, id, level; };
    out.nodes.assign(2, RtuBvhNode{});
    out.elements.clear();
    std::vector<Job> queue;
    queue.push_back({0, nf, 1, 1});
    auto area = [](const float* lo, const float* hi) {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    };
    for (size_t qi = 0; qi < queue.size(); qi++) {
        const Job j = queue[qi];
        float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f}, clo[3] = {1e30f, 1e30f, 1e30f}, chi[3] = {-1e30f, -1e30f, -1e30f};
        for (uint32_t t = j.begin; t < j.end; t++)
            for (int k = 0; k < 3; k++) {
                uint32_t f = idx[t];
                if (bmin[3 * f + k] < lo[k]) lo[k] = bmin[3 * f + k];
                if (bmax[3 * f + k] > hi[k]) hi[k] = bmax[3 * f + k];
                if (cen[3 * f + k] < clo[k]) clo[k] = cen[3 * f + k];
                if (cen[3 * f + k] > chi[k]) chi[k] = cen[3 * f + k];
            }
        if (out.nodes.size() <= j.id) out.nodes.resize(j.id + 1, RtuBvhNode{});
        RtuBvhNode n{};
        for (int k = 0; k < 3; k++) { n.bmin[k] = lo[k]; n.bmax[k] = hi[k]; }
        if (j.level > out.depth) out.depth = j.level;
        const uint32_t count = j.end - j.begin;
        if (count <= max_leaf) {
            n.index = (uint32_t)out.elements.size();
            n.count = count;
            for (uint32_t t = j.begin; t < j.end; t++) out.elements.push_back(idx[t]);
            out.nodes[j.id] = n;
            continue;
        }
        // best binned split over the three axes
        const int NB = 16;
        int bestAxis = -1, bestBin = 0;
        float bestCost = 3.0e38f;
        for (int ax = 0; ax < 3; ax++) {
            float ext = chi[ax] - clo[ax];
            if (!(ext > 0)) continue;
            uint32_t cnt[NB] = {};
            float blo[NB][3], bhi[NB][3];
            for (int b = 0; b < NB; b++) for (int k = 0; k < 3; k++) { blo[b][k] = 1e30f; bhi[b][k] = -1e30f; }
            for (uint32_t t = j.begin; t < j.end; t++) {
                uint32_t f = idx[t];
                int b = (int)((cen[3 * f + ax] - clo[ax]) / ext * NB);
                if (b >= NB) b = NB - 1;
                if (b < 0) b = 0;
                cnt[b]++;
                for (int k = 0; k < 3; k++) {
                    if (bmin[3 * f + k] < blo[b][k]) blo[b][k] = bmin[3 * f + k];
                    if (bmax[3 * f + k] > bhi[b][k]) bhi[b][k] = bmax[3 * f + k];
                }
            }
            // sweep: left = bins [0,s], right = (s,NB)
            float rArea[NB];
            uint32_t rCnt[NB];
            {
                float rl[3] = {1e30f, 1e30f, 1e30f}, rh[3] = {-1e30f, -1e30f, -1e30f};
                uint32_t rc = 0;
                for (int b = NB - 1; b > 0; b--) {
                    for (int k = 0; k < 3; k++) { if (blo[b][k] < rl[k]) rl[k] = blo[b][k]; if (bhi[b][k] > rh[k]) rh[k] = bhi[b][k]; }
                    rc += cnt[b];
                    rArea[b] = rc ? area(rl, rh) : 0.0f;
                    rCnt[b] = rc;
                }
            }
            float ll[3] = {1e30f, 1e30f, 1e30f}, lh[3] = {-1e30f, -1e30f, -1e30f};
            uint32_t lc = 0;
            for (int sI = 0; sI < NB - 1; sI++) {
                for (int k = 0; k < 3; k++) { if (blo[sI][k] < ll[k]) ll[k] = blo[sI][k]; if (bhi[sI][k] > lh[k]) lh[k] = bhi[sI][k]; }
                lc += cnt[sI];
                if (lc == 0 || rCnt[sI + 1] == 0) continue;
                float cost = area(ll, lh) * (float)lc + rArea[sI + 1] * (float)rCnt[sI + 1];
                if (cost < bestCost) { bestCost = cost; bestAxis = ax; bestBin = sI; }
            }
        }
        uint32_t mid;
        if (j.level > 28) bestAxis = -1;  // a degenerate distribution must not cost unbounded depth: halve from here on
        if (bestAxis < 0) {
            mid = j.begin + count / 2;  // all centroids coincide: split the list in half
        } else {
            float ext = chi[bestAxis] - clo[bestAxis];
            uint32_t i = j.begin, e = j.end;
            while (i < e) {
                uint32_t f = idx[i];
                int b = (int)((cen[3 * f + bestAxis] - clo[bestAxis]) / ext * NB);
                if (b >= NB) b = NB - 1;
                if (b < 0) b = 0;
                if (b <= bestBin) i++;
                else { e--; uint32_t tmp = idx[i]; idx[i] = idx[e]; idx[e] = tmp; }
            }
            mid = i;
            if (mid == j.begin || mid == j.end) mid = j.begin + count / 2;
        }
        const uint32_t child = (uint32_t)out.nodes.size() + (out.nodes.size() & 1u);  // even id: 64-byte aligned pair
        out.nodes.resize(child + 2, RtuBvhNode{});
        n.index = child;
        n.count = 0;
        out.nodes[j.id] = n;
        queue.push_back({j.begin, mid, child, j.level + 1});
        queue.push_back({mid, j.end, child + 1, j.level + 1});
    }
}

// Leaf-order the elements depth-first, so that every subtree owns a contiguous range of element
// slots (the 8-wide tree of the cooperative walk turns whole subtrees of <= 8 triangles into
// leaves). first/total: per binary node, the subtree's slot range.
void dfs_order(SahTree& t, std::vector<uint32_t>& first, std::vector<uint32_t>& total) {
    std::vector<uint32_t> elems;
    elems.reserve(t.elements.size());
    first.assign(t.nodes.size(), 0);
    total.assign(t.nodes.size(), 0);
    std::vector<std::pair<uint32_t, int>> stack;  // (node, state)
    stack.push_back({1u, 0});
    while (!stack.empty()) {
        auto [id, st] = stack.back();
        RtuBvhNode& n = t.nodes[id];
        if (n.count != 0) {
            first[id] = (uint32_t)elems.size();
            total[id] = n.count;
            for (uint32_t i = 0; i < n.count; i++) elems.push_back(t.elements[n.index + i]);
            n.index = first[id];
            stack.pop_back();
        } else if (st == 0) {
            first[id] = (uint32_t)elems.size();
            stack.back().second = 1;
            stack.push_back({n.index, 0});
        } else if (st == 1) {
            stack.back().second = 2;
            stack.push_back({n.index + 1, 0});
        } else {
            total[id] = total[n.index] + total[n.index + 1];
            stack.pop_back();
        }
    }
    t.elements.swap(elems);
}

// The binary SAH tree collapsed to eight children per node (for the cooperative walk, one child
// per lane): starting from a node's two children, the inner child with the largest surface area
// is replaced by ITS two children until eight are reached or only leaves remain. Breadth-first,
// so that the top of the tree is the prefix staged into LDS. Same leaves, same boxes.
void build_wide8(const SahTree& t, const std::vector<uint32_t>& first, const std::vector<uint32_t>& total, std::vector<float4>& out) {
    struct Job { uint32_t bin, id; };
    auto is_leaf = [&](uint32_t b) { return total[b] <= 8u; };  // a subtree of <= 8 triangles is one leaf round for eight lanes
    out.assign(16, make_float4(0, 0, 0, 0));
    std::vector<Job> queue;
    queue.push_back({1u, 0u});
    auto area = [&](uint32_t b) {
        const RtuBvhNode& n = t.nodes[b];
        float dx = n.bmax[0] - n.bmin[0], dy = n.bmax[1] - n.bmin[1], dz = n.bmax[2] - n.bmin[2];
        return dx * dy + dy * dz + dz * dx;
    };
    for (size_t qi = 0; qi < queue.size(); qi++) {
        const Job j = queue[qi];
        std::vector<uint32_t> set;
        if (is_leaf(j.bin)) {
            set.push_back(j.bin);  // a mesh of <= 8 triangles: the root is a leaf
        } else {
            set.push_back(t.nodes[j.bin].index);
            set.push_back(t.nodes[j.bin].index + 1);
            while (set.size() < 8) {
                int best = -1;
                float bestA = -1.0f;
                for (size_t i = 0; i < set.size(); i++)
                    if (!is_leaf(set[i]) && area(set[i]) > bestA) { bestA = area(set[i]); best = (int)i; }
                if (best < 0) break;
                const uint32_t b = set[(size_t)best];
                set[(size_t)best] = t.nodes[b].index;
                set.push_back(t.nodes[b].index + 1);
            }
        }
        for (uint32_t c = 0; c < 8; c++) {
            float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0);
            uint32_t ref = RTU_REF8_EMPTY;
            if (c < set.size()) {
                const RtuBvhNode& n = t.nodes[set[c]];
                lo = make_float4(n.bmin[0], n.bmin[1], n.bmin[2], 0);
                hi = make_float4(n.bmax[0], n.bmax[1], n.bmax[2], 0);
                if (is_leaf(set[c])) {
                    ref = first[set[c]] | (total[set[c]] << 28);
                } else {
                    ref = (uint32_t)(out.size() / 16);
                    out.resize(out.size() + 16, make_float4(0, 0, 0, 0));
                    queue.push_back({set[c], ref});
                }
            }
            memcpy(&lo.w, &ref, 4);
            out[(size_t)j.id * 16 + 2 * c] = lo;
            out[(size_t)j.id * 16 + 2 * c + 1] = hi;
        }
    }
}

// ... and to FOUR children per node for the one-lane-per-ray walk (half the dependent fetches of the
// binary tree at the same instruction count). A node is 8 float4, structure of arrays so that a lane
// picks the near / far plane arrays by the sign of its ray: {min.x[4]} {min.y[4]} {min.z[4]}
// {max.x[4]} {max.y[4]} {max.z[4]} {ref[4]} {-}. stack_need: the deepest stack a walk can build
// (a step pushes all hit children but the nearest).
void build_wide4(const SahTree& t, std::vector<float4>& out, uint32_t& stack_need) {
    struct Job { uint32_t bin, id, pushed; };
    out.assign(8, make_float4(0, 0, 0, 0));
    std::vector<Job> queue;
    queue.push_back({1u, 0u, 0u});
    stack_need = 1;
    auto area = [&](uint32_t b) {
        const RtuBvhNode& n = t.nodes[b];
        float dx = n.bmax[0] - n.bmin[0], dy = n.bmax[1] - n.bmin[1], dz = n.bmax[2] - n.bmin[2];
        return dx * dy + dy * dz + dz * dx;
    };
    for (size_t qi = 0; qi < queue.size(); qi++) {
        const Job j = queue[qi];
        std::vector<uint32_t> set;
        if (t.nodes[j.bin].count != 0) {
            set.push_back(j.bin);
        } else {
            set.push_back(t.nodes[j.bin].index);
            set.push_back(t.nodes[j.bin].index + 1);
            while (set.size() < 4) {
                int best = -1;
                float bestA = -1.0f;
                for (size_t i = 0; i < set.size(); i++)
                    if (t.nodes[set[i]].count == 0 && area(set[i]) > bestA) { bestA = area(set[i]); best = (int)i; }
                if (best < 0) break;
                const uint32_t b = set[(size_t)best];
                set[(size_t)best] = t.nodes[b].index;
                set.push_back(t.nodes[b].index + 1);
            }
        }
        const uint32_t pushed = j.pushed + (uint32_t)set.size() - 1u;
        if (pushed + 1u > stack_need) stack_need = pushed + 1u;
        float v[7][4];
        for (uint32_t c = 0; c < 4; c++) {
            for (int k = 0; k < 3; k++) { v[k][c] = INFINITY; v[3 + k][c] = -INFINITY; }
            uint32_t ref = RTU_REF8_EMPTY;
            if (c < set.size()) {
                const RtuBvhNode& n = t.nodes[set[c]];
                for (int k = 0; k < 3; k++) { v[k][c] = n.bmin[k]; v[3 + k][c] = n.bmax[k]; }
                if (n.count != 0) {
                    ref = n.index | (n.count << 28);
                } else {
                    ref = (uint32_t)(out.size() / 8);
                    out.resize(out.size() + 8, make_float4(0, 0, 0, 0));
                    queue.push_back({set[c], ref, pushed});
                }
            }
            memcpy(&v[6][c], &ref, 4);
        }
        for (int r = 0; r < 7; r++) out[(size_t)j.id * 8 + r] = make_float4(v[r][0], v[r][1], v[r][2], v[r][3]);
    }
}

// 64-byte triangle records (TriRec, rtu_intersect.h) in the order of `elements`: the
// ray-independent part of TriObj::IntersectTriangle (objFunctions.cpp:259-300) evaluated with
// the same float ops.
void build_tri_records(const RtuMesh& m, const uint32_t* elements, uint32_t n, std::vector<float4>& tri) {
    tri.resize((size_t)n * 4);
    for (uint32_t e = 0; e < n; e++) mu_slot_record(m.f, m.v, elements, e, &tri[4 * (size_t)e]);  // (rtu_meshrec.h: shared with the device)
}

// the reference's tree renumbered breadth-first (sibling pairs stay adjacent, the root stays node 1): same tree, same traversal
// order. any_empty: some box has min > max (cannot come from triangles).
void renumber_bfs(const RtuMesh& m, std::vector<RtuBvhNode>& bfs, uint32_t& any_empty) {
    any_empty = 0;
    for (uint32_t i = 1; i < m.n_bvh_nodes; i++) {
        const RtuBvhNode& bn = m.bvh[i];
        if (bn.bmin[0] > bn.bmax[0] || bn.bmin[1] > bn.bmax[1] || bn.bmin[2] > bn.bmax[2]) any_empty = 1;
    }
    bfs.resize(m.n_bvh_nodes);
    memset(bfs.data(), 0, bfs.size() * sizeof(RtuBvhNode));
    std::vector<std::pair<uint32_t, uint32_t>> queue;  // (old id, new id)
    queue.push_back({1u, 1u});
    uint32_t next_free = 2;
    for (size_t qi = 0; qi < queue.size(); qi++) {
        auto [oldId, newId] = queue[qi];
        RtuBvhNode nn = m.bvh[oldId];
        if (nn.count == 0) {
            queue.push_back({nn.index, next_free});
            queue.push_back({nn.index + 1, next_free + 1});
            nn.index = next_free;
            next_free += 2;
        }
        bfs[newId] = nn;
    }
}

namespace {

double abs_row_norm(const double* m) {  // || |M| ||_inf of a row-major 3 x 3 matrix
    double r = 0;
    for (int i = 0; i < 3; i++) r = std::max(r, std::fabs(m[3 * i]) + std::fabs(m[3 * i + 1]) + std::fabs(m[3 * i + 2]));
    return r;
}
void mul33(const double* a, const double* b, double* out) {
    double t[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) t[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
    memcpy(out, t, sizeof t);
}

// The margin of the rays that start at hit points, delta = c1 max(m0, pm), and the scale the occluder lists are built with
// (rtu_intersect.h, THE NEAR MARGIN, has the argument): 1e-4 max(wscale, pm) and wscale themselves, bit for bit, unless the far
// term at the scene's own extent exceeds twelve near margins. omega1: 1 + the largest |coordinate| of the origin of any node's space.
void near_margin(float wscale, float wnoise, double omega1, WorldFar& out) {
    out.near_m0 = wscale; out.near_c1 = 1e-4f; out.wlist = wscale;
    const double ws = wscale, P = 2.0 * ws, wn = wnoise;
    const auto f = [&](double m) { return 1e-4 * std::max(ws, m) + wn * (m + omega1) * (m + ws); };
    const double DP = wn * (P + omega1) * (P + ws);
    if (!(DP >= 12.0 * 1e-4 * ws)) return;  // (a scale or a chain that is not finite: no node has a bound, world_bounds)
    const double c1 = f(P) / P * (1 + 1e-6);
    // f is convex and c1 m passes above f(P): c1 m >= f(m) exactly on an interval [m*, P]
    double lo = 0, hi = P;
    for (int i = 0; i < 64; i++) {
        const double mid = 0.5 * (lo + hi);
        if (c1 * mid >= f(mid)) hi = mid; else lo = mid;
    }
    const double m0 = hi * (1 + 1e-6), wl = (ws + 1e4 * DP) * (1 + 1e-6);
    out.near_m0 = m0 < 1e30 ? (float)m0 : 1e30f;
    out.near_c1 = c1 < 1e30 ? (float)c1 : 1e30f;
    out.wlist = wl < 1e30 ? (float)wl : 1e30f;
}

}  // namespace

void world_far(const RtuSceneDesc* s, double wscale, WorldFar& out) {
    const double u = 0x1p-24;
    double K = 0, omega = 0, sph_cond = 0, sph_T = 0;
    for (uint32_t i = 0; i < s->n_nodes; i++) {
        const int type = s->nodes[i].obj_type;
        if (type != RTU_OBJ_SPHERE && type != RTU_OBJ_PLANE && type != RTU_OBJ_TRIMESH) continue;
        std::vector<int> chain;
        for (int j = (int)i; j >= 0; j = s->nodes[j].parent) chain.push_back(j);
        // root first: T = tm_0 ... tm_(j-1) takes space j to the world, Ti is its inverse, o the world position of the origin of space j
        double T[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Ti[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};
        double k_node = 0, om = 0;
        for (size_t c = chain.size(); c-- > 0;) {
            const RtuNode& a = s->nodes[chain[c]];
            double tm[9], itm[9], prod[9];
            for (int r = 0; r < 3; r++)
                for (int q = 0; q < 3; q++) { tm[3 * r + q] = a.tm[3 * q + r]; itm[3 * r + q] = a.itm[3 * q + r]; }  // (RtuNode: column-major)
            for (int r = 0; r < 3; r++)
                for (int q = 0; q < 3; q++)
                    prod[3 * r + q] = std::fabs(tm[3 * r]) * std::fabs(itm[q]) + std::fabs(tm[3 * r + 1]) * std::fabs(itm[3 + q]) + std::fabs(tm[3 * r + 2]) * std::fabs(itm[6 + q]);
            k_node += abs_row_norm(T) * abs_row_norm(Ti) * (3.0 + 6.0 * abs_row_norm(prod));
            for (int r = 0; r < 3; r++) o[r] += T[3 * r] * a.pos[0] + T[3 * r + 1] * a.pos[1] + T[3 * r + 2] * a.pos[2];
            om = std::max(om, std::max(std::fabs(o[0]), std::max(std::fabs(o[1]), std::fabs(o[2]))));
            mul33(T, tm, T);
            mul33(itm, Ti, Ti);
        }
        const double cond = abs_row_norm(T) * abs_row_norm(Ti);
        if (!std::isfinite(k_node) || !std::isfinite(om) || !std::isfinite(cond)) continue;  // such a node has no bound at all (world_bounds)
        K = std::max(K, k_node);
        omega = std::max(omega, om);
        if (type == RTU_OBJ_SPHERE) { sph_cond = std::max(sph_cond, cond); sph_T = std::max(sph_T, abs_row_norm(T)); }
    }
    out.wnoise = (float)(1.74 * u * K * (1 + 1e-6));
    out.wreach = (float)(std::max(wscale, omega + 1.0) * (1 + 1e-6));
    out.sph_k = (float)(5.2e-3 * sph_cond * (1 + 1e-6));
    out.sph_r = (float)(1.74 * sph_T * (1 + 1e-6));
    near_margin((float)wscale, out.wnoise, omega + 1.0, out);
}
// NODE-LEVEL BOUNDS (DevNode::wmin / wmax; the argument is in rtu_intersect.h, trace): the object's own bounding box —
// the unit cube of a sphere, the unit square of a plane (objects.h:25,37), the mesh's box — taken corner by corner through
// the node's chain of transformations (p -> tm p + pos, scene.h:508-512) in binary64, then widened by
//   * 1e-5 of the largest coordinate (the chain itself is binary32 on the device and in the reference), and
//   * for a sphere, what the cancellation in b*b - 4ac can move a grazing root (objFunctions.cpp:25-27): the discriminant
//     carries an error of ~4 ulp of b*b, i.e. the ray may "touch" a sphere it passes at up to ~2.4e-7 * (D/R)^2 radii, and a
//     grazing root is off by up to ~5e-4 * D in t; with D bounded by the scene's diameter S both stay below
//     4e-6 * S^2 / R + 1e-3 * S ... the latter only matters when R < 1e-3 * S, where the former is already larger. R is the
//     smallest half-extent of the sphere's world box.
//     (That D is the distance inside the scene. A ray from further away is covered per ray: rtu_intersect.h, cull_margin and
//     sphere_slack.)
// Returns the largest |coordinate| of all bounds (the scale of the per-ray margin).
float world_bounds(const RtuSceneDesc* s, std::vector<DevNode>& nodes) {
    const uint32_t n = s->n_nodes;
    std::vector<std::array<double, 6>> box(n);
    std::vector<bool> has(n, false);
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t i = 0; i < n; i++) {
        const RtuNode& nd = s->nodes[i];
        double l[3], h[3];
        if (nd.obj_type == RTU_OBJ_SPHERE) { l[0] = l[1] = l[2] = -1; h[0] = h[1] = h[2] = 1; }
        else if (nd.obj_type == RTU_OBJ_PLANE) { l[0] = l[1] = -1; h[0] = h[1] = 1; l[2] = h[2] = 0; }
        else if (nd.obj_type == RTU_OBJ_TRIMESH) {
            const RtuMesh& m = s->meshes[nd.mesh_id];
            for (int k = 0; k < 3; k++) { l[k] = m.bound_min[k]; h[k] = m.bound_max[k]; }
        } else continue;
        double wl[3] = {1e300, 1e300, 1e300}, wh[3] = {-1e300, -1e300, -1e300};
        for (int c = 0; c < 8; c++) {
            double p[3] = {(c & 1) ? h[0] : l[0], (c & 2) ? h[1] : l[1], (c & 4) ? h[2] : l[2]};
            for (int j = (int)i; j >= 0; j = s->nodes[j].parent) {
                const RtuNode& a = s->nodes[j];
                const double q[3] = {p[0] * a.tm[0] + p[1] * a.tm[3] + p[2] * a.tm[6] + a.pos[0],
                                     p[0] * a.tm[1] + p[1] * a.tm[4] + p[2] * a.tm[7] + a.pos[1],
                                     p[0] * a.tm[2] + p[1] * a.tm[5] + p[2] * a.tm[8] + a.pos[2]};
                p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
            }
            for (int k = 0; k < 3; k++) { wl[k] = std::min(wl[k], p[k]); wh[k] = std::max(wh[k], p[k]); }
        }
        for (int k = 0; k < 3; k++) { box[i][k] = wl[k]; box[i][3 + k] = wh[k]; lo[k] = std::min(lo[k], wl[k]); hi[k] = std::max(hi[k], wh[k]); }
        has[i] = true;
    }
    double S = 0;
    for (int k = 0; k < 3; k++) if (hi[k] >= lo[k]) S += (hi[k] - lo[k]) * (hi[k] - lo[k]);
    S = std::sqrt(S);
    double scale = 0;
    for (uint32_t i = 0; i < n; i++) {
        DevNode& d = nodes[i];
        for (int k = 0; k < 3; k++) { d.wmin[k] = -INFINITY; d.wmax[k] = INFINITY; }
        if (!has[i]) continue;
        double m = 0;
        for (int k = 0; k < 6; k++) m = std::max(m, std::fabs(box[i][k]));
        double widen = 1e-5 * m;
        if (s->nodes[i].obj_type == RTU_OBJ_SPHERE) {
            double R = 1e300;
            for (int k = 0; k < 3; k++) R = std::min(R, 0.5 * (box[i][3 + k] - box[i][k]));
            widen += R > 0 ? 4e-6 * S * S / R : INFINITY;
            if (R < 1e-3 * S) widen += 1e-3 * S;
        }
        bool finite = std::isfinite(widen);
        for (int k = 0; k < 3 && finite; k++) finite = std::isfinite(box[i][k]) && std::isfinite(box[i][3 + k]);
        if (!finite) continue;  // NaN / infinite transformation: no bound (everything passes an infinite box)
        for (int k = 0; k < 3; k++) {
            d.wmin[k] = std::nextafter((float)(box[i][k] - widen), -INFINITY);
            d.wmax[k] = std::nextafter((float)(box[i][3 + k] + widen), INFINITY);
            scale = std::max(scale, std::max(std::fabs((double)d.wmin[k]), std::fabs((double)d.wmax[k])));
        }
    }
    return (float)scale;
}

// the box of the ray-sort keys (rtu_ray_sort_box): the union of the finite node-level bounds world_bounds left, else [-wscale, wscale]^3
void sort_box_of(const std::vector<DevNode>& nodes, float wscale, float out[6]) {
    for (int k = 0; k < 3; k++) { out[k] = INFINITY; out[3 + k] = -INFINITY; }
    bool any_bound = false;
    for (const DevNode& d : nodes) {
        bool finite = true;
        for (int k = 0; k < 3; k++) finite = finite && std::isfinite(d.wmin[k]) && std::isfinite(d.wmax[k]);
        if (!finite) continue;
        any_bound = true;
        for (int k = 0; k < 3; k++) {
            out[k] = std::min(out[k], d.wmin[k]);
            out[3 + k] = std::max(out[3 + k], d.wmax[k]);
        }
    }
    if (!any_bound)
        for (int k = 0; k < 3; k++) { out[k] = -wscale; out[3 + k] = wscale; }
}

// OCCLUDER LISTS OF SHADOW RAYS (DevLightMask): for each of the first RTU_LMASK_LIGHTS non-ambient lights and each masked mesh
// node, the mesh as the light sees it — through a pinhole at a point light, looking at the centre of the mesh; along the
// direction of a direct light — on a G x G grid, and per cell the triangles that a shadow ray whose ORIGIN projects into the
// cell can possibly touch. A triangle is entered into every cell that its projection, grown by a slack S, overlaps (exact
// triangle / square overlap: the separating-axis test on the square's sides and the triangle's edges), where S covers
//   * the cull margin: the ray's line, its rounded direction and the binary32 transformation chain stay within
//     wid = 1e-4 * scene scale + 1e-5 * |coordinates| of the ideal segment origin -> light (shadow rays start on the scene's
//     surfaces: |origin| <= the scene's scale); a displacement of wid on every axis moves a projection by at most
//     wid * sqrt(3) * (1 + |u|) / (depth - wid * sqrt(3)) (pinhole; wid * sqrt(3) orthographic);
//   * the device's binary32 evaluation of the cell coordinates (err: a few 1e-6 of the operands, bounded below per list;
//     a list whose bound exceeds a quarter of a cell is not used);
//   * a quarter of a cell on top.
// A list is unusable when some corner of a triangle's widened box is not in front of the pinhole (the light is inside or too
// close to the mesh's hull) or the mesh has no extent from there. G grows with the triangle count (a triangle spans a few
// cells) up to RTU_LGRID_MAX and is halved while the lists would hold more than 32 M entries. (The records: CoverMesh and
// HostLightList, rtu_capi.h.)

// ---- the scalar decisions of rtu_lightlist.h ----
bool ll_frame(const RtuLight& l, const double lo[3], const double hi[3], LlFrame& F) {
    memset(&F, 0, sizeof F);
    const bool point = l.type == RTU_LIGHT_POINT;
    F.point = point ? 1 : 0;
    double* L = F.L;
    double* Z = F.Z;
    double* X = F.X;
    double* Y = F.Y;
    if (point) {
        for (int k = 0; k < 3; k++) { L[k] = l.vec[k]; Z[k] = 0.5 * (lo[k] + hi[k]) - L[k]; }
    } else {
        for (int k = 0; k < 3; k++) Z[k] = l.vec[k];
    }
    const double zl = std::sqrt(Z[0] * Z[0] + Z[1] * Z[1] + Z[2] * Z[2]);
    if (!(zl > 0) || !std::isfinite(zl)) return false;
    for (int k = 0; k < 3; k++) Z[k] /= zl;
    int ax = std::fabs(Z[0]) <= std::fabs(Z[1]) ? (std::fabs(Z[0]) <= std::fabs(Z[2]) ? 0 : 2) : (std::fabs(Z[1]) <= std::fabs(Z[2]) ? 1 : 2);
    double A[3] = {0, 0, 0};
    A[ax] = 1;
    X[0] = Z[1] * A[2] - Z[2] * A[1]; X[1] = Z[2] * A[0] - Z[0] * A[2]; X[2] = Z[0] * A[1] - Z[1] * A[0];
    const double xl = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    for (int k = 0; k < 3; k++) X[k] /= xl;
    Y[0] = Z[1] * X[2] - Z[2] * X[1]; Y[1] = Z[2] * X[0] - Z[0] * X[2]; Y[2] = Z[0] * X[1] - Z[1] * X[0];
    return true;
}

uint32_t ll_first_grid(size_t nf) {
    // grid size: a triangle of an evenly tessellated surface spans ~ G / sqrt(nf / 2) cells; aim at six of them
    uint32_t G = 64;
    static const double kSpan = [] { const char* e = getenv("RTU_LGRID_SPAN"); return e ? atof(e) : 6.0; }();  // tuning knob (any value renders the same image)
    while (G < RTU_LGRID_MAX && (double)G < kSpan * std::sqrt((double)nf * 0.5)) G *= 2;
    return G;
}

bool ll_extent_ok(double U0, double U1, double V0, double V1, double& mag) {
    if (!(U1 > U0) || !(V1 > V0)) return false;
    mag = std::max(std::max(std::fabs(U0), std::fabs(U1)), std::max(std::fabs(V0), std::fabs(V1)));
    return !(!std::isfinite(mag) || (U1 - U0) < 1e-4 * mag || (V1 - V0) < 1e-4 * mag);
}

bool ll_grid_at(uint32_t G, double U0, double U1, double V0, double V1, double ratio, double mag, LlGrid& g) {
    memset(&g, 0, sizeof g);
    g.G = G;
    // the grid spans the extent plus two cells on every side
    g.du = (U1 - U0) / ((double)G - 4); g.dv = (V1 - V0) / ((double)G - 4);
    g.gu0 = U0 - 2 * g.du; g.gv0 = V0 - 2 * g.dv;
    // the device's binary32 cell coordinate: (dot(p - L, X) [/ depth] - u0) * su — every operand good to a few ulp
    const double coord = 16e-7 * ratio * (1.0 + mag);
    const double err_cells = std::max(coord / g.du, coord / g.dv) + 4e-7 * (double)G;
    if (!(err_cells < 0.25)) return false;
    g.S0 = 0.25 + err_cells;
    return true;
}

void ll_mask(const LlFrame& F, const LlGrid& g, DevLightMask& m) {
    for (int k = 0; k < 3; k++) { m.X[k] = (float)F.X[k]; m.Y[k] = (float)F.Y[k]; m.Z[k] = (float)F.Z[k]; m.L[k] = (float)F.L[k]; }
    m.u0 = (float)g.gu0; m.v0 = (float)g.gv0; m.su = (float)(1.0 / g.du); m.sv = (float)(1.0 / g.dv);
    m.point = F.point ? 1u : 0u;
    m.G = g.G;
}

// One list: pure host arithmetic (no GPU) — the frame, the grid and the cells' entries {slot, zmin bits} of light `l` looking at the mesh
// `cm`. false: no usable list from there. (rtu_debug_light_list hands the result to the CPU tests, which check it ray by ray.)
bool compute_light_list(const RtuLight& l, const CoverMesh& cm, float wscale, HostLightList& out) {
    DevLightMask& m = out.m;
    memset(&m, 0, sizeof m);
    std::vector<uint32_t>& off = out.off;
    std::vector<uint32_t>& ent = out.ent;
    const std::vector<float4>& boxes = cm.boxes;
    const size_t nf = boxes.size() / 2;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (size_t f = 0; f < nf; f++) {
        const float4 a = boxes[2 * f], b = boxes[2 * f + 1];
        const double al[3] = {a.x, a.y, a.z}, bh[3] = {b.x, b.y, b.z};
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], al[k]); hi[k] = std::max(hi[k], bh[k]); }
    }
    LlFrame F;
    if (!ll_frame(l, lo, hi, F)) return false;  // unusable
    // per triangle: the rectangle of its widened box in the light's (u, v) — the extent of the grid, and the check that
    // everything the list stands for lies in front of the pinhole
    double U0 = 1e300, U1 = -1e300, V0 = 1e300, V1 = -1e300, ratio = 1.0;
    std::vector<double> wid_of(nf);
    for (size_t f = 0; f < nf; f++) {
        wid_of[f] = ll_face_wid(boxes[2 * f], boxes[2 * f + 1], wscale);
        if (!ll_face_corners(boxes[2 * f], boxes[2 * f + 1], wid_of[f], F, U0, U1, V0, V1, ratio)) return false;
    }
    double mag;
    if (!ll_extent_ok(U0, U1, V0, V1, mag)) return false;
    LlGrid g;
    for (uint32_t G = ll_first_grid(nf);; G /= 2) {
        if (G < 16u) return false;
        if (!ll_grid_at(G, U0, U1, V0, V1, ratio, mag, g)) continue;  // (a coarser grid has larger cells)
        off.assign((size_t)G * G + 1, 0u);
        size_t total = 0;
        bool too_many = false;
        for (int pass = 0; pass < 2 && !too_many; pass++) {
            if (pass == 1) {
                uint32_t run = 0;
                for (size_t i = 0; i < (size_t)G * G; i++) { const uint32_t n = off[i]; off[i] = run; run += n; }
                off[(size_t)G * G] = run;
                ent.assign(2 * total, 0u);
            }
            for (size_t f = 0; f < nf; f++) {
                LlFaceCells c;
                ll_face_cells(cm.verts.data() + 9 * f, wid_of[f], F, g, wscale, c);
                const uint32_t slot = cm.slot_of[f];
                for (int y = c.y0; y <= c.y1; y++)
                    for (int x = c.x0; x <= c.x1; x++) {
                        if (!ll_cell_in(c, x, y)) continue;
                        const size_t cell = (size_t)y * G + (size_t)x;
                        if (pass == 0) { off[cell]++; total++; }
                        else { const uint32_t at = off[cell]++; ent[2 * (size_t)at] = slot; ent[2 * (size_t)at + 1] = c.zbits; }
                    }
                if (pass == 0 && total > RTU_LLIST_MAX_ENTRIES) { too_many = true; break; }
            }
        }
        if (too_many) continue;
        // pass 1 advanced every offset to the end of its cell: shift back
        for (size_t i = (size_t)G * G; i > 0; i--) off[i] = off[i - 1];
        off[0] = 0;
        {   // nearest to the light first: a walk of the list ends at the first entry that lies beyond the ray's origin
            std::vector<std::pair<float, uint32_t>> tmp;
            for (size_t cell = 0; cell < (size_t)G * G; cell++) {
                const uint32_t b = off[cell], e = off[cell + 1];
                if (e - b < 2u) continue;
                tmp.clear();
                for (uint32_t i = b; i < e; i++) { float z; memcpy(&z, &ent[2 * (size_t)i + 1], 4); tmp.push_back({z, ent[2 * (size_t)i]}); }
                std::stable_sort(tmp.begin(), tmp.end(), [](const std::pair<float, uint32_t>& a, const std::pair<float, uint32_t>& b2) { return a.first < b2.first; });
                for (uint32_t i = b; i < e; i++) { memcpy(&ent[2 * (size_t)i + 1], &tmp[i - b].first, 4); ent[2 * (size_t)i] = tmp[i - b].second; }
            }
        }
        ll_mask(F, g, m);
        break;
    }
    m.usable = 1u;
    return true;
}

// The triangles of mesh node `node` in world space: every vertex through the chain p -> tm p + pos in binary64; per face its three
// vertices and their box rounded outwards. fast_elements: slot of the mesh's fast tree -> face.
LlChain node_chain(const RtuSceneDesc* s, uint32_t node) {
    LlChain c;
    memset(&c, 0, sizeof c);
    for (int j = (int)node; j >= 0 && c.n < RTU_MAX_NODE_DEPTH; j = s->nodes[j].parent, c.n++) {
        memcpy(c.tm[c.n], s->nodes[j].tm, sizeof c.tm[0]);
        memcpy(c.pos[c.n], s->nodes[j].pos, sizeof c.pos[0]);
    }
    return c;
}

void make_cover_mesh(const RtuSceneDesc* s, uint32_t node, const std::vector<uint32_t>& fast_elements, CoverMesh& cm) {
    const RtuMesh& m = s->meshes[s->nodes[node].mesh_id];
    const LlChain chain = node_chain(s, node);
    cm.boxes.assign((size_t)m.nf * 2, make_float4(0, 0, 0, 0));
    cm.verts.assign((size_t)m.nf * 9, 0.0);
    for (uint32_t f = 0; f < m.nf; f++) {
        const uint32_t* fv = m.f + 3 * (size_t)f;
        ll_cover_face(chain, m.v + 3 * (size_t)fv[0], m.v + 3 * (size_t)fv[1], m.v + 3 * (size_t)fv[2], cm.verts.data() + 9 * (size_t)f,
                      cm.boxes[2 * (size_t)f], cm.boxes[2 * (size_t)f + 1]);
    }
    cm.slot_of.assign(m.nf, 0u);
    for (uint32_t sl = 0; sl < (uint32_t)fast_elements.size(); sl++) cm.slot_of[fast_elements[sl]] = sl;
}

int build_light_lists(RtuContext* ctx, const RtuSceneDesc* s, const std::vector<CoverMesh>& cover, float wscale, DevScene& ds) {
    ds.lmask = nullptr;
    std::vector<uint32_t> lights;
    for (uint32_t i = 0; i < s->n_lights && lights.size() < RTU_LMASK_LIGHTS; i++)
        if (s->lights[i].type != RTU_LIGHT_AMBIENT) lights.push_back(i);
    const uint32_t nc = (uint32_t)cover.size();
    if (lights.empty() || nc == 0) return RTU_OK;
    std::vector<DevLightMask> masks(lights.size() * nc);
    memset(masks.data(), 0, masks.size() * sizeof(DevLightMask));
    for (size_t j = 0; j < lights.size(); j++)
        for (uint32_t c = 0; c < nc; c++) {
            HostLightList hl;
            if (!compute_light_list(s->lights[lights[j]], cover[c], wscale, hl)) continue;
            DevLightMask& m = masks[j * nc + c];
            m = hl.m;
            m.usable = 0u;
            int rc;
            const int slot = P_LIST + 2 * (int)(j * nc + c);
            if ((rc = place_upload(ctx, slot, hl.off.data(), hl.off.size(), &m.cell_off)) != RTU_OK) return rc;
            if ((rc = place_upload(ctx, slot + 1, hl.ent.data(), hl.ent.size(), &m.cell_tri)) != RTU_OK) return rc;
            m.usable = 1u;
            uint32_t longest = 0;
            for (size_t i = 0; i < (size_t)m.G * m.G; i++) longest = std::max(longest, hl.off[i + 1] - hl.off[i]);
            ctx->light_list_info.push_back({(uint32_t)j, c, m.G, (uint32_t)(hl.ent.size() / 2), longest});
        }
    ctx->lmask_host = masks;
    return place_upload(ctx, P_LMASK, masks.data(), masks.size(), &ds.lmask);
}

// The same lists built on the GPU (rtu_scene_update.hip) from the cover meshes already there: `covers` per masked mesh node,
// `lohi` the box extents of each. Same decisions, same order, same lists.
int build_light_lists_device(RtuContext* ctx, const RtuSceneDesc* s, const std::vector<LlCover>& covers, const std::vector<double>& lohi, float wscale,
                             DevScene& ds) {
    ds.lmask = nullptr;
    ctx->lmask_host.clear();
    std::vector<uint32_t> lights;
    for (uint32_t i = 0; i < s->n_lights && lights.size() < RTU_LMASK_LIGHTS; i++)
        if (s->lights[i].type != RTU_LIGHT_AMBIENT) lights.push_back(i);
    const uint32_t nc = (uint32_t)covers.size();
    if (lights.empty() || nc == 0) return RTU_OK;
    std::vector<DevLightMask> masks(lights.size() * nc);
    memset(masks.data(), 0, masks.size() * sizeof(DevLightMask));
    std::vector<LlFrame> frames;
    std::vector<int> pair_cover, pair_of;  // pairs with a frame: their cover node and their index j * nc + c
    for (size_t j = 0; j < lights.size(); j++)
        for (uint32_t c = 0; c < nc; c++) {
            LlFrame F;
            if (!ll_frame(s->lights[lights[j]], &lohi[6 * c], &lohi[6 * c + 3], F)) continue;
            frames.push_back(F);
            pair_cover.push_back((int)c);
            pair_of.push_back((int)(j * nc + c));
        }
    std::vector<double> ext(6 * frames.size() + 6);
    RTU_HIP(ctx, ll_build_extents(ctx->llb, ctx->stream, covers.data(), pair_cover.data(), frames.data(), (int)frames.size(), wscale, ext.data()));
    for (size_t p = 0; p < frames.size(); p++) {
        const double* e = &ext[6 * p];
        double mag;
        if (e[5] == 0.0 || !ll_extent_ok(e[0], e[1], e[2], e[3], mag)) continue;
        const int c = pair_cover[p];
        const LlCover& cv = covers[(size_t)c];
        LlGrid g;
        for (uint32_t G = ll_first_grid(cv.nf); G >= 16u; G /= 2) {
            if (!ll_grid_at(G, e[0], e[1], e[2], e[3], e[4], mag, g)) continue;
            size_t entries = 0;
            RTU_HIP(ctx, ll_count(ctx->llb, ctx->stream, cv, c, frames[p], g, wscale, &entries));
            if (entries > RTU_LLIST_MAX_ENTRIES) continue;
            DevLightMask& m = masks[(size_t)pair_of[p]];
            ll_mask(frames[p], g, m);
            const int slot = P_LIST + 2 * pair_of[p];
            void *off = nullptr, *ent = nullptr;
            int rc;
            if ((rc = ensure_place(ctx, slot, sizeof(uint32_t) * ((size_t)G * G + 1), &off)) != RTU_OK) return rc;
            if ((rc = ensure_place(ctx, slot + 1, sizeof(uint32_t) * 2 * entries, &ent)) != RTU_OK) return rc;
            uint32_t longest = 0;
            RTU_HIP(ctx, ll_fill(ctx->llb, ctx->stream, cv, g, (uint32_t*)off, (uint32_t*)ent, &longest));
            m.cell_off = (const uint32_t*)off;
            m.cell_tri = (const uint32_t*)ent;
            m.usable = 1u;
            ctx->light_list_info.push_back({(uint32_t)(pair_of[p] / (int)nc), (uint32_t)c, G, (uint32_t)entries, longest});
            break;
        }
    }
    ctx->lmask_host = masks;
    return place_upload(ctx, P_LMASK, masks.data(), masks.size(), &ds.lmask);
}
