// mesh_edit.cpp — deforming a mesh of a loaded scene (then rtu_update_meshes, rtu_render.h): new vertex positions on the loaded
// connectivity, followed by exactly what TriObj::Load does after reading the file (objects.h:56-58), so that the edited scene is
// the scene a load of an .obj with those vertices gives.
#include "scene_graph.h"

#include <cstring>

namespace {

rtu::MeshData* mesh_of(RtuScene* scene, uint32_t mesh, const char* what) {
    rtu::Scene* s = scene ? scene->impl : nullptr;
    if (!s) { rtu::set_error(std::string(what) + ": scene is NULL"); return nullptr; }
    if (mesh >= s->meshes.size()) { rtu::set_error(std::string(what) + ": no mesh " + std::to_string(mesh)); return nullptr; }
    return &s->meshes[mesh];
}

}  // namespace

extern "C" int rtu_scene_set_mesh_vertices(RtuScene* scene, uint32_t mesh, const float* v, const float* vn) {
    rtu::MeshData* m = mesh_of(scene, mesh, "rtu_scene_set_mesh_vertices");
    if (!m) return -1;
    if (!v) { rtu::set_error("rtu_scene_set_mesh_vertices: v is NULL"); return -1; }
    if (m->v.data() != v) memcpy(m->v.data(), v, m->v.size() * sizeof(float));
    if (vn && m->vn.data() != vn) memcpy(m->vn.data(), vn, m->vn.size() * sizeof(float));
    rtu::ComputeBoundingBox(*m);   // objects.h:57
    rtu::BuildBVH(*m, 4);          // objects.h:58
    scene->impl->rebuild_desc();
    return 0;
}

extern "C" int rtu_scene_recompute_normals(RtuScene* scene, uint32_t mesh) {
    rtu::MeshData* m = mesh_of(scene, mesh, "rtu_scene_recompute_normals");
    if (!m) return -1;
    // only normals of ComputeNormals' own form: one per vertex, indexed like the vertices (a file without vn lines)
    if (m->vn.size() != m->v.size() || m->fn != m->f) {
        rtu::set_error("rtu_scene_recompute_normals: mesh " + std::to_string(mesh) + " carries normals of its own (not one per vertex with fn == f)");
        return -1;
    }
    rtu::ComputeNormals(*m);       // objects.h:56
    scene->impl->rebuild_desc();
    return 0;
}
