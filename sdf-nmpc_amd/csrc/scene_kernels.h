// Analytic scenes (csrc/scene.hip): range / depth images of a known world rendered on the device, the camera
// pose of a state, and the exact signed distance to the scene; static scenes, and scenes whose primitives carry a
// rigid frame that is a function of time (oriented and moving obstacles).  The producer side of the perception loop whose
// consumers are vae_enc.hip (images -> latents), ref_pack.hip (latents + pose -> p) and df_truth.hip (labels).
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_bvh.h"

namespace sdfn {

constexpr int SCENE_MAX_PRIMS = 32;  // SDFNMPC_SCENE_MAX_PRIMS
constexpr int SCENE_BLOCK = 256;
constexpr size_t SCENE_LDS_MAX = 48 * 1024;

// kinds (SDFNMPC_PRIM_*): 0 sphere a = (cx, cy, cz, r); 1 axis-aligned box a = (lo xyz, hi xyz);
// 2 capped cylinder along z a = (cx, cy, r, z0, z1)
struct ScenePrimF {  // 32 bytes: two 16-byte LDS reads
    float a[6];
    int kind, pad;
};
struct ScenePrimD {
    double a[6];
    int kind, pad;
};

// A primitive of a dynamic scene set: the canonical shape (centred: sphere h = (r, -, -), box h = half extents,
// cylinder h = (r, r, half height)) with its frame at time t, c(t) = c0 + v t + amp sin(omega t + phase),
// R(t) = Rz(yaw_rate t) R0 (R0 row-major, formed from the unit quaternion on the host in fp64)
struct ScenePrimDyn {  // 200 bytes
    double c0[3], R0[9], v[3], amp[3];
    double yaw_rate, omega, phase;
    double h[3];
    int kind, pad;
};
// what a block of the dynamic render kernel stages per primitive: the camera origin o' = R(t)^T (W_p_C - c(t)) and
// M = R(t)^T W_R_C, formed in fp64 and rounded once
struct ScenePrimFrame {  // 64 bytes: four 16-byte LDS reads; what only a box reads comes last
    float o[3], h0;      // sphere / cylinder: the radius; box: the half extent along x
    float M[9];
    int kind;
    float hz, h1;        // box / cylinder: the half extent along z; box: along y
};

// The uniform grid of one scene of an indexed set (sdfnmpc_scene_create_large; scene_grid.hip).  Cell (i, j, k) is
// the cube org + (i, j, k) cell .. org + (i + 1, j + 1, k + 1) cell; its primitives are the scene-local indices
// cell_items[cell_start[cell_off + id] .. cell_start[cell_off + id + 1]), id = (k n[1] + j) n[0] + i, in ascending
// order.  A primitive is listed in every cell that its bounding box, inflated by `infl`, overlaps; the grid's box
// is the primitives' bounding box padded by 2 infl, so no primitive is within infl of the grid's boundary.  org and
// cell are representable in fp32: both precisions see the same planes.
struct SceneGridHdr {
    double org[3], cell, inv;  // inv = 1 / cell
    int n[3];                  // cells per axis, each >= 1
    int count;                 // primitives of the scene
    int prim_off;              // the scene's first primitive in SceneDev.pf / .pd
    int cell_off;              // the scene's first entry in SceneDev.cell_start (n[0] n[1] n[2] + 1 entries)
};
constexpr int SCENE_LARGE_MAX_PRIMS = 65536;       // SDFNMPC_SCENE_LARGE_MAX_PRIMS
constexpr int SCENE_GRID_MAX_AXIS = 1024;          // SDFNMPC_SCENE_GRID_MAX_AXIS
constexpr long long SCENE_GRID_MAX_CELLS = 1 << 22;  // SDFNMPC_SCENE_GRID_MAX_CELLS, per scene
constexpr long long SCENE_GRID_MAX_ITEMS = 1 << 26;  // SDFNMPC_SCENE_GRID_MAX_ITEMS, per set (cells + list entries)

// S scenes in both precisions on the device: up to SCENE_MAX_PRIMS primitives each at a stride of SCENE_MAX_PRIMS, or
// (ghdr != nullptr: an indexed set) up to SCENE_LARGE_MAX_PRIMS each, packed scene after scene, with a grid
struct SceneDev {
    int S;
    const int* count;        // [S]
    const ScenePrimF* pf;    // [S][SCENE_MAX_PRIMS]; indexed: [sum of count]
    const ScenePrimD* pd;    // [S][SCENE_MAX_PRIMS]; indexed: [sum of count]
    const SceneGridHdr* ghdr;  // [S], or nullptr: not indexed (the brute-force kernels)
    const int* cell_start;
    const int* cell_items;
};

// A mesh set on the device (sdfnmpc_scene_create_mesh; scene_mesh.hip): S scenes of triangles behind a hierarchy each
// (the layout and the build: mesh_bvh.h).  The arrays hold scene after scene; hdr[s] says where scene s lies in them.
struct MeshDev {
    const MeshHdr* hdr;      // [S]
    const MeshNode* nodes;   // [sum of nnodes], preorder per scene; first is relative to the scene's tri_off
    const MeshTriF* tf;      // [sum of ntri], in the hierarchy's order
    const MeshTriD* td;      // [sum of ntri], the same order
    const MeshTriN* tn;      // [sum of ntri], the same order; nullptr: an open set (unsigned distance)
};

struct SceneRenderArgs {
    SceneDev sc;
    const int* scene_of;     // [B] or nullptr (scene 0); entries are the caller's to keep in [0, S)
    int B, H, W;
    const double* W_p_C;     // [B][3]
    const double* W_R_C;     // [B][9] row-major
    float dmax, scale;
    float hfov, vfov;        // spherical: half fields of view
    float ty0, ty1, tz0, tz1;  // pinhole: tangent coordinates ty = ty0 + ty1 u, tz = tz0 + tz1 v
    int is_depth, is_spherical;
    float* img;              // [B][H][W]
};

struct SceneRenderDynArgs {
    SceneRenderArgs r;
    const ScenePrimDyn* dyn; // [S][SCENE_MAX_PRIMS]
    double t;
    // a mixed set (sdfnmpc_scene_create_mixed; r.sc.ghdr != nullptr): dyn holds mcount[s] <= SCENE_MAX_PRIMS movers per
    // scene beside the indexed static primitives that r.sc.count counts.  Last, here and below: the dynamic kernels'
    // arguments stay where they were
    const int* mcount;       // [S], or nullptr: a dynamic set
};

struct ScenePoseArgs {
    int B;
    const double* x;         // [B][10]
    double B_p_C[3], B_R_C[9];
    double *W_p_Bo, *W_R_Bo, *W_p_C, *W_R_C;  // [B][3], [B][9], [B][3], [B][9]
};

struct SceneDistArgs {
    SceneDev sc;
    const double* points;    // [n][3]
    const int* p_to_scene;   // [n] or nullptr: point j -> scene j / per_scene
    long long n, per_scene;
    double* out;             // [n]
};

struct SceneDistDynArgs {
    SceneDistArgs d;
    const ScenePrimDyn* dyn; // [S][SCENE_MAX_PRIMS]
    const double* times;     // [n] or nullptr (t = 0)
    const int* mcount;       // [S]: the movers of a mixed set (SceneRenderDynArgs), or nullptr
};

// scene_sdf.hip: the scene's exact distance written as the SDF row of h / J_h for rows = B (N+1) node rows
struct SceneSdfArgs {
    SceneDev sc;
    const ScenePrimDyn* dyn; // [S][SCENE_MAX_PRIMS], or nullptr: a static set
    const int* scene_of;     // [B] or nullptr (scene 0)
    long long rows;          // B (N+1)
    int N1, np;              // nodes per instance, parameters per node
    const double* x;         // [rows][10]: the world position is x[r][0:3]
    const double* p;         // [rows][np]: the flag is p[r][0]
    double* h;               // [rows][3]: column 2 is written
    double* Jh;              // [rows][10][3]: column 2 is written
    double max_df, t0;
    const double* tau;       // [N1] or nullptr: node k at time t0 + tau[k] (dynamic sets)
    const int* mcount;       // [S]: the movers of a mixed set (SceneRenderDynArgs), or nullptr
    MeshDev mesh;            // a mesh set (launch_scene_sdf_rows_mesh; sc carries S only); last: the other kernels'
                             // arguments stay where they were
};

// scene_swept.hip: the minimum of the scene's distance over n segments of space-time (p0, t0) -> (p1, t1), one lane each
struct SceneSweptArgs {
    SceneDev sc;
    const ScenePrimDyn* dyn; // [S][SCENE_MAX_PRIMS], or nullptr: a set that is not dynamic (the times are not read)
    const int* mcount;       // [S]: the movers of a mixed set (SceneRenderDynArgs), or nullptr
    const double* vmax;      // [S]: the bound V on the speed of any surface point of the scene's movers (dynamic sets)
    const double* p0;        // [n][3]
    const double* p1;        // [n][3]
    const int* p_to_scene;   // [n] or nullptr: segment j -> scene j / per_scene
    const double* t0;        // [n], or nullptr together with t1: t = 0
    const double* t1;        // [n]
    long long n, per_scene;
    double eps;              // an interval whose lower bound is within eps of the best value is not searched
    int max_evals;           // evaluations of the distance per segment, >= 2
    double* dmin;            // [n]: the smallest value found, at the parameter s
    double* s;               // [n] or nullptr
    double* gap;             // [n] or nullptr: the true minimum lies in [dmin - gap, dmin]
    int* evals;              // [n] or nullptr: evaluations used
    MeshDev mesh;            // a mesh set (launch_scene_swept_mesh); last: the other kernels' arguments stay where they were
};

// scene_mesh.hip: a mesh set's render and distance; r.sc / d.sc carry S only (count, pf, pd are not read)
struct MeshRenderArgs {
    SceneRenderArgs r;
    MeshDev mesh;
};
struct MeshDistArgs {
    SceneDistArgs d;
    MeshDev mesh;
};
// scene_mesh.hip: a mesh set with movers (sdfnmpc_scene_create_mesh_mixed): dyn holds mcount[s] <= SCENE_MAX_PRIMS movers
// per scene beside the mesh.  Structures of their own: the mesh kernels' arguments stay where they were.  The rows and
// the swept kernel of such a set read dyn, mcount and mesh of SceneSdfArgs / SceneSweptArgs, all three non-null
struct MeshRenderMixedArgs {
    SceneRenderArgs r;
    MeshDev mesh;
    const ScenePrimDyn* dyn; // [S][SCENE_MAX_PRIMS]
    const int* mcount;       // [S]
    double t;
};
struct MeshDistMixedArgs {
    SceneDistArgs d;
    MeshDev mesh;
    const ScenePrimDyn* dyn; // [S][SCENE_MAX_PRIMS]
    const int* mcount;       // [S]
    const double* times;     // [n] or nullptr (t = 0)
};

// scene_inst.hip: an instanced set (sdfnmpc_scene_create_instanced).  The MeshDev beside it is the pool of parts:
// hdr[part] says where a part lies in the arrays, each part stored once in its own coordinates.  Scene s holds the
// instances rec[ioff[s] .. ioff[s] + icount[s]), icount[s] <= SCENE_MAX_INSTANCES; an instance is a ScenePrimDyn record
// read for its frame alone (prim_frame), with the part's index in `kind` and nothing in h.
constexpr int SCENE_MAX_INSTANCES = 256;  // SDFNMPC_SCENE_MAX_INSTANCES
struct InstDev {
    int nparts;
    const int* icount;         // [S]
    const int* ioff;           // [S]
    const ScenePrimDyn* rec;   // [sum of icount]
};
// what a block of the instanced render kernel stages per instance: the camera in the instance's frame at time t,
// o' = R(t)^T (W_p_C - c(t)) and M = R(t)^T W_R_C, formed in fp64 and rounded once, and the part
struct SceneInstFrame {  // 64 bytes: four 16-byte LDS reads
    float o[3];
    int part;
    float M[9];
    int pad[3];
};
// structures of their own: every other kernel's arguments stay where they were.  r.sc / d.sc carry S only
struct InstRenderArgs {
    SceneRenderArgs r;
    MeshDev mesh;
    InstDev inst;
    double t;
};
struct InstDistArgs {
    SceneDistArgs d;
    MeshDev mesh;
    InstDev inst;
    const double* times;     // [n] or nullptr (t = 0)
};
struct InstSdfArgs {         // a.mesh: the pool of parts; a.dyn and a.mcount are not read
    SceneSdfArgs a;
    InstDev inst;
};
struct InstSweptArgs {       // a.mesh: the pool of parts; a.vmax [S]: the instances' speed bound; a.dyn, a.mcount not read
    SceneSweptArgs a;
    InstDev inst;
};

inline size_t scene_render_lds_bytes(int h, int w, int is_spherical) {
    return is_spherical ? (size_t)2 * ((size_t)h + (size_t)w) * sizeof(float) : 0;
}

hipError_t launch_scene_render(const SceneRenderArgs& a, hipStream_t s);
hipError_t launch_scene_pose(const ScenePoseArgs& a, hipStream_t s);
hipError_t launch_scene_distance(const SceneDistArgs& a, hipStream_t s);
hipError_t launch_scene_render_dyn(const SceneRenderDynArgs& a, hipStream_t s);
hipError_t launch_scene_distance_dyn(const SceneDistDynArgs& a, hipStream_t s);
hipError_t launch_scene_sdf_rows(const SceneSdfArgs& a, hipStream_t s);
// scene_grid.hip: the three queries of an indexed set (a.sc.ghdr != nullptr), the bits of the brute-force kernels
hipError_t launch_scene_render_grid(const SceneRenderArgs& a, hipStream_t s);
hipError_t launch_scene_distance_grid(const SceneDistArgs& a, hipStream_t s);
hipError_t launch_scene_sdf_rows_grid(const SceneSdfArgs& a, hipStream_t s);
// scene_grid.hip: the same queries of a mixed set (a.sc.ghdr, dyn and mcount all non-null): the minimum over the
// indexed static primitives and the movers at the query's time
hipError_t launch_scene_render_mixed(const SceneRenderDynArgs& a, hipStream_t s);
hipError_t launch_scene_distance_mixed(const SceneDistDynArgs& a, hipStream_t s);
hipError_t launch_scene_sdf_rows_mixed(const SceneSdfArgs& a, hipStream_t s);
// scene_swept.hip: one kernel per kind of set -- plain, dynamic, indexed, mixed -- over the distance functions above
hipError_t launch_scene_swept(const SceneSweptArgs& a, hipStream_t s);
hipError_t launch_scene_swept_dyn(const SceneSweptArgs& a, hipStream_t s);
hipError_t launch_scene_swept_grid(const SceneSweptArgs& a, hipStream_t s);
hipError_t launch_scene_swept_mixed(const SceneSweptArgs& a, hipStream_t s);
// scene_mesh.hip, and scene_swept.hip's kernel over its distance function: the queries of a mesh set
hipError_t launch_scene_render_mesh(const MeshRenderArgs& a, hipStream_t s);
hipError_t launch_scene_distance_mesh(const MeshDistArgs& a, hipStream_t s);
hipError_t launch_scene_swept_mesh(const SceneSweptArgs& a, hipStream_t s);
hipError_t launch_scene_sdf_rows_mesh(const SceneSdfArgs& a, hipStream_t s);  // a.mesh.hdr != nullptr
// the same four of a mesh set with movers: the minimum over the mesh and the movers at the query's time
hipError_t launch_scene_render_mesh_mixed(const MeshRenderMixedArgs& a, hipStream_t s);
hipError_t launch_scene_distance_mesh_mixed(const MeshDistMixedArgs& a, hipStream_t s);
hipError_t launch_scene_swept_mesh_mixed(const SceneSweptArgs& a, hipStream_t s);
hipError_t launch_scene_sdf_rows_mesh_mixed(const SceneSdfArgs& a, hipStream_t s);  // a.mesh.hdr, a.dyn, a.mcount
// scene_inst.hip, and scene_swept.hip's kernel over its distance function: the queries of an instanced set
hipError_t launch_scene_render_inst(const InstRenderArgs& a, hipStream_t s);
hipError_t launch_scene_distance_inst(const InstDistArgs& a, hipStream_t s);
hipError_t launch_scene_swept_inst(const InstSweptArgs& a, hipStream_t s);
hipError_t launch_scene_sdf_rows_inst(const InstSdfArgs& a, hipStream_t s);

}  // namespace sdfn
