// gm_simplify.hip -- the arithmetic of mesh simplification: gm_mesh_quadrics gives every vertex its error quadric (Garland & Heckbert 1997),
// gm_mesh_collapse_round picks one round of edge collapses that can all be applied at once.  The stage behind mesh_simplify.simplify, which
// takes a surface-nets proxy mesh (its face count set by the grid) down to the ~15 k faces every later stage is sized for.
//
// THE RESULT IS DEFINED BY ARITHMETIC (the contract gm_tsdf.hip has): everything in float32, no contraction (file pragma), correctly rounded
// sqrt and division, the order of operations as written here; tests/simplify_ref.py restates it in numpy, bit for bit.
// dot(x, y) = (x.x y.x + x.y y.y) + x.z y.z, cross(x, y) = (x.y y.z - x.z y.y, x.z y.x - x.x y.z, x.x y.y - x.y y.x).
//
// SUBSET PLACEMENT: a collapse i -> j removes vertex i and moves nothing; the output vertices are rows of the input.  The quadrics are the
// only floating-point state.
//
// gm_mesh_quadrics: Q[v] = 10 floats, the upper triangle of the 4 x 4 quadric in row order 00 01 02 03 11 12 13 22 23 33, from 0, over the
// faces of v in the order of the vertex -> face CSR (deform.vertex_face_adjacency: ascending face id), per face (a, b, c):
//     n = cross(b - a, c - a), l = sqrt(dot(n, n)); not (l > 0 and l <= FLT_MAX): the face adds nothing (zero area, a NaN or an overflow)
//     u = n / l per component, p = (u.x, u.y, u.z, -dot(u, a)), area = l * 0.5f;  Q[k] = Q[k] + area * (p_r * p_c)   for k = (r, c)
//   One thread per vertex, a gather: no float atomics.
//
// gm_mesh_collapse_round, on the live faces.  Given (integer bookkeeping the caller does with sort / unique / cumsum): the unique undirected
// edges (lo, hi), lo < hi, sorted by lo Vm + hi - an edge's index is its id e -, each edge's face count, the vertex -> face CSR.
//   locked[v]: v is an end of an edge whose face count != 2 (borders, and the four-face edges naive surface nets leave).
//   candidates: per edge with face count 2, per direction i -> j (i removed) whose i is not locked:
//     link:  the distinct vertices w (w != i, w != j) that share a face with i and share a face with j are exactly 2, and no face of i
//            without j has its other two corners in one face of j (the edge part of the link condition: a tetrahedron never folds flat,
//            no collapse makes two faces over the same three vertices)
//     flip:  over every face of i that does not hold j, (p0, p1, p2) its corners' positions in row order, n0 = cross(p1 - p0, p2 - p0), n1 the
//            same with V[j] at i's corner, d = dot(n0, n1), s = dot(n0, n0) * dot(n1, n1): the direction stands only if for every such face
//            d > 0 and d d <= FLT_MAX and s <= FLT_MAX and d d >= min_cos^2 * s   (every comparison false on NaN; min_cos^2 rounded once)
//     cost:  q[k] = Q[i][k] + Q[j][k], (x, y, z) = V[j],
//            r0 = ((q00 x + q01 y) + q02 z) + q03, r1 = ((q01 x + q11 y) + q12 z) + q13, r2 = ((q02 x + q12 y) + q22 z) + q23,
//            r3 = ((q03 x + q13 y) + q23 z) + q33, c = ((x r0 + y r1) + z r2) + r3; not |c| <= FLT_MAX: rejected; cost = c > 0 ? c : +0;
//            cost > max_error: rejected (max_error = +inf: no bound)
//     the edge keeps the cheaper direction that stands; on a tie it removes the larger id (hi -> lo).  key = (bits of cost) << 32 | e as an
//     unsigned 64-bit value (the bits of a non-negative float order as integers); no direction stands: key = all ones, from = to = -1.
//   selection: vmin[v] = the least key among the candidate edges at v (all ones: none).  Candidate e = (i, j) is selected iff
//     key(e) == min of vmin[u] over u in N[i] + N[j] + {i, j}  (N[v]: the corners of the faces of v).
//   WHY A ROUND'S COLLAPSES COMMUTE.  Let e and e' be selected and an end u of e' lie in the closed neighbourhood of an end x of e.  e' is a
//   candidate at u, so vmin[u] <= key(e'), and e is selected, so key(e) <= vmin[u]: key(e) <= key(e').  Adjacency is symmetric: x lies in the
//   closed neighbourhood of u, an end of e', so key(e') <= vmin[x] <= key(e).  The keys are equal, they hold the edge id, e = e'.  Hence no
//   end of another selected edge is i, j or a neighbour of either.  A face that i -> j changes holds i; one that i' -> j' changes holds i';
//   a common one would make i' a neighbour of i: the face sets are disjoint.  The corners the flip test of i read are neighbours of i and j
//   itself: none of them is removed, and nothing ever moves.  N[i] and N[j] change only if i or j neighbours a removed vertex or is a
//   target: the link test stays true.  So every selected collapse is still valid after any subset of the others; all j are distinct and
//   no j is an i.
//   vmin is a 64-bit atomicMin, the count an integer atomicAdd: order-independent, the same bits every run.  No workgroup waits for
//   another: the phases (clear, lock, candidates, selection) meet at launch boundaries.
// Cost: one thread per edge walks the faces of both ends; the link test compares every corner at i with the corners before it and with the
// faces of j, so an edge costs O(valence(i)^2 + valence(i) valence(j)) face reads.  Surface-nets meshes have valences of 4 to 8; a mesh
// with a vertex of valence in the thousands makes the threads of its edges run millions of iterations while their waves wait.
// Vertex ids read from faces and edges, face ids and offsets read from the CSR are forced into range: no fault, no meaning.
// Conventions of gm_closest_face: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#pragma clang fp contract(off)   // every product and sum rounds on its own, as the definition above says

namespace gm {

#define SP_NONE 0xFFFFFFFFFFFFFFFFull
#define SP_FLT_MAX 3.4028234663852886e38f

struct SpMesh {
  int Vm, F;
  const float* __restrict__ V;
  const int* __restrict__ faces;
  const int* __restrict__ off;
  const int* __restrict__ adj;
  __device__ __forceinline__ int vid(int v) const { return clamp_index(v, Vm); }
  __device__ __forceinline__ void range(int v, int& b, int& e) const {
    const int nnz = 3 * F;
    b = off[v]; e = off[v + 1];
    b = b < 0 ? 0 : (b > nnz ? nnz : b);
    e = e < b ? b : (e > nnz ? nnz : e);
  }
  __device__ __forceinline__ void face(int s, int id[3]) const {
    int f = adj[s];
    f = f < 0 ? 0 : (f >= F ? F - 1 : f);
    id[0] = vid(faces[3 * (size_t)f]); id[1] = vid(faces[3 * (size_t)f + 1]); id[2] = vid(faces[3 * (size_t)f + 2]);
  }
  __device__ __forceinline__ void pos(int v, float p[3]) const { p[0] = V[3 * (size_t)v]; p[1] = V[3 * (size_t)v + 1]; p[2] = V[3 * (size_t)v + 2]; }
};

struct SpWs {
  unsigned long long* vmin;      // [Vm] least candidate key at the vertex
  uint8_t* locked;               // [Vm]
  char* end;
  static SpWs from(void* ws, size_t Vm) {
    char* p = reinterpret_cast<char*>(ws);
    SpWs k;
    k.vmin = carve<unsigned long long>(p, Vm);
    k.locked = carve<uint8_t>(p, Vm);
    k.end = p;
    return k;
  }
};

__device__ __forceinline__ float sp_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void sp_normal(const float p0[3], const float p1[3], const float p2[3], float n[3]) {
  const float x[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, y[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  n[0] = x[1] * y[2] - x[2] * y[1];
  n[1] = x[2] * y[0] - x[0] * y[2];
  n[2] = x[0] * y[1] - x[1] * y[0];
}

__global__ __launch_bounds__(256) void sp_quadrics(SpMesh m, float* __restrict__ Q) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= m.Vm) return;
  int b, e;
  m.range(v, b, e);
  float q[10];
#pragma unroll
  for (int k = 0; k < 10; k++) q[k] = 0.f;
  for (int s = b; s < e; s++) {
    int id[3];
    m.face(s, id);
    float pa[3], pb[3], pc[3], n[3];
    m.pos(id[0], pa); m.pos(id[1], pb); m.pos(id[2], pc);
    sp_normal(pa, pb, pc, n);
    const float l = sqrtf(sp_dot(n, n));
    if (!(l > 0.f && l <= SP_FLT_MAX)) continue;
    float p[4] = {n[0] / l, n[1] / l, n[2] / l, 0.f};
    p[3] = -sp_dot(p, pa);
    const float area = l * 0.5f;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = r; c < 4; c++, k++) q[k] = q[k] + area * (p[r] * p[c]);
  }
#pragma unroll
  for (int k = 0; k < 10; k++) Q[10 * (size_t)v + k] = q[k];
}

// ---- one round ----
__global__ __launch_bounds__(256) void sp_clear(int Vm, unsigned long long* __restrict__ vmin, uint8_t* __restrict__ locked, int* __restrict__ count) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v == 0) *count = 0;
  if (v >= Vm) return;
  vmin[v] = SP_NONE;
  locked[v] = 0;
}

__global__ __launch_bounds__(256) void sp_lock(int Vm, int E, const int* __restrict__ edges, const int* __restrict__ uses, uint8_t* __restrict__ locked) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E || uses[e] == 2) return;
  const int lo = edges[2 * (size_t)e], hi = edges[2 * (size_t)e + 1];
  locked[clamp_index(lo, Vm)] = 1;       // (every writer stores the same byte)
  locked[clamp_index(hi, Vm)] = 1;
}

// does w hold a corner of a face of a
__device__ bool sp_adjacent(const SpMesh& m, int a, int w) {
  int b, e;
  m.range(a, b, e);
  for (int s = b; s < e; s++) {
    int id[3];
    m.face(s, id);
    if (id[0] == w || id[1] == w || id[2] == w) return true;
  }
  return false;
}

// the distinct w outside {i, j} that share a face with i and with j (counted at their first appearance in the walk over the faces of i)
__device__ int sp_common(const SpMesh& m, int i, int j) {
  int b, e, n = 0;
  m.range(i, b, e);
  for (int s = b; s < e; s++) {
    int id[3];
    m.face(s, id);
    for (int c = 0; c < 3; c++) {
      const int w = id[c];
      if (w == i || w == j) continue;
      bool seen = false;
      for (int s2 = b; s2 <= s && !seen; s2++) {
        int id2[3];
        m.face(s2, id2);
        const int lim = s2 == s ? c : 3;
        for (int c2 = 0; c2 < lim; c2++) seen = seen || id2[c2] == w;
      }
      if (!seen && sp_adjacent(m, j, w)) n++;
    }
  }
  return n;
}

// a face of i without j and a face of j without i hold the same two other corners: the collapse would fold them onto each other
__device__ bool sp_shared_opposite(const SpMesh& m, int i, int j) {
  int b, e, bj, ej;
  m.range(i, b, e);
  m.range(j, bj, ej);
  for (int s = b; s < e; s++) {
    int id[3];
    m.face(s, id);
    if (id[0] == j || id[1] == j || id[2] == j) continue;
    const int c = id[0] == i ? 0 : (id[1] == i ? 1 : 2);
    const int x = id[(c + 1) % 3], y = id[(c + 2) % 3];
    for (int t = bj; t < ej; t++) {
      int jd[3];
      m.face(t, jd);
      if ((jd[0] == x || jd[1] == x || jd[2] == x) && (jd[0] == y || jd[1] == y || jd[2] == y)) return true;
    }
  }
  return false;
}

// flip test and cost of i -> j; false: the direction does not stand
__device__ bool sp_direction(const SpMesh& m, const float* __restrict__ Q, int i, int j, float mc2, float max_error, float& cost) {
  float xj[3];
  m.pos(j, xj);
  int b, e;
  m.range(i, b, e);
  for (int s = b; s < e; s++) {
    int id[3];
    m.face(s, id);
    if (id[0] == j || id[1] == j || id[2] == j) continue;
    float p[3][3], n0[3], n1[3];
#pragma unroll
    for (int c = 0; c < 3; c++) m.pos(id[c], p[c]);
    sp_normal(p[0], p[1], p[2], n0);
#pragma unroll
    for (int c = 0; c < 3; c++)
      if (id[c] == i) { p[c][0] = xj[0]; p[c][1] = xj[1]; p[c][2] = xj[2]; }
    sp_normal(p[0], p[1], p[2], n1);
    const float d = sp_dot(n0, n1), sq = sp_dot(n0, n0) * sp_dot(n1, n1), dd = d * d;
    if (!(d > 0.f && dd <= SP_FLT_MAX && sq <= SP_FLT_MAX && dd >= mc2 * sq)) return false;
  }
  float q[10];
#pragma unroll
  for (int k = 0; k < 10; k++) q[k] = Q[10 * (size_t)i + k] + Q[10 * (size_t)j + k];
  const float x = xj[0], y = xj[1], z = xj[2];
  const float r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3];
  const float r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6];
  const float r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8];
  const float r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9];
  const float c = ((x * r0 + y * r1) + z * r2) + r3;
  if (!(fabsf(c) <= SP_FLT_MAX)) return false;
  cost = c > 0.f ? c : 0.f;
  return !(cost > max_error);
}

__global__ __launch_bounds__(256) void sp_candidates(SpMesh m, const float* __restrict__ Q, int E, const int* __restrict__ edges,
                                                     const int* __restrict__ uses, float mc2, float max_error, const uint8_t* __restrict__ locked,
                                                     unsigned long long* __restrict__ vmin, int* __restrict__ from, int* __restrict__ to,
                                                     unsigned long long* __restrict__ key) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  unsigned long long k = SP_NONE;
  int fi = -1, tj = -1;
  if (uses[e] == 2) {
    const int lo = m.vid(edges[2 * (size_t)e]), hi = m.vid(edges[2 * (size_t)e + 1]);
    const bool free_lo = !locked[lo], free_hi = !locked[hi];
    if (lo != hi && (free_lo || free_hi) && sp_common(m, lo, hi) == 2 && !sp_shared_opposite(m, lo, hi)) {
      float c_hi = 0.f, c_lo = 0.f;
      const bool ok_hi = free_hi && sp_direction(m, Q, hi, lo, mc2, max_error, c_hi);      // hi -> lo: removes the larger id
      const bool ok_lo = free_lo && sp_direction(m, Q, lo, hi, mc2, max_error, c_lo);
      if (ok_hi || ok_lo) {
        const bool take_lo = ok_lo && (!ok_hi || c_lo < c_hi);
        fi = take_lo ? lo : hi;
        tj = take_lo ? hi : lo;
        k = ((unsigned long long)__float_as_uint(take_lo ? c_lo : c_hi) << 32) | (unsigned long long)(unsigned)e;
        atomicMin(&vmin[lo], k);
        atomicMin(&vmin[hi], k);
      }
    }
  }
  from[e] = fi;
  to[e] = tj;
  key[e] = k;
}

__device__ unsigned long long sp_ring_min(const SpMesh& m, const unsigned long long* __restrict__ vmin, int v) {
  unsigned long long r = vmin[v];
  int b, e;
  m.range(v, b, e);
  for (int s = b; s < e; s++) {
    int id[3];
    m.face(s, id);
#pragma unroll
    for (int c = 0; c < 3; c++) { const unsigned long long x = vmin[id[c]]; r = x < r ? x : r; }
  }
  return r;
}

__global__ __launch_bounds__(256) void sp_select(SpMesh m, int E, const int* __restrict__ from, const int* __restrict__ to,
                                                 const unsigned long long* __restrict__ key, const unsigned long long* __restrict__ vmin,
                                                 uint8_t* __restrict__ selected, int* __restrict__ count) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const unsigned long long k = key[e];
  uint8_t sel = 0;
  if (k != SP_NONE) {
    const unsigned long long a = sp_ring_min(m, vmin, from[e]), b = sp_ring_min(m, vmin, to[e]);
    sel = k == (a < b ? a : b) ? 1 : 0;
    if (sel) atomicAdd(count, 1);
  }
  selected[e] = sel;
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_mesh_collapse_round_workspace_bytes(int Vm) {
  SpWs k = SpWs::from(nullptr, (size_t)(Vm > 0 ? Vm : 0));
  return (size_t)k.end + 256;
}

int gm_mesh_quadrics(int Vm, const float* vertices, int F, const int* faces, const int* vf_offsets, const int* vf_faces, float* out_quadrics,
                     void* stream) {
  const char* fn = "gm_mesh_quadrics";
  if (Vm < 0 || F < 0) { set_error("%s: negative size Vm=%d F=%d", fn, Vm, F); return GM_ERR_INVALID_ARG; }
  if (F > 0x7FFFFFFF / 3) { set_error("%s: F=%d: 3 F must fit an int", fn, F); return GM_ERR_INVALID_ARG; }
  if (Vm == 0) return GM_OK;
  if (!vertices || !vf_offsets || !out_quadrics || (F > 0 && (!faces || !vf_faces))) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  const ByteRange rg[5] = {{vertices, 12 * (size_t)Vm, "vertices", false}, {faces, 12 * (size_t)F, "faces", false},
                           {vf_offsets, 4 * ((size_t)Vm + 1), "vf_offsets", false}, {vf_faces, 12 * (size_t)F, "vf_faces", false},
                           {out_quadrics, 40 * (size_t)Vm, "out_quadrics", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const SpMesh m = {Vm, F, vertices, faces, vf_offsets, vf_faces};
  hipLaunchKernelGGL(sp_quadrics, dim3((unsigned)((Vm + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), m, out_quadrics);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_mesh_collapse_round(int Vm, const float* vertices, const float* quadrics, int F, const int* faces, const int* vf_offsets, const int* vf_faces,
                           int E, const int* edges, const int* edge_faces, float min_cos, float max_error, unsigned char* out_selected, int* out_from,
                           int* out_to, unsigned long long* out_key, int* out_count, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_mesh_collapse_round";
  if (Vm < 0 || F < 0 || E < 0) { set_error("%s: negative size Vm=%d F=%d E=%d", fn, Vm, F, E); return GM_ERR_INVALID_ARG; }
  if (F > 0x7FFFFFFF / 3) { set_error("%s: F=%d: 3 F must fit an int", fn, F); return GM_ERR_INVALID_ARG; }
  if (!(min_cos >= 0.f) || min_cos > 3.4028234e38f) { set_error("%s: min_cos must be >= 0, finite and not NaN", fn); return GM_ERR_INVALID_ARG; }
  if (!(max_error >= 0.f)) { set_error("%s: max_error must be >= 0 and not NaN (+inf: no bound)", fn); return GM_ERR_INVALID_ARG; }
  if (E == 0) return GM_OK;
  if (Vm == 0 || F == 0) { set_error("%s: %d edges of an empty mesh (Vm == %d, F == %d)", fn, E, Vm, F); return GM_ERR_INVALID_ARG; }
  if (!vertices || !quadrics || !faces || !vf_offsets || !vf_faces || !edges || !edge_faces || !out_selected || !out_from || !out_to || !out_key ||
      !out_count || !workspace) {
    set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG;
  }
  if (reinterpret_cast<uintptr_t>(out_key) & 7) { set_error("%s: out_key must be 8-byte aligned", fn); return GM_ERR_INVALID_ARG; }
  const ByteRange rg[13] = {{vertices, 12 * (size_t)Vm, "vertices", false}, {quadrics, 40 * (size_t)Vm, "quadrics", false}, {faces, 12 * (size_t)F, "faces", false},
                            {vf_offsets, 4 * ((size_t)Vm + 1), "vf_offsets", false}, {vf_faces, 12 * (size_t)F, "vf_faces", false},
                            {edges, 8 * (size_t)E, "edges", false}, {edge_faces, 4 * (size_t)E, "edge_faces", false},
                            {out_selected, (size_t)E, "out_selected", true}, {out_from, 4 * (size_t)E, "out_from", true}, {out_to, 4 * (size_t)E, "out_to", true},
                            {out_key, 8 * (size_t)E, "out_key", true}, {out_count, 4, "out_count", true}, {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = gm_mesh_collapse_round_workspace_bytes(Vm);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SpWs k = SpWs::from(workspace, (size_t)Vm);
  const SpMesh m = {Vm, F, vertices, faces, vf_offsets, vf_faces};
  const float mc2 = min_cos * min_cos;
  const dim3 threads(256), vb((unsigned)((Vm + 255) / 256)), eb((unsigned)((E + 255) / 256));
  hipLaunchKernelGGL(sp_clear, vb, threads, 0, s, Vm, k.vmin, k.locked, out_count);
  hipLaunchKernelGGL(sp_lock, eb, threads, 0, s, Vm, E, edges, edge_faces, k.locked);
  hipLaunchKernelGGL(sp_candidates, eb, threads, 0, s, m, quadrics, E, edges, edge_faces, mc2, max_error, k.locked, k.vmin, out_from, out_to, out_key);
  hipLaunchKernelGGL(sp_select, eb, threads, 0, s, m, E, out_from, out_to, out_key, k.vmin, out_selected, out_count);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
