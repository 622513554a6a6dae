/*
 * gmesh_hip.h -- C ABI of libgmesh_hip.so: the MI355X (gfx950) implementation of the GaussianMesh
 * hot path.  Plain pointers and sizes only; every device pointer is a HIP device address, every
 * call is stream-ordered on `stream` (a hipStream_t passed as void*; NULL = the null stream).
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repo root; RAST = gaussian_renderer/diff_gaussian_rasterizater/cuda_rasterizer).  The reference
 * exposes these as C++ static members called from Jittor `jt.code` JIT stubs
 * (rasterize_points.py:123-190, 197-269, 311-396); INTEGRATION.md shows the stub a maintainer
 * would write against this header instead.
 *
 * Conventions shared by all calls
 *   - return value: 0 = GM_OK, otherwise a GM_ERR_* code; gm_last_error() gives a thread-local
 *     human-readable message (replaces the C++ exceptions of RAST/rasterizer_impl.cu:372-375 and
 *     the CHECK_CUDA macro, RAST/auxiliary.h:165-172).
 *   - `debug` != 0: synchronise and check for errors after every kernel launch (CHECK_CUDA semantics).
 *   - ownership: the caller owns every buffer; the library never allocates device memory
 *     (as in the reference, where python allocates geomBuffer/binningBuffer/imgBuffer,
 *     rasterize_points.py:118-121, 192-194).  Scratch buffers are opaque; their layout depends only
 *     on (base address mod 256, P/R/W/H) so the SAME buffers at the SAME addresses must be passed to
 *     gm_forward_1 and gm_backward after gm_forward_0 (reference: rasterizer_impl.cu:546-548).
 *   - nullable inputs: shs | colors_precomp (exactly one), (scales,rotations) | cov3D_precomp
 *     (exactly one), radii (optional output).  NULL means "feature off" for all of them.
 *   - all float data is IEEE binary32, contiguous, in the layouts of the reference python boundary:
 *     means3D [P,3], shs [P,M,3], colors_precomp [P,3], opacities [P], scales [P,3],
 *     rotations [P,4] (r,x,y,z), cov3D_precomp [P,6] (xx,xy,xz,yy,yz,zz),
 *     viewmatrix/projmatrix 16 floats (the transposed 4x4 of scene/cameras.py:47-49),
 *     cam_pos 3 floats, background 3 floats, out_color planar [3,H,W].
 */
#ifndef GMESH_HIP_H_INCLUDED
#define GMESH_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GM_OK 0
#define GM_ERR_INVALID_ARG 1   /* bad size / null where not allowed / misuse */
#define GM_ERR_HIP 2           /* a HIP runtime call or kernel failed */
#define GM_ERR_BUFFER 3        /* a caller-provided buffer is too small */

/* ABI version of this header; bumped on any signature change. */
#define GM_ABI_VERSION 3
int gm_abi_version(void);
const char* gm_last_error(void);

/* Instance emission policy: an ARGUMENT of the extended entry points (gm_forward_0_async, gm_forward_0_deformed_async,
 * gm_forward_1_geom, gm_backward_p, gm_binning_field); the entry points with the reference's signatures (gm_forward_0,
 * gm_forward_1, gm_backward) use GM_POLICY_DEFAULT.  The library keeps no policy state: calls on distinct buffers are
 * independent and thread-safe.  The halves of one pass must be given the same policy; it is latched in the geometry
 * buffer by the first half, and a second half under another policy emits nothing and renders the background.
 * out_color, radii and all gradients are the same under every policy; num_rendered and the internal lists differ.
 *   0: emit every tile of the bounding rectangle exactly as the reference does (RAST/rasterizer_impl.cu:98-109);
 *      num_rendered, point_list and ranges are then identical to the reference's.
 *   1: a (Gaussian, tile) instance is emitted only if the Gaussian can reach alpha >= 1/255 somewhere in the 16x16
 *      tile (exact conservative test).  Dropped instances are skipped by every pixel of the tile in the reference too
 *      (RAST/forward.cu:344).
 *   2 (default), 3: the same test, but instances are (Gaussian, PARENT tile) pairs for parents of 2x2 / 4x4 tiles; the
 *      key of an instance carries the mask of the parent's child tiles the Gaussian reaches (bits 16+), and the 16x16
 *      blend workgroups walk their parent's list.  The instance stream (and the sort over it) shrinks ~2x / ~3x. */
#define GM_POLICY_REFERENCE 0
#define GM_POLICY_DEFAULT 2

/* Scratch sizes.  Replace CudaRasterizer::required<GeometryState|ImageState|BinningState>(n)
 * (RAST/rasterizer_impl.h:67-73; python side rasterize_points.py:63-86). */
size_t gm_geom_bytes(int P);
size_t gm_image_bytes(int W, int H);
size_t gm_work_hint_bytes(int W, int H);      /* gm_forward_1_geom's optional work_hint buffer */
size_t gm_binning_bytes(int64_t num_rendered);

/* Replaces CudaRasterizer::Rasterizer::forward_0 (RAST/rasterizer.h:31-51, rasterizer_impl.cu:338-413):
 * per-Gaussian preprocess (cull, cov3D, EWA cov2D, conic, radius, tile rect, SH->RGB) and the
 * count of (Gaussian, tile) instances.  Performs the ONE host synchronisation of a forward pass
 * (reference: cudaMemcpy D2H at rasterizer_impl.cu:411) and stores the count in *num_rendered.
 * radii (int32 [P], may be NULL) receives the screen radius (0 = culled).
 * Frame sizes (every forward entry point, the batched ones included; refused on the arguments alone): at most 65536 list tiles under
 * the emission policy (2048 for a batch), and under EVERY policy a grid of at most 4095 x 4095 16-px tiles (65520 pixels a side) - a
 * Gaussian's tile rectangle travels in 12 bits per field. */
int gm_forward_0(void* geom_buffer, int P, int D, int M, const float* background, int width, int height,
                 const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                 const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                 const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                 float tan_fovy, int prefiltered, int* radii, int debug, void* stream, int* num_rendered);

/* gm_forward_0 without its host synchronisation, with the emission policy as an argument: everything is enqueued on
 * `stream`, including a copy of the instance count into *num_rendered_host (page-locked host memory; may be NULL), issued as
 * soon as the count is known (before the depth ordering finishes).  count_event (a hipEvent_t, may be NULL) is recorded
 * right behind that copy: the caller keeps feeding the GPU (e.g. the next frame's gm_forward_0_async on another stream)
 * and completes the frame with gm_forward_1_geom once the event has fired.  This hides the one host round trip of the
 * reference design; gm_forward_1_geom's sync-free mode removes it. */
int gm_forward_0_async(int emission_policy, void* geom_buffer, int P, int D, int M, const float* background, int width, int height,
                       const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                       const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                       float tan_fovy, int prefiltered, int* radii, int debug, void* stream, int* num_rendered_host,
                       void* count_event);

/* Replaces CudaRasterizer::Rasterizer::forward_1 (RAST/rasterizer.h:53-76, rasterizer_impl.cu:416-511):
 * instance emission, (tile, depth) ordering, tile ranges, front-to-back alpha blend.
 * binning_buffer must hold gm_binning_bytes(num_rendered), image_buffer gm_image_bytes(W,H). */
int gm_forward_1(void* geom_buffer, void* binning_buffer, void* image_buffer, int P, int D, int M, int num_rendered,
                 const float* background, int width, int height, const float* means3D, const float* shs,
                 const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                 const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color, int* radii,
                 int debug, void* stream);

/* Replaces CudaRasterizer::Rasterizer::backward (RAST/rasterizer.h:103-132, rasterizer_impl.cu:515-609).
 * Gradient outputs: dL_dmean2D [P,3] (x,y used), dL_dconic [P,4] (slots 0,1,3 used), dL_dopacity [P],
 * dL_dcolor [P,3], dL_dmean3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3], dL_dscale [P,3], dL_drot [P,4].
 * Unlike the reference (which needs them zero-filled by the caller, rasterize_points.py:302-310) the
 * library zeroes every gradient output itself, so on return they hold exactly this pass's gradients.
 * dL_dsh may be NULL when shs is NULL; dL_dscale/dL_drot may be NULL when scales is NULL.  The intermediates of the chain rule may be
 * declined with NULL (they are then not written: 52 of ~600 bytes per Gaussian): dL_dconic always, dL_dcolor when shs is given,
 * dL_dcov3D when scales is given. */
int gm_backward(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                const float* campos, float tan_fovx, float tan_fovy, const int* radii, void* geom_buffer,
                void* binning_buffer, void* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                float* dL_dscale, float* dL_drot, int debug, void* stream);

/* gm_backward for lists built under an explicit emission policy (the one given to the forward halves). */
int gm_backward_p(int emission_policy, int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                  const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                  const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                  const float* campos, float tan_fovx, float tan_fovy, const int* radii, void* geom_buffer,
                  void* binning_buffer, void* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                  float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                  float* dL_dscale, float* dL_drot, int debug, void* stream);

/* gm_backward_p with the gradients of gm_forward_1_aux's maps (backward.cu:399-557 with two more colour channels: depth, of
 * colour z_i, and alpha, of colour 1, both with background 0).  dL_ddepth / dL_dalpha: [H,W], either may be NULL; with both NULL
 * this is gm_backward_p.  Their terms enter dL/dalpha of every (entry, pixel) and so the opacity, conic and mean2D chain;
 * dL/dz_i = sum over pixels of dL/ddepth alpha_i T_i becomes dL_dmean3D += dL/dz_i (viewmatrix[2], viewmatrix[6], viewmatrix[10]).
 * dL_dz ([P], may be NULL) receives dL/dz_i itself; it may not overlap dL_dmean3D, dL_dmean2D or dL_dopacity.  The forward must
 * have kept its state (not GM_FWD_IMAGE_ONLY), as for gm_backward_p. */
int gm_backward_aux(int emission_policy, int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                    const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                    const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                    const float* campos, float tan_fovx, float tan_fovy, const int* radii, void* geom_buffer,
                    void* binning_buffer, void* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                    float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                    float* dL_dscale, float* dL_drot, const float* dL_ddepth, const float* dL_dalpha, float* dL_dz, int debug, void* stream);

/* gm_backward_p for a TRAINING step whose SH rows are the optimizer's parameter (scene/mesh_based_gaussian_model.py:242-263: the "f_dc" and
 * "f_rest" groups of training_setup; jittor.nn.Adam): the Adam step of those rows is applied inside the backward pass instead of by
 * gm_adam_step afterwards.  dL/dSH of a Gaussian is produced whole by the thread that owns it (RAST/backward.cu:20-139), so the 192-byte
 * gradient row never has to travel: per trainable Gaussian 192 B of dL/dSH written + read and 192 B of parameter read disappear (at SH
 * degree 3, where 27 000 of the reference's 30 000 iterations run, the SH group is 48 of a Gaussian's 59 parameters).
 *   shs [P,16,3]: updated IN PLACE for rows [0, rows) (rows behind them - a frozen cloud sharing the operand - are read only);
 *   exp_avg / exp_avg_sq [rows,16,3]: Adam's moments; lr_dc steps coefficient 0, lr_rest the others; step >= 1 = the step being taken;
 *   the update is m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps), element for
 *   element what gm_adam_step computes from the same gradient (culled Gaussians: g = 0, their moments decay and p moves, as in the reference).
 * dL/dSH, dL/dcolour and dL/dconic are not produced.  The backward of a REFUSED forward (sync-free capacity overflow: zero gradients, the
 * caller repeats the iteration) leaves parameter and moments untouched.  colors_precomp input is not supported (nothing to step). */
int gm_backward_sh_step(int emission_policy, int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                        float* shs, const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                        const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                        void* geom_buffer, void* binning_buffer, void* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dopacity,
                        float* dL_dmean3D, float* dL_dcov3D, float* dL_dscale, float* dL_drot, int rows, float* exp_avg, float* exp_avg_sq,
                        float lr_dc, float lr_rest, double beta1, double beta2, double eps, int step, int debug, void* stream);

/* Replaces CudaRasterizer::Rasterizer::markVisible (RAST/rasterizer.h:24-29, rasterizer_impl.cu:141-153).
 * present: uint8 [P], 1 if view-space z > 0.2. */
int gm_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                    void* stream);

/* Read-only views into the opaque scratch buffers (tests / debugging; the reference exposes the
 * same data as the GeometryState/ImageState/BinningState structs, RAST/rasterizer_impl.h:29-65).
 * Each returns a device pointer inside the given buffer, or NULL for an unknown name.
 *   geom:    "splat" float[P][gm_splat_floats()] = {x,y,conic.x,conic.y | conic.z,opacity,r,g | b} (9 floats: the record the blend
 *            kernels gather), "depth_key" uint32[P] (float bits of the view-space depth, 0xFFFFFFFF for a culled Gaussian; not
 *            written by the direct depth placement),
 *            "radii" int32[P] (internal copy: filled only by a forward that was given NO radii array; gm_backward reads it when it
 *            is given none either - pass the forward's array otherwise), "tiles_touched" uint32[P] (gm_forward_0_deformed_async
 *            fills it only for rectangles of 65535 instances or more: the count rides in the emission record), "cov3D" float[P][6],
 *            "clamped" uint8[P] (bit ch set = channel ch clamped), "order" uint32[V] (ids of the V visible Gaussians
 *            in (depth, id) order; V = "bucket_start"[2048]), "bucket_start" uint32[2049], "counters" uint32[32], and the depth-bucket
 *            table of the frame, for tests that ask which route the ordering took: "dmap" uint32[2048] (coarse bin key >> 20 ->
 *            first bucket << 16 | buckets), "bmap" uint32[2048][2] (bucket -> first key, bits of the key range; partition path only);
 *            the emission's inputs: "bin" uint32[P][4] (the emission record of each Gaussian, written by the preprocess kernels of the
 *            partition path and read in place), "inst16" uint16[P] (the record's instance count: 0xFFFF = 65535 or more, see
 *            "tiles_touched"; 0 for a culled row), "bin_sorted" uint32[V][4] (the records in depth order: direct placement only);
 *            "grad_acc" float[P][12] (the backward pass's accumulators: the last field, gm_geom_bytes(P) ends 256 bytes behind it)
 *   image:   "final_T" float[H*W], "n_contrib" uint32[H*W], "ranges" uint32[T][2], "tile_order" uint32[T] (the forward blend's
 *            dispatch order: a permutation of the list tiles)
 *   binning: "pairs" uint32[R][2] = (list tile id | child mask << 16, Gaussian id) per instance, sorted by tile then
 *            (depth, id): column 1 is the reference's point_list, column 0 its sorted tile keys (child mask: policy 0/1
 *            = 1; policy 2 = the 4 x 4 8-pixel quadrants of the 32-px list tile, bit 4 qy + qx; policy 3 = the 4 x 4
 *            16-px tiles of the 64-px list tile, bit 4 ty + tx) */
int gm_splat_floats(void);
void* gm_geom_field(void* geom_buffer, int P, const char* name);
void* gm_image_field(void* image_buffer, int W, int H, const char* name);
void* gm_binning_field(void* binning_buffer, int64_t R, int W, int H, int emission_policy, const char* name);

/* Replaces SimpleKNN::knn (scene/simple_knn/cuda_headers/simple_knn.h:18, simple_knn.cu:185-221):
 * meanDists[i] = mean of the 3 smallest squared distances from point i to the other points.
 * The reference allocates its temporaries internally (cudaMalloc/thrust); here the caller passes a
 * workspace of gm_knn_workspace_bytes(P).  Performs one host synchronisation (bounding box readback,
 * as simple_knn.cu:197,200). */
size_t gm_knn_workspace_bytes(int P);
int gm_knn(int P, const float* points, float* meanDists, void* workspace, size_t workspace_bytes, void* stream);

/* Nearest reference point of every query point (k = 1): the neighbour pruning of train_bg_gaussian.py:129-137, which removes
 * background Gaussians close to the object's.  query float [Pq,3], ref float [Pr,3]; out_d2 float [Pq] = the SQUARED distance
 * (dx*dx + dy*dy) + dz*dz with d = query - ref, evaluated in float32 without contraction; out_idx int32 [Pq] = the reference
 * index, the lowest one on ties.  The result is bit-identical to a float32 brute force.  Pr == 0 is an error (refused before
 * any GPU work); Pq == 0 does nothing.  Caller workspace of gm_knn_nearest_workspace_bytes(Pq, Pr) (O(Pq + Pr)); no host
 * synchronisation. */
size_t gm_knn_nearest_workspace_bytes(int Pq, int Pr);
int gm_knn_nearest(int Pq, const float* query, int Pr, const float* ref, float* out_d2, int* out_idx, void* workspace, size_t workspace_bytes,
                   void* stream);

/* Closest triangle of a mesh for every point: what binds a plain Gaussian cloud to a proxy mesh (the branch of
 * SingleObjectDeform.load_mesh that runs without face ids, edittool/__init__.py:68-85, igl.point_mesh_squared_distance there).
 * points float [N,3], vertices float [Vm,3], faces int32 [F,3] vertex ids.  out_d2 float [N] = squared distance to the closest face,
 * out_face int32 [N] = its index, out_closest float [N,3] (may be NULL) = the closest point q on it.
 * The result is defined by arithmetic, not by the search structure: per (point p, face (a, b, c)) in float32, no contraction, correctly
 * rounded divisions, dot(u, w) = (u.x*w.x + u.y*w.y) + u.z*w.z (Ericson 5.1.5 as edittool.point_mesh_squared_distance evaluates it):
 *   ab = b - a, ac = c - a, cb = c - b;  d1 = dot(ab, p - a), d2 = dot(ac, p - a), d3 = dot(ab, p - b), d4 = dot(ac, p - b),
 *   d5 = dot(ab, p - c), d6 = dot(ac, p - c);  vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4;
 *   denom = 1 / ((va + vb) + vc), v = vb*denom, w = vc*denom;  x = d4 - d3, y = d5 - d6;
 *   q = (a + ab*v) + ac*w, replaced by the LAST of these that holds (the precedence vertex a, b, c, edge ab, ac, bc, interior):
 *     b + cb*(x / (x + y))      if va <= 0, x >= 0, y >= 0        a + ac*(d2 / (d2 - d6))   if vb <= 0, d2 >= 0, d6 <= 0
 *     a + ab*(d1 / (d1 - d3))   if vc <= 0, d1 >= 0, d3 <= 0      c   if d6 >= 0, d5 <= d6
 *     b   if d3 >= 0, d4 <= d3                                    a   if d1 <= 0, d2 <= 0
 *   e = p - q, d2(p, face) = (e.x*e.x + e.y*e.y) + e.z*e.z.
 * Winner: the smallest d2, ties to the LOWEST face index; a NaN d2 (a degenerate face: 0 / 0) never wins; if every face gives NaN the
 * point gets out_face = -1, out_d2 = +inf, out_closest = NaN.  So (out_d2, out_face, out_closest) equal a float32 brute force over all
 * F faces bit for bit, for every finite input (csrc/gm_closest.hip: the search structure and why no box that matters is skipped).
 * Refused with GM_ERR_INVALID_ARG before any GPU work: a negative size, F == 0 or Vm == 0 with N > 0, a NULL among points, vertices,
 * faces, out_d2, out_face, workspace; with GM_ERR_BUFFER: a workspace below gm_closest_face_workspace_bytes(N, F) (O(N + F), monotonic
 * in both).  N == 0 succeeds and launches nothing.  Face indices outside [0, Vm) CANNOT be checked here without a read-back: they are
 * forced into range, so such a face reads some other vertex - no fault, no meaningful result; a caller that holds the faces on the
 * host checks them there (mesh_bind.closest_faces does).  Stream-ordered, no device allocation, no host synchronisation. */
size_t gm_closest_face_workspace_bytes(int N, int F);
int gm_closest_face(int N, const float* points, int Vm, const float* vertices, int F, const int* faces, float* out_d2, int* out_face,
                    float* out_closest, void* workspace, size_t workspace_bytes, void* stream);

/* As-rigid-as-possible deformation of a proxy mesh from dragged handles (Sorkine & Alexa 2007): the deformed mesh itself, which
 * gm_mesh_rs then reads (R, S) from.  (row_offsets int32 [Vm+1], cols int32 [nnz], weights double [nnz]): the symmetric edge CSR with
 * positive weights (arap.edge_csr: per face corner opposite edge (a, b) max(0.5 cot, 1e-3), mesh_rs_kernel's weights).  V0 float
 * [Vm,3] rest vertices; fixed [Vm]: 1 = the row is held (a handle, a pinned vertex), and a row whose weights sum to 0 is held too;
 * V_init float [Vm,3] the starting positions, whose held rows already carry their targets; V_out float [Vm,3].
 *   E(P', R) = sum_i sum_j w_ij |(p'_i - p'_j) - R_i (p_i - p_j)|^2.  Per outer iteration, in float64:
 *   local:  S_i = sum_j w_ij (p'_i - p'_j)(p_i - p_j)^T, R_i = U diag(1, 1, det(U V^T)) V^T (S_i = U Sigma V^T); rank <= 1
 *           (second singular value <= 1e-12 of the first): R_i = I.  R_i is formed from the eigenvectors of S_i^T S_i, which squares
 *           the condition number: for a one-ring whose second singular value s1 is below about 1e-3 of the first, s0, R_i is that
 *           maximiser of tr(R^T S_i) only to within 8 sqrt(eps) s0 = 1.2e-7 s0 (64 eps s0 above 1e-2), and NOT element by element the
 *           SVD's rotation: it differs by a turn about the strongest direction, which costs E at most twice that bar;
 *   global: for every free row sum_j w_ij (p'_i - p'_j) = sum_j (w_ij / 2)(R_i + R_j)(p_i - p_j), the three coordinates separately by
 *           Jacobi-preconditioned conjugate gradients from the current positions, until |r|_2 <= cg_tolerance |b|_2 or cg_iterations
 *           steps; no number of steps raises E.
 * stats: NULL, or double [outer_iterations][8] = E after the local step, E after the global step, CG steps used for x / y / z, final
 * |r| / |b| for x / y / z; with NULL no energy is computed.  outer_iterations == 0 copies V_init to V_out.  V_out == V_init is allowed
 * (the state lives in the workspace); any other overlap among V0, V_init, V_out, stats and the workspace is refused.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: Vm <= 0, outer_iterations < 0, cg_iterations < 1, a cg_tolerance that is negative
 * or not finite, a NULL among row_offsets, cols, weights, V0, fixed, V_init, V_out, workspace, an overlap; with GM_ERR_BUFFER a workspace
 * below gm_arap_workspace_bytes(Vm) (O(Vm), monotonic).  The CSR cannot be checked here without a read-back: column ids are forced into
 * [0, Vm); row_offsets must ascend within the arrays (arap.ArapSolver builds all three itself).  A component of the edge graph with a
 * free row and no held one makes the system singular: the caller rules that out (ArapSolver does).
 * One workgroup per coordinate runs that column's whole solve; sums are taken in a fixed order and there are no atomics, so two calls
 * on the same input give the same bits.  Stream-ordered, no device allocation, no host synchronisation. */
size_t gm_arap_workspace_bytes(int Vm);
int gm_arap_solve(int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const unsigned char* fixed,
                  const float* V_init, int outer_iterations, int cg_iterations, double cg_tolerance, float* V_out, double* stats,
                  void* workspace, size_t workspace_bytes, void* stream);

/* gm_arap_solve with the global step spread over the whole chip: the same definition, parameters, stats layout and refusals, rows over
 * ceil(Vm / 256) workgroups that meet only at kernel boundaries (no grid barrier, no flag, no cooperative launch).  Per CG step two
 * launches (single-reduction recurrences of Chronopoulos & Gear), enqueued for the full cg_iterations: a coordinate that has converged,
 * or whose p . A p is no longer positive, is frozen, and once all three are the remaining launches return after reading the carried
 * state.  Only the order of the sums differs from gm_arap_solve, and with it the last bits; it is fixed by Vm alone, so two calls on the
 * same input give the same bits.  Its own workspace: gm_arap_grid_workspace_bytes(Vm) (O(Vm), monotonic, the same for 0 and 1).
 * cg_iterations has no upper bound here either, but each step of the cap is two host launches per outer iteration, stopped or not:
 * choose the cap near the steps wanted (the column step, whose loop leaves on the device, takes any cap for free). */
size_t gm_arap_grid_workspace_bytes(int Vm);
int gm_arap_solve_grid(int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const unsigned char* fixed,
                       const float* V_init, int outer_iterations, int cg_iterations, double cg_tolerance, float* V_out, double* stats,
                       void* workspace, size_t workspace_bytes, void* stream);

/* B solves of one mesh and one handle set in ONE launch chain: item b of V_out (and of stats) is bit for bit what gm_arap_solve
 * (global_step 0) or gm_arap_solve_grid (global_step 1) returns for V_init[b] and the same other arguments.  The CSR, weights, V0 and
 * fixed are shared by all items; V_init float [B][Vm][3], whose held rows already carry item b's targets; V_out float [B][Vm][3], which
 * may be V_init itself; stats NULL or double [B][outer_iterations][8], the single solve's rows.  The batch is the second grid dimension
 * of every kernel, so the chain has exactly the launches of one single solve; every item stops on its own sums: one that converges at
 * once neither holds back nor disturbs one that runs to the cap.  outer_iterations == 0 copies V_init to V_out.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: B < 1 or B > GM_ARAP_BATCH_MAX, a global_step other than 0 or 1, everything
 * gm_arap_solve refuses, any overlap among V0, V_init, V_out, stats and the workspace over their full [B] extents other than
 * V_out == V_init; with GM_ERR_BUFFER a workspace below gm_arap_batch_workspace_bytes(Vm, B, global_step) (0 for arguments that would
 * be refused).  Stream-ordered, no device allocation, no host synchronisation, no atomics. */
#define GM_ARAP_BATCH_MAX 64
size_t gm_arap_batch_workspace_bytes(int Vm, int B, int global_step /* 0 column / 1 grid */);
int gm_arap_solve_batch(int B, int global_step, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0,
                        const unsigned char* fixed, const float* V_init, int outer_iterations, int cg_iterations, double cg_tolerance,
                        float* V_out, double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* The ARAP energy of a pose as a function of the pose alone, and its gradient: a bending-aware rigidity term for an optimiser of the
 * vertices (arap.ArapEnergy, pose_fit.PoseFitter(regularizer="arap")).  The CSR and V0 of gm_arap_solve; V1 float [Vm,3] the pose, read
 * as float64.  With e_ij = p_i - p_j:
 *   E(x) = sum_i sum_j w_ij |(x_i - x_j) - R_i e_ij|^2,  R_i = the local step's rotation of S_i = sum_j w_ij (x_i - x_j) e_ij^T (rank <= 1: I);
 *   dE/dx_i = 4 sum_j w_ij [ (x_i - x_j) - (R_i + R_j) e_ij / 2 ]  - the R_i minimise E, so this partial derivative at fixed R is the
 *   total one (it is 4 times the residual of the global step's equation).
 * A row whose pose edges equal its rest edges bit for bit takes R_i = I exactly, so the rest pose gives E = 0 and a zero gradient
 * exactly.  A row whose weights sum to 0 adds nothing to E and gets a zero gradient row.
 * energy_out: one double.  grad_out: double [Vm,3], or NULL when only E is wanted (the same bits of E either way).
 * Three launches (rotations; rows of the gradient with one energy partial per workgroup of 256 rows; the partials added in index
 * order), sums in a fixed order and no atomics: two calls on the same input give the same bits.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: Vm <= 0, a NULL among row_offsets, cols, weights, V0, V1, energy_out, workspace,
 * any overlap of energy_out, grad_out or the workspace with another buffer of the call (V0 and V1 may coincide); with GM_ERR_BUFFER a
 * workspace below gm_arap_energy_workspace_bytes(Vm) (O(Vm), monotonic).  Column ids are forced into [0, Vm), as in gm_arap_solve.
 * Stream-ordered, no device allocation, no host synchronisation. */
size_t gm_arap_energy_workspace_bytes(int Vm);
int gm_arap_energy_grad(int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const float* V1,
                        double* energy_out, double* grad_out, void* workspace, size_t workspace_bytes, void* stream);

/* One-ring smoothing of per-vertex rows over the same CSR: `sweeps` Jacobi sweeps of (I + lambda L) y = g started at y = g,
 *   y_i <- (g_i + lambda sum_j w_ij y_j) / (1 + lambda d_i),  d_i = sum_j w_ij
 * (the Sobolev gradient of g: each sweep is a convex combination of g_i and the neighbours' values, so max |y| never grows, a constant
 * field stays constant and a row with d_i = 0 keeps g_i).  g_in, out double [Vm,3]; out may be g_in itself.  sweeps == 0 copies g_in
 * to out.  One launch per sweep between two copies of the state in the workspace, plus one that forms d_i; no atomics, the same bits
 * from call to call.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: Vm <= 0, sweeps < 0, a lambda that is negative or not finite, a NULL among
 * row_offsets, cols, weights, g_in, out, workspace, any overlap among g_in, out and the workspace other than out == g_in; with
 * GM_ERR_BUFFER a workspace below gm_mesh_smooth_workspace_bytes(Vm) (O(Vm), monotonic).  Stream-ordered, no device allocation, no
 * host synchronisation. */
size_t gm_mesh_smooth_workspace_bytes(int Vm);
int gm_mesh_smooth_rows(int Vm, const int* row_offsets, const int* cols, const double* weights, const double* g_in, double lambda, int sweeps,
                        double* out, void* workspace, size_t workspace_bytes, void* stream);

/* The meshes between two key poses A and B of one proxy mesh (pose_interp.PoseInterpolator): T in-betweens in ONE launch chain.
 * Every face's deformation gradient is interpolated in polar form - the rotation along its geodesic, the stretch linearly - and the
 * vertices are recovered from one Poisson solve per coordinate and frame over the cotangent Laplacian of gm_arap_solve's CSR
 * (definition: csrc/gm_pose_interp.hip).  row_offsets / cols / weights: that CSR (arap.edge_csr); V0, A, B
 * float [Vm,3] (V0, A and B may be one another: a key may be the rest pose); faces int32 [F,3]; vf_offsets int32 [Vm+1], vf_faces int32
 * [3F]: the faces at every vertex (deform.vertex_face_adjacency); held unsigned char [Vm]: rows with held[i] != 0, and rows whose
 * weights sum to 0, stay at (1 - t) A_i + t B_i.  C > 0: the rows of component k are comp_rows[comp_offsets[k] .. comp_offsets[k + 1])
 * (comp_offsets int32 [C+1]), label int32 [Vm] names each vertex's component (or -1), and every component is translated so that its
 * mean is (1 - t) mean_A + t mean_B; C == 0: the three may be NULL and nothing is translated.  ts double [T] ON THE DEVICE, each in
 * [0, 1] (the caller's check: it cannot be made here without a read-back).  V_out float [T,Vm,3].  stats (optional) double [T,6]: CG
 * steps used for x / y / z, final |r| / |b| for x / y / z.  Frame t of V_out and stats is bit for bit what a call with T = 1 and ts[t]
 * writes; no atomics, the same bits from call to call.  Ids are forced into range (vertex ids into [0, Vm), face ids into [0, F),
 * labels outside [0, C) mean none); the offset arrays must ascend within their arrays.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: T < 1 or T > GM_POSE_INTERP_BATCH_MAX, Vm < 1, F < 0, C < 0 or C > Vm,
 * cg_iterations < 1, a cg_tolerance that is negative or not finite, a NULL among the required pointers (faces and vf_faces only when
 * F > 0), any overlap of V_out, stats or the workspace with one another or with V0, A, B, ts; with GM_ERR_BUFFER a workspace below
 * gm_pose_interp_workspace_bytes(Vm, F, T) (O(Vm T + F T), monotonic; 0 for arguments that would be refused).  Stream-ordered, no
 * device allocation, no host synchronisation. */
#define GM_POSE_INTERP_BATCH_MAX 64
size_t gm_pose_interp_workspace_bytes(int Vm, int F, int T);
int gm_pose_interp(int T, int Vm, int F, const int* row_offsets, const int* cols, const double* weights, const float* V0, const int* faces,
                   const int* vf_offsets, const int* vf_faces, const unsigned char* held, int C, const int* comp_offsets, const int* comp_rows,
                   const int* label, const float* A, const float* B, const double* ts, int cg_iterations, double cg_tolerance, float* V_out,
                   double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* The proxy mesh posed from a skeleton (skinning.SkinBinding; definition: csrc/gm_skin.hip, INTEGRATION.md section AE).
 * gm_skin_weights: the bone-heat weights (Baran & Popovic 2007) of J bones - rest segments bone_a[j] -> bone_b[j], float [J,3] - over the
 * mesh of gm_arap_solve's CSR (row_offsets / cols / weights, arap.edge_csr); V0 float [Vm,3], area double [Vm] (dynamics.vertex_masses at
 * density 1).  One workgroup per bone solves (diag(h) + L) w_j = h o p_j by the Jacobi-preconditioned CG of gm_arap_solve's global step,
 * h_i = heat area_i / d2min_i, stopped at |r| <= cg_tolerance |b| or after cg_iterations steps.  Of a vertex's J weights the
 * max_influences (1 .. 4) largest are kept, negatives clamped to 0, renormalised: out_ids int32 [Vm,4], out_w float [Vm,4], by falling
 * weight; an unused slot repeats slot 0's id with weight 0.  out_full (or NULL): the columns before compaction, double [J,Vm].  out_stats
 * (or NULL) double [J,2]: CG steps used, final |r| / |b| per bone.  No atomics: the same bits from call to call.  Column ids of the CSR
 * are forced into [0, Vm); row_offsets must ascend.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: Vm < 1, J < 1 or J > GM_SKIN_BONES_MAX, a heat that is not positive and finite,
 * cg_iterations < 1, a cg_tolerance that is negative or not finite, max_influences outside 1 .. 4, a NULL among the required pointers,
 * any overlap of an output or the workspace with one another or with V0, area, bone_a, bone_b; with GM_ERR_BUFFER a workspace below
 * gm_skin_weights_workspace_bytes(Vm, J) (O(J Vm), monotonic; 0 for arguments that would be refused).
 * gm_skin_pose: T frames of the rest mesh skinned by transforms float [T,J,3,4] (rest-to-posed [A | t] per frame and bone), ids int32
 * [Vm,4] (forced into [0, J)) and w float [Vm,4] from gm_skin_weights or from anywhere; out float [T,Vm,3].  blend GM_SKIN_BLEND_LINEAR:
 * x' = (sum_k w_k (A_k x + t_k)) / (sum_k w_k); GM_SKIN_BLEND_DQS: dual-quaternion blending (Kavan et al. 2008), for which every A must be
 * a rotation (the caller's to check; anything else gives numbers, never a fault).  float64 arithmetic, rounded once; frame t is bit for
 * bit what a call with T = 1 and its transforms writes.  Refused with GM_ERR_INVALID_ARG: T < 1, Vm < 1, J outside 1 .. GM_SKIN_BONES_MAX,
 * another blend, a NULL pointer, out overlapping an input.  Both are stream-ordered, without device allocation or host synchronisation. */
#define GM_SKIN_BONES_MAX 256
#define GM_SKIN_BLEND_LINEAR 0
#define GM_SKIN_BLEND_DQS 1
size_t gm_skin_weights_workspace_bytes(int Vm, int J);
int gm_skin_weights(int Vm, int J, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* area,
                    const float* bone_a, const float* bone_b, double heat, int cg_iterations, double cg_tolerance, int max_influences,
                    int* out_ids, float* out_w, double* out_full, double* out_stats, void* workspace, size_t workspace_bytes, void* stream);
int gm_skin_pose(int T, int Vm, int J, const float* V0, const int* ids, const float* w, const float* transforms, int blend, float* out,
                 void* stream);
/* gm_skin_pose_bwd: the gradient of gm_skin_pose with respect to its transforms (skinning.skin_pose_differentiable; definition:
 * csrc/gm_skin.hip, INTEGRATION.md section AF).  g_out float [T,Vm,3] is dL/d out; g_transforms double [T,J,3,4] receives the
 * vector-Jacobian product of the forward's own float64 arithmetic, the forward's decisions (Shepperd branch, quaternion signs, the
 * |b_r| < 1e-12 fallback, the sum == 0 row) held constant.  bone_offsets int32 [J+1] / bone_entries int32 [bone_offsets[J]]: per bone
 * the (vertex, slot) pairs that name it with a nonzero weight, as 4 vertex + slot, ascending (skinning.bone_incidence); offsets are
 * forced into [0, 4 Vm] and an entry outside [0, 4 Vm) is skipped, the list's consistency with ids being the caller's.  Every element of
 * g_transforms is written; a bone with an empty list gets exact zeros.  Two launches per 32768 frames, no atomics, float64 sums in one
 * fixed order: the same bits from call to call, and frame t is bit for bit what a call with T = 1 and its transforms and g_out writes.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: T < 1, Vm < 1, J outside 1 .. GM_SKIN_BONES_MAX, another blend, a NULL pointer,
 * g_transforms or the workspace overlapping one another or an input; with GM_ERR_BUFFER a workspace below
 * gm_skin_pose_bwd_workspace_bytes(T, Vm, J, blend) (O(T Vm), monotonic; 0 for arguments that would be refused).  Stream-ordered, without
 * device allocation or host synchronisation. */
size_t gm_skin_pose_bwd_workspace_bytes(int T, int Vm, int J, int blend);
int gm_skin_pose_bwd(int T, int Vm, int J, const float* V0, const int* ids, const float* w, const float* transforms, int blend,
                     const float* g_out, const int* bone_offsets, const int* bone_entries, double* g_transforms, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Secondary motion of a proxy mesh (dynamics.MeshDynamics): T implicit-Euler steps of an elastic mesh whose potential is the ARAP energy,
 * in ONE launch chain - the local/global iteration of projective dynamics (Bouaziz et al. 2014) over gm_arap_solve's CSR, whose global
 * step's matrix gains the positive diagonal mu (definition: csrc/gm_dynamics.hip, INTEGRATION.md section AA).  row_offsets / cols /
 * weights: that CSR (arap.edge_csr); V0 float [Vm,3] the rest vertices; mass double [Vm], positive wherever d_i > 0; held unsigned char [Vm]:
 * rows with held[i] != 0, and rows whose weights sum to 0, are not unknowns; handle_ids int32 [H]: the held rows whose positions are
 * scripted, handle_targets float [T,H,3] their position in every step (H == 0: both may be NULL); x_in, v_in float [Vm,3] the state.
 * With h = dt, k = stiffness, g = damping, a = (gx, gy, gz), step t takes (x, v) to (x', v'):
 *   y_i = x_i + h v_i + h^2 a;   X_i = y_i on free rows, handle_targets[t] on handle rows, x_i on the other held rows;
 *   `iterations` times: R_i = the local step's rotation at X (gm_arap_solve's), then for every free row and coordinate
 *     mu_i X_i + sum_j w_ij (X_i - X_j) = mu_i y_i + sum_j (w_ij / 2)(R_i + R_j)(p_i - p_j),  mu_i = mass_i / (2 k h^2),
 *     by Jacobi-preconditioned CG (diagonal mu_i + d_i) warm-started from X and stopped at |r| <= cg_tolerance |b|, at p . A p <= 0 or
 *     after cg_iterations steps;
 *   x' = float32(X);  v'_i = float32((1 - g)(X_i - x_i) / h) on free rows, float32((X_i - x_i) / h) on held rows.
 * X_out float [T,Vm,3]: x' of every step; v_out float [Vm,3]: v' of the last step (it may be v_in itself); stats (optional) double [T,6]:
 * CG steps used for x / y / z and final |r| / |b| for x / y / z in the step's last iteration.  The state is rounded to float32 at every
 * step boundary, so a call of T steps is bit for bit T calls of one step; no atomics, the same bits from call to call.  With no held
 * row the system is still positive definite: a free body.  Column and handle ids are forced into [0, Vm).  THE CALLER'S CHECKS (they
 * cannot be made here without a read-back): every mass positive on a row with an edge, every handle id a held row and given once.
 * 1 + (H > 0) + 2 T iterations launches: the global step of a step's last iteration also writes the step's result and the next step's
 * prediction for its own coordinate.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: T < 1 or T > GM_MESH_DYNAMICS_STEPS_MAX, Vm < 1, H < 0 or H > Vm, a dt or
 * stiffness that is not finite and positive, a damping outside [0, 1), a gravity or cg_tolerance that is not finite, a negative
 * cg_tolerance, iterations < 1, cg_iterations < 1, a NULL among the required pointers (handle_ids and handle_targets only when H > 0),
 * any overlap of X_out, v_out, stats or the workspace with one another or with an input, other than v_out == v_in; with GM_ERR_BUFFER a
 * workspace below gm_mesh_dynamics_workspace_bytes(Vm) (O(Vm), monotonic; 0 for Vm < 1).  Stream-ordered, no device allocation, no
 * host synchronisation. */
#define GM_MESH_DYNAMICS_STEPS_MAX 64
size_t gm_mesh_dynamics_workspace_bytes(int Vm);
int gm_mesh_dynamics(int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* mass,
                     const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in, const float* v_in,
                     double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations, int cg_iterations,
                     double cg_tolerance, float* X_out, float* v_out, double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* gm_mesh_dynamics with unilateral contact against K analytic colliders (dynamics.MeshDynamics(colliders=...); definition:
 * csrc/gm_dynamics.hip, INTEGRATION.md section AB).  Every argument of gm_mesh_dynamics means what it means there.  K in
 * 0 .. GM_MESH_CONTACT_COLLIDERS_MAX; collider_kind int32 [K]: 0 a half-space, 1 a sphere; collider_rows float [T,K,4]: step t reads rows
 * [t]: (nx, ny, nz, d) of a half-space, whose solid is n . x < d: phi = n . x - d and the normal is n AS GIVEN (the caller normalises
 * it; the kernel does not), or (cx, cy, cz, r) of a sphere: phi = |x - c| - r, normal (x - c) / |x - c|, (0, 1, 0) at the centre;
 * collider_friction double [K], each >= 0; contact_stiffness kc > 0.  All float64 on the float32 rows.  In each of a step's iterations,
 * at the iterate X the local step reads and before its right-hand side is used, every free row i (held and handle rows never):
 *   k* = the collider of the smallest phi_k(X_i): compared as phi < best from +inf, so ties go to the lowest k and a NaN is never chosen;
 *   the row is active iff phi* < 0;  kappa_i = mu_i (kc h^2) if active, else 0;
 *   c_i = X_i - phi* n - scale t,  u = X_i - xs_i (xs: the state at the step's start), t = u - (n . u) n, lim = friction_k* |phi*|,
 *   scale = |t| <= lim ? 1 : lim / |t|;
 *   the global step solves (mu_i + kappa_i) X_i + sum_j w_ij (X_i - X_j) = mu_i y_i + kappa_i c_i + (the rotations' term) with the Jacobi
 *   diagonal (mu_i + kappa_i) + d_i, warm start and stopping rules unchanged.
 * - the contact energy sum_i (kc mass_i / 2) min(phi(X_i), 0)^2 with Coulomb-limited friction against the world frame; restitution 0.  The
 * step's end is gm_mesh_dynamics's.  contact_out (optional) int32 [T,Vm]: 1 + k* of every row active in the step's LAST iteration, 0
 * elsewhere, held rows included.  A step stays 2 * iterations launches.  With K == 0 the launches are gm_mesh_dynamics's own and so are
 * the bits (contact_out, if given, is zeroed).  THE CALLER'S CHECKS, beyond gm_mesh_dynamics's: every kind 0 or 1 (in the kernel a
 * collider of any other kind has phi = NaN and is never chosen), every friction >= 0, half-space normals of unit length.
 * Refused as gm_mesh_dynamics refuses, and with GM_ERR_INVALID_ARG: K < 0 or K > GM_MESH_CONTACT_COLLIDERS_MAX, a contact_stiffness that is
 * not finite and positive, a NULL among collider_kind / collider_rows / collider_friction when K > 0, any overlap of contact_out with
 * another buffer or of an output or the workspace with a collider array; with GM_ERR_BUFFER a workspace below
 * gm_mesh_dynamics_contact_workspace_bytes(Vm) (gm_mesh_dynamics's plus six doubles per vertex; required for every K). */
#define GM_MESH_CONTACT_COLLIDERS_MAX 16
size_t gm_mesh_dynamics_contact_workspace_bytes(int Vm);
int gm_mesh_dynamics_contact(int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* mass,
                             const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in,
                             const float* v_in, double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations,
                             int cg_iterations, double cg_tolerance, int K, const int* collider_kind, const float* collider_rows,
                             const double* collider_friction, double contact_stiffness, float* X_out, float* v_out, int* contact_out,
                             double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* A sampled signed-distance field for contact (dynamics.SdfGrid; definition: csrc/gm_sdf.hip and csrc/gm_sdf.h, INTEGRATION.md section AC).
 * The reference has no such stage: the results are defined by arithmetic.
 * gm_sdf_grid_prepare: values float [nz,ny,nx], sample (ix, iy, iz) at origin + (i + 0.5) voxel (TsdfVolume's layout); weight (optional)
 * float of the same shape.  A sample is VALID iff its value is not NaN and (weight == NULL or weight >= min_weight).  grid_out float
 * [nz,ny,nx,4], 16-byte aligned: an invalid sample gets four NaNs, a valid one (phi, gx, gy, gz), in float32, no contraction, correctly
 * rounded division, with phi- / phi+ the phi of the VALID neighbour inside the grid one sample down / up the axis:
 *   phi = value * scale;   per axis  (phi+ - phi-) / (2.f * voxel) with both neighbours,  (phi+ - phi) / voxel with only the upper,
 *   (phi - phi-) / voxel with only the lower,  0 with neither.
 * One thread per sample, no atomics: the same bits from call to call, and those of the restatement in numpy float32.  For a TSDF scale
 * is the truncation distance (the volume stores distance / trunc).
 * gm_sdf_grid_sample: points float [N,3]; phi_out double [N], n_out double [N,3].  Per row, in float64 and in this order:
 *   g_a = (X_a - origin_a) / voxel - 0.5 per axis; OUTSIDE unless 0 <= g_a < n_a - 1 on all three (a NaN is outside): phi = NaN;
 *   i_a = floor(g_a), f_a = g_a - i_a; the eight corners (ix + dx, iy + dy, iz + dz) as eight 16-byte loads; a corner whose phi is NaN:
 *   phi = NaN; each of the four channels, widened to double, interpolated along x, then y, then z, every interpolation
 *   fma(f, q1 - q0, q0); s = sqrt(fma(g2, g2, fma(g1, g1, g0 g0))); !(s > 0) or s not finite: phi = NaN; else n = g / s per coordinate.
 * Where phi_out is NaN, n_out is three NaNs.  The normal interpolates the prepared gradients, so it is continuous across cell faces.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: a side below 2, more than 2^28 samples, a voxel that is not finite and positive,
 * an origin that is not finite, a scale that is not finite, N < 1, a NULL among the required pointers, a grid that is not 16-byte
 * aligned, any overlap of an output with another buffer.  Stream-ordered, no device allocation, no host synchronisation. */
int gm_sdf_grid_prepare(int nx, int ny, int nz, const float* values, const float* weight, float min_weight, float scale, float voxel,
                        float* grid_out, void* stream);
int gm_sdf_grid_sample(int N, const float* points, int nx, int ny, int nz, const float* origin, float voxel, const float* grid, double* phi_out,
                       double* n_out, void* stream);

/* gm_mesh_dynamics_contact with one more collider: a prepared signed-distance grid (dynamics.MeshDynamics(field=...); INTEGRATION.md
 * section AC).  Every argument of gm_mesh_dynamics_contact means what it means there; nx, ny, nz, origin (three floats on the HOST),
 * voxel and field_grid describe the grid gm_sdf_grid_prepare wrote, static over the call; field_friction >= 0.  In every iteration a free
 * row evaluates the K analytic colliders exactly as gm_mesh_dynamics_contact does (k ascending, phi < best from +inf) and then the field,
 * (phi, n) = gm_sdf_grid_sample's at the iterate X_i, as candidate K with the same phi < best: ties go to the analytic collider, and a
 * NaN field value - a row outside the grid, next to an unknown sample, on a gradient without a direction - is never chosen, so such a
 * row is simply not in contact with the field.  An active row takes gm_mesh_dynamics_contact's kappa_i, c_i and Coulomb cap, in its
 * rounding order:
 *   u = X - xs per coordinate;  nu = fma(n2, u2, fma(n1, u1, n0 u0));  t = fma(-nu, n, u) per coordinate;
 *   s = sqrt(fma(t2, t2, fma(t1, t1, t0 t0)));  lim = friction fabs(phi);  scale = s <= lim ? 1 : lim / s;
 *   c = fma(-scale, t, fma(-phi, n, X)) per coordinate
 * with the winner's (phi, n, friction): the field's and field_friction when k* == K.  contact_out reports 1 + K for the field.  K may
 * be 0; the launches are the field's for every K (one local kernel of its own; the global kernel is gm_mesh_dynamics_contact's), a step
 * stays 2 * iterations launches, and the workspace is gm_mesh_dynamics_contact_workspace_bytes(Vm).
 * Refused as gm_mesh_dynamics_contact refuses, and with GM_ERR_INVALID_ARG: a side of the grid below 2, more than 2^28 samples, a voxel
 * that is not finite and positive, an origin that is NULL or not finite, a NULL or not 16-byte aligned field_grid (it is not routed to
 * gm_mesh_dynamics_contact), a field_friction that is negative or NaN, any overlap of the grid with an output or the workspace. */
int gm_mesh_dynamics_field(int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* mass,
                           const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in, const float* v_in,
                           double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations, int cg_iterations,
                           double cg_tolerance, int K, const int* collider_kind, const float* collider_rows, const double* collider_friction,
                           double contact_stiffness, int nx, int ny, int nz, const float* origin, float voxel, const float* field_grid,
                           double field_friction, float* X_out, float* v_out, int* contact_out, double* stats, void* workspace, size_t workspace_bytes,
                           void* stream);

/* gm_mesh_dynamics_field with a TABLE of F prepared grids, each under a rigid pose of its own per step: obstacles that move
 * (dynamics.MeshDynamics(fields=[...]), run(field_poses=); INTEGRATION.md section AG).  Every argument of gm_mesh_dynamics_contact means
 * what it means there.  fields: F entries on the HOST, 0 <= F <= GM_MESH_FIELDS_MAX, each the (nx, ny, nz, origin, voxel, grid, friction)
 * of gm_mesh_dynamics_field; the grids themselves are on the device and static over the call.  field_poses: double [T + 1,F,3,4] on the
 * device, row-major (R | t) with world = R local + t; R is to be a rotation (THE CALLER'S CHECK: dynamics.MeshDynamics checks host
 * arrays; another matrix gives the arithmetic below, no fault).  Row 0 is every field's pose at the state's time, before the call's first
 * step; row t + 1 is its pose during step t, in all its iterations - as step t reads row t of collider_rows.
 * Field f is candidate K + f behind the K analytic colliders, f ascending, each taken with the same phi < best: a tie goes to the lower
 * index, a NaN is never chosen.  At the iterate X, with P = (R | t) of row t + 1, in float64 without contraction:
 *   d = X - t per coordinate;  Xl_a = fma(R_2a, d_2, fma(R_1a, d_1, R_0a d_0))        (R^T d: column a of R)
 *   (phi, nl) = gm_sdf_grid_sample's at Xl;  kept iff phi < best
 *   the winner's normal  n_a = fma(R_a2, nl_2, fma(R_a1, nl_1, R_a0 nl_0))              (R nl: row a of R)
 * FRICTION IN THE OBSTACLE'S FRAME.  The tangential pull of gm_mesh_dynamics_contact goes back towards xs, the row's position at the
 * step's start.  When field f wins, the anchor is the point of the obstacle that was at xs, carried to where the obstacle is now:
 * with Pb = row t, Pn = row t + 1 of field f,
 *   e = xs - tb per coordinate;  q_a = fma(Rb_2a, e_2, fma(Rb_1a, e_1, Rb_0a e_0));  xs'_a = fma(Rn_a2, q_2, fma(Rn_a1, q_1, fma(Rn_a0, q_0, tn_a)))
 * and where the twelve numbers of Pb and Pn compare equal xs' = xs itself, with no arithmetic.  Then u = X - xs' and the rest is
 * gm_mesh_dynamics_field's, with field f's friction.  An analytic collider that wins keeps the world-frame anchor xs.  contact_out
 * reports 1 + K + f.  With identity poses the bits are gm_mesh_dynamics_field's (Xl = X - 0 and n = nl exactly: every product with 0 or
 * 1 is exact); with F == 0 the launches are gm_mesh_dynamics_contact's (field_poses is not read and may be NULL).  A step stays
 * 2 * iterations launches (a local kernel of its own, gm_mesh_dynamics_contact's global kernel); the workspace is
 * gm_mesh_dynamics_contact_workspace_bytes(Vm); no atomics, nothing waits for the device.
 * Refused as gm_mesh_dynamics_contact refuses, and with GM_ERR_INVALID_ARG: F < 0 or F > GM_MESH_FIELDS_MAX, a NULL table with F > 0,
 * per field what gm_mesh_dynamics_field refuses of its grid (sides, samples, voxel, origin, a NULL or misaligned grid) and a friction that
 * is negative or NaN, a NULL field_poses with F > 0, any overlap of a grid or of the poses with an output or the workspace. */
#define GM_MESH_FIELDS_MAX 4
typedef struct gm_dynamics_field {
  int nx, ny, nz;
  float origin[3];
  float voxel;
  const float* grid;   /* device, float [nz,ny,nx,4], 16-byte aligned */
  double friction;
} gm_dynamics_field;
int gm_mesh_dynamics_fields(int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* mass,
                            const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in, const float* v_in,
                            double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations, int cg_iterations,
                            double cg_tolerance, int K, const int* collider_kind, const float* collider_rows, const double* collider_friction,
                            double contact_stiffness, int F, const gm_dynamics_field* fields, const double* field_poses, float* X_out, float* v_out,
                            int* contact_out, double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* First hit of every ray on a mesh: what takes an editor from a pixel to a vertex of the current, deformed proxy mesh
 * (mesh_pick.ray_mesh_hits / pick / visible_vertices).  The reference has no such stage: the result is defined by arithmetic.
 * origins, dirs float [R,3], vertices float [Vm,3], faces int32 [F,3] vertex ids.  out_t float [R], out_face int32 [R], out_uv float
 * [R,2] (may be NULL).  Per (ray (o, d), face (a, b, c)) in float32, no contraction, correctly rounded division,
 * dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z, cross products per component as x.y*y.z - x.z*y.y (Moeller & Trumbore, two-sided):
 *   e1 = b - a, e2 = c - a, p = d x e2, det = dot(e1, p), s = o - a, q = s x e1, inv = 1 / det
 *   u = dot(s, p) * inv, v = dot(d, q) * inv, t = dot(e2, q) * inv
 *   hit iff u >= 0 and v >= 0 and (u + v) <= 1 and t >= t_min and t <= t_max (every comparison false on NaN; no epsilon on det:
 *   det == 0 gives inf or NaN, which fail by themselves).  d is not normalised: t is in units of |d|.
 * Winner: the smallest t, ties to the LOWEST face index; out_t = t + 0.0f (-0 reported as +0), out_face, out_uv = (u, v) of that face.
 * No hit: out_face = -1, out_t = +inf, out_uv = NaN.  So the outputs equal a float32 brute force over all F faces bit for bit, for
 * every finite input, and two calls give the same bits (csrc/gm_raycast.hip: every pair is evaluated, nothing is skipped).
 * Refused with GM_ERR_INVALID_ARG before any GPU work: a negative size, t_min < 0, a NaN bound, and with R > 0: F == 0 or Vm == 0, a
 * NULL among origins, dirs, vertices, faces, out_t, out_face, workspace, more than 2^31 - 1 workgroups (ceil(R / 256) * ceil(F / 64):
 * split the rays); with GM_ERR_BUFFER: a workspace below gm_ray_mesh_workspace_bytes(R, F) (O(R + F), monotonic in both, positive at
 * (0, 0)).  R == 0 succeeds and launches nothing.  Face indices outside [0, Vm) are forced into range, as in gm_closest_face: no
 * fault, no meaningful result for that face; mesh_pick.ray_mesh_hits checks them on the host.  Stream-ordered, no device allocation, no
 * host synchronisation. */
size_t gm_ray_mesh_workspace_bytes(int R, int F);
int gm_ray_mesh(int R, const float* origins, const float* dirs, int Vm, const float* vertices, int F, const int* faces, float t_min, float t_max,
                float* out_t, int* out_face, float* out_uv, void* workspace, size_t workspace_bytes, void* stream);

/* The generalized winding number of a mesh at every point of a set, and the signed distance composed from it and gm_closest_face: what
 * turns a triangle mesh into an obstacle of gm_mesh_dynamics_field (mesh_sdf.winding_numbers / inside / signed_distances / grid_values,
 * dynamics.SdfGrid.from_mesh; INTEGRATION.md section AD).  The reference has no such stage: the result is defined by arithmetic.
 * points float [N,3], vertices float [Vm,3], faces int32 [F,3] vertex ids; out_w double [N].
 * Per (point p, face (v0, v1, v2)) the float32 inputs are widened to float64 and every operation after that is float64, no contraction,
 * dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z, cross products per component as x.y*y.z - x.z*y.y (Van Oosterom & Strackee 1983):
 *   a = v0 - p, b = v1 - p, c = v2 - p;  la = sqrt(dot(a, a)), lb, lc likewise;  det = dot(a, b x c)
 *   den = (((la*lb)*lc + dot(a, b)*lc) + dot(b, c)*la) + dot(c, a)*lb;   omega = 2 atan2(det, den)
 * atan2(0, 0) = 0: a point on a vertex of the face and a face with two equal corners contribute nothing.  The order of summation is
 * part of the definition: the faces in chunks of 1024 (chunk k = faces [1024 k, 1024 (k + 1))), within a chunk in face order from 0.0,
 * the chunk sums in chunk order from 0.0, and w = that total / (4 pi), 4 pi = 4 * 0x1.921fb54442d18p+1.  The chunking depends on F
 * alone, and there are no float atomics: a point's w has the same bits in every run, however its points are batched.  sqrt and the
 * division are correctly rounded; atan2 is the device library's (about 1 ulp), so a float64 restatement on the host agrees to about
 * F * 1e-16, not bit for bit.  w is 1 inside a closed mesh wound outwards, -1 inside one wound inwards, 0 outside, and degrades
 * gracefully where a mesh is open or non-manifold (Jacobson et al. 2013).  Every (point, face) pair is evaluated: O(N F).
 * gm_mesh_signed_distance: out_phi float [N]; out_face int32 [N], out_closest float [N,3], out_w double [N] may each be NULL.
 * (d2, out_face, out_closest) are gm_closest_face's, bit for bit; out_w is gm_mesh_winding's; and
 *   out_phi = NaN if w is NaN or the point has no closest face (face -1);  +0 if d2 == 0;  otherwise s * sqrtf(d2) with the float32
 *   square root correctly rounded, s = -1 iff fabs(w) > 0.5 and +1 else - fabs: a mesh wound inwards is solid inside all the same.
 * Both refuse with GM_ERR_INVALID_ARG before any GPU work (every refusal, the workspace's too): a negative size, and with N > 0: F == 0
 * or Vm == 0, more than 2^31 - 1 workgroups (ceil(N / 256) * ceil(F / 1024): split the points), a NULL among points, vertices, faces,
 * out_w (gm_mesh_winding) / out_phi (gm_mesh_signed_distance), workspace, a workspace below gm_mesh_winding_workspace_bytes(N, F) /
 * gm_mesh_signed_distance_workspace_bytes(N, F) (48 F + 8 N ceil(F / 1024) bytes, plus gm_closest_face's and 16 N for the signed
 * distance; monotonic in both, positive at (0, 0)), an output or the workspace overlapping another buffer of the call.  N == 0
 * succeeds and launches nothing.  Face indices outside [0, Vm) are forced into range, as in gm_closest_face; mesh_sdf checks them on
 * the host.  Stream-ordered, no device allocation, no host synchronisation. */
size_t gm_mesh_winding_workspace_bytes(int N, int F);
int gm_mesh_winding(int N, const float* points, int Vm, const float* vertices, int F, const int* faces, double* out_w, void* workspace,
                    size_t workspace_bytes, void* stream);
size_t gm_mesh_signed_distance_workspace_bytes(int N, int F);
int gm_mesh_signed_distance(int N, const float* points, int Vm, const float* vertices, int F, const int* faces, float* out_phi, int* out_face,
                            float* out_closest, double* out_w, void* workspace, size_t workspace_bytes, void* stream);

/* Shortest-path distances along a proxy mesh from B independent source sets: what grows a picked vertex into a surface region
 * (mesh_region.SurfaceGraph.distances / region_handles).  The reference has no such stage: the result is defined by arithmetic.
 * (row_offsets int32 [Vm+1], cols int32 [nnz], lengths float [nnz]): a symmetric CSR with lengths >= 0 (mesh_region.surface_graph: the
 * mesh's edges and one unfolded edge across each interior edge).  source_offsets int32 [B+1], sources int32 [source_offsets[B]]: set b
 * is sources[source_offsets[b] .. source_offsets[b+1]); dist float [B,Vm], unsettled int32 [1].  ALL ON THE DEVICE.  Per set:
 *   d*[v] = the minimum over paths s = p0, .., pk = v from a source s of the float32 sum taken left to right,
 *   fl(..fl(fl(0 + l01) + l12).. ); 0 at sources, +inf where no path arrives; dist[b][v] = d*[v] if d*[v] <= max_distance, else +inf
 *   (the cutoff is inclusive; +inf: none).  A candidate above the cutoff is dropped, a NaN candidate never wins.
 * fl(d + l) >= d and d <= d' => fl(d + l) <= fl(d' + l), so every order of relaxations d[v] <- min(d[v], fl(d[u] + l_uv)) run until
 * none lowers anything ends at d*: the bits are those of a float32 Dijkstra, whatever the schedule (csrc/gm_geodesic.hip).
 * resume == 0: dist is initialised (+inf, then 0 at each source of its own set; a source id outside [0, Vm) is skipped, an empty set
 * leaves its row +inf).  resume != 0: dist is taken as it stands and source_offsets / sources are not read.  Then `sweeps` relaxation
 * launches on a grid of ceil(Vm / 256) x B are enqueued, in place, one thread per row, only the row's thread stores it; each counts the
 * rows it lowered, and one whose predecessor lowered nothing returns at once.  *unsettled = the count of the last sweep: 0 means dist
 * is final; otherwise call again with resume = 1 (no workgroup ever waits for another: termination is decided between launches).
 * At most Vm sweeps are ever needed.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: a negative size, sweeps < 1, a NaN or negative max_distance, and with Vm > 0: B
 * outside 1 .. 65535, a NULL among the pointers (sources and source_offsets too, also with resume); with GM_ERR_BUFFER: a workspace
 * below gm_mesh_geodesic_workspace_bytes(Vm, B, sweeps) (O(sweeps), monotonic, positive at 0).  Vm == 0 succeeds and launches nothing.
 * The CSR cannot be checked here without a read-back: column ids are forced into [0, Vm) - no fault, no meaning -, row_offsets and
 * source_offsets must ascend within their arrays (SurfaceGraph builds them itself); negative lengths are the caller's error, and the
 * sweep budget bounds the work regardless.  Stream-ordered, no device allocation, no host synchronisation. */
size_t gm_mesh_geodesic_workspace_bytes(int Vm, int B, int sweeps);
int gm_mesh_geodesic(int Vm, const int* row_offsets, const int* cols, const float* lengths, int B, const int* source_offsets, const int* sources,
                     float max_distance, int sweeps, int resume, float* dist, int* unsettled, void* workspace, size_t workspace_bytes, void* stream);

/* Fuse the depth / opacity maps of K views of one resolution into a truncated signed distance volume: the first half of the step from a
 * trained cloud to its proxy mesh (proxy_mesh.TsdfVolume.integrate).  The reference has no such stage: the result is defined by arithmetic.
 * depth, alpha float [K,H,W]: the rasterizer's own maps (depth = sum alpha_i T_i z_i, not normalised; alpha = 1 - T).  views float
 * [K,16]: each view's world_view_transform, stored transposed as everywhere here (v[4 r + c]); tanfov float [K,2]: tan(FoVx/2),
 * tan(FoVy/2).  All four on the device.  origin: three floats ON THE HOST, the low corner of the box; voxel: the cell size; sample
 * (ix, iy, iz) of tsdf / weight float [nz,ny,nx] (read AND written: the volume is state; a fresh one is tsdf = weight = 0) sits at the
 * voxel's centre.  Per voxel, per view k = 0 .. K-1 in this order, in float32, no contraction, correctly rounded division:
 *   p = origin + ((float)i + 0.5f) * voxel per axis; xv = ((p.x v[0] + p.y v[4]) + p.z v[8]) + v[12], yv (v[1 + ..]), zv (v[2 + ..])
 *   not (zv > 0): skip.  px = ((xv / (zv tanx) + 1) W - 1) 0.5, py alike with H; fx = floor(px + 0.5), fy = floor(py + 0.5): the nearest
 *   pixel; outside the image: skip.  a = alpha[k, fy, fx].
 *   not (a >= alpha_min): with carve != 0 the sample is FREE SPACE, t = 1; with carve == 0 skip.
 *   else s = depth[k, fy, fx] / a - zv; not (s >= -trunc): skip (behind the surface: UNOBSERVED, not inside); t = min(1, s / trunc).
 *   w' = w + 1, D = (D w + t) / w', w = w'.
 * Every comparison is false on NaN: a NaN skips the view.  K views in one call equal K calls of one view each, bit for bit.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: K < 0, H or W outside [1, 2^24], a grid side < 1 or more than 2^28 samples, a
 * NULL origin, tsdf or weight (and with K > 0: depth, alpha, views, tanfov), voxel or trunc not positive and finite, a NaN alpha_min or
 * origin, tsdf overlapping weight, either overlapping a map or the camera rows.  K == 0 succeeds and launches nothing.  One thread per
 * voxel; the volume is read once and written once per call.  Stream-ordered, no device allocation, no host synchronisation. */
int gm_tsdf_integrate(int K, int H, int W, const float* depth, const float* alpha, const float* views, const float* tanfov, int nx, int ny, int nz,
                      const float* origin, float voxel, float trunc, float alpha_min, int carve, float* tsdf, float* weight, void* stream);

/* The volume's zero surface as an indexed triangle mesh, by naive surface nets (no case table; one vertex per crossed cell, shared by
 * construction; two triangles per crossed grid edge): the second half (proxy_mesh.TsdfVolume.extract).  Defined by arithmetic, float32.
 * Cell (cx, cy, cz) has the corners (cx + dx, cy + dy, cz + dz), numbered dx + 2 dy + 4 dz; `inside` is D < 0 (an exact 0 is outside).
 *   A cell is active iff every corner has weight >= min_weight and its corners differ in `inside`.  Its vertex: over the edges in the
 *   order x: (0,1) (2,3) (4,5) (6,7), y: (0,2) (1,3) (4,6) (5,7), z: (0,4) (1,5) (2,6) (3,7), for each edge (a, b) whose ends differ:
 *   t = D[a] / (D[a] - D[b]) and three running sums (from 0) each take corner a's offset on their axis, t on the edge's own; m = sum /
 *   (float)count; position = origin + (((float)c + m) + 0.5f) * voxel per axis.  Vertex ids: the exclusive scan of the active flags over
 *   the cells in linear order, x fastest.
 *   Faces: per sample g in linear order and axis a = x, y, z (u, v the next two axes cyclically) the grid edge g -> g + e_a yields a quad
 *   iff its ends differ and the cells q0 = g - e_u - e_v, q1 = g - e_v, q2 = g, q3 = g - e_u all exist and are active; rows
 *   (q0, q1, q2), (q0, q2, q3) when g is inside, (q0, q2, q1), (q0, q3, q2) otherwise: the normal points from negative to positive.
 *   Rows 2 r and 2 r + 1, r the exclusive scan of the quads over (g, a).  An edge next to an inactive cell or the grid's side yields
 *   nothing: a half-observed volume gives an open boundary there.
 * out_vertices float [max_vertices,3], out_faces int32 [max_faces,3], out_counts int32 [2] ON THE DEVICE = {vertices, faces} the volume
 * needs.  A row at or beyond its capacity is NOT written - the rows below it are the prefix of the full result (faces may then name
 * vertices beyond max_vertices) - and the counts still say what is needed: the caller reads them and re-runs with more room.
 * The scan is three plain passes between kernel boundaries (sums per 256 entries, recursively; scan of the sums; scatter): the same
 * bits every run, and no workgroup waits for another.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: a grid side < 2, more than 2^28 samples, a NULL origin, tsdf, weight, out_counts
 * or workspace (out_vertices / out_faces with a capacity > 0), voxel not positive and finite, NaN origin or min_weight, a negative
 * capacity, an output or the workspace overlapping anything else; with GM_ERR_BUFFER: a workspace below
 * gm_surface_nets_workspace_bytes(nx, ny, nz) (about 6 bytes a sample, monotonic in each side, positive at (2, 2, 2)).
 * Stream-ordered, no device allocation, no host synchronisation. */
size_t gm_surface_nets_workspace_bytes(int nx, int ny, int nz);
int gm_surface_nets(int nx, int ny, int nz, const float* origin, float voxel, const float* tsdf, const float* weight, float min_weight,
                    int max_vertices, float* out_vertices, int max_faces, int* out_faces, int* out_counts, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Close the unobserved holes of a volume by volumetric diffusion (Davis, Marschner, Garr, Levoy 2002), between fusion and extraction
 * (proxy_mesh.TsdfVolume.fill_holes): the observed samples stay fixed and their distances diffuse into the samples no view saw, until
 * inside and outside values meet in a zero crossing where the fused volume alone ends in a border.  Defined by arithmetic, float32, no
 * contraction, correctly rounded division; tests/tsdf_fill_ref.py restates it in numpy bit for bit.  Volumes float [nz,ny,nx], x fastest.
 *   src(g) = weight_in[g] >= min_weight (false on NaN); val_0(g) = src ? tsdf_in[g] : +0, known_0 = src.
 *   Iteration t = 0 .. iterations-1 is a Jacobi step that reads only val_t / known_t: s = known_t(g) ? val_t(g) : 0, c = known_t(g) ? 1 : 0;
 *   then over the six face neighbours in the order -x, +x, -y, +y, -z, +z: one inside the grid with known_t: s = s + val_t(nb), c++; one
 *   outside the grid: with boundary_free != 0 s = s + 1 (free space) and c++, otherwise nothing.  not src(g) and c > 0: val_{t+1}(g) =
 *   s / (float)c, known_{t+1}(g) = 1; otherwise both carry over.  Sources never change; a filled sample is averaged again in every later
 *   iteration.  After n iterations every sample within n six-connected steps of a known one (or, with boundary_free, of the grid's
 *   side) has a value: iterations is a reach, not a convergence test.
 *   tsdf_out = val_N; weight_out = src ? weight_in : (known_N ? fill_weight : 0); out_counts int32 [2] ON THE DEVICE, may be NULL =
 *   {samples filled, samples still unknown} (integer atomics: the same in every run).  iterations == 0 copies the sources and zeroes
 *   the rest.  tsdf_in / weight_in are only read (they may be one buffer): the volume can take more views afterwards.
 * One launch per iteration between two copies of the state, one of them in the workspace; the last step always writes tsdf_out.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: a grid side < 2, more than 2^28 samples, iterations < 0, a NaN min_weight or
 * fill_weight, a NULL tsdf_in, weight_in, tsdf_out, weight_out or workspace, an output, out_counts or the workspace overlapping anything
 * else; with GM_ERR_BUFFER: a workspace below gm_tsdf_fill_workspace_bytes(nx, ny, nz) (about 6 bytes a sample, monotonic in each side,
 * positive at (2, 2, 2)).  Stream-ordered, no device allocation, no host synchronisation. */
size_t gm_tsdf_fill_workspace_bytes(int nx, int ny, int nz);
int gm_tsdf_fill(int nx, int ny, int nz, const float* tsdf_in, const float* weight_in, float min_weight, int iterations, int boundary_free,
                 float fill_weight, float* tsdf_out, float* weight_out, int* out_counts, void* workspace, size_t workspace_bytes, void* stream);

/* Mesh simplification by rounds of quadric-error edge collapses with SUBSET PLACEMENT (mesh_simplify.simplify): a collapse i -> j removes
 * vertex i and moves nothing, so the output vertices are rows of the input; the error quadrics (Garland & Heckbert 1997) are the only
 * floating-point state.  The reference sends its users to MeshLab for this step: the result is defined by arithmetic - float32, no
 * contraction, correctly rounded sqrt and division, dot(x, y) = (x.x y.x + x.y y.y) + x.z y.z, cross(x, y) = (x.y y.z - x.z y.y,
 * x.z y.x - x.x y.z, x.x y.y - x.y y.x) - and tests/simplify_ref.py restates it in numpy bit for bit.  ALL ARRAYS ON THE DEVICE.
 * vertices float [Vm,3], faces int32 [F,3] (the live faces), (vf_offsets int32 [Vm+1], vf_faces int32 [3F]): the faces at each vertex in
 * ascending face order (deform.vertex_face_adjacency).
 * gm_mesh_quadrics: out_quadrics float [Vm,10], the upper triangle of the 4 x 4 quadric in row order 00 01 02 03 11 12 13 22 23 33; from 0,
 * over the faces (a, b, c) of v in CSR order:
 *   n = cross(b - a, c - a), l = sqrt(dot(n, n)); not (l > 0 and l <= FLT_MAX): the face adds nothing (zero area, NaN, overflow)
 *   u = n / l per component, p = (u.x, u.y, u.z, -dot(u, a)), area = l * 0.5f; Q[k] = Q[k] + area * (p_r * p_c) for k = (r, c).
 *   One thread per vertex, a gather, no float atomics.
 * gm_mesh_collapse_round: one round.  edges int32 [E,2]: the unique undirected edges (lo, hi), lo < hi, of the live faces sorted by
 * lo Vm + hi - the index is the edge id e -, edge_faces int32 [E]: how many faces hold each; quadrics float [Vm,10] the current quadrics.
 *   locked[v]: v is an end of an edge whose face count != 2 (borders; the four-face edges naive surface nets leave).
 *   Candidates: per edge with face count 2 and per direction i -> j (i removed) whose i is not locked:
 *     link: the distinct vertices w outside {i, j} that share a face with i and share a face with j are exactly 2, and no face of i
 *       without j has its other two corners in one face of j (a tetrahedron never folds flat, no two faces over the same three vertices);
 *     flip: over every face of i that does not hold j, (p0, p1, p2) its corners' positions in row order, n0 = cross(p1 - p0, p2 - p0), n1
 *       the same with V[j] at i's corner, d = dot(n0, n1), s = dot(n0, n0) * dot(n1, n1): the direction stands only if on every such face
 *       d > 0 and d d <= FLT_MAX and s <= FLT_MAX and d d >= (min_cos * min_cos) * s (every comparison false on NaN);
 *     cost: q[k] = Q[i][k] + Q[j][k], (x, y, z) = V[j], r0 = ((q00 x + q01 y) + q02 z) + q03, r1 = ((q01 x + q11 y) + q12 z) + q13,
 *       r2 = ((q02 x + q12 y) + q22 z) + q23, r3 = ((q03 x + q13 y) + q23 z) + q33, c = ((x r0 + y r1) + z r2) + r3; not |c| <= FLT_MAX:
 *       rejected; cost = c > 0 ? c : +0; cost > max_error: rejected (+inf: no bound).
 *   The edge keeps the cheaper direction that stands, on a tie the one that removes the larger id.  out_key uint64 [E] = (bits of cost)
 *   << 32 | e (the bits of a non-negative float order as integers); out_from / out_to int32 [E] = i / j.  No direction stands: key all
 *   ones, from = to = -1.
 *   Selection: vmin[v] = the least key among the candidate edges at v; out_selected uint8 [E] = 1 iff the edge is a candidate and its key
 *   == the minimum of vmin[u] over u in N[i] + N[j] + {i, j} (N[v]: the corners of the faces of v).  *out_count int32 = how many.
 *   If e and e' are both selected and an end u of e' lies in the closed neighbourhood of an end x of e, then key(e) <= vmin[u] <= key(e')
 *   and, adjacency being symmetric, key(e') <= vmin[x] <= key(e): the keys hold the edge id, e = e'.  So no end of one selected edge is an
 *   end or a neighbour of an end of another: the collapses of a round change disjoint face sets, read no corner that another removes (and
 *   nothing ever moves), leave each other's N[i], N[j] as they were, all j are distinct and no j is an i - each one's link and flip tests
 *   stay true while any of the others apply, in any order (the caller may apply only the smallest keys to land on a face count).
 *   vmin by 64-bit atomicMin, the count by integer atomicAdd: order-independent, the same bits every run; no workgroup waits for another.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: a negative size, F > (2^31 - 1) / 3, and for the round: min_cos negative, NaN or
 * infinite, max_error negative or NaN, E > 0 with Vm == 0 or F == 0, a NULL pointer, out_key not 8-byte aligned, an output or the workspace
 * overlapping anything else (gm_mesh_quadrics: a NULL with Vm > 0, out_quadrics overlapping an input); with GM_ERR_BUFFER: a workspace below
 * gm_mesh_collapse_round_workspace_bytes(Vm) (9 bytes a vertex, monotonic, positive at 0).  Vm == 0 (quadrics) / E == 0 (round) succeeds
 * and launches nothing: then *out_count is not written.  Vertex ids read from faces and edges, face ids and offsets read from the CSR are
 * forced into range: no fault, no meaning; mesh_simplify.simplify checks the faces on the host.  An edge's thread reads
 * O(valence(i)^2 + valence(i) valence(j)) faces: made for proxy meshes (valence 4 to 8), slow at a vertex of valence in the thousands.  Stream-ordered, no device allocation, no
 * host synchronisation. */
int gm_mesh_quadrics(int Vm, const float* vertices, int F, const int* faces, const int* vf_offsets, const int* vf_faces, float* out_quadrics,
                     void* stream);
size_t gm_mesh_collapse_round_workspace_bytes(int Vm);
int gm_mesh_collapse_round(int Vm, const float* vertices, const float* quadrics, int F, const int* faces, const int* vf_offsets, const int* vf_faces,
                           int E, const int* edges, const int* edge_faces, float min_cos, float max_error, unsigned char* out_selected, int* out_from,
                           int* out_to, unsigned long long* out_key, int* out_count, void* workspace, size_t workspace_bytes, void* stream);

/* Colour on the proxy mesh (mesh_color.VertexColors / color_from_cloud, proxy_mesh.from_cloud(vertex_colors=True)): vertex normals, the
 * views' own renders fused into one colour per vertex, and a spread over the vertices no view coloured.  Defined by arithmetic, as
 * gm_tsdf_integrate is - float32, no contraction, correctly rounded division, the order written here - and tests/mesh_color_ref.py
 * restates all three in numpy bit for bit.  ALL ARRAYS ON THE DEVICE unless said otherwise.  vertices float [Vm,3], faces int32 [F,3],
 * (adj_offsets int32 [Vm+1], adj_faces int32 [3F]): the faces at each vertex in ascending face order (deform.vertex_face_adjacency).
 * gm_mesh_vertex_normals: out_normals float [Vm,3], unnormalised and area-weighted.  Per vertex i from N = 0, over j = adj_offsets[i] ..
 *   adj_offsets[i + 1] - 1 in this order, f = adj_faces[j], (a, b, c) = faces[f]: e1 = V[b] - V[a], e2 = V[c] - V[a],
 *   cr = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x) - each product rounds, then the difference -, N = N + cr.
 *   A vertex without faces gets (0, 0, 0).
 * gm_mesh_color_integrate: image float [K,3,H,W], depth / alpha float [K,H,W] the rasterizer's maps (depth alpha-weighted, not normalised),
 *   views float [K,16] the world_view_transform rows (stored transposed), tanfov float [K,2]; csum float [Vm,3] and wsum float [Vm] are
 *   STATE, read and written.  Per vertex P with normal N and per view k = 0 .. K-1 in this order:
 *   1. xv = ((P.x v[0] + P.y v[4]) + P.z v[8]) + v[12], yv (v[1 + ..]), zv (v[2 + ..]); not (zv > 0): skip the view.
 *   2. px, py, fx = floor(px + 0.5), fy = floor(py + 0.5) exactly as gm_tsdf_integrate; outside the image: skip.
 *   3. a = alpha[k, fy, fx]; not (a >= alpha_min): skip.
 *   4. s = depth[k, fy, fx] / a - zv; not (s >= -depth_tol and s <= depth_tol): skip - something else is in front, or the vertex is off
 *      the rendered surface.
 *   5. nv.x = (N.x v[0] + N.y v[4]) + N.z v[8], nv.y with v[1], v[5], v[9], nv.z with v[2], v[6], v[10].
 *   6. d = (nv.x xv + nv.y yv) + nv.z zv; with two_sided == 0: not (d < 0): skip - the vertex faces away.
 *   7. nn = (nv.x nv.x + nv.y nv.y) + nv.z nv.z, pp = (xv xv + yv yv) + zv zv, wgt = (d d) / (nn pp): the squared cosine of the viewing
 *      angle; not (wgt > 0): skip (a zero normal gives 0 / 0).
 *   8. c[ch] = image[k, ch, fy, fx]; a channel with c - c != 0 (NaN, inf): skip.
 *   9. csum[ch] = csum[ch] + wgt c[ch], wsum = wsum + wgt.
 *   Every comparison is false on NaN.  K views in one call equal K calls of one view each, bit for bit.  One thread per vertex.
 * gm_mesh_color_spread: seen uint8 [Vm] (non-zero: the vertex has a colour), colors float [Vm,3] in / out (read where seen), fallback
 *   three floats ON THE HOST, out_has uint8 [Vm], out_counts int32 [2] = {filled: has and not seen, unreached: not has}.  State (colour,
 *   has), has_0 = seen, colour_0 = colors where seen and +0 elsewhere.  Step t = 0 .. iterations-1 is a Jacobi step that reads only
 *   (colour_t, has_t): a seen vertex keeps both; otherwise sum = 0, n = 0, and over j in adjacency order and within face adj_faces[j] its
 *   corners q = 0, 1, 2 with u = faces[f][q]: u != i and has_t[u]: sum = sum + colour_t[u] per channel, n++ (a neighbour across an
 *   interior edge counts once per shared face); n > 0: colour_{t+1}[i] = sum / (float)n, has_{t+1}[i] = 1; otherwise both carry over.
 *   After the last step colors = has ? colour : fallback.  iterations is a REACH, not a convergence test: after n steps exactly the
 *   vertices within n edges of a seen one have a value; iterations == 0 returns the seen colours and fallback elsewhere.  One launch per
 *   step between two copies of the state, one of them in the workspace; the last step always writes colors.  No atomics.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: a negative Vm, F or K, Vm or F above (2^31 - 1) / 3, H or W outside [1, 2^24], a NaN
 * alpha_min, a NaN or negative depth_tol, iterations < 0, a NULL pointer that would be read or written (fallback, out_counts and workspace
 * always), an output - out_normals; csum, wsum; colors, out_has, out_counts, workspace - overlapping an input or another output; with
 * GM_ERR_BUFFER: a workspace below gm_mesh_color_spread_workspace_bytes(Vm) (about 13 bytes a vertex, monotonic, positive at 0).  Vm == 0,
 * K == 0 and iterations == 0 succeed (Vm == 0: out_counts = {0, 0}).  Vertex ids read from faces, face ids and offsets read from the CSR
 * are forced into range: no fault, no meaning.  Stream-ordered, no device allocation, no host synchronisation. */
int gm_mesh_vertex_normals(int Vm, int F, const float* vertices, const int* faces, const int* adj_offsets, const int* adj_faces, float* out_normals,
                           void* stream);
int gm_mesh_color_integrate(int K, int H, int W, const float* image, const float* depth, const float* alpha, const float* views, const float* tanfov,
                            int Vm, const float* vertices, const float* normals, float alpha_min, float depth_tol, int two_sided, float* csum,
                            float* wsum, void* stream);
size_t gm_mesh_color_spread_workspace_bytes(int Vm);
int gm_mesh_color_spread(int Vm, int F, const int* faces, const int* adj_offsets, const int* adj_faces, const unsigned char* seen, int iterations,
                         const float* fallback, float* colors, unsigned char* out_has, int* out_counts, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Mesh-driven deformation of bound Gaussians; replaces the Jittor tensor algebra of
 * SingleObjectDeform.deform_gaussian (edittool/__init__.py:116-131), tensor-in form:
 *   tri int32 [N,3] vertex ids of the bound face, w float [N,3] barycentric weights,
 *   dV float [Vm,3] = V_deformed - V_rest, Rv / Sv float [Vm,3,3] per-vertex rotation / shear
 *   (pyACAP GetRS output), cov float [N,3,3] rest covariance, pos float [N,3] rest position.
 * Outputs: pos_out [N,3], cov_out [N,3,3] (= RS cov RS^T, RS = Rb^T Sb), rot_out [N,3,3] (= Rb^T).
 * cov6_out (may be NULL): float [N,6] strip_symmetric(cov_out) ready for cov3D_precomp
 * (edittool/general_utils.py:26-37). */
int gm_deform(int N, const int* tri, const float* w, const float* dV, const float* Rv, const float* Sv,
              const float* cov, const float* pos, float* pos_out, float* cov_out, float* rot_out, float* cov6_out,
              void* stream);

/* View-dependent colour of deformed Gaussians; replaces edittool/__init__.py:442-448:
 *   dir = normalize(pos - campos); dir_rot = rot^T dir; rgb = max(SH_deg(dir_rot) + 0.5, 0).
 * rot may be NULL (identity: the train-time convert_SHs_python path, gaussian_renderer/__init__.py:84-89). */
int gm_sh_colors(int N, int deg, int M, const float* pos, const float* campos, const float* rot, const float* shs,
                 float* rgb, void* stream);

/* Fused edit-loop step: gm_deform followed by gm_sh_colors(rot = the deformed rotation) in ONE pass over the cloud
 * (what ObjectVisualTool.render_gaussian consumes per frame, edittool/__init__.py:421-472): pos_out [N,3],
 * cov6_out [N,6] (cov3D_precomp), rgb_out [N,3] (colors_precomp).  cov_out / rot_out ([N,3,3] each) are optional
 * (both or neither) for callers that also want SingleObjectDeform's gaussian_deform_cov / gaussian_deform_rot. */
int gm_deform_shade(int N, int deg, int M, const int* tri, const float* w, const float* dV, const float* Rv, const float* Sv,
                    const float* cov, const float* pos, const float* shs, const float* campos, float* pos_out, float* cov6_out,
                    float* rgb_out, float* cov_out, float* rot_out, void* stream);

/* The same step for a render loop that receives the mesh state of a frame as ONE [Vm][21] array (V1 | R | S per vertex,
 * what rank 0 broadcasts per deformation frame): gm_pack_mesh_state subtracts the rest pose verts [Vm,3] and writes the
 * gather table packed (float [Vm][24], 16-byte aligned: {dV,0} {R0..3} {R4..7} {R8,S0,S1,S2} {S3..6} {S7,S8,0,0});
 * gm_deform_shade_packed is gm_deform_shade reading that table (18 16-byte gathers per Gaussian instead of 63 4-byte
 * ones).  Needs M == 16 and 16-byte aligned shs / cov / outputs. */
int gm_pack_mesh_state(int Vm, const float* state, const float* verts, float* packed, void* stream);
int gm_deform_shade_packed(int N, int deg, int M, const int* tri, const float* w, const float* packed, const float* cov,
                           const float* pos, const float* shs, const float* campos, float* pos_out, float* cov6_out,
                           float* rgb_out, float* cov_out, float* rot_out, void* stream);

/* Edit-loop fast path (ObjectVisualTool.render_gaussian, edittool/__init__.py:421-472, one frame): gm_deform_shade_packed
 * and the first half of the forward in ONE pass over the cloud - the deformed position / covariance / colour of a
 * Gaussian go straight into its projection, conic, radius and instance count without a round trip through HBM.
 * Equivalent, bit for bit, to gm_deform_shade_packed followed by gm_forward_0_async(colors_precomp = rgb_out,
 * cov3D_precomp = cov6_out, means3D = pos_out, scale_modifier 1).  pos_out / cov6_out / rgb_out: all three or all NULL.
 * Complete the frame with gm_forward_1_geom.
 * A deformed frame is FORWARD-ONLY: its geometry buffer does not hold everything gm_backward reads.  Not written by this pass (the
 * buffer keeps whatever an earlier call left there): "clamped" (the SH clamp flags), "tiles_touched" except for saturated rectangles,
 * the internal radii copy when `radii` is given, and - in the stream variant with a plan - "bin" and "depth_key".  Do not call
 * gm_backward / gm_backward_p on such a buffer; differentiate through gm_deform_shade_packed + gm_forward_0_async instead. */
int gm_forward_0_deformed_async(int emission_policy, void* geom_buffer, int P, int deg, int M, int width, int height, const int* tri,
                                const float* w, const float* packed, const float* cov, const float* pos, const float* shs,
                                const float* opacities, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                float tan_fovx, float tan_fovy, float* pos_out, float* cov6_out, float* rgb_out, int* radii, int debug,
                                void* stream, int* num_rendered_host, void* count_event);

/* The same first half for the frames of ONE VIEW STREAM (consecutive cameras of an orbit, an edit session: the edit tool's render
 * loop).  depth_plan (gm_depth_plan_bytes() bytes, zeroed once by the caller, shared by the stream's frames - also by frames in
 * flight on different HIP streams) carries depth-bucket tables from frame to frame.
 *   flags & GM_STREAM_DIRECT: the pass itself appends every visible Gaussian to its depth bucket, looked up in the newest table earlier frames
 *     left in the plan (depth_slab: gm_depth_slab_bytes(P) bytes of scratch PER FRAME IN FLIGHT, like geom_buffer); the depth
 *     partition's three launches and the gather of the emission records disappear.  The (depth, id) order does not depend on the table,
 *     only the balance of the buckets does.  A frame the direct placement cannot order - no table yet, a table too stale for this view
 *     (a bucket above its slab), piles of equal depths - is REFUSED: its second half renders the background and status word 3 reads 2
 *     (gm_forward_1_geom's status_host / gm_forward_status_async; num_rendered_host is the correct total either way); begin it again
 *     without the flag.
 *   without GM_STREAM_DIRECT: the partition path of gm_forward_0_deformed_async, which also leaves its table in the plan (depth_slab unused,
 *     may be NULL): how a stream's first frame and refused frames are rendered.
 * Images, radii and lists are those of gm_forward_0_deformed_async, bit for bit. */
size_t gm_depth_plan_bytes(void);
size_t gm_depth_slab_bytes(int P);
int gm_forward_0_deformed_stream_async(int emission_policy, void* geom_buffer, int P, int deg, int M, int width, int height, const int* tri,
                                       const float* w, const float* packed, const float* cov, const float* pos, const float* shs,
                                       const float* opacities, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                       float tan_fovx, float tan_fovy, float* pos_out, float* cov6_out, float* rgb_out, int* radii,
                                       int debug, void* stream, int* num_rendered_host, void* count_event, void* depth_slab,
                                       unsigned int* depth_plan, int flags);
#define GM_STREAM_DIRECT 1   /* direct depth placement, see above */
#define GM_STREAM_COV6 2     /* cov holds the rest covariances as [N][6] rows xx xy xz yy yz zz instead of [N][9]: for clouds whose 3x3
                              * matrices are symmetric BIT FOR BIT (the six mirrored reads then return the same floats and every result
                              * is the one of the [N][9] call); 12 of the pass's 340 bytes per Gaussian less */

/* Second half of a forward without the per-Gaussian input pointers gm_forward_1 does not read: instance emission, tile
 * sort, tile ranges, blend.
 *   num_rendered >= 0: the instance count the first half reported; binning_buffer holds gm_binning_bytes(num_rendered);
 *                      binning_capacity is ignored.
 *   num_rendered <  0: SYNC-FREE mode - the host never learns the count.  binning_buffer holds
 *                      gm_binning_bytes(binning_capacity); the kernels read the count on the device.  If it exceeds the
 *                      capacity nothing is emitted, the image is the background and the overflow is reported by
 *                      gm_forward_status_async (grow the buffer and render the frame again).
 * status_host (page-locked, device-accessible host memory, 4 x int32; may be NULL) receives the frame's status words
 * {num_rendered, prefilter violation, policy, refused}, written by the blend kernel itself (no copy launch behind the frame); they are valid once
 * the stream has passed this call.  refused != 0: nothing was emitted (capacity overflow or policy mismatch).
 * gm_forward_status_async copies the same four words of the forward that last used geom_buffer, stream-ordered.
 * flags: 0, or GM_FWD_IMAGE_ONLY for a frame no backward pass will follow (the edit / viewer loop): the blend writes out_color
 * only - the per-pixel final transmittance and contributor count in image_buffer (forward.cu:369-370, read by
 * backward.cu:444-447 alone) are left untouched, so gm_backward on that image_buffer is undefined.
 * work_hint (may be NULL): device buffer of gm_work_hint_bytes(width, height) bytes, zeroed once by the caller and then handed
 * to the consecutive frames of one view stream (an orbit, an edit session at one resolution and policy).  The blend leaves in
 * it what each list tile cost; the next frames dispatch the tiles that were expensive first instead of the ones with the
 * longest lists, which shortens the kernel's tail (list length says little: a long list under an opaque surface saturates
 * early, a short one on a silhouette is walked to its end).  It only moves work in time: images are bit-identical with and
 * without it, frames in flight on several streams may share one buffer. */
#define GM_FWD_IMAGE_ONLY 1
/* GM_FWD_EXACT_EXPONENT: a forward that a BACKWARD pass follows (not with GM_FWD_IMAGE_ONLY).  The blend then evaluates every
 * exponent per pixel, with the expression gm_backward_p evaluates, instead of the matrix-core polynomial (absolute error ~1e-5 in
 * the exponent): both halves of the training step take the SAME alpha >= 1/255 decision for every (entry, pixel), as the
 * reference's do, whose backward.cu repeats forward.cu's expression (forward.cu:330-352, backward.cu:481-497).  Costs 17 us
 * of a 100-us blend at 1 M Gaussians / 1080p; the image differs from the default's by <= 3e-5 outside decision thresholds. */
#define GM_FWD_EXACT_EXPONENT 2
int gm_forward_1_geom(int emission_policy, void* geom_buffer, void* binning_buffer, void* image_buffer, int P, int num_rendered,
                      int64_t binning_capacity, const float* background, int width, int height, float* out_color, int debug, void* stream,
                      int* status_host, int flags, unsigned int* work_hint);
int gm_forward_status_async(void* geom_buffer, int P, int* status_host, void* stream);

/* Depth and opacity maps of the same blend (the reference renders the colour image only; the maps are the convention of the
 * common 3DGS rasterizer forks).  Over the entries the colour blend accepts (forward.cu:330-365: same order, same alpha >= 1/255
 * skips, same T < 1e-4 stop), per pixel:
 *   out_alpha = 1 - T_final, from the float T the colour output uses: a frame that keeps its state has out_alpha == 1 - final_T
 *               bit for bit;
 *   out_depth = sum_i alpha_i T_i z_i, z_i = the view-space depth p_view.z of the Gaussian (the float of "depth_key").  NOT
 *               normalised and without a background term (the background contributes 0): divide by out_alpha for the
 *               surface depth.
 * Both float32 [H,W]; either may be NULL.  Neither may overlap out_color or the other (GM_ERR_INVALID_ARG before any GPU work).
 * A refused frame (sync-free overflow, policy mismatch, direct-placement refusal) has out_alpha = out_depth = 0.
 *
 * gm_forward_1_aux: gm_forward_1_geom (same arguments, same image, radii, lists and status words bit for bit) that also writes the
 * maps.  It completes every single-frame first half (gm_forward_0_async, gm_forward_0_deformed_async, and
 * gm_forward_0_deformed_stream_async without GM_STREAM_DIRECT).  A GM_STREAM_DIRECT first half does not write depth_key; it
 * latches that in the geometry buffer, and gm_forward_1_aux REFUSES such a frame: background, both maps 0, status word 3 = 3
 * (begin it again without the flag).  The maps of a batch: gm_forward_deformed_batch_aux_async (below, next to the batch). */
int gm_forward_1_aux(int emission_policy, void* geom_buffer, void* binning_buffer, void* image_buffer, int P, int num_rendered,
                     int64_t binning_capacity, const float* background, int width, int height, float* out_color, int debug, void* stream,
                     int* status_host, int flags, unsigned int* work_hint, float* out_depth, float* out_alpha);

/* Per-Gaussian blend weights of a completed frame: what lifting 2-D masks onto a cloud and pruning by contribution sum.
 * One more walk of the frame's tile lists with the arithmetic of the GM_FWD_EXACT_EXPONENT blend (forward.cu:330-365): per (entry, pixel)
 *   oG = opacity * min(1, exp2(E)); skipped when oG < 1/255; alpha = min(0.99, oG); w = alpha * T; stop WITHOUT applying the entry when
 *   T - w < 1e-4; T starts at 1 -
 * the float32 w is the value the colour blend multiplies the entry's colour by.  Per Gaussian i, over the pixels of the frame, the call ADDS
 *   sums[2 i]     += sum of u,      u = (uint32) rintf(w * 2^24)      (total weight, unit 2^-24)
 *   sums[2 i + 1] += sum of u * k,  k = the pixel's mask byte 0..255  (weight inside the mask, unit 2^-24 / 255; mask == NULL: 255 everywhere)
 *   peak[i]        = max(peak[i], float bits of w)                    (w >= 0: an unsigned max on the bits is a max on the value; may be NULL)
 * to what the buffers hold: the caller zeroes sums (uint64 [P][2]) and peak (uint32 [P]) once and hands them to every view.  Integer
 * accumulators: the result does not depend on the emission policy, on the order of the views or on the run, bit for bit.
 * The call follows ANY completed second half (gm_forward_1_geom / gm_forward_1_aux, whatever its flags, image-only frames and frames
 * begun with GM_STREAM_DIRECT included: neither colour, final_T, n_contrib nor depth_key is read) on the same stream, with the same policy,
 * geometry, binning and image buffers, before they are reused.  binning_capacity: the instance count the binning buffer was laid out
 * for - the second half's num_rendered when that was >= 0, else its binning_capacity (gm_backward's R).
 * A refused frame (status word 3 != 0) or one whose lists were built under another policy adds nothing (decided on the device).
 * Refused with GM_ERR_INVALID_ARG before any GPU work: a policy outside 0..3, P < 0, a frame size the forward entry points refuse, a
 * negative capacity, and with P > 0: a NULL geom_buffer, binning_buffer, image_buffer or sums; sums or peak overlapping each other, the
 * mask or one of the three buffers (taken as gm_geom_bytes(P), gm_binning_bytes(binning_capacity), gm_image_bytes(width, height)).
 * P == 0 returns GM_OK and touches nothing. */
int gm_blend_weights(int emission_policy, void* geom_buffer, void* binning_buffer, void* image_buffer, int P, int64_t binning_capacity,
                     int width, int height, const uint8_t* mask, unsigned long long* sums, unsigned int* peak, int debug, void* stream);

/* K frames of ONE view stream per launch chain (the edit tool replaying a deformation sequence, a camera path: the frames the render
 * loop would otherwise keep in flight on K HIP streams).  Equivalent, frame by frame and bit for bit (radii, lists, image, status words), to
 *   gm_forward_0_deformed_stream_async(policy, frame.geom_buffer, ..., frame.packed, ..., frame.viewmatrix, ..., flags & GM_BATCH_COV6)
 *   gm_forward_1_geom(policy, frame.geom_buffer, frame.binning_buffer, frame.image_buffer, P, -1, binning_capacity, background, ...,
 *                     frame.out_color, debug, stream, frame.status_host, flags & GM_BATCH_IMAGE_ONLY, work_hint)
 * for each of the K frames, but
 *   - the static cloud (face ids, weights, rest covariance and position, SH rows, opacity: 256 of the 321 bytes per Gaussian the fused pass
 *     of a frame moves) is read from HBM ONCE for the batch: one pass loops over the frames' (gather table, camera) pairs
 *     (edittool/__init__.py:103-131, 421-472: what one frame consumes; RAST/forward.cu:155-256), and
 *   - every later stage is ONE launch over the K frames (grid z = frame): a batch is 12 launches instead of 12 K, each K times as large.
 * Sync-free second half only (the instance counts stay on the device; binning_capacity instances per frame; a frame that outgrows it is
 * refused in its own status words and rendered again by the caller through the single-frame calls).  1 <= K <= GM_BATCH_MAX; M == 16;
 * emission policies with at most 2048 list tiles (the one-pass tile sort); every scratch buffer base 256-byte aligned; the frames'
 * buffers distinct.  Like every deformed frame: forward only.  Depth / alpha maps: gm_forward_deformed_batch_aux_async below. */
#define GM_BATCH_MAX 8
#define GM_BATCH_IMAGE_ONLY 1    /* as GM_FWD_IMAGE_ONLY */
#define GM_BATCH_COV6 2          /* as GM_STREAM_COV6 */
typedef struct gm_batch_frame {
  const float* packed;           /* [Vm][24] gather table of this frame (gm_mesh_rs_packed / gm_mesh_rs_packed_batch / gm_pack_mesh_state) */
  const float* viewmatrix; const float* projmatrix; const float* cam_pos;
  float tan_fovx, tan_fovy;
  void* geom_buffer; void* binning_buffer; void* image_buffer;      /* gm_geom_bytes(P) / gm_binning_bytes(binning_capacity) / gm_image_bytes(W, H) */
  float* out_color;              /* [3,H,W] */
  int* radii;                    /* [P], may be NULL */
  int* status_host;              /* 4 x int32, page-locked, may be NULL */
} gm_batch_frame;
int gm_forward_deformed_batch_async(int emission_policy, int K, const gm_batch_frame* frames, int P, int deg, int M, int width, int height,
                                    const int* tri, const float* w, const float* cov, const float* pos, const float* shs, const float* opacities,
                                    const float* background, int64_t binning_capacity, int flags, unsigned int* work_hint, int debug, void* stream);
/* gm_forward_deformed_batch_async that also renders each frame's depth and opacity maps, as gm_forward_1_aux defines them (above).
 * out_depth / out_alpha: host arrays of K device pointers, one float32 [H,W] map per frame (the convention of gm_mesh_rs_packed_batch);
 * each array is NULL (no such map) or holds K non-null pointers.  Frame by frame and bit for bit: colour, radii, lists, status words and
 * per-pixel state equal those of gm_forward_deformed_batch_async, and the maps equal those of gm_forward_0_deformed_stream_async (without
 * GM_STREAM_DIRECT) + gm_forward_1_aux in sync-free mode; a refused frame has both maps 0 (rendered again through those two calls, its
 * maps come out exact).  Refused with GM_ERR_INVALID_ARG before any GPU work: everything gm_forward_deformed_batch_async refuses, a NULL
 * inside a non-null array, a map (H*W floats) that shares memory with any frame's out_color (3*H*W floats) or with any other map. */
int gm_forward_deformed_batch_aux_async(int emission_policy, int K, const gm_batch_frame* frames, int P, int deg, int M, int width, int height,
                                        const int* tri, const float* w, const float* cov, const float* pos, const float* shs, const float* opacities,
                                        const float* background, int64_t binning_capacity, int flags, unsigned int* work_hint, int debug, void* stream,
                                        float* const* out_depth, float* const* out_alpha);
/* K frames of a SCENE per launch chain: a free-standing background cloud plus mesh-bound objects (SceneVisualTool,
 * edittool/__init__.py:133-231).  The P rows are in the order SceneVisualTool.render_gaussian concatenates them: the background
 * (rows before object_rows[0]), then object j = rows [object_rows[j], object_rows[j+1]) for j < n_objects (host array of n_objects + 1
 * ascending entries in [0, P]).  Equivalent, frame by frame and bit for bit (radii, lists, image, status words), to
 *   gm_cov_to_scale_rot(the rows' covariances) + gm_forward_0_async(policy, ..., means = the rows' positions, shs, opacities, scales, 1.0,
 *   rotations, ...) + gm_forward_1_geom(..., -1, binning_capacity, ...) as gm_forward_deformed_batch_async states it,
 * where a row is, in frame k, one of
 *   static    a background row, or a row of object j with bit j of deformed[k] clear: position pos, (scale, rotation) = (scales, rots),
 *             which the caller computes once per state as gm_cov_to_scale_rot of the row's covariance;
 *   deformed  a row of object j with bit j of deformed[k] set: gm_deform of its rest position pos and rest covariance cov[row - object_rows[0]]
 *             by frame k's gather table (frames[k].packed; tri / w as for gm_forward_deformed_batch_async, face ids into that table),
 *             then gm_cov_to_scale_rot of the result.
 * Colours from the SH rows with the unrotated view direction (the rasterizer's own).  deformed: host array of K masks; frames[k].packed
 * may be NULL in a frame whose mask is 0; tri / w / cov ([*,3] int32, [*,3], [*,9]: the object rows only) may be NULL when every mask is 0.
 * pos [P,3], scales [P,3], rots [P,4] (16-byte aligned), shs [P,16,3] (16-byte aligned), opacities [P].  flags: GM_BATCH_IMAGE_ONLY or 0.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: everything gm_forward_deformed_batch_async refuses (a NULL packed aside),
 * n_objects outside 0..GM_SCENE_OBJECTS_MAX, object_rows that do not ascend or leave [0, P], a mask bit at or above n_objects, a set bit
 * with packed == NULL, and frames whose buffers overlap as ranges (geometry, binning, image, out_color, non-null radii and status_host). */
#define GM_SCENE_OBJECTS_MAX 32   /* objects of a scene batch (gm_forward_scene_batch_async): the width of its per-frame masks */
int gm_forward_scene_batch_async(int emission_policy, int K, const gm_batch_frame* frames, int P, int deg, int M, int width, int height,
                                 int n_objects, const int* object_rows, const unsigned int* deformed, const float* pos, const float* scales,
                                 const float* rots, const float* shs, const float* opacities, const int* tri, const float* w, const float* cov,
                                 const float* background, int64_t binning_capacity, int flags, unsigned int* work_hint, int debug, void* stream);
/* gm_mesh_rs_packed for the K deformed meshes of such a batch in one launch: V1[k] -> packed[k] (host arrays of K device pointers). */
int gm_mesh_rs_packed_batch(int K, int Vm, int nfaces, const float* V0, const float* const* V1, const int* faces, const int* adj_offsets,
                            const int* adj_faces, float* const* packed, void* stream);

/* Per-vertex rotation / stretch of a deformed proxy mesh: replaces pyACAP.GetRS(rest vertices, deformed vertices, ...) at
 * edittool/__init__.py:102, 109 (pyACAP is a binary missing from the reference tree, so the contract is the one its call
 * site implies).  V0 / V1 float [Vm,3] rest / deformed vertices, faces int32 [nfaces,3], adj_offsets int32 [Vm+1] and
 * adj_faces int32 [3 nfaces]: CSR list of the faces incident to each vertex (built once per mesh by the caller).
 * Per vertex the affine map of its one-ring, T = argmin sum_j c_ij |(p'_i - p'_j) - T (p_i - p_j)|^2 with cotangent weights of
 * the rest mesh (ACAP / ARAP deformation gradient), is split by polar decomposition T = Q S (Q proper rotation, S symmetric).
 * Outputs, row-major [Vm,3,3]: R = Q^T (the row-vector convention deform_gaussian expects: it uses
 * gaussian_deform_rot = blend(R)^T and transforms covariances by R^T S, edittool/__init__.py:118-129) and S.
 * state (optional, float [Vm,21]) receives V1 | R | S per vertex - the frame record gm_pack_mesh_state consumes.
 * R and S: both or neither; at least one of (R, S) / state.
 * gm_mesh_rs_packed writes, instead, the 96-byte-per-vertex gather table gm_pack_mesh_state would make of that record
 * (float [Vm,24], 16-byte aligned): what gm_deform_shade_packed / gm_forward_0_deformed_async read - one launch per frame. */
int gm_mesh_rs(int Vm, int nfaces, const float* V0, const float* V1, const int* faces, const int* adj_offsets, const int* adj_faces,
               float* R, float* S, float* state, void* stream);
int gm_mesh_rs_packed(int Vm, int nfaces, const float* V0, const float* V1, const int* faces, const int* adj_offsets, const int* adj_faces,
                      float* packed, void* stream);

/* Covariance -> (scale, rotation): replaces the per-frame eigh + host-side det sign + sqrt + matrix->quaternion of
 * SceneVisualTool.render_gaussian (edittool/__init__.py:204-207, 23-38).  cov float [N,3,3] (symmetric),
 * scales float [N,3] = sqrt of the eigenvalues in ascending order, rots float [N,4] = unit quaternion (w,x,y,z) of the
 * eigenvector matrix made right-handed, such that R(q) diag(scales^2) R(q)^T reproduces cov. */
int gm_cov_to_scale_rot(int N, const float* cov, float* scales, float* rots, void* stream);

/* Spherical-harmonics rows re-expressed in the unrotated frame: the colour half of baking an edit into a plain cloud (deform.rotate_sh).
 * shs_out row i, coefficients k < (deg+1)^2: the unique c' with  SH_deg(d) . c' == SH_deg(A_i^T d) . c_i  for every unit d,
 * SH_deg the polynomial of gm_sh.h, A_i = rot[9 i ..] row-major (what gm_deform writes as rot_out), so A^T d is
 * gm_sh_colors' dir_rot.  Coefficients k >= (deg+1)^2 of a row are copied bit for bit; deg == 0 copies the rows.
 * shs, shs_out float [N,M,3]; rot float [N,3,3]; shs_out == shs is allowed (a row is read before it is written).  Exact for any 3x3
 * matrix up to float32 rounding (csrc/gm_shrot.hip); non-finite entries of rot or shs propagate into that row only.  No workspace, no
 * device allocation, no host wait: stream-ordered; the same input gives the same bits.  N == 0 succeeds and launches nothing.
 * Refused with GM_ERR_INVALID_ARG before any GPU work, when N > 0: N < 0, deg outside 0..3, M < (deg+1)^2, a NULL pointer, shs_out
 * overlapping shs other than exactly equal, shs_out overlapping rot. */
int gm_sh_rotate(int N, int deg, int M, const float* shs, const float* rot, float* shs_out, void* stream);

/* Backward of gm_deform_shade (csrc/gm_deform_bwd.hip): from the gradients of its three outputs - g_pos [N,3], g_cov6 [N,6] (may be NULL),
 * g_rgb [N,3] (may be NULL); a NULL stands for zeros and gives the bits an all-zero tensor gives - to the gradients of the per-vertex
 * tables, g_dV [Vm,3], g_Rv [Vm,9], g_Sv [Vm,9] (mandatory), and optionally (NULL switches each off) of the SH rows g_shs [N,M,3]
 * (coefficients k >= (deg+1)^2 are written as 0), the rest covariances g_cov [N,9] and the rest positions g_rest_pos [N,3].  No gradient
 * to w or campos.  The forward's inputs are the forward's: tri int32 [N,3], w [N,3], dV [Vm,3], Rv / Sv [Vm,9], cov [N,9], pos [N,3],
 * shs [N,M,3], campos [3]; the forward is recomputed with its own arithmetic, so the clamp gate is the one behind the rgb it wrote.
 * Vertex sums are deterministic and use no atomics: they run over the vertex -> (row, corner) incidence list in CSR form,
 * inc_offsets int32 [Vm+1] (inc_offsets[0] = 0, inc_offsets[Vm] = 3 N) and inc_entries int32 [3N] with entry 3 * row + corner, ascending
 * within a vertex (deform.DeformBinding builds it once per binding).  THE CALLER'S CONTRACT: entry e lies in vertex tri[e]'s list, each
 * e in [0, 3N) exactly once; the call does not check it (an entry outside [0, 3N) is skipped, nothing else).  A vertex's sum is a fixed
 * function of its list: the same bits every run.  A vertex with an empty list gets exact zeros; every element of g_dV / g_Rv / g_Sv is
 * written (no pre-zeroing).  workspace: gm_deform_shade_bwd_workspace_bytes(N, Vm) bytes, fully written before it is read.
 * Stream-ordered: no device allocation, no host wait.  N == 0 writes zero tables; Vm == 0 with N == 0 does nothing.
 * Refused with GM_ERR_INVALID_ARG before any GPU work: N < 0 or Vm < 0, deg outside 0..3, M < (deg+1)^2, N > 0 with Vm == 0, a NULL
 * mandatory pointer, g_shs without both g_rgb and g_cov6, a workspace shorter than gm_deform_shade_bwd_workspace_bytes, an output or the
 * workspace overlapping an input or another output. */
size_t gm_deform_shade_bwd_workspace_bytes(int N, int Vm);
int gm_deform_shade_bwd(int N, int deg, int M, int Vm, const int* tri, const float* w, const float* dV, const float* Rv, const float* Sv,
                        const float* cov, const float* pos, const float* shs, const float* campos, const int* inc_offsets,
                        const int* inc_entries, const float* g_pos, const float* g_cov6, const float* g_rgb, float* g_dV, float* g_Rv,
                        float* g_Sv, float* g_shs, float* g_cov, float* g_rest_pos, void* workspace, size_t workspace_bytes, void* stream);

/* Photometric loss of the training loop (train_mesh_gaussian.py:92-94): replaces utils/loss_utils.py:17-18 (l1_loss) and
 * :23-81 (ssim: 11x11 Gaussian window of sigma 1.5, zero padding 5, depthwise) and the autograd pass through them.
 * img1 (rendered) / img2 (ground truth): float [planes,H,W] (planes = channels, or batch x channels).
 * gm_ssim_fwd writes per 32x32-pixel workgroup {sum of the ssim map, sum of |img1-img2|} into partial
 * (float [gm_ssim_partials(planes,H,W)][2], plane-major then tile rows): ssim(...) = sum/(planes H W), per-image means
 * for size_average=False by summing a plane range.  dS_dmu1 / dS_dE11 / dS_dE12 (float [planes,H,W] each; all three or
 * all NULL) receive the per-pixel partial derivatives gm_ssim_bwd needs; partial holds the same bits with and without them.
 * gm_ssim_bwd: dL_dimg1 = g_ssim[plane] * d(sum of ssim map)/d img1 + g_l1[0] * sign(img1 - img2); g_ssim (device float
 * [planes]) and g_l1 (device float [1], may be NULL) carry the upstream gradient times 1/count, so no host
 * synchronisation is needed between forward and backward.
 * gm_loss_combine: out[0] = offset + c_ssim * sum_i partial[i][0] + c_l1 * sum_i partial[i][1] (sums in double, one launch):
 * with c_ssim = -lambda/count, c_l1 = (1 - lambda)/count, offset = lambda this is the training loss
 * (1 - lambda) * l1_loss + lambda * (1 - ssim) of train_mesh_gaussian.py:92-94 as a device scalar. */
int64_t gm_ssim_partials(int planes, int H, int W);
int gm_ssim_fwd(const float* img1, const float* img2, int planes, int H, int W, float* dS_dmu1, float* dS_dE11, float* dS_dE12,
                float* partial, void* stream);
int gm_ssim_bwd(const float* img1, const float* img2, const float* dS_dmu1, const float* dS_dE11, const float* dS_dE12, int planes,
                int H, int W, const float* g_ssim, const float* g_l1, float* dL_dimg1, void* stream);
int gm_loss_combine(const float* partial, int64_t n_partials, double c_ssim, double c_l1, double offset, float* out, void* stream);

/* The same two kernels with the ground truth as the 8-bit planes a dataset holds, composited while it is loaded
 * (train_mesh_gaussian.py:89-91: gt * mask + bg * (1 - mask), every iteration, with a fresh random bg in the --is_exist_bg mode).
 * rgb: uint8 [3,H,W] planar (planes must be 3).  mask: uint8 [Cm,H,W] or NULL; mask_plane_stride = elements between the mask
 * planes of two channels: 0 for one shared plane (Cm = 1), H*W (or more) for Cm = 3.  background: DEVICE float[3] (needed with a
 * mask): a colour drawn on the device never crosses the host.
 * Target of plane c at a pixel, float32, every operation rounded on its own, in this order - the bits the tensor expression gives:
 *   g = rgb/255, m = mask/255 (correctly rounded quotients), t1 = g*m, t2 = 1 - m, t3 = background[c]*t2, y = t1 + t3;  no mask: y = g.
 * Everything else - partial layout, derivative maps, g_ssim / g_l1 - as gm_ssim_fwd / gm_ssim_bwd, whose results on the float
 * image y these reproduce bit for bit. */
int gm_ssim_fwd_u8(const float* img1, const uint8_t* rgb, const uint8_t* mask, int64_t mask_plane_stride, const float* background,
                   int planes, int H, int W, float* dS_dmu1, float* dS_dE11, float* dS_dE12, float* partial, void* stream);
int gm_ssim_bwd_u8(const float* img1, const uint8_t* rgb, const uint8_t* mask, int64_t mask_plane_stride, const float* background,
                   const float* dS_dmu1, const float* dS_dE11, const float* dS_dE12, int planes, int H, int W, const float* g_ssim,
                   const float* g_l1, float* dL_dimg1, void* stream);

/* Training-loop fusions around the rasterizer ("MeshBasedGaussianModel.get_xyz ... fused into the op").
 * gm_mesh_activate_fwd: raw parameters -> rasterizer inputs in one pass, replacing the Jittor elementwise chains of
 *   get_xyz = softmax(bc).(v1,v2,v3) + alpha r (sigmoid(dist) - 0.5) normal   (scene/mesh_based_gaussian_model.py:138-152)
 *   get_scaling = exp(scaling), get_rotation = normalize(rotation) (:122-128), get_opacity = sigmoid(opacity) (:172-174).
 *   bc/scaling/v1/v2/v3/normal float [N,3]; dist/opacity/r float [N]; rotation float [N,4] (16-byte aligned).
 *   Outputs xyz [N,3], scales [N,3], rots [N,4] (16-byte aligned), opac [N].
 *   mr_partial (may be NULL; float [ceil(N/256)]): per-workgroup sums of the mesh-restrict loss term
 *   max(0, max_axis(scales) - mr_weight * sqrt(|AB x AC|)) (utils/loss_utils.py:86-108, train_mesh_gaussian.py:93); their
 *   sum is mesh_restrict_loss(scales, v1, v2, v3, mr_weight).
 * gm_mesh_activate_bwd: the adjoint (what Jittor's autograd derives op by op); d_xyz / d_scales / d_rots / d_opac may be
 *   NULL (= zero); d_mr (device float [1], may be NULL) is the upstream gradient of that loss term; writes d_bc, d_dist,
 *   d_scaling, d_rotation, d_opacity. */
int gm_mesh_activate_fwd(int N, float alpha, const float* bc, const float* dist, const float* scaling, const float* rotation,
                         const float* opacity, const float* v1, const float* v2, const float* v3, const float* normal, const float* r,
                         float* xyz, float* scales, float* rots, float* opac, float mr_weight, float* mr_partial, void* stream);
int gm_mesh_activate_bwd(int N, float alpha, const float* bc, const float* dist, const float* scaling, const float* rotation,
                         const float* opacity, const float* v1, const float* v2, const float* v3, const float* normal, const float* r,
                         const float* d_xyz, const float* d_scales, const float* d_rots, const float* d_opac, float* d_bc, float* d_dist,
                         float* d_scaling, float* d_rotation, float* d_opacity, float mr_weight, const float* d_mr, void* stream);

/* gm_plain_activate_fwd: the plain 3DGS model's raw parameters -> rasterizer inputs (scene/gaussian_model.py:26-43, 96-117) in one pass:
 *   out_xyz = xyz, out_scales = exp(scaling), out_rots = rotation / max(|rotation|, 1e-12), out_opac = sigmoid(opacity).
 *   Inputs xyz/scaling float [N,3], rotation float [N,4] (16-byte aligned), opacity float [N].  The outputs are rows
 *   [row0, row0 + N) of buffers of `capacity` rows (out_rots 16-byte aligned): the head of joint [background; object] buffers.
 * gm_plain_activate_bwd: the adjoint.  g_xyz / g_scales / g_rots / g_opac (rows [row0, row0 + N) of `capacity`-row buffers; each
 *   may be NULL = zero) -> d_xyz = g_xyz, d_scaling = g_scales * exp(scaling), d_rotation = the normalisation's Jacobian applied to
 *   g_rots, d_opacity = g_opac * s (1 - s); outputs [N] rows. */
int gm_plain_activate_fwd(int N, const float* xyz, const float* scaling, const float* rotation, const float* opacity, float* out_xyz,
                          float* out_scales, float* out_rots, float* out_opac, int row0, int capacity, void* stream);
int gm_plain_activate_bwd(int N, const float* scaling, const float* rotation, const float* opacity, const float* g_xyz, const float* g_scales,
                          const float* g_rots, const float* g_opac, int row0, int capacity, float* d_xyz, float* d_scaling, float* d_rotation,
                          float* d_opacity, void* stream);

/* jittor.nn.Adam's update (the optimizer of training_setup, scene/mesh_based_gaussian_model.py:242-263) for up to 8
 * parameter tensors in one launch:  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *   p -= lr sqrt(1-b2^step)/(1-b1^step) m / (sqrt(v) + eps).
 * The arrays are HOST arrays of `count` entries (device pointers, element counts, learning rates).  period/split/lr_rest
 * (may be NULL) give a tensor two rates: elements with (index % period) < split use lr, the others lr_rest - the SH
 * tensor [P,16,3] with period 48, split 3 is the reference's "f_dc" and "f_rest" groups without splitting the rows.
 * All tensors 16-byte aligned; gradients are read, not cleared.  beta1 / beta2 / eps are doubles: Jittor forms (1 - beta) in
 * python double precision before it meets the float32 tensors, and (1 - beta2) taken from a float32 0.999 is off by 1.3e-5. */
int gm_adam_step(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                 const uint64_t* sizes, const float* lr, const float* lr_rest, const uint32_t* period, const uint32_t* split,
                 double beta1, double beta2, double eps, int step, void* stream);
/* The same with `active` (host array, may be NULL; 0 = the whole tensor): of every period of tensor i only the elements with
 * (index % period) < active[i] - rounded up to a 16-byte granule - are read and written.  For the SH tensor while the model's
 * active degree D is below its maximum (train_mesh_gaussian.py:70-71 raises it every 1000 iterations): active = 3 (D+1)^2.
 * Coefficients above the active degree have g = m = v = 0, the update rule leaves them unchanged, so skipping them gives the
 * result of gm_adam_step bit for bit (the caller guarantees their gradients are zero: the rasterizer's backward writes zeros
 * there).  Needs sizes[i] % period[i] == 0. */
int gm_adam_step_active(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                        const uint64_t* sizes, const float* lr, const float* lr_rest, const uint32_t* period, const uint32_t* split,
                        const uint32_t* active, double beta1, double beta2, double eps, int step, void* stream);

/* Densification statistics of a training iteration in one pass (train_mesh_gaussian.py:119-126 and
 * scene/mesh_based_gaussian_model.py:587-589): for every Gaussian with radii[i] > 0 (render()'s visibility_filter)
 *   max_radii2D[i] = max(max_radii2D[i], radii[i]);  grad_accum[i] += |viewspace_grad[i, 0:2]|;  denom[i] += 1.
 * radii int32 [N]; viewspace_grad float [N,3] (the gradient of means2D); the three accumulators float [N]. */
int gm_densify_stats(int N, const int* radii, const float* viewspace_grad, float* max_radii2D, float* grad_accum, float* denom, void* stream);

/* Per-stage GPU timing (HIP events recorded on `stream` around each kernel group).  Off by default.
 * gm_profile_enable(1) starts collecting, gm_profile_read synchronises the recorded events and returns
 * accumulated milliseconds and launch count for a stage name ("preprocess","depth_sort","scan",
 * "duplicate","tile_sort","ranges","render","render_bwd","preprocess_bwd","deform","sh_colors","loss","loss_bwd");
 * gm_profile_reset clears the accumulators. */
void gm_profile_enable(int on);
void gm_profile_reset(void);
int gm_profile_read(const char* stage, double* total_ms, int64_t* launches);

/* Debugging aids of the repository's tools, never called by the package: while a device buffer is registered the forward
 * blend (tools/wave_trace.py: 8 x uint64 per wave - start / end clock, list length, entries evaluated ...) / the depth-bucket
 * sort and the two scatter kernels of the ordering (tools/bucket_stats.py, tools/pipeline_trace.py: 3 x uint64 per workgroup -
 * start / end clock, entries; 2048 records for the bucket sort, then 2048 for the depth partition's scatter, then 4096 for the tile
 * pass's: 3 * 8192 words) write per-wave / per-workgroup records into it; NULL switches the tracing off again.
 * Process-wide, not thread-safe.
 * One more measurement aid, read once from the environment: GM_DEBUG_STOP_AFTER = deform | depth | dup | tile makes every forward
 * stop launching after that stage (tools/stage_marginal.sh times the pipelined loop with it: what the remaining stages cost);
 * the frames are then garbage.  Unset in any real use. */
void gm_debug_render_trace(void* buffer);
void gm_debug_bucket_trace(void* buffer);

#ifdef __cplusplus
}
#endif
#endif
