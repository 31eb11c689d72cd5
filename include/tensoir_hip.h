/*
 * tensoir_hip.h -- C ABI of libtensoir_hip.so (MI355X / gfx950).
 *
 * The reference (Haian-Jin/TensoIR) has no FFI of its own: its hot path is a chain of ATen ops
 * behind a Python call surface.  This header is the boundary a maintainer
 * binds instead of those op chains; every entry point names the reference code it replaces
 * (paths relative to the TensoIR repository root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no framework types.  Every pointer is a DEVICE pointer unless it is
 *     a `const Tir*` descriptor struct, which lives in HOST memory and is copied at launch.
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library allocates nothing
 *     and keeps no state.  Calls are asynchronous on `stream` (a hipStream_t passed as void*);
 *     no hipDeviceSynchronize inside; safe for hipGraph capture.
 *   - fp32 I/O, int32 indices, int64 sizes.  Return 0 on success, a negative TIR_ERR_* /
 *     -(hipError_t) on failure; nothing throws across the ABI.
 *   - re-entrant; no internal threads.
 *
 * The Python binding (tensoir_amd/_lib.py) is generated from this file at import: the `typedef struct X { ... } X;` blocks, the
 * prototypes and the `#define TIR_NAME value` lines (an integer, a floating literal without suffix or a parenthesised quotient of
 * two; other macros are not published).  Its parser reads plain declarations only and refuses the rest, so keep to these type
 * names: int, int32_t, int64_t, uint64_t, float, double and the structs by value; void, char, unsigned, unsigned long long, uint8_t,
 * uint16_t, uint32_t behind a pointer.  Parameters are named, no function pointers, no #if beyond the guard and __cplusplus.
 */
#ifndef TENSOIR_HIP_H
#define TENSOIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIR_VERSION 100            /* 0.1.0 */

#define TIR_OK               0
#define TIR_ERR_ARG         -1001  /* null pointer / negative size / inconsistent descriptor      */
#define TIR_ERR_UNSUPPORTED -1002  /* shape outside what the gfx950 kernels were built for        */
#define TIR_ERR_NO_DEVICE   -1003  /* no HIP device / kernel image not loadable on this device    */

/* ---------------------------------------------------------------------------------------------
 * Packed VM field (device-resident shadow of TensorVMSplit's parameters).
 * Reference layout: density_plane[i] [1,C,H_i,W_i], density_line[i] [1,C,R_i,1]
 * (models/tensoRF_rotated_lights.py:19-29); here channel-last so one bilinear tap is one
 * contiguous C*4-byte run (64 B for C=16, 192 B for C=48).
 *   plane i: H_i = grid[matMode[i][1]], W_i = grid[matMode[i][0]]; line i: R_i = grid[vecMode[i]]
 *   matMode = {{0,1},{0,2},{1,2}}, vecMode = {2,1,0}   (models/tensorBase_rotated_lights.py:398-399)
 * ------------------------------------------------------------------------------------------- */
typedef struct TirField {
    float aabb_min[3];
    float aabb_max[3];
    float inv_aabb[3];       /* 2/(max-min), fp32 as update_stepSize computes it (:611-612)        */
    int32_t grid[3];         /* gridSize x,y,z                                                      */
    float step_size;         /* stepSize (:615)                                                     */
    float distance_scale;    /* 25  (opt.py:77)                                                     */
    float density_shift;     /* -10 (opt.py:79)                                                     */
    float weight_thres;      /* rayMarch_weight_thres 1e-4 (:354)                                   */
    float near_, far_;       /* near_far (:385)                                                     */
    int32_t act;             /* 0 = softplus, 1 = relu  (feature2density :813-817)                  */
    int32_t n_dcomp;         /* density channels per plane (16), multiple of 4                      */
    int32_t n_acomp;         /* appearance channels per plane (48), multiple of 4                   */
    int32_t app_dim;         /* 27                                                                  */
    int32_t n_lights;
    const float* dplane[3];  /* [H_i][W_i][n_dcomp]                                                 */
    const float* dline[3];   /* [R_i][n_dcomp]                                                      */
    const float* aplane[3];  /* [H_i][W_i][n_acomp]                                                 */
    const float* aline[3];   /* [R_i][n_acomp]                                                      */
    const float* basis_t;    /* [3*n_acomp][32]: basis_mat^T, app_dim padded to 32 with zeros       */
    const float* light_line; /* [n_lights][3*n_acomp]  (light_line.weight)                          */
    const float* light_mean; /* [3*n_acomp] mean over lights (tensoRF_rotated_lights.py:160-161)    */
    const uint8_t* occ_nbr;  /* AlphaGridMask as 2x2x2 neighbourhood bytes (tir_pack_occupancy); NULL = no mask */
    int32_t occ_dim[3];      /* W,H,D of the mask volume                                            */
    float occ_aabb_min[3];   /* the mask's own aabb (:105) ...                                      */
    float occ_inv[3];        /* ... and (1/size)*2 (:107)                                           */
    float occ_lo[3];         /* world-space box that contains every point the mask can report as occupied (the occupied   */
    float occ_hi[3];         /* voxels' extent + one cell): the secondary march skips 32-sample steps that lie outside.  */
                             /* occ_lo >= occ_hi on any axis (e.g. all zeros) = not given, nothing is skipped.            */
    /* Launch options (performance only, results are identical either way).  They travel WITH the descriptor: the library
     * keeps no settable state and reads no environment variable, so two embedders in one process cannot disturb each other. */
    int32_t tune_lds_lines;  /* secondary march with the density lines staged in LDS: 0 = default (on), 1 = on, 2 = off */
    int32_t tune_xcd_order;  /* contiguous per-XCD work ranges in the gathers / secondary march: 0 = default (off), 1 = on, 2 = off */
    /* Optional dense density-feature volume (tir_dense_sigma_build): V[z][y][x] = the VM density feature at grid corner
     * (x, y, z), fp32, x fastest, rows of dense_pitch >= grid[0] + 1 floats (the element behind a row's last corner is 0).
     * Inside a grid cell the VM feature is multilinear, so the trilinear lookup of V equals it in real arithmetic (fp32
     * results differ in the last bits).  The secondary march reads V instead of the 18 VM taps when it is given;
     * NULL / 0 (a zeroed descriptor) = no volume, the VM kernels run.  The caller rebuilds V when the field changes. */
    const float* dense_sigma;
    int32_t dense_pitch;
    /* Optional dense appearance-feature volume of a field with ONE light (tir_dense_app_build): for grid corner (x, y, z) the
     * 27 radiance features basis_mat . (plane x line x light row 0) as fp16, [z][y][x of dense_app_pitch >= grid[0] + 1]
     * [half 2][16]: half 0 = features 0..13, half 1 = features 14..26, unused slots 0, 64 bytes per corner, 16-byte aligned,
     * below 4 GiB.  Inside a grid cell the features are multilinear, so the trilinear lookup equals them in real arithmetic.
     * The fp16 indirect-light entries (tir_vm_app_fwd_h16, tir_indirect_fused_fwd) read it instead of the fp16 shadow taps when
     * it is given and n_lights == 1; NULL / 0 = no volume.  The caller rebuilds it when the field changes. */
    int32_t dense_app_pitch;
    const void* dense_app;
} TirField;

/* fp16 shadow of the appearance planes / lines (same channel-last element order as TirField::aplane / aline; 16-byte aligned),
 * produced by tir_pack_half and read by tir_vm_app_fwd_h16. */
typedef struct TirFieldHalf {
    const void* aplane[3];   /* [H_i][W_i][n_acomp] fp16 */
    const void* aline[3];    /* [R_i][n_acomp]      fp16 */
} TirFieldHalf;

/* (internal launch records of tir_pack_half) */
#define TIR_HALF_MAX_JOBS 8
typedef struct TirHalfJob { const float* src; void* dst; int64_t n; unsigned* absmax; } TirHalfJob;
typedef struct TirHalfJobs { TirHalfJob job[TIR_HALF_MAX_JOBS]; } TirHalfJobs;

/* One 3-layer decoder (in -> hidden ReLU -> hidden ReLU -> out, then activation):
 * MLPRender_Fea / MLPBRDF_PEandFeature (models/tensorBase_rotated_lights.py:122-146, :182-208).
 * `packed` is produced by tir_pack_mlp. */
typedef struct TirMlp {
    const float* packed;
    int32_t feat_dim;        /* 27                                                                  */
    int32_t pe;              /* fea_pe == view_pe == pos_pe (2)                                     */
    int32_t hidden;          /* 128                                                                 */
    int32_t out_dim;         /* 3 (rgb, normal) or 4 (albedo+roughness)                             */
    int32_t act;             /* 0 = sigmoid, 1 = tanh                                               */
    int32_t tune_grid;       /* launch option: persistent workgroups of a decoder launch, 0 = default (256 = one per CU) */
} TirMlp;

/* Environment light as spherical Gaussians + per-light z-rotation
 * (models/tensorBase_rotated_lights.py:461-488, :577-606). */
typedef struct TirEnvSG {
    const float* sgs;        /* [n_sg][7]  lobe xyz, lambda, mu rgb (raw parameters)                */
    const float* rot;        /* [n_lights][9] row-major light_rotation_matrix                       */
    int32_t n_sg;
    int32_t n_lights;
} TirEnvSG;

int  tir_version(void);
const char* tir_error_string(int code);
/* 0 when a gfx950 device is present and the code object loads. */
int  tir_device_check(void);

/* ---- packing (build the shadow copies; re-run after any parameter update / upsample / shrink:
 *      train_tensoIR.py:385-422) -------------------------------------------------------------- */
/* [C,H,W] -> [H,W,C]   (also lines with W=1) */
int tir_pack_plane(const float* src, float* dst, int32_t C, int32_t H, int32_t W, void* stream);
/* float volume [D][H][W] -> (D+1)*(H+1)*(W+1) neighbourhood bytes: byte (z0+1,y0+1,x0+1), bit dx+2dy+4dz =
 * voxel (x0+dx,y0+dy,z0+dz) inside the grid and > 0.5 (0.5 itself is not occupied).  The trilinear
 * "sample_alpha(...) > 0" test of a point then needs one byte.  Base voxels run from -1 to dim-1 per axis: the
 * volume is zero outside its grid (grid_sample's zero padding), so the bytes of base -1 and of base dim-1 hold
 * the one-cell skirt round the mask's box in which a point can still be a hit. */
int tir_pack_occupancy(const float* vol, uint8_t* nbr, int32_t W, int32_t H, int32_t D, void* stream);
/* basis_mat.weight [app_dim][n_in] -> [n_in][32] */
int tir_pack_basis(const float* w, float* dst, int32_t app_dim, int32_t n_in, void* stream);
/* light_line.weight [L][n] -> mean over L [n] */
int tir_light_mean(const float* light_line, float* mean, int32_t L, int32_t n, void* stream);
int64_t tir_mlp_packed_floats(int32_t feat_dim, int32_t pe, int32_t hidden, int32_t out_dim);
/* nn.Linear weights ([out][in] row-major) + biases of mlp.{0,2,4} -> packed blob */
int tir_pack_mlp(const float* w0, const float* b0, const float* w1, const float* b1,
                 const float* w2, const float* b2, int32_t feat_dim, int32_t pe, int32_t hidden,
                 int32_t out_dim, float* packed, void* stream);

/* ---- K2: compute_densityfeature + feature2density (models/tensoRF_rotated_lights.py:95-110,
 *      models/tensorBase_rotated_lights.py:813-817).  xyz normalised to [-1,1]^3.
 *      feat / sigma may each be NULL. */
int tir_vm_density_fwd(const TirField* f, const float* xyz, float* feat, float* sigma,
                       int64_t n, void* stream);

/* ---- a2: AlphaGridMask.sample_alpha(xyz) > 0 (models/tensorBase_rotated_lights.py:112-119) at
 *      world-space points; hit[n] = 1/0.  Needs f->occ_nbr.  The lookup, shared by every kernel that culls by the
 *      mask: index coordinates i = ((q + 1) / 2) * (dim - 1), q = (p - occ_aabb_min) * occ_inv - 1, each step
 *      rounded to float32 (the reference's own steps) -- in the MASK's box, which need not be the field's (after
 *      shrink it is larger).  The point is a hit when one of the 8 voxels round it (base floor(i), zero outside the
 *      grid) is occupied AND has a non-zero trilinear weight: a coordinate with fraction exactly 0 sees only its
 *      base voxel on that axis.  Points up to one cell outside the mask's box can therefore be hits (the skirt),
 *      points further out never are.  A coordinate that is NaN, +-inf or far beyond the box (+-1e30: floor(i) is
 *      clamped to [-2, dim] before the integer conversion) makes the point a miss. */
int tir_occupancy_query(const TirField* f, const float* xyz, uint8_t* hit, int64_t n, void* stream);

/* ---- occupancy-grid maintenance (models/tensorBase_rotated_lights.py:737-811, :819-837).
 *      tir_dense_alpha: getDenseAlpha + compute_alpha on a gx*gy*gz lattice spanning the aabb; lin_* are the
 *      caller's linspace(0,1,g) tables (device), alpha [gx][gy][gz] = 1 - exp(-sigma * length), sigma = 0 where the
 *      current mask (f->occ_nbr, may be NULL) culls the point.
 *      tir_alpha_pool: updateAlphaMask's clamp -> transpose -> 3x3x3 max-pool -> threshold; vol [gz][gy][gx] float 0/1:
 *      vol[z][y][x] = 1 when the maximum of min(max(alpha[x'][y'][z'], 0), 1) over the neighbours inside the lattice
 *      (the window is cut at the borders, nothing wraps) is >= thres, compared in float32.  A NaN alpha counts as 0
 *      (fmaxf drops it, where max_pool3d would spread it): it passes thres <= 0 only.  bbox (optional, 6 ints pre-set
 *      by the caller to the sentinels {INT_MAX x3, -1 x3}) receives min x, y, z and max x, y, z of the occupied
 *      voxels through atomic min / max; when no voxel passes the words keep the sentinels (bbox[3] < 0: empty scene).
 *      tir_filter_rays: filtering_rays; mask[i] = ray i may hit something.  Slab test of the FIELD's box: a zero
 *      direction component (+0 or -0) is replaced by +1e-6f, rates (aabb - o) / d by IEEE division, tmin the largest
 *      of the three smaller rates, tmax the smallest of the larger.  bbox_only: mask = tmax > tmin, strictly (a ray
 *      through an edge or a corner, tmax == tmin, gives 0, as the reference does).  Otherwise t0 = min(max(tmin,
 *      near_), far_) and mask = some sample k in [0, n_samples) at o + d * (t0 + step_size * k) is a hit of the
 *      lookup above (samples are not tested against the box; one wave per ray, 64 samples per pass). */
int tir_dense_alpha(const TirField* f, const float* lin_x, const float* lin_y, const float* lin_z,
                    int32_t gx, int32_t gy, int32_t gz, float length, float* alpha, void* stream);
int tir_alpha_pool(const float* alpha, int32_t gx, int32_t gy, int32_t gz, float thres, float* vol,
                   int32_t* bbox, void* stream);
int tir_filter_rays(const TirField* f, const float* rays, int64_t n, int32_t n_samples, int32_t bbox_only,
                    uint8_t* mask, void* stream);

/* ---- dense density-feature volume (TirField::dense_sigma).
 *      tir_dense_sigma_build: vol [grid z][grid y][pitch] (pitch >= grid x + 1, at most 4 GB) receives the VM density
 *      feature at every grid corner: the sum over the 3 * n_dcomp plane x line products accumulated in fp64 and rounded
 *      to fp32 once; elements [grid x, pitch) of every row are set to 0.  f->dense_sigma is not read.
 *      tir_dense_sigma_fwd: tir_vm_density_fwd through the trilinear lookup of f->dense_sigma (the secondary march's
 *      arithmetic; UNSUPPORTED without a volume).  Out-of-range corners carry weight 0 as in the VM gather. */
int tir_dense_sigma_build(const TirField* f, float* vol, int32_t pitch, void* stream);
int tir_dense_sigma_fwd(const TirField* f, const float* xyz, float* feat, float* sigma, int64_t n, void* stream);

/* ---- dense appearance-feature volume (TirField::dense_app; 48 components per plane, app_dim 27, ONE light).
 *      tir_dense_app_build: vol [grid z][grid y][pitch][2][16] fp16 (pitch >= grid x + 1 corners, 16-byte aligned, below
 *      4 GiB) receives the radiance features of light row 0 at every grid corner: the 144 plane x line x light products and
 *      their basis_mat sums in fp32, rounded to fp16 once (saturating); corners [grid x, pitch) of every row and the unused
 *      slots are 0.  f->dense_app is not read.  TIR_ERR_ARG: null / misaligned volume, pitch without the spare corner;
 *      TIR_ERR_UNSUPPORTED: n_lights != 1, another width, a volume beyond 32-bit byte offsets. */
int tir_dense_app_build(const TirField* f, void* vol, int32_t pitch, void* stream);

/* ---- K6: analytic d sigma/d xyz and derived normal -normalize(grad, eps=1e-6)
 *      (compute_derived_normals models/tensorBase_rotated_lights.py:839-856 ->
 *       compute_densityfeature_with_xyz_grad models/tensoRF_rotated_lights.py:113-129 ->
 *       models/relight_utils.py:57-107).  sigma/grad/normal may each be NULL.  n_dev: as tir_vm_app_fwd. */
int tir_density_grad_fwd(const TirField* f, const float* xyz, float* sigma, float* grad,
                         float* normal, int64_t n, const int32_t* n_dev, void* stream);
/* compute_densityfeature_with_xyz_grad (models/tensoRF_rotated_lights.py:113-129): feat [n] = the density feature with the
 *      border-clamped taps of models/relight_utils.py:57-107 (clamped indices, unclamped weights; equal to
 *      tir_vm_density_fwd's inside [-1,1]^3), grad [n][3] = d feat / d xyz -- before the activation, unlike
 *      tir_density_grad_fwd's `grad`.  Either output may be NULL. */
int tir_density_feat_grad_fwd(const TirField* f, const float* xyz, float* feat, float* grad, int64_t n, void* stream);

/* ---- K4: compute_appfeature / compute_intrinfeature / compute_bothfeature
 *      (models/tensoRF_rotated_lights.py:132-224).  light_idx (per point, or per `idx_map` entry when
 *      idx_map != NULL: light_idx[idx_map[p]]; with idx_div > 1 the selector is divided by idx_div first, e.g.
 *      pair id -> surface point) may be NULL when rad_feat is NULL.
 *      rad_feat / int_feat [n][out_stride] (app_dim <= out_stride <= 32; columns >= app_dim are written
 *      as 0; 32 gives aligned 128-byte rows), either may be NULL.
 *      n_dev (optional device pointer): the kernels process min(n, *n_dev) points, so a caller that sized its
 *      buffers for n can launch before the producing kernel's count has reached the host. */
int tir_vm_app_fwd(const TirField* f, const float* xyz, const int32_t* light_idx,
                   const int32_t* idx_map, float* rad_feat, float* int_feat, int32_t out_stride,
                   int32_t idx_div, int64_t n, const int32_t* n_dev, void* stream);

/* Intrinsic feature of JITTERED points xyz + scale * N(0,1) (the smoothness pass of
 * models/tensorBase_rotated_lights.py:937-938) with the noise drawn inside the gather kernel: Philox4x32-10 keyed by
 * (seed, offset) -- the caller framework's generator state -- with the point index as counter, Box-Muller.  rng_state
 * (device int64 {seed, offset}, optional) overrides the by-value pair (HIP-graph replays).  xyz_out [n][3] receives the
 * jittered points (aux input of the BRDF decoder), int_feat [n][out_stride] their intrinsic features. */
int tir_vm_app_jitter_fwd(const TirField* f, const float* xyz, int64_t n, const int32_t* n_dev, float scale,
                          uint64_t seed, uint64_t offset, const int64_t* rng_state, float* xyz_out,
                          float* int_feat, int32_t out_stride, void* stream);

/* tir_vm_app_fwd (radiance + intrinsic features of xyz) and tir_vm_app_jitter_fwd (intrinsic features of the jittered xyz)
 * in ONE launch -- the two appearance gathers of the primary stage (n_acomp == 48).  Arguments as in the two calls. */
int tir_vm_app_primary_fwd(const TirField* f, const float* xyz, const int32_t* light_idx, const int32_t* idx_map,
                           float* rad_feat, float* int_feat, int32_t out_stride, int64_t n, const int32_t* n_dev,
                           float scale, uint64_t seed, uint64_t offset, const int64_t* rng_state, float* xyz_out,
                           float* int_feat_jit, void* stream);
/* the same launch with basis_mat's contraction (models/tensoRF_rotated_lights.py:159-165, :191-195) on v_mfma_f32_16x16x32_f16 and
 * both operands split x = hi + lo in fp16 (three products, fp32 accumulate: ~2^-21 relative per product -- the features agree with
 * the exact-fp32 contraction of tir_vm_app_primary_fwd to ~2e-6 of their scale): a quarter of the matrix-pipe time of the exact-fp32
 * instruction, which runs at the vector rate.  Opt-in (TENSOIR_APP_CONTRACTION=x3): fp16 residues of products below 0.125 are
 * subnormal, so the features are good to ~1e-6 of their scale, which a trained BRDF decoder amplifies to 1e-4 on the albedo map. */
int tir_vm_app_primary_x3_fwd(const TirField* f, const float* xyz, const int32_t* light_idx, const int32_t* idx_map,
                              float* rad_feat, float* int_feat, int32_t out_stride, int64_t n, const int32_t* n_dev,
                              float scale, uint64_t seed, uint64_t offset, const int64_t* rng_state, float* xyz_out,
                              float* int_feat_jit, void* stream);
/* tir_vm_app_fwd with the contraction on v_mfma_f32_16x16x32_f16 and both operands split x = hi + lo in fp16 (three products,
 * ~2^-21 relative per product; see tir_vm_app_primary_x3_fwd): n_acomp 16 / 24 / 48. */
int tir_vm_app_fwd_x3(const TirField* f, const float* xyz, const int32_t* light_idx,
                      const int32_t* idx_map, float* rad_feat, float* int_feat, int32_t out_stride,
                      int32_t idx_div, int64_t n, const int32_t* n_dev, void* stream);
/* same contract with the 144 x 27 contraction on v_mfma_f32_16x16x32_bf16 and every operand split x = hi + lo in bf16
 * (three products, fp32 accumulate: parity grade, features agree with the exact kernel to ~1e-6); n_acomp <= 64. */
int tir_vm_app_fwd_bf16x3(const TirField* f, const float* xyz, const int32_t* light_idx,
                          const int32_t* idx_map, float* rad_feat, float* int_feat, int32_t out_stride,
                          int32_t idx_div, int64_t n, const int32_t* n_dev, void* stream);
/* same contract, one-sample-per-lane VALU kernel (cross-check of the matrix-core kernel) */
int tir_vm_app_fwd_valu(const TirField* f, const float* xyz, const int32_t* light_idx,
                        const int32_t* idx_map, float* rad_feat, float* int_feat, int32_t out_stride,
                        int32_t idx_div, int64_t n, const int32_t* n_dev, void* stream);

/* ---- K5: positional_encoding + 3-layer MLP + activation
 *      (models/tensorBase_rotated_lights.py:12-17, :136-146, :198-208).
 *      input row = [feat, aux, PE(feat), PE(aux)]; aux row p is aux[aux_map ? aux_map[p] : p];
 *      feat rows are feat_stride floats apart (>= feat_dim).  aux_mod > 0: the aux row index is taken modulo
 *      aux_mod (pair id -> direction).  n_dev: as tir_vm_app_fwd.
 *      Columns >= feat_dim of a feature row never reach a result: they may hold anything (NaN included) in every decoder
 *      entry from here to tir_mlp_bwd_multi_bf16x3, forward, tir_mlp_inputs and backward-data alike; the row loads that
 *      fetch column 27 (16-byte aligned rows, stride % 4 == 0) discard it (tests/test_gpu_decoder_kernels.py). */
int tir_mlp_fwd(const TirMlp* m, const float* feat, int32_t feat_stride, const float* aux,
                const int32_t* aux_map, int32_t aux_mod, float* out, int64_t n, const int32_t* n_dev,
        void* stream);
/* same contract on v_mfma_f32_32x32x16_bf16 with every operand split x = hi + lo in bf16 and the three
 * products hi*hi + hi*lo + lo*hi accumulated in fp32 (~16 mantissa bits; measured <= 2e-6 abs on the
 * decoder outputs): the parity-grade fast path. */
int tir_mlp_fwd_bf16x3(const TirMlp* m, const float* feat, int32_t feat_stride, const float* aux,
                       const int32_t* aux_map, int32_t aux_mod, float* out, int64_t n, const int32_t* n_dev,
        void* stream);

/* ---- precision policy for INDIRECT light (the radiance of the secondary-ray records, models/relight_utils.py:818-832).
 *      tir_pack_half: fp32 -> fp16 copies (round to nearest even, SATURATING: |x| > 65504 -> +-65504, never inf) of up to
 *      TIR_HALF_MAX_JOBS tables in one launch; srcs / dsts / counts are HOST arrays, tables 16-byte aligned.
 *      tir_pack_half_checked: the same, and absmax[i] (DEVICE floats, zeroed by the caller before the call) receives max |x| of
 *      table i (a NaN anywhere in the table is reported as NaN; its fp16 copy is -65504, the saturating clamp orders a NaN below
 *      every number); dsts[i] == NULL scans table i without writing a copy (light rows, basis_mat).
 *      RANGE CONTRACT of the fp16 gather below: interpolation and the products (plane * line) * light-row run
 *      on the packed fp16 pipe WITHOUT a saturation test in the hot loop, so the caller must establish
 *      max|plane_i| * max|line_i| * max(1, max|light row|) < 65504 for i = 0..2 and max|basis_mat| < 65504 from these maxima
 *      (bilinear taps are convex combinations, so the bound is rigorous) and use the fp32 gather (tir_vm_app_fwd) otherwise --
 *      the host mirror does exactly that (tensoir_amd/relight.py: _indirect_mode, ops.HalfRange).
 *      tir_vm_app_fwd_h16 = tir_vm_app_fwd(rad_feat only) for n_acomp == 48 on the fp16 shadow `fh` of f->aplane / f->aline:
 *      half the bytes through the vector L1 (the bound of the fp32 gather), interpolation and light-row product on the packed
 *      fp16 pipe (v_pk_fma_f16: two channels per instruction, rounded after every step), the basis_mat contraction on
 *      v_mfma_f32_32x32x16_f16 (fp32 accumulate).  In full: the light rows and basis_mat are rounded to fp16 in the kernel
 *      (saturating, like the shadow), the bilinear weights wx * wy (formed in fp32) and the line weights are rounded to fp16, and
 *      every step of pl = a w00 + b w01 + c w10 + d w11, ln = e l0 + g l1 and (pl * ln) * light rounds to fp16.  The light row
 *      is light_idx[(idx_map ? idx_map[s] : s) / idx_div] clamped to [0, n_lights - 1].  On a descriptor that carries
 *      dense_app (one light; no index is read) the features are instead the sum over the 8 cell corners of the volume's fp16
 *      corner features (accumulated in fp32 from the fp32 parameters, rounded once) times wx wy wz (formed in fp32, rounded to
 *      fp16), on the packed fp16 pipe: one fp16 rounding per step, clamped to +-65504; columns >= 27 are 0.  ~5e-4 relative on a
 *      feature: NOT parity grade on its own -- the product path uses it only for the secondary-ray records, whose radiance is
 *      averaged over a ray's records and the light directions before it reaches rgb_with_brdf_map.  Other arguments as
 *      tir_vm_app_fwd. */
int tir_pack_half(const float* const* srcs, void* const* dsts, const int64_t* counts, int32_t n_tables, void* stream);
int tir_pack_half_checked(const float* const* srcs, void* const* dsts, const int64_t* counts, int32_t n_tables, float* absmax,
                          void* stream);
int tir_vm_app_fwd_h16(const TirField* f, const TirFieldHalf* fh, const float* xyz, const int32_t* light_idx,
                       const int32_t* idx_map, float* rad_feat, int32_t out_stride, int32_t idx_div, int64_t n,
                       const int32_t* n_dev, void* stream);

/* The two launches above fused (north_star: gathers and decoder "in one pass"): for every record s < min(n, *n_dev) the radiance
 * features of xyz[s] (light row light_idx[rec_map[s] / idx_div]) are gathered from the fp16 shadow, contracted with basis_mat and
 * decoded by `m` (the radiance decoder; view-direction columns from `table` row rec_map[s] % aux_mod, tir_mlp_aux_table) without
 * the feature rows ever reaching HBM.  The light index is clamped to [0, n_lights - 1] (a field with one light reads none: row 0);
 * the features are clamped to +-65504 before they enter the decoder; a descriptor with dense_app takes the volume lookup of
 * tir_vm_app_fwd_h16.  out [n][m->out_dim].  n_acomp == 48, app_dim == 27.  Same precision class as the pair
 * tir_vm_app_fwd_h16 + tir_mlp_fwd_auxtab_f16 (results agree to fp32 summation order). */
int tir_indirect_fused_fwd(const TirField* f, const TirFieldHalf* fh, const TirMlp* m, const float* xyz,
                           const int32_t* light_idx, const int32_t* rec_map, int32_t idx_div, int32_t aux_mod,
                           const float* table, float* out, int64_t n, const int32_t* n_dev, void* stream);

/* The same stage (models/relight_utils.py:818-829: compute_appfeature -> renderModule on the secondary-ray records) in one
 * launch at the precision a TRAINED checkpoint needs (the auto policy's fallback when its self-check rejects the fp16 kernel;
 * before round 6 that fallback was tir_vm_app_fwd + tir_mlp_fwd_auxtab_bf16x3 with the feature rows through HBM): fp32 taps from
 * the parameters themselves (no shadow), fp32 interpolation, basis_mat contraction on fp16 hi + lo operands (three products),
 * decoder with fp16 activations and weights as fp16 + fp8 residue (tir_pack_mlp's OFF_F8 image, multiplied on the block-scaled
 * fp8 matrix instruction with the scale 2^-17 into the same fp32 accumulators; layer 3 exact).  n_lights <= 8 (more:
 * TIR_ERR_UNSUPPORTED, nothing is written).  Arguments as tir_indirect_fused_fwd without the shadow.  In full: each product
 * (plane * line) * light is clamped to +-65504 and split hi = fp16(x), lo = fp16(x - hi), basis_mat the same way, and hi hi + hi lo
 * + lo hi are summed in fp32; the features are clamped to +-65504.  The residue is e4m3((W - fp16(W)) 2^17) clamped to +-448 (it
 * saturates from |W| >= 7); the activations it multiplies are e4m3 as well -- the positional-encoding values as they are, the raw
 * feature clamped to +-448 first, the hidden activations cut at 448 -- so the residue corrects the weights, not the fp16 rounding
 * of the activations (~5e-4 of a record's output; it averages out, the weight rounding does not).  Range: a lo part below 2^-14 is
 * an fp16 subnormal and one below 2^-25 is nothing, so with products or basis_mat entries below ~2^-3 the contraction loses bits
 * step by step, and with products below 2^-14 (or basis_mat entries below ~1e-4) it is that of single fp16 operands: no better
 * than tir_indirect_fused_fwd there (tests/test_indirect_cpu.py prints the figures).  Deviation from the exact decoder on
 * rgb_with_brdf_map: measured per checkpoint by the policy's self-check (profiles/r06_*). */
int tir_indirect_fused_hp_fwd(const TirField* f, const TirMlp* m, const float* xyz, const int32_t* light_idx,
                              const int32_t* rec_map, int32_t idx_div, int32_t aux_mod, const float* table, float* out,
                              int64_t n, const int32_t* n_dev, void* stream);

/* Up to four decoders over the SAME n rows in one launch (split-bf16 matrix cores): the primary stage evaluates the
 * radiance, BRDF, jittered-BRDF and normal decoders (models/tensorBase_rotated_lights.py:927-955) on the same records.
 * mlps / feats / auxs / aux_maps / outs are HOST arrays of n_jobs entries (aux_maps or its entries may be NULL); feature
 * rows must be 16-byte aligned with a stride that is a multiple of 4 floats; outs[i] is [n][mlps[i]->out_dim]. */
int tir_mlp_fwd_multi_bf16x3(const TirMlp* const* mlps, const float* const* feats, int32_t feat_stride,
                             const float* const* auxs, const int32_t* const* aux_maps, float* const* outs,
                             int32_t n_jobs, int64_t n, const int32_t* n_dev, void* stream);

/* ---- aux-table variant of the split-bf16 decoder.  The 3 aux inputs of MLPRender_Fea are the view direction
 *      (models/tensorBase_rotated_lights.py:137-142): one value per ray in the primary stage, one per light direction for the
 *      secondary records -- few distinct rows for many decoder rows.  tir_mlp_aux_table evaluates, per aux row a, the part of
 *      layer 1 that depends on it alone: table[a][unit] = b0[unit] + sum over the 15 columns (aux, sin / cos PE(aux)) of
 *      W0[unit][col] x_col  (exact fp32; table is [n_aux][hidden], 16-byte aligned).  tir_mlp_fwd_auxtab_bf16x3 is
 *      tir_mlp_fwd_bf16x3 with that table in place of `aux` (row aux_map[s] -- or s when NULL -- modulo aux_mod when > 0): the
 *      layer-1 accumulators start from the table row, the matrix product runs over the other 135 inputs (9 instead of 10
 *      k-blocks).  Same results to fp32 rounding.  tir_mlp_fwd_multi_auxtab_bf16x3: tables[i] != NULL selects the variant for
 *      job i (auxs[i] is then unused and may be NULL). */
int tir_mlp_aux_table(const TirMlp* m, const float* aux, int64_t n_aux, float* table, void* stream);
int tir_mlp_fwd_auxtab_bf16x3(const TirMlp* m, const float* feat, int32_t feat_stride, const float* table,
                              const int32_t* aux_map, int32_t aux_mod, float* out, int64_t n, const int32_t* n_dev,
                              void* stream);
/* The aux-table decoder with ONE fp16 product per tile (v_mfma_f32_32x32x16_f16; operands rounded to 11 bits, fp32 accumulate,
 * layer 3 exact fp32): a third of the matrix work of tir_mlp_fwd_auxtab_bf16x3 at ~1e-4 absolute error per decoder output.
 * NOT parity grade by itself: meant for the radiance of the secondary-ray records (models/relight_utils.py:818-832), whose
 * error is averaged over a ray's records and the light directions before it reaches rgb_with_brdf_map.  Same arguments. */
int tir_mlp_fwd_auxtab_f16(const TirMlp* m, const float* feat, int32_t feat_stride, const float* table,
                           const int32_t* aux_map, int32_t aux_mod, float* out, int64_t n, const int32_t* n_dev,
                           void* stream);
/* The same launch for the training forward (h1, h2 [n][128] post-ReLU, as tir_mlp_train_fwd_bf16x3).  With aux_map == NULL and
 * aux_mod == 0 the table has one row PER DECODER ROW: that is how normals_kind == 'residue_prediction' is evaluated -- its decoder
 * MLPNormal_normal_and_PExyz (models/tensorBase_rotated_lights.py:236-262) feeds the derived normal as three more inputs of layer 1,
 * which the caller adds to the table rows (table += n W0[:, 3:6]^T) before the launch. */
int tir_mlp_train_fwd_auxtab_bf16x3(const TirMlp* m, const float* feat, int32_t feat_stride, const float* table,
                                    const int32_t* aux_map, int32_t aux_mod, float* out, float* h1, float* h2, int64_t n,
                                    const int32_t* n_dev, void* stream);
int tir_mlp_fwd_multi_auxtab_bf16x3(const TirMlp* const* mlps, const float* const* feats, int32_t feat_stride,
                                    const float* const* auxs, const int32_t* const* aux_maps,
                                    const float* const* tables, float* const* outs, int32_t n_jobs, int64_t n,
                                    const int32_t* n_dev, void* stream);
/* The same launch for the training forward: every job also writes its post-ReLU hidden activations h1s[i], h2s[i]
 * [n][128] (what tir_mlp_train_fwd_bf16x3 returns for one decoder). */
int tir_mlp_train_fwd_multi_bf16x3(const TirMlp* const* mlps, const float* const* feats, int32_t feat_stride,
                                   const float* const* auxs, const int32_t* const* aux_maps, float* const* outs,
                                   float* const* h1s, float* const* h2s, int32_t n_jobs, int64_t n,
                                   const int32_t* n_dev, void* stream);
/* single bf16 product (8 mantissa bits): reduced-precision mode, NOT parity grade (normals ~5e-3).  Everything that enters
 * a matrix product is rounded to bf16 once -- inputs, weights AND layer 1's bias, which rides as the weight of a constant-1
 * input: a bias of magnitude b carries an error of up to 2^-9 b (the split-bf16 entry keeps ~16 bits of it, the exact entry
 * all); tests/test_gpu_parity.py::test_decoder_large_biases states the resulting bounds. */
int tir_mlp_fwd_bf16(const TirMlp* m, const float* feat, int32_t feat_stride, const float* aux,
                     const int32_t* aux_map, int32_t aux_mod, float* out, int64_t n, const int32_t* n_dev,
        void* stream);
/* same contract, plain VALU kernel (any hidden size); used to cross-check the MFMA kernel */
int tir_mlp_fwd_valu(const TirMlp* m, const float* feat, int32_t feat_stride, const float* aux,
                     const int32_t* aux_map, int32_t aux_mod, float* out, int64_t n, const int32_t* n_dev,
        void* stream);

/* ---- K1+K2+K3 primary march: sample_ray + alpha-mask cull + density + raw2alpha
 *      (models/tensorBase_rotated_lights.py:705-724, :892-921, :21-28).
 *      rays [B][6]; ray_jitter [B] (is_train stratification, :717) or NULL.
 *      Outputs: weight [B][S]; acc[B] = sum w; depth[B] = sum w*z; t_end[B] = prod(1-a+1e-10);
 *      app_count[B] = #{w > weight_thres}.  t_stop: a ray stops marching once its running
 *      transmittance drops below t_stop (remaining weights are written as 0; the error in acc is
 *      < t_stop); pass 0 for the exact full march.
 *      stats (optional, NULL to skip): *stats += number of samples whose density was gathered
 *      (in bbox and not culled by the occupancy mask) -- the unit of the roofline accounting. */
int tir_march_primary_fwd(const TirField* f, const float* rays, const float* ray_jitter,
                          int32_t B, int32_t S, float t_stop, float* weight, float* acc,
                          float* depth, float* t_end, int32_t* app_count,
                          unsigned long long* stats, void* stream);

/* tir_march_primary_fwd plus the by-products that used to be separate launches of a step (each optional, NULL/0 to skip):
 *   viewdirs [B][3]     rays[:, 3:6] as a contiguous table = aux input of the radiance decoder
 *                       (the `viewdirs` of models/tensorBase_rotated_lights.py:872);
 *   zero_words[n_zero]  int32 counters of LATER kernels of the same pass, re-armed here (n_zero <= 256);
 *   ticket/offsets/cap/total  tir_exclusive_scan_capped(app_count) -> offsets[B+1], *total, done by the workgroup that
 *                       finishes last; `ticket` is one device int32 that must be zero before the first use (it re-arms
 *                       itself).  Replaces the boolean-mask bookkeeping of :924-926 without a second launch. */
int tir_march_primary_fused_fwd(const TirField* f, const float* rays, const float* ray_jitter,
                                int32_t B, int32_t S, float t_stop, float* weight, float* acc,
                                float* depth, float* t_end, int32_t* app_count, unsigned long long* stats,
                                float* viewdirs, int32_t* zero_words, int32_t n_zero, int32_t* ticket,
                                int32_t* offsets, int32_t cap, int32_t* total, void* stream);

/* exclusive scan of counts[n] -> offsets[n+1] (offsets[n] = total) */
int tir_exclusive_scan(const int32_t* counts, int32_t* offsets, int32_t n, void* stream);
/* same, with every offset clamped to `cap` (a record capacity chosen before the counts are known on the host):
 * consumers that index records through the offsets then stay inside buffers of `cap` records; *total (optional)
 * receives the unclamped total so the caller can detect the overflow afterwards and redo the pass. */
int tir_exclusive_scan_capped(const int32_t* counts, int32_t* offsets, int32_t n, int32_t cap,
                              int32_t* total, void* stream);

/* Record-capacity check of a captured (HIP-graph) step.  `state` (device, int64[5], zeroed by the caller, never cleared
 * by the call): running maximum of each of up to 4 device-side record counters [0..3] and a sticky overflow flag [4]
 * (set when counters[i] > caps[i]).  `host_out` (pinned host memory the device can write, int64[9]) receives this
 * launch's counters [0..3], the running maxima [4..7] and the flag [8].  `counters` / `caps` are HOST arrays. */
int tir_record_check(const int32_t* const* counters, const int64_t* caps, int32_t n, int64_t* state,
                     int64_t* host_out, void* stream);

/* Compact the samples with weight > thres into records ordered by (ray, sample) -- the order of
 * the reference's boolean-mask indexing xyz_sampled[app_mask] (:924-926).
 * rec_ray [A], rec_k [A], rec_w [A], rec_xyz [A][3] (normalised coords, :916). */
int tir_compact_primary(const TirField* f, const float* rays, const float* ray_jitter,
                        const float* weight, const int32_t* offsets, int32_t B, int32_t S,
                        int32_t* rec_ray, int32_t* rec_k, float* rec_w, float* rec_xyz,
                        void* stream);

/* ---- compositing + tone mapping of the primary pass (models/tensorBase_rotated_lights.py:973-1031).
 *      Per-record decoder outputs are summed per ray in sample order.  is_relight == 0 follows
 *      the early-return branch (:978-986).  Any per-record pointer may be NULL (treated as 0).
 *      out_maps [B][20]: rgb3 depth1 normal3 albedo3 rough1 fresnel3 acc1 ndiff1 norient1
 *                        albcost1 rghcost1 (pad1). */
#define TIR_MAP_STRIDE 20
int tir_composite_primary(const float* rays, const int32_t* offsets, const float* rec_w,
                          const float* rgb, const float* brdf, const float* brdf_jit,
                          const float* pred_normal, const float* derived_normal,
                          const float* acc, const float* depth, int32_t B, int32_t white_bg,
                          int32_t is_relight, float fixed_fresnel, float* out_maps, void* stream);

/* tir_composite_primary plus (a) the two smoothness losses = means over all B rays of map columns 17 / 18
 * (models/tensorBase_rotated_lights.py:999-1000) written to smooth_out[2] by the workgroup that finishes last
 * (`ticket`: one device int32, zero before the first use, re-arms itself; both or neither), and (b) the per-pass
 * advance of a device-side jitter-noise state rng_state = int64 {seed, offset}: offset += rng_step (NULL to skip). */
int tir_composite_primary_fused(const float* rays, const int32_t* offsets, const float* rec_w,
                                const float* rgb, const float* brdf, const float* brdf_jit,
                                const float* pred_normal, const float* derived_normal,
                                const float* acc, const float* depth, int32_t B, int32_t white_bg,
                                int32_t is_relight, float fixed_fresnel, float* out_maps, int32_t* ticket,
                                float* smooth_out, int64_t* rng_state, int64_t rng_step, void* stream);


/* ---- K7 secondary march: sample_ray_equally + cull + density + raw2alpha
 *      (models/relight_utils.py:707-722, :657-705, :777-834).
 *      Ray p starts at origins[org_map ? org_map[p] : p] along dirs[dir_map ? dir_map[p] : p];
 *      (with both maps NULL and n_dirs > 0: origin p / n_dirs, direction p % n_dirs -- the dense
 *      [surface point][direction] pair grid);  active[p] == 0 skips the ray (outputs 0).  n_sample <= 256.
 *      z_vals [n_sample] (device) are the sample distances near*(1-t)+far*t, t = linspace(0,1,n)
 *      (:716-717) -- passed in so that they are bit-identical to the caller framework's linspace.
 *      vis[p] = T_end, one_minus_acc[p] = 1 - sum w (either may be NULL).
 *      When rec_counter != NULL (TWO int32, zeroed by the caller) the samples with w > weight_thres are appended
 *      (contiguously per ray, in sample order; ray segments in arbitrary order) to rec_* (capacity rec_cap records;
 *      overflowing rays are dropped; rec_counter[0] still counts them = the capacity a re-run needs, rec_counter[1] =
 *      length of the record prefix that was actually written -- the row count consumers may process) and
 *      ray_rec_off[p] / ray_rec_cnt[p] locate ray p's segment.  stats: as tir_march_primary_fwd.
 *      With f->dense_sigma set the density feature comes from the trilinear lookup of that volume (any n_dcomp; with
 *      records n_sample <= 96, else the VM kernels run): same results up to the fp32 rounding of the feature. */
int tir_march_secondary_fwd(const TirField* f, const float* origins, const int32_t* org_map,
                            const float* dirs, const int32_t* dir_map, const uint8_t* active,
                            int64_t n_rays, int32_t n_dirs, int32_t n_sample, const float* z_vals,
                            float t_stop, float* vis, float* one_minus_acc,
                            int32_t* rec_counter, int64_t rec_cap, int32_t* rec_ray,
                            float* rec_w, float* rec_xyz, int32_t* ray_rec_off,
                            int32_t* ray_rec_cnt, unsigned long long* stats, void* stream);

/* tir_march_secondary_fwd over a LIST of rays: ray_ids[0 .. min(n_rays, *n_ids_dev)) are pair ids (as produced by
 * tir_shade_setup_compact); origin / direction / active / every output (vis, one_minus_acc, ray_rec_off, ray_rec_cnt,
 * rec_ray entries) are addressed by the pair id, so the per-pair arrays keep their dense [M*D] shape while no half-wave
 * is spent on a masked pair.  ray_ids == n_ids_dev == NULL: identical to tir_march_secondary_fwd. */
int tir_march_secondary_ids_fwd(const TirField* f, const float* origins, const int32_t* org_map,
                                const float* dirs, const int32_t* dir_map, const uint8_t* active,
                                int64_t n_rays, int32_t n_dirs, int32_t n_sample, const float* z_vals,
                                float t_stop, float* vis, float* one_minus_acc,
                                int32_t* rec_counter, int64_t rec_cap, int32_t* rec_ray,
                                float* rec_w, float* rec_xyz, int32_t* ray_rec_off,
                                int32_t* ray_rec_cnt, unsigned long long* stats, const int32_t* ray_ids,
                                const int32_t* n_ids_dev, void* stream);

/* indirect[p] = sum over ray p's records of w * rgb  (models/relight_utils.py:832) */
int tir_accumulate_records(const int32_t* ray_rec_off, const int32_t* ray_rec_cnt,
                           const float* rec_w, const float* rec_rgb, int64_t n_rays,
                           float* indirect, void* stream);

/* ---- a15: get_light_rgbs for spherical Gaussians (models/tensorBase_rotated_lights.py:577-588,
 *      :70-86).  dirs [D][3] -> out [n_lights][D][3]. */
int tir_env_sg_fwd(const TirEnvSG* e, const float* dirs, int32_t D, float* out, void* stream);

/* ---- a15, light_kind == 'pixel' (models/tensorBase_rotated_lights.py:585-605): the environment map is a learnable image
 *      light_rgbs [H][W][3] (`_light_rgbs`, :459-460) behind softplus(beta = 5); env[l][d][:] = bilinear lookup
 *      (F.grid_sample, align_corners=False, zero padding) at the equirectangular position of dirs[d] . rot[l]
 *      (rot [n_lights][9] row-major light_rotation_matrix).  env [n_lights][n_dirs][3].
 *      softplus = 0: the image is used as it is -- light_kind == 'gt', the data set's own probe (`dataset.lights_probes`, :592-593).
 *      _bwd: g_light [H][W][3] += d loss / d light_rgbs given g_env (atomics; zero-fill first; the softplus form only:
 *      the 'gt' probe is not trained). */
int tir_env_pixel_fwd(const float* light_rgbs, int32_t H, int32_t W, const float* rot, const float* dirs,
                      int32_t n_lights, int64_t n_dirs, int32_t softplus, float* env, void* stream);
int tir_env_pixel_bwd(const float* light_rgbs, int32_t H, int32_t W, const float* rot, const float* dirs,
                      int32_t n_lights, int64_t n_dirs, const float* g_env, float* g_light, void* stream);

/* ---- geometry of render_with_BRDF (models/relight_utils.py:417-435): surface point, view
 *      vector and the cosine mask.  maps = [M][TIR_MAP_STRIDE] rows of the selected rays,
 *      rays [M][6], dirs [D][3].  surf [M][3], active [M][D] = cosine > 1e-6 and acc > acc_thres
 *      (acc_mask of :1031 / renderer.py:86; pass a large negative value to shade every row). */
int tir_shade_setup(const float* maps, const float* rays, const float* dirs, int32_t M,
                    int32_t D, float acc_thres, float* surf, uint8_t* active, void* stream);

/* tir_shade_setup that also emits the compacted list of active pairs -- the reference's boolean-mask indexing
 * surf2l[cosine_mask] (models/relight_utils.py:440-441): pair_ids[0 .. *n_active) = m * D + d of the pairs with
 * active != 0 (order of wave-sized groups arbitrary), *n_active += their number (caller zeroes it, or lets
 * tir_shade_integrate_records re-arm it); vis[pair] = 0 and ray_rec_cnt[pair] = 0 (either may be NULL) for the masked
 * pairs, which then need no secondary ray at all (tir_march_secondary_ids_fwd).  pair_order (launch option, same results):
 * 0 = default = 1 = direction-major list (a march workgroup walks a bundle of parallel rays from neighbouring points),
 * 2 = point-major. */
int tir_shade_setup_compact(const float* maps, const float* rays, const float* dirs, int32_t M,
                            int32_t D, float acc_thres, float* surf, uint8_t* active, int32_t* pair_ids,
                            int32_t* n_active, float* vis, int32_t* ray_rec_cnt, int32_t pair_order, void* stream);

/* ---- K8: GGX_specular + rendering-equation sum + tone map
 *      (models/relight_utils.py:17-50, :452-480, :489-515).
 *      vis [M][D], indirect [M][D][3] (NULL = no indirect), env [n_lights][D][3],
 *      weight_d [D] = light_area_weight (or NULL with equal_area != 0: mean * 4pi, :470-471).
 *      out_rgb [M][3]; rows with acc <= acc_thres get the white background (renderer.py:105-106). */
int tir_shade_integrate(const float* maps, const float* rays, const float* dirs,
                        const int32_t* light_idx, const float* vis, const float* indirect,
                        const float* env, const float* weight_d, int32_t M, int32_t D,
                        int32_t n_lights, int32_t equal_area, int32_t use_srgb, float acc_thres,
                        float* out_rgb, void* stream);

/* Same as tir_shade_integrate with the indirect radiance of pair (m, d) summed inside the kernel from that ray's
 * records (ray_rec_off / ray_rec_cnt of tir_march_secondary_fwd, rec_rgb [A][3] = decoder output per record), i.e.
 * tir_accumulate_records fused into the integration: the [M][D][3] indirect buffer is never written.
 * reset_counter (optional): a device int the kernel sets to 0 -- the pair counter of tir_shade_setup_compact, re-armed by
 * the last consumer of the step so that no separate fill launch is needed (also under HIP-graph replay). */
int tir_shade_integrate_records(const float* maps, const float* rays, const float* dirs,
                                const int32_t* light_idx, const float* vis, const int32_t* ray_rec_off,
                                const int32_t* ray_rec_cnt, const float* rec_w, const float* rec_rgb,
                                const float* env, const float* weight_d, int32_t M, int32_t D,
                                int32_t n_lights, int32_t equal_area, int32_t use_srgb, float acc_thres,
                                float* out_rgb, int32_t* reset_counter, void* stream);

/* ---- K9: importance-sampled HDR relighting, loop body of scripts/relight_importance.py:119-170.
 *      Per surface point m and sample s: light_dir/rgb [M][Ns][3], pdf [M][Ns], vis [M][Ns].
 *      albedo [M][3], rough [M], fresnel [M][3], normal [M][3], rays_d [M][3].  out [M][3]. */
int tir_relight_importance(const float* normal, const float* albedo, const float* rough,
                           const float* fresnel, const float* rays_d, const float* light_dir,
                           const float* light_rgb, const float* light_pdf, const float* vis,
                           int32_t M, int32_t Ns, float* out_rgb, void* stream);

/* ---- K9 on the device (models/relight_utils.py:150-205, scripts/relight_importance.py:119-171).
 * tir_env_sample_setup: Environment_Light.sample_light + the cosine mask.  For every (point m, sample s) one cell of the
 *   H x W map is drawn from pdf_sample ~ (R+G+B) sin(theta) by inverse-CDF search -- row_cdf [H] = inclusive prefix sum of
 *   the row marginals (last = 1), col_cdf [H][W] = inclusive prefix sums of every row normalised to 1 -- with Philox
 *   uniforms keyed by (seed, offset), counter = m*Ns + s (the reference: torch.multinomial on the same pdf).
 *   cell [M][Ns] = flat cell index; active [M][Ns] = (env_dir[cell] . normal[m] > 1e-6) (:125-127).
 * tir_relight_importance_cells: tir_relight_importance with light_dir / rgb / pdf looked up by cell in the map's tables
 *   env_dir [H*W][3], env_rgb [H*W][3], env_pdf [H*W] (= hdr_pdf_return).
 * tir_env_lookup: Environment_Light.get_light, bilinear background lookup (align_corners=True) at n directions. */
int tir_env_sample_setup(const float* row_cdf, const float* col_cdf, int32_t H, int32_t W, const float* env_dir,
                         const float* normal, int32_t M, int32_t Ns, uint64_t seed, uint64_t offset,
                         int32_t* cell, uint8_t* active, void* stream);
/* tir_env_sample_setup_list: the same draws and mask (same Philox counters: identical cells), plus what the visibility
 *   query of :128-160 needs -- the UNMASKED pairs only, as a list.  pair_ids [M*Ns] receives the ids m*Ns + s of the pairs
 *   that pass the cosine mask, n_active [1] (zero on entry) their count; vis [M][Ns] is set to 0 for the masked pairs (the
 *   march -- tir_march_secondary_ids_fwd with ray_ids = pair_ids, n_ids_dev = n_active -- fills the rest).  The list is
 *   grouped: blocks of `block_pairs` consecutive pairs (256 ... 32768), inside a block by direction bin (bins_r x bins_c
 *   equal cells of the map, <= 255 bins; 1 x 1 = plain compaction), so that neighbouring list entries are nearly parallel
 *   rays from neighbouring surface points.  The order of the list enters no result.
 *   row_guide [guide_rows + 1] / col_guide [H][guide_cols + 2] (both or neither; sizes powers of two; a column row holds
 *   guide_cols + 1 entries and one pad): guide[k] = the search result for u = k / G (last entry = n - 1); the inverse-CDF
 *   search then starts inside [guide[k], guide[k+1]], k = floor(u G), and returns the same cell as the full search.
 *   dir_stride: floats between the directions of consecutive cells in env_dir (3 = the [H*W][3] table; 8 = the packed records
 *   of tir_relight_importance_cells_packed, whose first three floats are the direction). */
int tir_env_sample_setup_list(const float* row_cdf, const float* col_cdf, int32_t H, int32_t W, const float* env_dir,
                                int32_t dir_stride, const float* normal, int32_t M, int32_t Ns, uint64_t seed, uint64_t offset,
                                int32_t bins_r, int32_t bins_c, int32_t block_pairs, const int32_t* row_guide,
                                const uint16_t* col_guide, int32_t guide_rows, int32_t guide_cols, int32_t* cell,
                                float* vis, int32_t* pair_ids, int32_t* n_active, void* stream);
int tir_relight_importance_cells(const float* normal, const float* albedo, const float* rough,
                                 const float* fresnel, const float* rays_d, const int32_t* cell,
                                 const float* env_dir, const float* env_rgb, const float* env_pdf,
                                 const float* vis, int32_t M, int32_t Ns, float* out_rgb, void* stream);
/* the same with the three per-cell tables interleaved: env_cell [H*W][8] = {dir.x, dir.y, dir.z, pdf_return, r, g, b, 0}
 * (16-byte aligned): one 32-byte record per sample instead of three reads at unrelated addresses; same arithmetic. */
int tir_relight_importance_cells_packed(const float* normal, const float* albedo, const float* rough,
                                        const float* fresnel, const float* rays_d, const int32_t* cell,
                                        const float* env_cell, const float* vis, int32_t M, int32_t Ns,
                                        float* out_rgb, void* stream);
int tir_env_lookup(const float* env_rgb, int32_t H, int32_t W, const float* dirs, int64_t n, float* out, void* stream);

/* A relight chunk without a host round trip (scripts/relight_importance.py:99-113 selects the acc > 0.5 rows with boolean
 * masks -- a device-to-host synchronisation per chunk -- and :166-171 puts the relit colours back with index_put_):
 * tir_surface_compact: the rows of a chunk's primary maps [B][20] (tir_composite_primary layout) with acc > acc_thres as
 *   compacted surface-point arrays in ascending row order -- surf = o + depth d (:104), normal, albedo, rough [.], fresnel,
 *   rays_d (capacity B rows each; rows >= the count are left untouched) --, slot [B] = compacted index of a row or -1, and
 *   n_hit [1] = the count, all on the device.
 * tir_env_sample_setup_list_n / tir_relight_importance_cells_packed_n: the entries above with the number of surface points
 *   read from device memory (m_dev [1], clamped to M = the arrays' capacity; NULL = M): what tir_surface_compact produced.
 *   Same Philox counters per (point, sample) as the host-compacted call, hence the same cells and colours.
 * tir_env_compose: out[i] (rows of out_stride floats) = fg_rgb[slot[i]] where slot[i] >= 0, else the background lookup of
 *   tir_env_lookup at dirs[i] (rows of dir_stride floats: 6 with dirs = rays + 3). */
int tir_surface_compact(const float* maps, const float* rays, int32_t B, float acc_thres, float* surf, float* normal,
                        float* albedo, float* rough, float* fresnel, float* rays_d, int32_t* slot, int32_t* n_hit,
                        void* stream);
int tir_env_sample_setup_list_n(const float* row_cdf, const float* col_cdf, int32_t H, int32_t W, const float* env_dir,
                                int32_t dir_stride, const float* normal, int32_t M, int32_t Ns, uint64_t seed, uint64_t offset,
                                int32_t bins_r, int32_t bins_c, int32_t block_pairs, const int32_t* row_guide,
                                const uint16_t* col_guide, int32_t guide_rows, int32_t guide_cols, int32_t* cell,
                                float* vis, int32_t* pair_ids, int32_t* n_active, const int32_t* m_dev, void* stream);
int tir_relight_importance_cells_packed_n(const float* normal, const float* albedo, const float* rough,
                                          const float* fresnel, const float* rays_d, const int32_t* cell,
                                          const float* env_cell, const float* vis, int32_t M, int32_t Ns,
                                          float* out_rgb, const int32_t* m_dev, void* stream);
int tir_env_compose(const float* env_rgb, int32_t H, int32_t W, const float* dirs, int32_t dir_stride, int64_t n,
                    const int32_t* slot, const float* fg_rgb, float* out, int32_t out_stride, void* stream);

/* Relighting with multiple importance sampling of the map and the BRDF lobes.  N = n_l + n_b pairs per surface
 * point, Philox counter of pair (m, j) = m*N + j (four uniforms u0..u3), combined under the balance heuristic.
 * tir_env_mis_setup: pairs j < n_l draw a cell as tir_env_sample_setup_list does (same tables, guide tables and uniforms u0, u1:
 *   with n_b = 0 the cells are tir_env_sample_setup's at Ns = N) and place the direction uniformly in the cell's (polar, azimuth)
 *   rectangle, theta = (row + u2) pi / H, az = pi - (col + u3) 2 pi / W, w = (cos az sin theta, sin az sin theta, cos theta);
 *   density p_l(w) = P_cell H W / (2 pi^2 sin theta(w)).  Pairs j >= n_l draw from a one-sample mixture: for u0 < lobe_select a
 *   cosine-weighted direction about the unit raw normal (cos = sqrt(1 - u1), phi = 2 pi u2), otherwise a half vector about the
 *   flipped normal Nf of GGX_specular from D(h) (Nf.h), cos = sqrt((1 - u1) / (1 + (alpha2 - 1) u1)), phi = 2 pi u2, alpha2 =
 *   rough^4, reflected as w = 2 (v.h) h - v, v = safe_l2_normalize(-rays_d); density p_b(w) = s max(n.w, 0) / pi +
 *   (1 - s) D(Nf.h) max(Nf.h, 0) / (4 v.h) with h = normalize(v + w); their cell is row = floor(acos(z) H / pi), col =
 *   floor((pi - atan2(y, x)) W / (2 pi)), clamped to the table.
 *   env_cell: the [H*W][8] records of tir_relight_importance_cells_packed (cell_stride 8) or the [H*W][3] direction table
 *   (cell_stride 3, then env_pdf [H*W] = hdr_pdf_return is required); row_sin [H]: the sin(theta) table pdf_return was divided
 *   by, so that pdf_return * row_sin[row] = P_cell H W / (2 pi^2).  normal / rays_d [M][3], rough [M].
 *   Outputs: dirs [M][N][3], cell [M][N], pdf_mix [M][N] = (n_l p_l + n_b p_b) / N, vis [M][N] (0 written on inactive pairs; the
 *   march -- tir_march_secondary_ids_fwd on `dirs` with ray_ids = pair_ids, n_ids_dev = n_active -- fills the rest), pair_ids
 *   [M*N] = ids of the active pairs (blocks of `block_pairs` consecutive pairs, 256 ... 32768, in pair order within a block),
 *   n_active [1] (zero on entry).  A pair is inactive when normal.w <= 1e-6 or, for a lobe sample, v.h <= 0: pdf_mix = 1 there.
 *   m_dev [1] or NULL: device-side point count, as in tir_env_sample_setup_list_n.
 * tir_relight_mis: out [M][3] = (1 / N) sum_j (albedo / pi + GGX(w_j)) vis_j L[cell_j] (normal.w_j) / pdf_mix_j, L from the
 *   env_cell records (16-byte aligned); linear = 0: clamped to [0, 1] and sRGB-encoded, linear = 1: the raw mean. */
int tir_env_mis_setup(const float* row_cdf, const float* col_cdf, int32_t H, int32_t W, const float* env_cell,
                      int32_t cell_stride, const float* env_pdf, const float* row_sin, const float* normal,
                      const float* rays_d, const float* rough, int32_t M, int32_t n_l, int32_t n_b, float lobe_select,
                      uint64_t seed, uint64_t offset, int32_t block_pairs, const int32_t* row_guide,
                      const uint16_t* col_guide, int32_t guide_rows, int32_t guide_cols, float* dirs, int32_t* cell,
                      float* pdf_mix, float* vis, int32_t* pair_ids, int32_t* n_active, const int32_t* m_dev, void* stream);
int tir_relight_mis(const float* normal, const float* albedo, const float* rough, const float* fresnel,
                    const float* rays_d, const float* dirs, const int32_t* cell, const float* pdf_mix,
                    const float* env_cell, const float* vis, int32_t M, int32_t N, int32_t linear, float* out_rgb,
                    const int32_t* m_dev, void* stream);

/* GGX_specular alone (models/relight_utils.py:17-50): normal/v [M][3], l [M][D][3],
 * rough/fresnel [M][3] -> spec [M][D][3]. */
int tir_ggx_specular(const float* normal, const float* v, const float* l, const float* rough,
                     const float* fresnel, int32_t M, int32_t D, float* spec, void* stream);

/* =============================================================================================
 * Training (backward) entry points -- SURVEY.md section 8(f)-1.  The reference obtains these from
 * torch.autograd over its op chain (train_tensoIR.py:315-317 `total_loss.backward()`); here every
 * chain has a hand-written backward kernel.  Gradient buffers are caller-allocated and ACCUMULATED
 * into (zero them first); field gradients are in the packed channel-last layout of TirField.
 * Scatter-adds use hardware fp32 atomics (like ATen's grid_sampler backward), so the summation order --
 * not the set of addends -- varies from run to run.
 * ============================================================================================= */
typedef struct TirFieldGrad {
    float* dplane[3];        /* [H_i][W_i][n_dcomp]   d loss / d density_plane (channel-last)       */
    float* dline[3];         /* [R_i][n_dcomp]                                                      */
    float* aplane[3];        /* [H_i][W_i][n_acomp]                                                 */
    float* aline[3];         /* [R_i][n_acomp]                                                      */
    float* light_line;       /* [n_lights][3*n_acomp]  d loss / d light_line.weight                 */
    float* light_mean;       /* [3*n_acomp]  d loss / d mean-over-lights row (caller adds /L to every light) */
} TirFieldGrad;

/* tir_march_primary_fwd that additionally stores the per-sample density sigma [B][S] (0 for culled
 * samples) -- the only extra state the backward needs. */
int tir_march_primary_train_fwd(const TirField* f, const float* rays, const float* ray_jitter,
                                int32_t B, int32_t S, float t_stop, float* weight, float* sigma,
                                float* acc, float* depth, float* t_end, int32_t* app_count, void* stream);

/* Backward of tir_composite_primary (models/tensorBase_rotated_lights.py:973-1031).
 * g_maps [B][20]: d loss / d out_maps.  Outputs (written, not accumulated): per-record gradients g_rgb [A][3],
 * g_brdf [A][4] (w.r.t. the raw sigmoid outputs), g_brdf_jit [A][4], g_pred [A][3], g_der [A][3] (NULL where the
 * forward input was NULL; zeros where the input was given but the branch does not use it: everything but rgb with
 * is_relight == 0, derived_normal without pred_normal); g_weight [B][S] dense, MUST be zero-filled by the caller -- receives the record
 * part of d loss / d weight at (ray, rec_k); g_acc [B], g_depth [B]: gradients of the dense sums
 * acc = sum w, depth = sum w z. */
int tir_composite_primary_bwd(const float* rays, const int32_t* offsets, const int32_t* rec_k,
                              const float* rec_w, const float* rgb, const float* brdf,
                              const float* brdf_jit, const float* pred_normal,
                              const float* derived_normal, const float* acc, const float* depth,
                              int32_t B, int32_t S, int32_t white_bg, int32_t is_relight,
                              float fixed_fresnel, const float* g_maps, float* g_rgb, float* g_brdf,
                              float* g_brdf_jit, float* g_pred, float* g_der, float* g_weight,
                              float* g_acc, float* g_depth, void* stream);

/* Backward of raw2alpha + feature2density + compute_densityfeature along the primary rays
 * (models/tensorBase_rotated_lights.py:21-28, :813-817; models/tensoRF_rotated_lights.py:95-110):
 * d loss / d weight[b][k] = g_weight[b][k] + g_acc[b] + z_k g_depth[b]  ->  d alpha -> d sigma -> d feature,
 * scatter-added into g->dplane / g->dline.  g_feature (optional, NULL to skip): [B][S] receives d loss / d
 * density feature per sample (what is scattered). */
int tir_march_primary_bwd(const TirField* f, const TirFieldGrad* g, const float* rays,
                          const float* ray_jitter, int32_t B, int32_t S, const float* sigma,
                          const float* weight, const float* g_weight, const float* g_acc,
                          const float* g_depth, float* g_feature, void* stream);

/* Backward of tir_density_grad_fwd's derived normal w.r.t. the density planes/lines (the second-order
 * path of compute_derived_normals, models/tensorBase_rotated_lights.py:839-856: create_graph=True). */
int tir_density_grad_bwd(const TirField* f, const TirFieldGrad* g, const float* xyz,
                         const float* g_normal, int64_t n, void* stream);

/* ---- Per-point density backward at caller-given points (the autograd of the per-point methods, in any point order).
 * One point per 16-lane group (one channel per lane), eight consecutive points per group summed in registers while they
 * share a cell, line gradients summed in LDS per workgroup when they fit.  n_dcomp 4 / 8 / 16 / 32.
 * tir_vm_density_bwd: backward of tir_vm_density_fwd's feature (compute_densityfeature, models/tensoRF_rotated_lights.py:95-110;
 *      F.grid_sample taps: align_corners=True, zero padding).  g_feat [n] = d loss / d feature, scatter-added into
 *      g->dplane / g->dline.
 * tir_density_feat_bwd: backward of tir_density_feat_grad_fwd's feature (compute_densityfeature_with_xyz_grad,
 *      models/tensoRF_rotated_lights.py:113-129, border-clamped taps of models/relight_utils.py:81-92): the parameter
 *      scatter of g_feat [n] into g (NULL: skipped) and g_xyz_out [n][3] = g_feat * d feat / d xyz (NULL: skipped).
 * tir_density_feat_grad_bwd: its double backward (compute_derived_normals' create_graph=True,
 *      models/tensorBase_rotated_lights.py:839-856): for v [n][3], the VJP of sum_i v_i . d feat / d xyz (x_i) w.r.t. the
 *      planes and lines into g (NULL: skipped) and the Hessian-vector product g_xyz_out [n][3] = (d2 feat / d xyz2) v_i
 *      (NULL: skipped; bilinear / linear taps: mixed second derivatives only).
 * g and g_xyz_out may not both be NULL.  Float atomics: the summation order of the parameter gradients varies from run to run. */
int tir_vm_density_bwd(const TirField* f, const TirFieldGrad* g, const float* xyz, const float* g_feat, int64_t n,
                       void* stream);
int tir_density_feat_bwd(const TirField* f, const TirFieldGrad* g, const float* xyz, const float* g_feat,
                         float* g_xyz_out, int64_t n, void* stream);
int tir_density_feat_grad_bwd(const TirField* f, const TirFieldGrad* g, const float* xyz, const float* v,
                              float* g_xyz_out, int64_t n, void* stream);

/* Backward of tir_vm_app_fwd.  g_rad / g_int [n][stride] (either may be NULL; the first app_dim columns of a row are read,
 * the padding never).  The gradient buffers are ADDED to (float atomics: zero them first; a second call doubles them):
 * g->aplane, g->aline, g->light_line (the rows the samples used) and g->light_mean (the row the intrinsic feature used:
 * kept apart, the caller composes d light_line = light_line + light_mean / n_lights).  The y buffers are OVERWRITTEN:
 * y_rad / y_int [n][3*n_acomp] = (plane*line) (.) light row / light_mean,
 * the left operand of d basis_mat = g_feat^T y (tir_gemm_tn).  y_rad (y_int) is REQUIRED whenever g_rad (g_int) is
 * given: the buffer first holds dY = g_feat . basis_mat (an MFMA GEMM) and is then overwritten in place with y.
 * Sample i uses light row light_idx[idx_map ? idx_map[i] : i], CLAMPED to [0, n_lights - 1] (as tir_vm_app_fwd and
 * tir_shade_integrate do); idx_map (may be NULL) is read only when g_rad is given.
 * Samples should arrive in (ray, sample-along-ray) order -- tir_compact_primary's order: consecutive samples that
 * share a plane cell are summed in registers before they are scattered. */
int tir_vm_app_bwd(const TirField* f, const TirFieldGrad* g, const float* xyz,
                   const int32_t* light_idx, const int32_t* idx_map, const float* g_rad,
                   const float* g_int, int32_t stride, int64_t n, float* y_rad, float* y_int,
                   void* stream);

/* Decoder forward that also stores the post-ReLU hidden activations h1, h2 [n][hidden] (exact fp32 MFMA). */
int tir_mlp_train_fwd(const TirMlp* m, const float* feat, int32_t feat_stride, const float* aux,
                      const int32_t* aux_map, int32_t aux_mod, float* out, float* h1, float* h2,
                      int64_t n, const int32_t* n_dev, void* stream);
/* same on the split-bf16 matrix-core kernel (the product's default decoder precision; ~4x faster than exact fp32) */
int tir_mlp_train_fwd_bf16x3(const TirMlp* m, const float* feat, int32_t feat_stride, const float* aux,
                             const int32_t* aux_map, int32_t aux_mod, float* out, float* h1, float* h2,
                             int64_t n, const int32_t* n_dev, void* stream);
/* decoder input rows [n][160] = [feat, aux, PE(feat), PE(aux), 0-pad]  (right operand of d W0) */
int tir_mlp_inputs(const TirMlp* m, const float* feat, int32_t feat_stride, const float* aux,
                   const int32_t* aux_map, int32_t aux_mod, float* x, int64_t n, void* stream);
int64_t tir_mlp_bwd_packed_floats(int32_t feat_dim, int32_t pe, int32_t hidden, int32_t out_dim);
int tir_pack_mlp_bwd(const float* w0, const float* w1, const float* w2, int32_t feat_dim, int32_t pe,
                     int32_t hidden, int32_t out_dim, float* packed, void* stream);
/* Backward-data of one decoder: out / g_out [n][out_dim] (post-activation values and their gradients) ->
 * g_feat [n][32] (through the positional encoding; columns >= feat_dim are 0), and the pre-activation
 * gradients dz1, dz2 [n][hidden], dz3 [n][4] whose products with (x, h1, h2) are the weight gradients
 * (tir_gemm_tn).  `packed_bwd` from tir_pack_mlp_bwd. */
int tir_mlp_bwd(const TirMlp* m, const float* packed_bwd, const float* feat, int32_t feat_stride,
                const float* out, const float* g_out, const float* h1, const float* h2, int64_t n,
                float* g_feat, float* dz1, float* dz2, float* dz3, void* stream);
/* Same on the bf16 matrix pipe with split operands (3 products, fp32 accumulation; the blob of tir_pack_mlp_bwd
 * carries both images). */
int tir_mlp_bwd_bf16x3(const TirMlp* m, const float* packed_bwd, const float* feat, int32_t feat_stride,
                const float* out, const float* g_out, const float* h1, const float* h2, int64_t n,
                float* g_feat, float* dz1, float* dz2, float* dz3, void* stream);
/* tir_mlp_bwd_bf16x3 for up to four decoder invocations over the same n rows in one launch (the grid is split between
 * them; host arrays of n_jobs entries, arguments as in the single call). */
int tir_mlp_bwd_multi_bf16x3(const TirMlp* const* mlps, const float* const* packed_bwds, const float* const* feats,
                             int32_t feat_stride, const float* const* outs, const float* const* g_outs,
                             const float* const* h1s, const float* const* h2s, int32_t n_jobs, int64_t n,
                             float* const* g_feats, float* const* dz1s, float* const* dz2s, float* const* dz3s, void* stream);

/* C[M][ldc] += sum_j A_j^T B_j for up to three operand pairs over the same n rows, M <= 32, N <= 160: the gradient of
 * `basis_mat` (nn.Linear(144 -> 27, bias=False), models/tensoRF_rotated_lights.py:17) = g_feat^T y summed over the stage's
 * appearance gathers, in one launch.  A_j [n][lda] (first M columns), B_j [n][ldb] (first N columns).  Split-bf16 matrix
 * cores, fp32 accumulation; results are ADDED to C (atomics). */
int tir_gemm_tn_small_bf16x3(const float* const* As, int32_t lda, int32_t M, const float* const* Bs, int32_t ldb,
                             int32_t N, int32_t n_jobs, int64_t n, float* C, int32_t ldc, void* stream);

/* Weight gradients of up to four decoder invocations over the same n rows in ONE launch -- the `loss.backward()` leaves of
 * nn.Linear in MLPRender_Fea / MLPBRDF_PEandFeature (models/tensorBase_rotated_lights.py:122-146, :182-208;
 * train_tensoIR.py:315):   dW0 [128][150] += dz1^T x,  dW1 [128][128] += dz2^T h1,  dW2 [4][128] += dz3^T h2,
 * db0 [128] / db1 [128] / db2 [4] += the column sums of dz1 / dz2 / dz3.  dz1, dz2 [n][128], dz3 [n][4] from
 * tir_mlp_bwd*; h1, h2 [n][128] from the training forward; x is rebuilt in registers from feat [n][feat_stride] and
 * aux [.][3] (aux_maps[i] may be NULL: row s uses aux row s), so no input-row buffer exists.  Split-bf16 matrix cores,
 * fp32 accumulation; results are ADDED (atomics): zero-fill the outputs first.  Two jobs may share outputs (the BRDF
 * decoder's two invocations).  Host arrays of n_jobs entries.  max_workgroups (launch option, 0 = 256 = one per CU): a
 * workgroup occupies a whole CU, so a caller that runs this beside other kernels passes fewer. */
int tir_mlp_wgrad_multi(const float* const* dz1s, const float* const* dz2s, const float* const* dz3s,
                        const float* const* h1s, const float* const* h2s, const float* const* feats,
                        int32_t feat_stride, const float* const* auxs, const int32_t* const* aux_maps,
                        float* const* dW0s, float* const* db0s, float* const* dW1s, float* const* db1s,
                        float* const* dW2s, float* const* db2s, int32_t n_jobs, int64_t n, int32_t max_workgroups,
                        void* stream);

/* C[M][ldc] += A^T B (+ column N = A^T 1 when ones_col != 0: the bias gradient); A [n][lda] (first M columns),
 * B [n][ldb] (first N columns); M <= 128; N + ones_col <= 160 is one launch, a wider product runs as column blocks of
 * 128.  fp32 MFMA, split over n.  bias_out (may be NULL):
 * A^T 1 is added to bias_out[M] instead of column N of C, so that C can be the exact [M][N] weight gradient. */
int tir_gemm_tn(const float* A, int32_t lda, int32_t M, const float* B, int32_t ldb, int32_t N,
                int32_t ones_col, int64_t n, float* C, int32_t ldc, float* bias_out, void* stream);
/* Same product on the bf16 matrix pipe with every operand split x = hi + lo (3 products, fp32 accumulation:
 * ~2^-16 relative per product, the decoders' split-bf16 scheme). */
int tir_gemm_tn_bf16x3(const float* A, int32_t lda, int32_t M, const float* B, int32_t ldb, int32_t N,
                int32_t ones_col, int64_t n, float* C, int32_t ldc, float* bias_out, void* stream);

/* optimizer.step() of the training loop (train_tensoIR.py:317; torch.optim.Adam(grad_vars, betas=(0.9, 0.99)), :197) for a
 * list of tensors in one launch: torch's default Adam update (no amsgrad, no weight decay), element for element,
 *   m += (g - m)(1 - beta1);  v = v beta2 + (1 - beta2) g g;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).
 * Host arrays of n_tensors entries: device pointers p / g / m / v (dense storage in the same element order), element
 * counts, and per tensor lr, bias_correction1 = 1 - beta1^step, bias_correction2 = 1 - beta2^step. */
int tir_adam_step(int32_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                  const int64_t* count, const float* lr, const float* bias_correction1,
                  const float* bias_correction2, float beta1, float beta2, float eps, void* stream);

/* Backward of tir_shade_integrate w.r.t. the map rows (normal 4:7, albedo 7:10, roughness 10, fresnel 11:14)
 * and the environment radiance.  g_out [M][3] -> g_maps [M][20] (written), g_env [n_lights][D][3] (accumulated).
 * Visibility and indirect light are constants (compute_secondary_shading_effects is @torch.no_grad,
 * models/relight_utils.py:344). */
int tir_shade_integrate_bwd(const float* maps, const float* rays, const float* dirs,
                            const int32_t* light_idx, const float* vis, const float* indirect,
                            const float* env, const float* weight_d, int32_t M, int32_t D,
                            int32_t n_lights, int32_t equal_area, int32_t use_srgb, float acc_thres,
                            const float* g_out, float* g_maps, float* g_env, void* stream);

/* Backward of tir_env_sg_fwd: g_env [n_lights][D][3] -> g_sgs [n_sg][7] (accumulated). */
int tir_env_sg_bwd(const TirEnvSG* e, const float* dirs, int32_t D, const float* g_env, float* g_sgs,
                   void* stream);

/* ---- Mesh export: marching cubes on a dense lattice (scripts/export_mesh.py:15-24 -> utils.py:164-226,
 *      convert_sdf_samples_to_ply -> skimage.measure.marching_cubes; the lattice is tir_dense_alpha's output).
 *   vol [gx][gy][gz] fp32, contiguous, z fastest; array axis 0/1/2 = x/y/z.  gx, gy, gz >= 2.
 *   inside:    a lattice point is inside iff value > level (a value exactly at `level` is outside).
 *   vertices:  one per lattice edge that crosses the level (one end inside, the other not), owned by the edge's lower point p
 *              and axis; position origin + (idx(p) + t e_axis) * spacing per component, t = (level - v0) / (v1 - v0) along
 *              the edge, every fp32 operation rounded on its own (no contraction).
 *   normals:   -(central-difference gradient, one-sided on the lattice boundary, in index units) interpolated along the edge
 *              and normalised: they point toward decreasing values.
 *   faces:     int32 vertex triples from a sign-only case table (tensoir_amd/csrc/tir_mc_table.hpp, generated by
 *              tools/make_mc_table.py): ambiguous faces separate their inside corners, so the mesh is crack-free;
 *              every triangle's right-hand normal points from inside (high values) to outside.
 *   order:     vertices in (point linear index, axis x < y < z) order, faces in (cell linear index, table) order; no
 *              atomics, so two calls give bit-identical output.
 * Use: nb = tir_mc_blocks(g); tir_mc_count -> counts [2][nb] (vertices, faces per block of lattice points) and their
 * exclusive scans offsets [2][nb+1]; the caller reads the totals offsets[nb] and offsets[2*nb+1] back, allocates, then
 * tir_mc_emit writes verts [V][3], normals [V][3], faces [F][3] and the workspace vbase [gx*gy*gz] (int32, first vertex of
 * each point).  n_verts / n_faces are the totals (capacities of the outputs; nothing is written beyond them).
 * tir_mc_blocks returns nb, or TIR_ERR_ARG (a dimension < 2) / TIR_ERR_UNSUPPORTED (more than 2^31-1 lattice points, or a
 * lattice whose worst-case vertex or face total -- every edge crossing, every cell at the table's maximum -- overflows
 * int32); the two calls validate the same way, and null pointers, before any device work. */
int64_t tir_mc_blocks(int32_t gx, int32_t gy, int32_t gz);
int tir_mc_count(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, int32_t* counts, int32_t* offsets,
                 void* stream);
int tir_mc_emit(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, float spacing_x, float spacing_y,
                float spacing_z, float origin_x, float origin_y, float origin_z, const int32_t* offsets, int32_t n_verts,
                int32_t n_faces, int32_t* vbase, float* verts, float* normals, int32_t* faces, void* stream);

/* ---- Connected components of a dense lattice: removing detached blobs ("floaters") from the mesh and the occupancy mask.
 *   vol [gx][gy][gz] fp32, contiguous, z fastest (the tir_mc_* layout); every dimension >= 1; at most 2^31-1 points.
 *   inside:    vol[p] > level in fp32, the comparison of tir_mc_count (a value at `level`, or a NaN, is outside).
 *   links:     connectivity 6 joins inside points that differ by one step along one axis (the components whose boundaries are
 *              the closed surfaces of tir_mc_emit, whose case table separates inside corners on ambiguous faces);
 *              connectivity 26 also joins across edges and corners.
 *   labels [gx][gy][gz] int32: -1 where p is outside, otherwise the SMALLEST linear index ((x * gy + y) * gz + z) of any point
 *              of p's component.  The definition fixes the output whatever order the device worked in.
 *   table:     component k = 0 .. K-1 in ascending order of its root (the point with labels[p] == p):
 *              roots [K], sizes [K] (voxel count), boxes [K][6] = inclusive index bounds (x0, y0, z0, x1, y1, z1), all int32.
 *              Counts and bounds are integer atomics: exact, and bit-identical from call to call.  No float atomics anywhere.
 * Use: nb = tir_ccl_blocks(g) (blocks of 4096 points); tir_ccl_label writes labels and, as the caller's workspace, the number of
 * roots per block counts [nb] and its exclusive scan offsets [nb+1]; the caller reads K = offsets[nb] back, allocates roots /
 * sizes / boxes (the call initialises them) and runs tir_ccl_table(labels, g, offsets, K, ...).  K = 0: nothing is touched.
 * tir_ccl_filter: out[p] = vol[p] where p is outside or keep[component of p] != 0 (keep [K] bytes), else `fill`; fill <= level
 * is required, so a removed point is an outside point of `out` (out may not alias vol).  With K = 0, out = vol.
 * Labelling is a union-find whose links only ever point to smaller indices: inside 4 x 8 x 32 tiles in LDS, then across tile
 * borders with device-scope atomicMin, then a flattening pass; kernel boundaries are the only global synchronisation.
 * Every entry validates on the host before any device work: a null pointer, a connectivity other than 6 / 26, a dimension
 * <= 0, K < 0 or fill > level (or NaN) -> TIR_ERR_ARG; more than 2^31-1 points -> TIR_ERR_UNSUPPORTED (tir_ccl_blocks too). */
int64_t tir_ccl_blocks(int32_t gx, int32_t gy, int32_t gz);
int tir_ccl_label(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, int32_t connectivity, int32_t* labels,
                  int32_t* counts, int32_t* offsets, void* stream);
int tir_ccl_table(const int32_t* labels, int32_t gx, int32_t gy, int32_t gz, const int32_t* offsets, int32_t n_comp,
                  int32_t* roots, int32_t* sizes, int32_t* boxes, void* stream);
int tir_ccl_filter(const float* vol, const int32_t* labels, int32_t gx, int32_t gy, int32_t gz, float level,
                   const int32_t* roots, const uint8_t* keep, int32_t n_comp, float fill, float* out, void* stream);

/* ---- Mesh simplification by quadric vertex clustering (Rossignac-Borrel clusters, Lindstrom's quadric representative):
 *      a face budget for the exported mesh that keeps the full-resolution surface as its input.
 *   verts [V][3] fp32, faces [F][3] int32; cell[3] > 0, origin[3] (HOST floats), dims[3] >= 1 (HOST int32), reg >= 0.
 *   1. cell of a vertex: q = (v - origin) / cell, an fp32 subtract and an fp32 IEEE divide, each rounded on its own;
 *      i = clamp(floor(q), 0, dims - 1) per axis (a NaN goes to 0); key = (ix * dims_y + iy) * dims_z + iz.  Everything below
 *      takes the fp32 q as its input and works in cell units.
 *   2. output vertices = the occupied cells in ascending key order; cell_of_vertex [V] maps input to output vertices.
 *   3. per cell c, in its local frame u = q - (i_c + 0.5): from its vertices m = count, s = sum u; from every face corner whose
 *      vertex lies in c (once per corner), with n = (q1 - q0) x (q2 - q0), l = |n| (l = 0 faces skipped):
 *      A += n n^T / l,  b += n (n . (q0 - (i_c + 0.5))) / l,  N += n.
 *   4. mu = s / m, t = trace A; x = mu when t = 0, else the solution of (A + reg t I) x = b + reg t mu (mu as well when that
 *      solution is not finite: reg = 0 with a rank-deficient A); x is clamped to [-0.5, 0.5]^3.
 *      out_verts = origin + (i_c + 0.5 + x) * cell; out_normals = normalize(N / cell) -- the direction of the summed area
 *      normals in the coordinates of verts -- or (0, 0, 1) when N = 0.
 *   5. faces are remapped through cell_of_vertex; a face with two equal corners is dropped, the others keep their input order
 *      and winding.  Duplicates stay, so a closed oriented input keeps count(a -> b) = count(b -> a) for every directed edge.
 * Determinism: the sums of step 3 are 64-bit integer fixed point, added with integer atomics (order-independent); the per-face
 * terms and the 3 x 3 solve are fp64.  No float atomics: two calls give bit-identical outputs.  The fixed-point scales assume
 *   every face edge (q1 - q0, q2 - q0) and every vertex's u within TIR_SIMPLIFY_EXTENT cell edges per axis, F <= 2^28,
 * which bounds every sum below 2^63 whatever the mesh: s has 30 fraction bits in one word; A, N and b take two words each (the
 * value split at 2^-28, 2^-28 and 2^-24), 60, 60 and 56 fraction bits -- a cell that a sliver of the surface crosses has a tiny
 * trace, and its solution needs the terms to that relative precision.  The bounds are checked on the
 * device; status[2] collects TIR_SIMPLIFY_ERR_* bits and the caller must not use the outputs when it is non-zero.
 * Use: tir_simplify_count keys the vertices into the dense workspace slots [dims_x * dims_y * dims_z], scans it (blocks of 4096:
 * nbs = tir_simplify_blocks(slots), nbf = tir_simplify_blocks(F); counts [nbs + nbf], offsets [nbs + 1 + nbf + 1]), fills
 * cell_of_vertex, counts the surviving faces and writes status [4] = {V', F', error bits, 0}; the caller reads status back (one
 * 16-byte copy), allocates, and tir_simplify_emit accumulates into acc [V'][TIR_SIMPLIFY_ACC] (int64 workspace; keys [V'] int32
 * receives each output vertex's cell key), solves and compacts the faces.  V = 0 or F = 0 is valid.  No access leaves the
 * buffers for any input: cell indices are clamped, a face index outside [0, V) sets TIR_SIMPLIFY_ERR_FACE_INDEX and the face is
 * skipped everywhere.  Host validation before any device work: a null pointer, cell <= 0 (or NaN), dims < 1, reg < 0 (or NaN),
 * a negative count -> TIR_ERR_ARG; more than 2^31-1 slots or vertices, or F > 2^28 -> TIR_ERR_UNSUPPORTED. */
#define TIR_SIMPLIFY_EXTENT 4
#define TIR_SIMPLIFY_ACC 28
#define TIR_SIMPLIFY_ERR_FACE_INDEX  1   /* a face index outside [0, V)                                          */
#define TIR_SIMPLIFY_ERR_FACE_EXTENT 2   /* a face edge longer than TIR_SIMPLIFY_EXTENT cells along an axis (or NaN)  */
#define TIR_SIMPLIFY_ERR_VERTEX      4   /* a vertex more than TIR_SIMPLIFY_EXTENT - 0.5 cells outside the lattice (or NaN) */
int64_t tir_simplify_blocks(int64_t n);
int tir_simplify_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell,
                       const float* origin, const int32_t* dims, int32_t* slots, int32_t* cell_of_vertex, int32_t* counts,
                       int32_t* offsets, int32_t* status, void* stream);
int tir_simplify_emit(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell,
                      const float* origin, const int32_t* dims, double reg, const int32_t* cell_of_vertex,
                      const int32_t* offsets, int32_t n_out_verts, int32_t n_out_faces, int64_t* acc, int32_t* keys,
                      float* out_verts, float* out_normals, int32_t* out_faces, void* stream);

/* ---- Surface distance between meshes: area-weighted samples, a uniform grid over a mesh's faces, exact point-to-mesh distance
 *      (tensoir_amd/csrc/tir_distance.hip; ops.sample_surface / face_grid / point_mesh_distance, mesh.distance).
 *   verts [V][3] fp32, faces [F][3] int32, V < 2^31, F <= 2^TIR_DISTANCE_MAX_FACES_LOG2.  A face with an index outside [0, V) sets
 *   TIR_DISTANCE_ERR_FACE_INDEX in the status word of the entry that meets it, has no weight, is listed nowhere and is never
 *   followed.  Every fp64 operation named below is rounded on its own (nothing is contracted into an FMA).
 *
 * a. Samples.  weight of face f: w_f = sqrt(|n|^2), n = (v1 - v0) x (v2 - v0) from the corners converted to fp64, differences,
 *    products and the sum n_x^2 + n_y^2 + n_z^2 (added in that order) in fp64; a weight that is not finite counts as 0.
 *    w_max = the largest weight (an integer maximum over the bit patterns: exact).  Integer weight q_f = trunc((w_f / w_max) * 2^s)
 *    for w_f > 0, else 0, with s the largest integer <= 52 with F * 2^s <= 2^52: the total T = sum q_f stays below 2^53 and is the
 *    same whatever the order of the sums.  cdf[f] = q_0 + ... + q_f (int64, inclusive).
 *    Uniforms: hash(seed, i, ch), 64-bit wrapping arithmetic,
 *        x = seed + 0x9E3779B97F4A7C15 * (3 i + ch + 1);  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;
 *        x *= 0x94D049BB133111EB;  x ^= x >> 31;  u = x >> 40 (24 bits);  xi_ch = u * 2^-24 in [0, 1).
 *    Sample i of n is stratified: pos = ((i + xi_0) / n) * T in fp64 (add, divide, multiply), k = min(trunc(pos), T - 1); its face
 *    is the first f with cdf[f] > k (a face of integer weight 0 is never drawn).  Its point, in fp32 with xi_1, xi_2 as fp32:
 *        s = sqrt(xi_1), b0 = 1 - s, b1 = s * (1 - xi_2), b2 = s * xi_2;  point = (b0 v0 + b1 v1) + b2 v2.
 *    tir_mesh_sample_cdf fills cdf [F] (int64; sums [tir_distance_blocks(F)] int64 is workspace) and status [4] int64 = {T, error
 *    bits, faces of integer weight 0, the bits of w_max}.  tir_mesh_sample draws n samples from a cdf with T > 0 (with T = 0 every
 *    face is -1 and every point 0; the caller reads status first).  points [n][3] fp32, face [n] int32.
 *
 * b. Grid.  cell[3] > 0, origin[3] (HOST floats, finite), dims[3] in 1 .. TIR_DISTANCE_MAX_DIM (HOST int32).  The cell of a
 *    coordinate x along an axis is clamp(floor((x - origin) / cell), 0, dim - 1): an fp32 subtract and an fp32 IEEE divide, each
 *    rounded on its own.  The first and the last cell of an axis therefore reach to infinity; the function is monotone in x.
 *    A face is listed in every cell from the cell of its bounding box's low corner to that of its high corner.  A face with a
 *    non-finite corner, or with |n|^2 == 0 (a. above), is degenerate: listed nowhere, counted.
 *    tir_face_grid_count writes status [4] int64 = {pairs (faces x cells they are listed in), error bits, degenerate faces, listed
 *    faces} without visiting a cell.  The caller reads it back, REFUSES a total above its budget (nothing is ever truncated) and
 *    calls tir_face_grid_fill with n_pairs = that total: cursor [cells] int32 (cells = dims_x dims_y dims_z, key =
 *    (ix * dims_y + iy) * dims_z + iz), counts [tir_distance_blocks(cells)], offsets [that + 1] int32 workspace, pairs [n_pairs]
 *    int32.  Per-cell counts by integer atomics, block sums, tir_exclusive_scan, first slots, fill.  Afterwards cell key lists
 *    pairs[cursor[key - 1] .. cursor[key]) (from 0 for key 0), in an order that may differ from run to run.
 *
 * c. Distance.  tir_point_mesh_distance: points [n][3] fp32 -> dist [n] fp32 = the Euclidean distance to the nearest point of any
 *    listed face, face [n] int32 = that face, closest [n][3] fp32 = that point (NULL skips it), tested [n] int32 = point-triangle
 *    tests made (NULL skips it).  Per face, in fp64 on coordinates relative to corner a (ab = b - a, ac = c - a, ap = p - a), the
 *    seven regions of the closest point a + v ab + w ac:
 *        d1 = ab.ap, d2 = ac.ap, bp = ap - ab, d3 = ab.bp, d4 = ac.bp, cp = ap - ac, d5 = ab.cp, d6 = ac.cp,
 *        vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4; the first that holds of
 *        d1 <= 0 and d2 <= 0: (0, 0) | d3 >= 0 and d4 <= d3: (1, 0) | vc <= 0, d1 >= 0, d3 <= 0: (d1 / (d1 - d3), 0) |
 *        d6 >= 0 and d5 <= d6: (0, 1) | vb <= 0, d2 >= 0, d6 <= 0: (0, d2 / (d2 - d6)) |
 *        va <= 0, d4 - d3 >= 0, d5 - d6 >= 0: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w | else (vb, vc) / (va + vb + vc);
 *        D = |ap - (v ab + w ac)|^2.  dist = fp32(sqrt(min D)); among faces of equal D the smaller index wins.
 *    Search: from the cell of the point (clamped into the grid) over shells of growing Chebyshev radius r.  After shell r, every
 *    unvisited cell lies beyond one of the planes origin + (c - r) cell (if c - r > 0) or origin + (c + r + 1) cell (if c + r + 1 <
 *    dim) of some axis; b = the smallest distance of the point ITSELF (not of its clamped cell) to those planes, each reduced by
 *    TIR_DISTANCE_SLACK * cell, which exceeds the rounding of the cell function (two fp32 roundings on an index <= 2^8: 2^-14 of
 *    a cell).  The search stops only when b > 0 and b^2 > min D, and inside a shell a cell is skipped only when the squared
 *    distance of the point to the cell's box, widened by the same slack per axis, exceeds min D; so no face that could be as
 *    near, or tie, is left out: the
 *    outputs are bit-identical for every grid over the same faces, for every fill order, and for points far outside the grid.
 *    No listed face: dist = +inf, face = -1, closest = NaN.  A non-finite point: dist = NaN, face = -1, closest = NaN.
 *
 * Every entry validates on the host before any device work: a null pointer, a negative count, cell <= 0 (or not finite), a
 * non-finite origin, dims < 1 -> TIR_ERR_ARG; dims > TIR_DISTANCE_MAX_DIM, V or n or n_pairs > 2^31-1, F > 2^28 ->
 * TIR_ERR_UNSUPPORTED.  n = 0, F = 0 for the cdf and the count, n_pairs = 0 for the fill return TIR_OK before any device work:
 * the caller hands those three a zeroed status / cursor, which then stays as it is.  No access leaves the buffers for any
 * input: slots and list bounds are clamped to n_pairs, listed faces and their indices are checked again by the query. */
#define TIR_DISTANCE_MAX_FACES_LOG2 28
#define TIR_DISTANCE_MAX_DIM 256
#define TIR_DISTANCE_SLACK (1.0 / 8192.0)
#define TIR_DISTANCE_ERR_FACE_INDEX 1    /* a face index outside [0, V)                                          */
int64_t tir_distance_blocks(int64_t n);
int tir_mesh_sample_cdf(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int64_t* cdf, int64_t* sums,
                        int64_t* status, void* stream);
int tir_mesh_sample(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int64_t* cdf, int64_t n,
                    uint64_t seed, float* points, int32_t* face, void* stream);
int tir_face_grid_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell,
                        const float* origin, const int32_t* dims, int64_t* status, void* stream);
int tir_face_grid_fill(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell,
                       const float* origin, const int32_t* dims, int64_t n_pairs, int32_t* cursor, int32_t* counts,
                       int32_t* offsets, int32_t* pairs, void* stream);
int tir_point_mesh_distance(const float* points, int64_t n, const float* verts, int64_t n_verts, const int32_t* faces,
                            int64_t n_faces, const float* cell, const float* origin, const int32_t* dims, const int32_t* cursor,
                            const int32_t* pairs, int64_t n_pairs, float* dist, int32_t* face, float* closest, int32_t* tested,
                            void* stream);

/* ---- Ray cast against a mesh over the same grid (tensoir_amd/csrc/tir_distance.hip; ops.ray_mesh / mesh_inside, mesh.raycast,
 *      mesh.distance(signed=True)).  The mesh and grid arguments are those of tir_point_mesh_distance.
 *   origins [n][3], dirs [n][3] fp32 (a direction need not be unit: t is in units of |d|), trange [n][2] fp32 = {t0, t1} per ray
 *   (NULL: [0, +inf]; negative values reach behind the origin), bounds [6] fp32 ON THE DEVICE = {low xyz, high xyz} of a box that
 *   contains every listed face (ops.face_grid's "bounds": the box of the finite vertices, padded by 2^-16 max(max |coordinate|,
 *   largest extent)).
 *   t [n] fp32 = the parameter of the nearest accepted hit (+inf on a miss), face [n] int32 = its face (-1 on a miss),
 *   bary [n][2] fp32 = the weights of corners b and c at that hit (NaN on a miss; NULL skips), count [n] int32 (NULL skips),
 *   flags [n] int32 (NULL skips), tested [n] int32 = ray-triangle tests made (NULL skips; the one output that depends on the grid).
 *
 * Ray-triangle rule.  Everything in fp64 from the fp32 inputs, one rounding per operation, nothing contracted.  With A = a - o,
 *   B = b - o, C = c - o and
 *       e(P, Q) = (dx (Py Qz - Pz Qy) + dy (Pz Qx - Px Qz)) + dz (Px Qy - Py Qx),     u = e(B, C), v = e(C, A), w = e(A, B):
 *   the LINE meets the face iff u, v, w are all >= 0 or all <= 0, and not all zero.  n = (b - a) x (c - a), den = (dx nx + dy ny)
 *   + dz nz; den == 0 is a miss.  t = ((Ax nx + Ay ny) + Az nz) / den (IEEE division); the hit is ACCEPTED iff t0 <= t <= t1.
 *   bary = (v, w) / ((u + v) + w).  Nearest: the smaller fp64 t, an equal t goes to the smaller face index.  e(Q, P) == -e(P, Q)
 *   bit for bit, so the two faces of a shared edge see a ray on opposite sides of it: on a closed, consistently oriented mesh a
 *   ray with no zero edge value crosses the surface watertight, and the parity of its hits tells inside from outside.
 *   Only the faces a grid lists are met (4.15 b: a face without area or with a non-finite corner is listed nowhere).
 *
 * Modes and what they report.
 *   TIR_RAY_CLOSEST  t, face, bary of the nearest hit; count = 1 on a hit, 0 on a miss; flag bit 0 = THAT hit has an edge value
 *                    equal to zero.  The walk may stop early.
 *   TIR_RAY_COUNT    t, face, bary as above; count = the exact number of accepted hits; flag bit 0 = SOME accepted hit has an edge
 *                    value equal to zero (the ray passes exactly through an edge or a vertex, which count may then have counted
 *                    twice, or not at all).  No early stop.
 *   TIR_RAY_ANY      count = 0 or 1 only, flags reports bit 1 only; t, face and bary must be NULL (which face is met first depends
 *                    on the grid).  Stops at the first accepted hit.
 *   Flag bit 1, TIR_RAY_FLAG_INVALID: a non-finite origin or direction, d == 0, a NaN in trange or t0 > t1.  Then t = NaN,
 *   face = -1, bary = NaN, count = 0, tested = 0.
 *
 * Traversal (conservative; every loop runs on an integer counter whose bound is known before it starts, so no NaN, infinity or
 *   zero direction component keeps a lane running).  Per axis the slack is s = TIR_DISTANCE_SLACK * cell + TIR_RAY_COORD_SLACK *
 *   max |bounds| of that axis: the first term covers the rounding of the cell function (4.15 c), the second the rounding of a
 *   hit point to fp32 (2^-24 of a coordinate) sixteen times over.
 *   1. [T0, T1] = [t0, t1] clipped to `bounds` (fp64 slab test; an axis with d == 0 and the origin outside its slab: a miss).
 *      Clipping removes no hit, because no listed face leaves the box.
 *   2. The major axis m is the one of the largest |d| (the lower axis wins a tie).  Its slabs of cells are walked in the travel
 *      direction from cell(x_in -/+ s_m) to cell(x_out +/- s_m), x_in / x_out the major coordinates at T0 / T1.
 *   3. Slab k covers the coordinates [origin + k cell - s_m, origin + (k + 1) cell + s_m], open-ended for the first and the last
 *      cell of the axis; its t interval is that of those two planes, cut to [T0 - w, T1 + w], w = max_axis s / |d_m|.
 *   4. The two other coordinates are evaluated at both ends of the interval; the rectangle of cells from cell(min - s) to
 *      cell(max + s) per axis is visited, every face listed in a cell is tested (listed faces and their indices are checked again).
 *      Slabs differ in their major index: no cell is visited twice.
 *   5. TIR_RAY_CLOSEST stops before a slab only when the best t lies STRICTLY below that slab's widened entry.
 *   Counting each hit once (TIR_RAY_COUNT): a face is listed in several cells; its hit counts only in the cell of the hit point,
 *   cell(fp32(o + t d)) per axis (fp64 multiply and add, then rounded), clamped per axis into the cells the face is listed in.
 *   The widening guarantees that this cell is visited, so t, face, bary, count and flags are bit-identical for every grid over the
 *   same faces (1 x 1 x 1, the brute-force path, included), for every fill order and on every run -- for origins whose distance
 *   from the mesh is within fp64's reach of the slack (2^30 extents, say) and hits that are not seen at a grazing angle below 2^-30.
 *
 * ops.mesh_inside casts TIR_RAY_COUNT rays along three fixed directions (fp32, below) over [0, +inf]; a vote is an odd count.
 *
 * Host validation before any device work: a null pointer with n > 0, a negative count, an unknown mode, t / face missing in
 * TIR_RAY_CLOSEST / TIR_RAY_COUNT, count missing or t / face / bary given in TIR_RAY_ANY, the grid conditions above ->
 * TIR_ERR_ARG; n or n_pairs > 2^31-1 -> TIR_ERR_UNSUPPORTED; n == 0 -> TIR_OK.  The entry takes a stream and allocates nothing. */
#define TIR_RAY_CLOSEST 0
#define TIR_RAY_COUNT 1
#define TIR_RAY_ANY 2
#define TIR_RAY_FLAG_GRAZED 1
#define TIR_RAY_FLAG_INVALID 2
#define TIR_RAY_COORD_SLACK (1.0 / 1048576.0)
#define TIR_RAY_INSIDE_DIRECTIONS {{0.5345225f, 0.2672612f, 0.8017837f}, {-0.6882472f, 0.6246950f, -0.3692745f}, \
                                   {0.1825742f, -0.9128709f, -0.3651484f}}
int tir_ray_mesh(const float* origins, const float* dirs, const float* trange, int64_t n, const float* verts, int64_t n_verts,
                 const int32_t* faces, int64_t n_faces, const float* cell, const float* origin, const int32_t* dims,
                 const int32_t* cursor, const int32_t* pairs, int64_t n_pairs, const float* bounds, int mode, float* t,
                 int32_t* face, float* bary, int32_t* count, int32_t* flags, int32_t* tested, void* stream);

/* ---- Traced shadows of the light cells: one any-hit ray per (surface point, light cell) pair over the same grid
 *      (tensoir_amd/csrc/tir_distance.hip; ops.shadow_trace, raster.relight_mesh(shadows="traced"); restated in numpy
 *      by tests/shadowtrace_reference.py).  No maps, no bias in texels, no memory that grows with D S^2.
 *   pts, nrm [M][3] fp32: the surface point and the stored, unflipped normal of each row; cells [D][8]: tir_env_cells' records;
 *   the mesh and grid arguments are those of tir_ray_mesh; t0 fp32 >= 0: where the ray starts to count, in units of |L|.
 *   occl [D][ceil(M / 64)] uint64: bit m & 63 of word [d][m >> 6] is 1 iff pair (m, d) is OCCLUDED.  Every word is written (no
 *   clear is needed); the bits of rows beyond M are 0.
 *   The rule for pair (m, d), L = cells[d].dir as stored (not renormalised):
 *     it contributes iff c = n.L > 1e-6, c formed as tir_light_gbuffer and tir_shadow_lookup form it (sums of products may be
 *     fused); a contributing pair is occluded iff the ray with origin pts[m], direction L and range [t0, +inf] has an accepted hit
 *     under tir_ray_mesh's rule in TIR_RAY_ANY mode (the fp64 ray-triangle rule, the conservative walk: the same device function).
 *     A pair that does not contribute and an invalid ray (a non-finite point, a non-finite or zero L) give bit 0.
 *   The bits are identical for every grid over the same faces, for every fill order and on every run.
 *   One wave covers 64 consecutive rows and walks the cells in chunks of 16; a wave's 64 answers for a cell are one ballot.
 * Host validation before any device work: a negative count, D < 1, a t0 that is negative or not finite, the grid conditions of
 *   tir_ray_mesh, and with M > 0 a null pointer, cells not 16-byte or occl not 8-byte aligned -> TIR_ERR_ARG; D > 2^20, M or
 *   n_pairs > 2^31-1 -> TIR_ERR_UNSUPPORTED; M == 0 -> TIR_OK, nothing done.  The entry takes a stream and allocates nothing. */
int tir_shadow_trace(const float* pts, const float* nrm, const float* cells, int64_t M, int32_t D, const float* verts,
                     int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell, const float* origin, const int32_t* dims,
                     const int32_t* cursor, const int32_t* pairs, int64_t n_pairs, const float* bounds, float t0, uint64_t* occl,
                     void* stream);

/* ---- per-point bake of materials and direct lighting (tensoir_amd/bake.py).  Point p is marched inward from
 * origins[p] along dirs[p] by tir_march_secondary_fwd with records; the caller decodes every record (BRDF decoder output
 * rec_brdf [A][4] = albedo rgb + raw roughness, shading normal rec_normal [A][3]).
 *
 * tir_bake_composite reduces point p's record segment ray_rec_off[p] .. + ray_rec_cnt[p] (contiguous, in sample order; the
 * segments themselves in any order; entries reaching beyond n_rec -- the number of record rows that exist -- are clipped):
 *   acc = sum w,  A = sum w albedo,  R = sum w (0.9 raw + 0.09),  Nv = sum w normal,  depth = sum w z
 * with z = dot(world(rec_xyz) - origin, dir): the march records a sample's normalised position, world = aabb_min +
 * (rec_xyz + 1) (aabb_max - aabb_min) / 2.  aabb: SIX HOST floats {min xyz, max xyz}.  Output rows [n_points][TIR_BAKE_ROW]:
 *   [0..2] clamp(A / max(acc, 1e-6), 0, 1)   [3] clamp(R / max(acc, 1e-6), 0, 1)
 *   [4..6] Nv / max(|Nv|, 1e-6), or fallback_normal[p] when acc <= 0.5 or |Nv| <= 1e-6     [7] min(acc, 1) (coverage)
 *   [8..10] origin + dir * depth / max(acc, 1e-6) (surface)   [11] depth   [12..15] 0
 * No white background is mixed in.  A group of 8 lanes walks a segment and combines by shuffles in a fixed order: no atomics,
 * two calls give bit-identical rows.  rows and rec_brdf must be 16-byte aligned (16-byte vector accesses). */
#define TIR_BAKE_ROW 16
int tir_bake_composite(const int32_t* ray_rec_off, const int32_t* ray_rec_cnt, const float* rec_w, const float* rec_xyz,
                       const float* rec_brdf, const float* rec_normal, const float* origins, const float* dirs,
                       const float* fallback_normal, const float* aabb, int64_t n_points, int64_t n_rec, float* rows,
                       void* stream);

/* Direct light and ambient occlusion of baked points: rows [M][TIR_BAKE_ROW] of tir_bake_composite (normal, coverage are read),
 * dirs [D][3] unit light directions, vis [M][D] transmittance toward them (0 where the pair was not marched), env
 * [n_lights][D][3] radiance, weight_d [D] solid angles, light_idx [M] (clamped to the table).  With cos = dot(dirs[d], normal),
 * each product and sum rounded on its own (the caller's pair mask forms it the same way), over the d with cos > 1e-6:
 *   out[m] = { sum vis cos w / sum cos w  (1 when that denominator is 0),  sum vis env[light_idx[m]][d][c] cos w  (c = r, g, b) }
 * and {1, 0, 0, 0} for points with coverage <= 0.5.  One wave64 per point walks its vis row (16-byte loads when D % 4 == 0 and
 * vis is 16-byte aligned) and reduces by shuffles in a fixed order: no atomics, bit-reproducible.  Any D > 0; M = 0 is a no-op.
 * rows and out [M][4] must be 16-byte aligned. */
int tir_irradiance_integrate(const float* rows, const float* dirs, const float* vis, const float* env, const float* weight_d,
                             const int32_t* light_idx, int64_t M, int32_t D, int32_t n_lights, float* out, void* stream);

/* ---- Per-triangle texture atlas of a mesh (tensoir_amd/mesh.py, bake_atlas / export_textured).
 *   verts [V][3], normals [V][3] fp32, faces [F][3] int32; a size x size image (6 .. 8192) of cols x cols square cells of
 *   T x T texels (T >= 6).  No chart solver: faces 2c and 2c+1 share cell c, whose texel origin is ((c % cols) T, (c / cols) T).
 *   Texel (i, j) of a cell has centre (i + 0.5, j + 0.5); j counts image rows from the top and uv = texel / size (glTF's).
 *   1. ownership: the lower face 2c owns i + j <= T - 1, the upper face 2c+1 owns i + j >= T; when F is odd, face F-1 owns all
 *      of the last cell.  Texels outside the ceil(F / 2) used cells are unowned.
 *   2. UV corners (cell-local, corner order 0, 1, 2): lower (1, 1), (T-3, 1), (1, T-3); upper (T-1, T-1), (3, T-1), (T-1, 3),
 *      the lower triangle turned by 180 degrees about the cell centre.  A bilinear lookup anywhere inside a face's UV triangle
 *      reads only texels that face owns.  uv = (cell origin + corner) / size: ONE fp32 IEEE division of two integers.
 *   3. a texel's barycentrics: the texel centre is moved to the nearest point of the owner's UV triangle (exactly, in integer
 *      quarter texels; gutter texels thus repeat the edge), and with (qx, qy) that point relative to corner 0 along the two
 *      legs of length L = T - 4:  b1 = qx / L, b2 = qy / L, b0 = (L - qx - qy) / L, each one fp32 IEEE division of exact numbers.
 *   4. point = sum b_k v_k; outward = normalize(sum b_k n_k), the face normal normalize((v1 - v0) x (v2 - v0)) when that sum is
 *      shorter than 1e-20, and (0, 0, 1) when the face normal is too.
 *   5. tangent of a frame with unit normal n: t = normalize(e_u - n (n . e_u)), e_u = v1 - v0 for a lower and v0 - v1 for an
 *      upper face (the world direction of +u); when that vector is shorter than 1e-20, the same expression with the coordinate
 *      axis of n's smallest |component| (the first of equals) in place of e_u.  b = cross(n, t); w = +1 always.
 * tir_atlas_corners: the unwelded mesh.  Corner q = 3 f + k: pos / nrm [3F][3] = bit copies of verts / normals [faces[f][k]],
 *   uv [3F][2] (step 2), tan [3F][4] = (t, 1) of step 5 with n = the corner's normal normalised as in step 4 (b = unit vector k),
 *   both steps evaluated in double and rounded once (a vertex normal nearly along the edge makes step 5 cancel).
 * tir_atlas_texels: for the n_cells T T texels in cell-major order (c T T + j T + i): point [N][3], outward [N][3] (step 4),
 *   face [N] = the owner.  One thread per texel; 16-byte stores when point and outward are 16-byte aligned.
 * tir_atlas_pack: the three size x size RGBA8 images, in image order (row-major from the top), from the per-texel results of
 *   the bake in the cell-major order above: albedo [N][3], irradiance [N][3] or NULL, roughness [N], ao [N] or NULL, normal
 *   [N][3] (unit, in the coordinates of verts' frame), coverage [N].  With u8(x) = round(255 clamp(x, 0, 1)), half to even:
 *     base   = u8(srgb(c)), 255;  c = albedo, or clamp(albedo / pi * irradiance, 0, 1) when irradiance is given;
 *              srgb(x) = x <= 0.0031308 ? 12.92 x : 1.055 (x + 1e-6)^(1 / 2.4) - 0.055
 *     orm    = u8(ao) (255 when ao is NULL), u8(roughness), 0, 255
 *     normal = u8(0.5 + 0.5 (N . t, N . b, N . n)), 255 with the frame (t, b, n) of steps 4-5 at the texel, recomputed from the
 *              mesh; (128, 128, 255, 255) where coverage <= 0.5 (the bake returns `outward` there)
 *   unowned texels: (0, 0, 0, 255) in base and orm, (128, 128, 255, 255) in normal.
 * No atomics; two calls give identical bits.  No access leaves a buffer: a face with an index outside [0, V) is read nowhere,
 * its outputs are 0 (outward (0, 0, 1), texels as unowned) and *status, which every entry clears first, is set to 1; the caller
 * must not use the outputs then.  Host validation before any device work: a null pointer (irradiance and ao excepted; data
 * pointers may be null when F = 0), a negative count, size < 6, cols < 1, cols T > size, or more rows of cells than fit
 * -> TIR_ERR_ARG; T < 6, size > 8192 or V > 2^31-1 -> TIR_ERR_UNSUPPORTED; tan must be 16-byte, the images 4-byte aligned.
 * F = 0 returns TIR_OK and launches nothing (the images are then the caller's to fill). */
int tir_atlas_corners(const float* verts, int64_t n_verts, const float* normals, const int32_t* faces, int64_t n_faces,
                      int32_t size, int32_t cols, int32_t T, float* pos, float* nrm, float* tan, float* uv, int32_t* status,
                      void* stream);
int tir_atlas_texels(const float* verts, int64_t n_verts, const float* normals, const int32_t* faces, int64_t n_faces,
                     int32_t size, int32_t cols, int32_t T, float* point, float* outward, int32_t* face, int32_t* status,
                     void* stream);
int tir_atlas_pack(const float* verts, int64_t n_verts, const float* normals, const int32_t* faces, int64_t n_faces,
                   int32_t size, int32_t cols, int32_t T, const float* albedo, const float* irradiance, const float* roughness,
                   const float* ao, const float* normal, const float* coverage, uint8_t* base, uint8_t* orm,
                   uint8_t* normal_image, int32_t* status, void* stream);

/* ---- Deterministic z-buffer rasteriser of the exported mesh (tensoir_amd/raster.py; restated in numpy by
 * tests/raster_reference.py).
 *   Camera (the datasets' get_ray_directions + get_rays): pixel (i, j) has its centre at (i + 0.5, j + 0.5) and the camera-space
 *   direction ((i + 0.5 - W/2) / f, (j + 0.5 - H/2) / f, 1); c2w = [R | o] is [3][4], row-major, in HOST memory, its columns x
 *   right, y down, z forward.  p_cam = R^T (p - o);  x_px = f X / Z + W/2,  y_px = f Y / Z + H/2.
 *   Mesh: unwelded, corner q = 3 f + k, as write_glb writes it.
 * tir_raster_project: one thread per corner -> rows [3F][4] int32 = {sx, sy, bits(invz), flags}.  With every product, sum and
 *   quotient rounded to fp32 on its own, in this order:  d = p - o;  X = (R[0][0] d0 + R[1][0] d1) + R[2][0] d2 (Y, Z: columns 1,
 *   2);  x_px = (f X) / Z + W/2;  sx = rint(256 x_px), half to even (8 sub-pixel bits);  invz = 1 / Z.
 *   faces NULL: corner q reads pos[q] (n_verts >= 3 F).  faces [F][3] given: corner q reads pos[faces[q]] (an indexed mesh).
 *   A face is dropped when any of its corners has, tested in this order per corner: a vertex index outside [0, V) (the three
 *   indices are tested before any vertex is read, and no vertex of such a face is read); X, Y or Z not finite; Z <= near;
 *   |sx| or |sy| > TIR_RASTER_GUARD * 256 (an infinite x_px included).  There is no clipping.  All three rows of a dropped face are
 *   {0, 0, 0, flags} with flags the OR of its corners' TIR_RASTER_DROP_* bits; a kept face has flags 0.  status [4], cleared
 *   first, counts the dropped faces {index, near, guard, non-finite}, each face once under the first of index, non-finite, near,
 *   guard that any of its corners shows.
 * tir_raster_cover: keys [H W] uint64, cleared to 0 (= empty) by the entry.  All integer, int64, from the snapped corners
 *   (x_k, y_k):  A = (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0).  A == 0 draws nothing; cull != 0 draws only A < 0 (front-facing for
 *   an outward-oriented mesh in this camera); cull == 0 draws both signs.  With n = sign(A), the centre p = (256 i + 128,
 *   256 j + 128) of pixel (i, j) and cross(a, b) = a.x b.y - b.x a.y:
 *     E0 = n cross(v1 - p, v2 - p),  E1 = n cross(v2 - p, v0 - p),  E2 = n cross(v0 - p, v1 - p)      (E0 + E1 + E2 = |A|)
 *   Edge k runs from v_a to v_b (edge 0: v1 -> v2, 1: v2 -> v0, 2: v0 -> v1) with d = n (v_b - v_a); it OWNS its zero set when
 *   d.y < 0 (a left edge: the interior lies at larger x) or d.y == 0 and d.x > 0 (a top edge: the interior lies at larger y).
 *   The centre is inside when, for every k, E_k > 0, or E_k == 0 and edge k owns its zero set.  Two faces sharing an edge see
 *   opposite d, so exactly one of them owns a centre on it.
 *   Fragment depth, each step rounded on its own, E_k and |A| converted to fp32 (nearest even) first:
 *     invz = ((E0 w0 + E1 w1) + E2 w2) / |A|,  w_k = the corners' invz;   key = (bits(invz) << 32) | (0xFFFFFFFF - face)
 *   written by one 64-bit unsigned atomic max: the nearest fragment wins, the lower face index on equal depth, in any arrival
 *   order.  work: [F + 1] int32 the entry owns during the call (the list of faces whose box of pixel centres holds more than 64
 *   pixels; a second launch gives each a workgroup).
 * tir_raster_resolve: one thread per pixel -> out [H W][4] = {int32 face (-1 = empty), b1, b2, zc}: with t_k = E_k w_k and
 *   s = (t0 + t1) + t2 as above, b1 = t1 / s, b2 = t2 / s (perspective-correct), zc = 1 / invz of the key.
 * tir_raster_shade: one thread per pixel, what a glTF viewer does with the file -> out [H W][TIR_RASTER_ROW] fp32 =
 *   {albedo r g b, roughness, ao, normal x y z, coverage (1 or 0), 0, 0, 0}; an empty pixel is all zeros.  b0 = (1 - b1) - b2.
 *   uv = sum b_k uv_k; a bilinear lookup (LINEAR, CLAMP_TO_EDGE, sample position uv * size - 0.5, no mip-maps) in the three
 *   size x size RGBA8 images; the base colour is decoded per tap, before filtering, by the inverse of tir_atlas_pack's encoding,
 *   s <= 0.04045 ? s / 12.92 : max(((s + 0.055) / 1.055)^2.4 - 1e-6, 0), unless raw != 0; roughness = G and ao = R of orm;
 *   normal = normalize(tx t + ty b + tz n), (tx, ty, tz) = 2 c - 1 of the normal image, n = normalize(sum b_k nrm_k),
 *   t = normalize(sum b_k tan_k.xyz), b = cross(n, t) * tan.w of corner 0.  base, orm and normal all NULL (tan, uv unused): a
 *   geometry-only render, albedo / roughness / ao 0 and normal = n.
 * All entries validate on the host before any device work: a null pointer (data pointers may be null when F = 0), a negative
 *   count, W or H < 1, focal <= 0 or NaN, near < 0 or NaN, a misaligned buffer (rows, pix, out: 16 bytes; keys: 8; images: 4)
 *   -> TIR_ERR_ARG; W, H or size > TIR_RASTER_MAX_SIDE, F > TIR_RASTER_MAX_FACES -> TIR_ERR_UNSUPPORTED.  F = 0 gives an empty
 *   image.  They allocate nothing, and two calls give identical bits. */
#define TIR_RASTER_GUARD 16384              /* pixels: a corner snapped further from the origin drops its face */
#define TIR_RASTER_MAX_SIDE 8192
#define TIR_RASTER_MAX_FACES 715827882      /* (2^31 - 1) / 3 */
#define TIR_RASTER_ROW 12
#define TIR_RASTER_DROP_NEAR      1
#define TIR_RASTER_DROP_GUARD     2
#define TIR_RASTER_DROP_NONFINITE 4
#define TIR_RASTER_DROP_INDEX     8
int tir_raster_project(const float* pos, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* c2w, float focal,
                       int32_t W, int32_t H, float near_z, int32_t* rows, int32_t* status, void* stream);
int tir_raster_cover(const int32_t* rows, int64_t n_faces, int32_t W, int32_t H, int32_t cull, uint64_t* keys, int32_t* work,
                     void* stream);
int tir_raster_resolve(const int32_t* rows, int64_t n_faces, const uint64_t* keys, int32_t W, int32_t H, int32_t* out,
                       void* stream);
int tir_raster_shade(const int32_t* pix, int64_t n_faces, const float* nrm, const float* tan, const float* uv, const uint8_t* base,
                     const uint8_t* orm, const uint8_t* normal, int32_t size, int32_t raw, int32_t W, int32_t H, float* out,
                     void* stream);

/* ---- Lighting of the exported asset: environment -> light cells, deferred GGX lighting of a G-buffer (tensoir_amd/raster.py
 * relight_mesh / relight_glb / compare_asset(light=); restated in numpy by tests/light_reference.py).
 * tir_env_cells: an equirectangular map hdr [H][W][3] (row 0 at the top, as Environment_Light reads it) -> cells [h w][8] fp32 =
 *   {dir.x, dir.y, dir.z, Omega, r, g, b, 0}: the 32-byte record of tir_relight_importance_cells_packed with the cell's solid
 *   angle in the pdf slot.  H = a h and W = b w with integers a, b >= 1.  row_w [H] (device) is the exact solid angle of one
 *   texel of row i, Omega_i = (2 pi / W) * 2 sin(pi (i + 0.5) / H) * sin(pi / (2 H)), computed by the caller in float64 and
 *   rounded once (ops.env_row_weights; sum_i W Omega_i = 4 pi.  The 0.5 / H end points of the reference's sin_theta table are
 *   not copied: these weights belong to no reference function).  Cell (r, c) covers the texel rows [a r, a r + a) and columns
 *   [b c, b c + b):  Omega = b * sum_i row_w[i];  rgb = sum_i sum_j row_w[i] hdr[i][j] / sum_i sum_j row_w[i], numerator (fused
 *   multiply-adds) and denominator accumulated in fp32 in row-major order, one thread per cell;  dir = (cos t cos p, sin t cos p,
 *   sin p) with p = pi / 2 - (r + 0.5) pi / h and t = pi - (c + 0.5) 2 pi / w, the centre of the cell on the h x w grid by
 *   Environment_Light's formula (the angles are formed in double and rounded to fp32 once).
 *   H, W, h or w < 1, H % h or W % w != 0, a null pointer, cells not 16-byte aligned -> TIR_ERR_ARG; H W > 2^28 ->
 *   TIR_ERR_UNSUPPORTED.
 * tir_light_gbuffer: gbuf [M][TIR_RASTER_ROW] is what tir_raster_shade writes {albedo r g b, roughness, ao, normal x y z,
 *   coverage, 0, 0, 0}; view [M][3] the vector from the surface to the eye (any length); cells [D][8] as above; out [M][4] =
 *   {r, g, b, coverage}.  A row whose coverage is not > 0 gives four zeros and reads no light.  A covered row, with the surface
 *   terms of GGX_specular (models/relight_utils.py:22-49; the same formula as tir_ggx_specular) for a scalar roughness rho and a
 *   scalar fresnel F:
 *     V = view / max(|view|, 1e-12);  N = n / max(|n|, 1e-12) * sign(N.V) (n = the stored normal);  NoV = clamp(N.V, 1e-6, 1);
 *     alpha2 = rho^4;  k = (rho^2 + 2 rho + 1) / 8;  alb_pi = albedo / pi
 *   and for each cell d in ascending order, L = cells[d].dir as stored (not renormalised):
 *     c = n.L with the stored, unflipped normal (models/relight_utils.py:433-435); the pair contributes iff c > 1e-6, with
 *     Hv = (L + V) / 2;  Hv = Hv * rsq(max(|Hv|^2, 1e-24));  NoL, NoH, VoH = clamp(N.L, N.Hv, V.Hv to [1e-6, 1]);
 *     spec = (F + (1 - F) 2^((-5.55473 VoH - 6.98316) VoH)) alpha2
 *            / clamp(4 pi (NoH^2 (alpha2 - 1) + 1)^2 (NoV (1 - k) + k) (NoL (1 - k) + k), 1e-6, 4 pi)
 *     sum_q += (((alb_pi_q + spec) * rgb_d,q) * c) * Omega_d                               (q = r, g, b; products in this order)
 *   rsq, 2^x and the reciprocal of the denominator are the one-ulp hardware instructions; sums of products may be fused.
 *   TIR_LIGHT_OCCLUSION multiplies the sums by ao; TIR_LIGHT_SRGB then applies linear2srgb (clamp to [0, 1], x <= 0.0031308 ?
 *   12.92 x : 1.055 (x + 1e-6)^(1 / 2.4) - 0.055, models/relight_utils.py:489-515); without it the sums are not clamped.
 *   One thread per row over all M rows (no compaction of the covered rows); nothing is allocated, there are no atomics and the
 *   order per row is fixed: two calls give identical bits, and a row's result does not depend on where it stands in the buffer.
 *   Validated on the host before any device work: M < 0, D < 1, unknown flag bits, and with M > 0 a null pointer or gbuf, cells
 *   or out not 16-byte aligned -> TIR_ERR_ARG; D > 2^20 (or M > 2^36) -> TIR_ERR_UNSUPPORTED.  M = 0 does nothing. */
#define TIR_LIGHT_OCCLUSION 1
#define TIR_LIGHT_SRGB      2
int tir_env_cells(const float* hdr, int32_t H, int32_t W, const float* row_w, int32_t h, int32_t w, float* cells, void* stream);
int tir_light_gbuffer(const float* gbuf, const float* view, const float* cells, int64_t M, int32_t D, float fresnel, int32_t flags,
                      float* out, void* stream);

/* ---- Shadows of the exported asset: one orthographic z-buffer per light cell (tensoir_amd/raster.py relight_mesh(shadows=True) /
 * shadow_maps_for / compare_asset(shadows=True); restated in numpy by tests/shadow_reference.py).
 * Frames: frames [D][12] fp32 (ops.shadow_frames forms them in float64 on the host and rounds once).  With L = cells[d].dir
 *   normalised, a = the world axis with the smallest |L_a| (the lowest index on ties), u = normalize(e_a x L), v = L x u, c and r
 *   the centre and radius of a sphere round the mesh and g = S / (2 r), row d is
 *     {g u, S/2 - g (u.c),  g v, S/2 - g (v.c),  L / (4 r), 0.5 - (L.c) / (4 r)}
 *   and a point p has, every product and sum rounded to fp32 on its own, in this order,
 *     x_px = ((f0 p0 + f1 p1) + f2 p2) + f3,   y_px = ((f4 p0 + f5 p1) + f6 p2) + f7,   w = ((f8 p0 + f9 p1) + f10 p2) + f11.
 *   w lies in about [0.25, 0.75] inside the sphere; a larger w is nearer to the light, and a positive w's bits order as unsigned
 *   integers.  One texel is 1 / (2 S) in units of w.
 * tir_shadow_maps: pos [V][3], faces NULL (corner q reads pos[q], V >= 3 F) or [F][3] int32, as tir_raster_project -> maps
 *   [D][S][S] uint32, cleared to 0 (= empty) by the entry: every texel holds bits(w) of the surface nearest to cell d's light.
 *   Per (cell, face) pair: the three corners projected as above and snapped, sx = rint(256 x_px) (half to even).  The pair is
 *   dropped when, tested in this order: a vertex index lies outside [0, V) (no vertex of such a face is read); an x_px, y_px or w
 *   is not finite; an |sx| or |sy| exceeds TIR_RASTER_GUARD * 256.  status [4] int64, cleared first, counts the dropped PAIRS
 *   {index, 0, guard, non-finite} (the slots of tir_raster_project; there is no near plane).  Coverage is tir_raster_cover's
 *   integer rule with cull = 0 (both orientations cast shadows), texel (i, j) having its centre at (256 i + 128, 256 j + 128).
 *   Fragment depth, each step rounded on its own:  w = ((E0 w0 + E1 w1) + E2 w2) / |A|  (exact interpolation: the projection is
 *   affine); a fragment whose w is not > 0 is not written; the others go through one 32-bit unsigned atomic max.  The maps do not
 *   depend on the order of the faces, on the order fragments arrive in, or on work_cap.
 *   work: [2 + 2 work_cap] int32 the entry owns during the call: pairs whose box of texel centres holds more than 64 texels are
 *   listed there (at most work_cap of them) and walked by a workgroup each in a second launch; when the list is full the pair's
 *   thread walks the box itself.  work_cap = 0 is allowed.
 * tir_shadow_lookup (diagnostics and tests): pts, nrm [M][3], cells [D][8] (tir_env_cells' records) -> vis [M][D] uint8:
 *   0: the pair does not contribute, c = n.L <= 1e-6 with c formed as tir_light_gbuffer forms it (sums of products may be fused);
 *   2: lit;  1: shadowed.  THE VISIBILITY RULE: the point is projected as above; its texel is (floor(x_px), floor(y_px)), nearest,
 *   no filtering; it is lit when the texel lies outside [0, S)^2 (or a coordinate is NaN), when the texel is 0, or when
 *     w + bias >= as_float(texel),   bias = (bias_const + bias_slope * min(sqrt(max(1 - c c, 0)) * rcp(c), 8)) * texel_w
 *   with texel_w = 0.5f / S formed once on the host in fp32, sqrt and rcp the one-ulp hardware instructions, every other step
 *   rounded on its own.  bias_const and bias_slope are in texels.
 * tir_light_gbuffer_shadowed: tir_light_gbuffer (above) with pts [M][3], the world position of each row's surface point: the
 *   same thread layout, arithmetic, order, flags and validation; a pair with c > 1e-6 is added only when the visibility rule
 *   says lit, tested before the specular term.  With empty maps the result equals tir_light_gbuffer's bit for bit.  No atomics,
 *   a fixed order per row: two calls give identical bits, and a row's result does not depend on where it stands in the buffer.
 * All three validate on the host before any device work: a null pointer (pos may be null when F = 0; with M = 0 the lookup and
 *   the lighting do nothing and take null pointers), D < 1, S < 1, a negative count or work_cap, V < 3 F without faces, a
 *   negative or non-finite bias, unknown flag bits, frames / cells / gbuf / out not 16-byte, status not 8-byte, maps / work not
 *   4-byte aligned -> TIR_ERR_ARG; S > TIR_SHADOW_MAX_SIDE, F > TIR_RASTER_MAX_FACES, V > 2^31 - 1, D > 2^20, M > 2^36 ->
 *   TIR_ERR_UNSUPPORTED.  F = 0 gives empty maps.  They allocate nothing. */
#define TIR_SHADOW_MAX_SIDE 4096
int tir_shadow_maps(const float* pos, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* frames, int32_t D,
                    int32_t S, uint32_t* maps, int32_t* work, int32_t work_cap, int64_t* status, void* stream);
int tir_shadow_lookup(const float* pts, const float* nrm, const float* cells, const float* frames, const uint32_t* maps, int64_t M,
                      int32_t D, int32_t S, float bias_const, float bias_slope, uint8_t* vis, void* stream);
int tir_light_gbuffer_shadowed(const float* gbuf, const float* view, const float* cells, const float* pts, const float* frames,
                               const uint32_t* maps, int64_t M, int32_t D, int32_t S, float bias_const, float bias_slope, float fresnel,
                               int32_t flags, float* out, void* stream);

/* tir_light_gbuffer_occluded: tir_light_gbuffer with occl [D][occl_stride] uint64, the packed answers of
 *   tir_shadow_trace for the same rows and cells (occl_stride >= ceil(M / 64) words per cell): the same thread layout, arithmetic,
 *   order, flags and validation; a pair with c > 1e-6 is added only when bit m & 63 of word [d][m >> 6] is 0, tested where
 *   tir_light_gbuffer_shadowed tests its map, before the specular term.  With all words 0 the result equals tir_light_gbuffer's
 *   bit for bit; with the bits of tir_shadow_lookup's code 1 it equals tir_light_gbuffer_shadowed's.  Blocks start at multiples
 *   of 64 rows, so a wave reads one word per cell.  Validation as tir_light_gbuffer, and with M > 0 a null occl, occl not 8-byte
 *   aligned or occl_stride < ceil(M / 64) -> TIR_ERR_ARG. */
int tir_light_gbuffer_occluded(const float* gbuf, const float* view, const float* cells, const uint64_t* occl, int64_t occl_stride,
                               int64_t M, int32_t D, float fresnel, int32_t flags, float* out, void* stream);

/* ---- Image metrics of the evaluation loop (tensoir_amd/metrics.py; restated in numpy by tests/metrics_reference.py).
 * tir_ssim: the reference's rgb_ssim (utils.py:93-139) for N image pairs.  img0, img1 [N][H][W][C] fp32 on the device, channel
 *   last, 1 <= C <= 4.  taps: n_taps doubles in HOST memory, read during the call (they travel with the launch); the filtered value
 *   of z at output (i, j) is  sum_k taps[k] (sum_l taps[l] z[i + k][j + l])  over the n_taps x n_taps window whose first pixel is
 *   (i, j) ("valid" filtering: the map is [N][H - n_taps + 1][W - n_taps + 1][C]).
 *   Arithmetic: x x, y y and x y are fp32 products, each rounded on its own (the reference squares fp32 images in fp32); they and
 *   x, y are widened to double, and every sum is a double sum: over l first, then over k, each in ascending order (products and
 *   sums may be fused).  With the filtered m0, m1, e00, e11, e01, every step rounded on its own:
 *     mu00 = m0 m0; mu11 = m1 m1; mu01 = m0 m1; s00 = max(0, e00 - mu00); s11 = max(0, e11 - mu11); s01 = e01 - mu01;
 *     s01 = sign(s01) min(sqrt(s00 s11), |s01|);  value = ((2 mu01 + c1) (2 s01 + c2)) / ((mu00 + mu11 + c1) (s00 + s11 + c2)).
 *   map (may be null): every value, double.  mean [N], double, written on the device: the sum of the image's values / their count.
 *   One workgroup per TIR_SSIM_TILE x TIR_SSIM_TILE tile of the map.  The mean is a fixed-order sum: per-workgroup partials in
 *   `workspace`, added in tile order by the workgroup that finishes the image last.  No floating-point atomics: two calls give
 *   identical bits, and an image's results do not depend on what else is in the batch.  workspace: tir_ssim_workspace(...) doubles
 *   (8-byte aligned) the entry owns during the call; it may hold anything.  Nothing is allocated and the host does not wait.
 * tir_image_error: a, b [N][P][C] fp32, mask null or [N][P] uint8 (a pixel counts where its byte is not 0) -> out [N][3] double:
 *   {pixels counted, sum over them and their C channels of (a - b)^2 formed in double, sum over them of the angle in degrees}.  The
 *   angle is acos(clamp((a0 b0 + a1 b1) + a2 b2, -1, 1)) 180 / pi in double for C = 3 and angular != 0, else the third number is
 *   0; nothing is normalised.  The same tail: TIR_IMAGE_ERROR_SHARE pixels per workgroup, at most 256 workgroups per image.
 * Both validate on the host before any device work: a negative size, n_taps outside [1, TIR_SSIM_MAX_TAPS] or larger than H or W,
 *   and with N > 0 a null pointer (map and mask may be null; a, b too when P = 0) -> TIR_ERR_ARG; C outside [1, 4], or more than
 *   2^31 workgroups -> TIR_ERR_UNSUPPORTED (the workspace sizes return the same codes).  N = 0 does nothing. */
#define TIR_SSIM_TILE 16
#define TIR_SSIM_MAX_TAPS 31
#define TIR_IMAGE_ERROR_SHARE 2048
int64_t tir_ssim_workspace(int64_t N, int32_t H, int32_t W, int32_t C, int32_t n_taps);
int tir_ssim(const float* img0, const float* img1, int64_t N, int32_t H, int32_t W, int32_t C, const double* taps, int32_t n_taps,
             double c1, double c2, double* map, double* workspace, double* mean, void* stream);
int64_t tir_image_error_workspace(int64_t N, int64_t P);
int tir_image_error(const float* a, const float* b, const uint8_t* mask, int64_t N, int64_t P, int32_t C, int32_t angular,
                    double* workspace, double* out, void* stream);

/* ---- Total-variation regulariser of the VM planes (tensoir_amd/regularisers.py; restated in float64 by
 * tests/regulariser_reference.py): the reference's TVLoss (utils.py:143-162) over up to TIR_TV_MAX_PLANES planes, one launch forward
 * and one launch backward for the whole list.
 * planes, C, H, W, coef (and grads): arrays of n_planes entries in HOST memory, read during the call (they travel with the launch).
 *   Plane p is fp32 [1, C, H, W] in channel-last storage, [H][W][C] in device memory, H >= 2 and W >= 2, fewer than 2^31 elements.
 *   With  Sh = sum (x[h+1][w][c] - x[h][w][c])^2,  Sw = sum (x[h][w+1][c] - x[h][w][c])^2,  nh = C (H - 1) W,  nw = C H (W - 1):
 * tir_tv_fwd:  sums [n_planes][2] double = {Sh, Sw} per plane, and  loss (fp32) = sum_p coef[p] 2 (Sh_p / nh_p + Sw_p / nw_p).
 *   Arithmetic: the subtraction and the square are fp32 operations, each rounded on its own (the reference squares fp32
 *   differences in fp32); every term is widened to double and every sum is a double sum in a fixed order: a workgroup owns a
 *   contiguous share of one plane's floats (TIR_TV_SHARE of them, or more where the plane would otherwise get more than
 *   TIR_TV_FWD_GROUPS workgroups: a function of the plane's size alone) and leaves two double partials in `workspace`; the
 *   workgroup that draws the launch's last ticket adds each plane's partials in an order fixed by the plane's workgroup count,
 *   forms the loss in double in the order written above, plane by plane (no step fused with another), and rounds it once.  No floating-point atomics: two calls give identical bits, and a
 *   plane's sums do not depend on what else is in the call.  workspace: tir_tv_workspace(...) doubles (8-byte aligned) the entry
 *   owns during the call; it may hold anything.  Nothing is allocated and the host does not wait.
 * tir_tv_bwd:  grads[p] (same storage as plane p; null: the plane is skipped) receives, for the upstream gradient *g (ONE fp32 on
 *   the DEVICE, read by the kernel: the host never sees it),
 *     grad[h][w][c] = sh (dmh - dph) + sw (dmw - dpw),   sh = g ah,  sw = g aw   (fp32, each product rounded on its own),
 *     ah = fp32(4 coef[p] / nh),  aw = fp32(4 coef[p] / nw)   (formed in double on the host, rounded once),
 *     dph = x[h+1] - x[h] (0 on the last row),  dmh = x[h] - x[h-1] (0 on the first row),  dpw, dmw the same along W,
 *   every difference an fp32 subtraction rounded on its own; the final expression is fp32 and may fuse.  The stencil is recomputed
 *   from the plane; every element of grads[p] is written exactly once (no memset, no atomics).  grads[p] must not overlap a plane.
 * Both take 16-byte loads and stores on a plane with C % 4 == 0 whose tensors are 16-byte aligned, scalar ones otherwise.
 * Validation on the host before any device work: n_planes outside [0, TIR_TV_MAX_PLANES] -> TIR_ERR_ARG; n_planes = 0 does
 *   nothing (TIR_OK; the workspace size is 1); then a null C / H / W, C < 1, H < 2 or W < 2 -> TIR_ERR_ARG; a null planes, coef,
 *   workspace, sums, loss, g, grads or planes[p] -> TIR_ERR_ARG; a plane of 2^31 elements or more (which also keeps the launch far below 2^31
 *   workgroups) -> TIR_ERR_UNSUPPORTED (tir_tv_workspace returns the same codes). */
#define TIR_TV_MAX_PLANES 8
#define TIR_TV_SHARE 8192
#define TIR_TV_FWD_GROUPS 128
int64_t tir_tv_workspace(int32_t n_planes, const int32_t* C, const int32_t* H, const int32_t* W);
int tir_tv_fwd(const float* const* planes, const int32_t* C, const int32_t* H, const int32_t* W, const double* coef, int32_t n_planes,
               double* workspace, double* sums, float* loss, void* stream);
int tir_tv_bwd(const float* const* planes, const int32_t* C, const int32_t* H, const int32_t* W, const double* coef, int32_t n_planes,
               const float* g, float* const* grads, void* stream);

/* ---- Guided a-trous denoiser of relit views (tensoir_amd/denoise.py, relight.relight_view; restated in float64 by
 * tests/denoise_reference.py): the edge-avoiding wavelet filter of Dammertz et al. 2010, guided by the noise-free maps of the
 * primary pass.
 * tir_denoise_guide: maps [n][20] (the primary pass's map rows: depth 3, normal 4:7, albedo 7:10, roughness 10, acc 14) and
 *   rays [n][6] -> rows [row0, row0 + n) of guide [..][TIR_DENOISE_GUIDE] fp32, 16-byte aligned:
 *     {pos.xyz = o + depth d (one fused multiply-add per component), valid = acc > acc_thres ? 1 : 0,
 *      n.xyz = normal / max(|normal|, fp32(1e-6)) (|normal| = sqrt of the fp32 sum of squares), roughness, albedo.rgb, 0}.
 *   One launch; no other row of guide is touched.
 * tir_atrous_level: one level, out of place.  color_in, color_out [H W][K] fp32, the image row-major, K = 3 n_maps in
 *   3..TIR_ATROUS_MAX_K (the rows relight_chunk writes: every map of a view is filtered by one launch); guide [H W][12] as above,
 *   a pixel is valid where its fourth float exceeds 0.5.  An invalid pixel copies its input.  For a valid pixel p, over the taps
 *   q = p + step (i, j), i, j in -2..2, that lie inside the image and are valid:
 *     h   = k[|i|] k[|j|],  k = (3/8, 1/4, 1/16)
 *     a   = max(0, 1 - n_p.n_q) inv_sn + |(x_q - x_p).n_p| inv_sp + |alb_p - alb_q|^2 inv_sa2 + (r_p - r_q)^2 inv_sr2
 *     w_m = h exp(-(a + |c_p^m - c_q^m|^2 inv_sc2))  per map m      (inv_sc2 = 0: the colour term is off, one weight for all maps)
 *     out_p^m = sum_q w_m c_q^m / sum_q w_m                          (the centre tap has w = 9/64: the denominator is never 0)
 *   fp32 throughout, formed as c_p + sum_q w_m (c_q - c_p) / sum_q w_m with the centre tap's weight taken as 9/64 exactly: a
 *   pixel without a valid neighbour and a constant image are returned bit for bit.  The taps are added in the fixed order j,
 *   then i, one fused multiply-add per channel; no atomics and nothing
 *   that depends on the launch shape: two calls give identical bits, and a map's result does not depend on the other maps of the
 *   call (a K = 15 call equals five K = 3 calls bit for bit).  A step beyond the image's longer side leaves the centre tap.
 * Both validate on the host before any device work: n < 0, row0 < 0, H or W < 1, K no multiple of 3 or outside 3..24, step < 1,
 *   a negative or non-finite inv_*, a null pointer (n = 0 is asked for none and does nothing), color_in == color_out, a guide that
 *   is not 16-byte aligned -> TIR_ERR_ARG; an image of 2^31 pixels or a side of 2^29 or more -> TIR_ERR_UNSUPPORTED.  Nothing is
 *   allocated and the host does not wait. */
#define TIR_DENOISE_GUIDE 12
#define TIR_ATROUS_MAX_K 24
int tir_denoise_guide(const float* maps, const float* rays, int64_t n, float acc_thres, float* guide, int64_t row0, void* stream);
int tir_atrous_level(const float* color_in, float* color_out, const float* guide, int32_t H, int32_t W, int32_t K, int32_t step,
                     float inv_sn, float inv_sp, float inv_sa2, float inv_sr2, float inv_sc2, void* stream);

/* ---- Material editing (tensoir_amd/materials.py; restated in float64 by tests/materials_reference.py): albedo,
 * roughness and Fresnel term of surface rows changed between the primary pass and the shading stage (relight.relight_chunk), or
 * between the bake and the texture atlas (mesh.bake_atlas).
 * An EDIT LIST is n_edits in 0..TIR_MATERIAL_MAX_EDITS records of TIR_MATERIAL_EDIT_FLOATS fp32 in DEVICE memory (every lane reads
 * the same record: scalar loads).  Integers are stored as the floats that equal them.  Record:
 *    [0] selectors, the sum of 1 sphere, 2 box, 4 colour, 8 roughness band, 16 palette entry      [1] strength
 *    [2:5] sphere centre  [5] radius  [6] feather                 [7:10] box centre  [10:13] half extents  [13] feather
 *    [14:17] colour (linear RGB)  [17] tolerance  [18] feather    [19] lo  [20] hi  [21] feather           [22] palette id
 *    [23] albedo mode: 0 keep, 1 set, 2 multiply, 3 recolour      [24:27] target colour (linear RGB)
 *    [27] roughness scale  [28] roughness offset                  [29] 1: metallic is a target  [30] metallic   [31] 0
 * The PALETTE (optional) is k in 0..TIR_MATERIAL_MAX_PALETTE centroids [k][4] fp32 in device memory and the roughness weight wr.
 * A row has the position x, albedo a0, roughness r0 and Fresnel term f0.  State: base = a0, rough = r0, metal = 0.  Per edit, in
 * list order:
 *    w = strength x the product of the enabled selectors, all of which read the row's ORIGINAL x, a0, r0.  With
 *      smoothstep(t) = t t (3 - 2 t),  fall(d, r, f) = f > 0 ? 1 - smoothstep(clamp((d - r) / f, 0, 1)) : (d <= r ? 1 : 0):
 *      sphere  fall(|x - c|, radius, feather)             box     fall(max over the axes of (|x - c| - half), 0, feather)
 *      colour  fall(|a0 - colour|, tolerance, feather)    band    fall(max(lo - r0, r0 - hi), 0, feather)
 *      palette label(a0, r0) == id ? 1 : 0, label = the lowest j that minimises d2_j = ((D0 D0 + D1 D1) + D2 D2) + D3 D3,
 *              D = (a0.r, a0.g, a0.b, wr r0) - centroid j; wr r0, every difference, product and sum is ONE fp32 operation rounded
 *              on its own (tir::material_label, the function tir_kmeans_assign labels with); without a palette it is 0.
 *    an edit with w == 0 leaves the state as it is.  Otherwise
 *      target albedo: keep base; set colour; multiply base o colour; recolour colour Y(base) / max(Y(colour), 1e-6) with
 *              Y = 0.2126 r + 0.7152 g + 0.0722 b; clamped to [0, 1].   target roughness: clamp(rough scale + offset, 0.09, 0.99).
 *      v += w (target - v) for base, for rough unless scale = 1 and offset = 0 (an edit that does not ask for another roughness
 *      leaves rough as it is, also outside the clamp's range), and for metal where [29] is 1 (target [30]).
 * After the last edit: albedo = base (1 - metal), fresnel = f0 (1 - metal) + base metal (glTF's metallic-roughness model with the
 * row's own F0), roughness = rough.  fp32 throughout, every operation rounded on its own (no fused multiply-add: the two entries
 * below give the same bits on the same rows), sums of three terms from the left, smoothstep as (t t) (3 - 2 t).  A row on which
 * every edit has w == 0 -- an empty list included -- keeps the bits of its albedo, roughness and Fresnel term (base = a0, metal = 0).
 * tir_material_edit: rows i < min(M, *m_dev) (m_dev [1] in device memory or NULL = M) of plain arrays, row i of an array at
 *   i x its stride: points (stride >= 3), albedo (>= 3), rough (>= 1), fresnel (>= 3) -> out_albedo, out_rough, out_fresnel,
 *   out_base (may be NULL), out_metal (may be NULL), which are dense: [M][3], [M], [M][3], [M][3], [M].  An output may be its
 *   input where that is dense too.  Rows beyond the count are not written.
 * tir_material_edit_maps: in place on the albedo (7:10), roughness (10) and Fresnel (11:14) columns of the rows of maps [B][20]
 *   with acc (14) > acc_thres; x = o + depth d from rays [B][6], by the device function tir_surface_compact forms surf with (the
 *   same bits).  Only rows with an edit of w != 0 are written; n_edits = 0 does nothing.
 * Both: one lane per row, no atomics, no LDS, nothing allocated, the host does not wait.  Host validation before any device
 *   work: n_edits outside 0..TIR_MATERIAL_MAX_EDITS, k outside 0..TIR_MATERIAL_MAX_PALETTE, a negative M or B, a stride below its
 *   width, a non-finite wr or a NaN acc_thres, edits null with n_edits > 0, palette null with k > 0, and with M or B > 0 a null
 *   array (out_base and out_metal excepted) -> TIR_ERR_ARG; M > 2^31 - 1 -> TIR_ERR_UNSUPPORTED.
 * tir_atlas_metal: the B channel of tir_atlas_pack's orm image = round(255 clamp(metal, 0, 1)), half to even, on the owned
 *   texels (metal [N] in tir_atlas_texels' cell-major order); nothing else is written.  size, cols, T, n_faces: the layout, refused
 *   as tir_atlas_pack refuses it; a null pointer or an orm that is not 4-byte aligned -> TIR_ERR_ARG; F = 0 does nothing.
 *
 * Deterministic k-means (Lloyd) over rows with the feature (a.r, a.g, a.b, wr r), albedo [N][3], rough [N]; the host loops.
 *   Distances are tir::material_label's d2 in fp32; every sum is a double sum in a fixed order; no floating-point atomics: two
 *   calls give identical bits.  k in 1..TIR_MATERIAL_MAX_PALETTE, centroids [k][4] fp32, N >= 1.
 * tir_kmeans_seed: one farthest-point step given the first n_have centroids.  n_have = 0: centroid 0 = the feature of row 0.
 *   Otherwise mind[i] = min(mind[i], d2(row i, centroid n_have - 1)) (n_have = 1: mind[i] = d2, mind is not read), and centroid
 *   n_have = the feature of the row of largest mind, the lowest index among equals: one 64-bit integer atomic max of
 *   (bits(mind) << 32) | (0xFFFFFFFF - i) per wave into best [1] (8-byte aligned; the entry clears it first).
 * tir_kmeans_assign: labels [N] int32 = label of each row (read first unless first != 0: then every row counts as changed).
 *   Workgroup g owns rows [g TIR_KMEANS_ROWS, (g + 1) TIR_KMEANS_ROWS) and STORES part_sums [g][k][5] double = per cluster the
 *   sums of the four features and of d2 over its rows in row order, part_counts [g][k] int32, part_changed [g] int32.
 *   tir_kmeans_groups(N) = the number of workgroups.
 * tir_kmeans_update: one workgroup adds the partials in workgroup order: counts [k] int64, centroid = fp32(sum / count) (an empty
 *   cluster keeps its centroid), inertia [1] double = the sum of d2 in cluster order, changed [1] int32.
 * Validation: N < 0, n_have outside [0, k), k outside 1..TIR_MATERIAL_MAX_PALETTE, a non-finite wr, a null pointer, n_groups !=
 *   tir_kmeans_groups(N) -> TIR_ERR_ARG; N > 2^31 - 1 -> TIR_ERR_UNSUPPORTED; N = 0 -> TIR_ERR_ARG (there is nothing to seed from). */
#define TIR_MATERIAL_MAX_EDITS 16
#define TIR_MATERIAL_EDIT_FLOATS 32
#define TIR_MATERIAL_MAX_PALETTE 32
#define TIR_KMEANS_ROWS 256
int tir_material_edit(const float* edits, int32_t n_edits, const float* palette, int32_t k, float wr, const float* points,
                      int32_t point_stride, const float* albedo, int32_t albedo_stride, const float* rough, int32_t rough_stride,
                      const float* fresnel, int32_t fresnel_stride, float* out_albedo, float* out_rough, float* out_fresnel,
                      float* out_base, float* out_metal, int64_t M, const int32_t* m_dev, void* stream);
int tir_material_edit_maps(const float* edits, int32_t n_edits, const float* palette, int32_t k, float wr, float* maps,
                           const float* rays, int64_t B, float acc_thres, void* stream);
int tir_atlas_metal(uint8_t* orm, int32_t size, int32_t cols, int32_t T, int64_t n_faces, const float* metal, void* stream);
int64_t tir_kmeans_groups(int64_t N);
int tir_kmeans_seed(const float* albedo, const float* rough, int64_t N, float wr, float* centroids, int32_t k, int32_t n_have,
                    float* mind, uint64_t* best, void* stream);
int tir_kmeans_assign(const float* albedo, const float* rough, int64_t N, float wr, const float* centroids, int32_t k,
                      int32_t first, int32_t* labels, double* part_sums, int32_t* part_counts, int32_t* part_changed,
                      int64_t n_groups, void* stream);
int tir_kmeans_update(const double* part_sums, const int32_t* part_counts, const int32_t* part_changed, int64_t n_groups,
                      float* centroids, int32_t k, int64_t* counts, double* inertia, int32_t* changed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TENSOIR_HIP_H */
