// Dense appearance-feature volume of a one-light field (TirField::dense_app): the build kernel and its entry.  The lookup that
// reads the volume is tir::dense_app_lookup (tir_common.hpp), used by k_vm_app_dense (tir_field.hip) and k_indirect_fused_dense
// (tir_mlp.hip).
#include "tir_common.hpp"

using namespace tir;

// ------------------------------------------------------------------------------------------------
// Dense appearance-feature volume (TirField::dense_app; 48 components, app_dim 27, one light): for grid corner (x, y, z)
//     feature j = sum_k sum_c basis_mat[j][48 k + c] * (plane_k,c(corner) * line_k,c(corner) * light_row_0[48 k + c]).
// One thread per corner, x fastest; basis_mat^T (144 x 32 fp32) and the light row in LDS (every lane reads the same address: a
// broadcast).  The fp32 parameters are read, not their fp16 shadow; each product is (plane * line) * light in fp32 and the 144
// terms of a feature are accumulated with fp32 FMAs in channel order, then rounded to fp16 ONCE (saturating, as the shadow
// planes).  Output [z][y][x of pitch][half 2][16]: half 0 = features 0..13, half 1 = 14..26 (the decoder's lane halves,
// FUS_NF0 of tir_mlp.hip), unused slots and the corners [grid x, pitch) of a row are 0.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_dense_app_build(TirField f, uint4* __restrict__ vol, int pitch) {
    __shared__ __attribute__((aligned(16))) float Bt[3 * DA_CA * 32];
    __shared__ __attribute__((aligned(16))) float Lr[3 * DA_CA];
    for (int i = threadIdx.x * 4; i < 3 * DA_CA * 32; i += 256 * 4) *reinterpret_cast<float4*>(Bt + i) = ld4(f.basis_t + i);
    for (int i = threadIdx.x; i < 3 * DA_CA; i += 256) Lr[i] = f.light_line[i];
    __syncthreads();
    const int X = f.grid[0], Y = f.grid[1], Z = f.grid[2];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)pitch * Y * Z) return;
    const int x = (int)(i % pitch), y = (int)((i / pitch) % Y), z = (int)(i / ((int64_t)pitch * Y));
    float acc[32];                                           // (28 used: 27 features + the padding column)
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = 0.0f;
    if (x < X) {
        // plane k is [grid[m1]][grid[m0]][48] with (m0, m1) = (x, y), (x, z), (y, z); line k runs along z, y, x
        const float* const pl[3] = {f.aplane[0] + ((size_t)y * X + x) * DA_CA, f.aplane[1] + ((size_t)z * X + x) * DA_CA,
                                    f.aplane[2] + ((size_t)z * Y + y) * DA_CA};
        const float* const ln[3] = {f.aline[0] + (size_t)z * DA_CA, f.aline[1] + (size_t)y * DA_CA, f.aline[2] + (size_t)x * DA_CA};
#pragma unroll 1
        for (int k = 0; k < 3; ++k)
#pragma unroll 1
            for (int c = 0; c < DA_CA; c += 4) {
                const float4 a = ld4(pl[k] + c), b = ld4(ln[k] + c), l = *reinterpret_cast<const float4*>(Lr + k * DA_CA + c);
                const float p[4] = {(a.x * b.x) * l.x, (a.y * b.y) * l.y, (a.z * b.z) * l.z, (a.w * b.w) * l.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* bt = Bt + (k * DA_CA + c + e) * 32;
#pragma unroll
                    for (int j = 0; j < 28; j += 4) {       // (column 27 of basis_mat^T is zero padding)
                        const float4 w = *reinterpret_cast<const float4*>(bt + j);
                        acc[j] = fmaf(w.x, p[e], acc[j]); acc[j + 1] = fmaf(w.y, p[e], acc[j + 1]);
                        acc[j + 2] = fmaf(w.z, p[e], acc[j + 2]); acc[j + 3] = fmaf(w.w, p[e], acc[j + 3]);
                    }
                }
            }
    }
    unsigned pk[16];                                         // [half][8 pairs]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int nf = h ? DA_F - DA_NF0 : DA_NF0, j0 = (h ? DA_NF0 : 0) + 2 * q;
            const tir_h2 v = {2 * q < nf ? sat_half(acc[j0]) : (_Float16)0.0f, 2 * q + 1 < nf ? sat_half(acc[j0 + 1]) : (_Float16)0.0f};
            pk[8 * h + q] = __builtin_bit_cast(unsigned, v);
        }
    uint4* o = vol + i * 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = make_uint4(pk[4 * t], pk[4 * t + 1], pk[4 * t + 2], pk[4 * t + 3]);
}

extern "C" int tir_dense_app_build(const TirField* f, void* vol, int32_t pitch, void* stream) {
    if (!f) return TIR_ERR_ARG;
    if (int rc = tir_check_app_field(f, TirAppNeeds().aligned().no_light_mean().width(DA_CA).app_dim_is(DA_F).no_feature_rows(), 0)) return rc;
    if (!vol || pitch <= f->grid[0] || !tir_aligned16({vol, f->basis_t})) return TIR_ERR_ARG;
    if (f->n_lights != 1 || !tir_dense_app_index_ok(f->grid, pitch)) return TIR_ERR_UNSUPPORTED;
    const int64_t n = (int64_t)pitch * f->grid[1] * f->grid[2];
    return tir_launch(k_dense_app_build, 0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, tir_stream(stream), *f,
                      reinterpret_cast<uint4*>(vol), (int)pitch);
}
