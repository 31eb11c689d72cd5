// Material editing (tensoir_amd/materials.py; contract: include/tensoir_hip.h, tir_material_* / tir_kmeans_* / tir_atlas_metal;
// DESIGN 4.18; restated in float64 by tests/materials_reference.py).
//
// k_material_edit  one lane per row: the row's position, albedo, roughness and Fresnel term through the edit list.  The records
//                  and the palette are read at wave-uniform addresses (scalar loads); the row's state stays in registers.  ONE row
//                  function (material_row), instantiated for plain strided arrays (the bake's outputs, out of place) and for the
//                  [B][20] map rows of a relight chunk (in place, position = tir::surface_point of the ray).  No LDS, no atomics.
// k_orm_metal    one thread per texel of the orm image: the B byte of an owned texel.
// k_kmeans_*       deterministic Lloyd: a farthest-point seeding step (the one atomic: a 64-bit integer max per wave), the
//                  assignment with per-workgroup double partial sums in row order (stored, never atomically added), and the
//                  one-workgroup update that adds them in workgroup order.  Labels come from tir::material_label, the function the
//                  palette selector of k_material_edit calls.
#include "tir_common.hpp"

#include <cmath>

// No fused multiply-add anywhere in this file: every product and sum below is one fp32 (or double) operation rounded on its own.
// The two instantiations of k_material_edit must give the same bits on the same rows (the Fresnel rows of a relit chunk equal
// materials.apply on the compacted rows), and which of f0 (1 - metal) + base metal's products a compiler fuses is its choice per
// instantiation.
#pragma clang fp contract(off)

#define TIR_MATERIAL_THREADS 256
static_assert(TIR_KMEANS_ROWS == TIR_MATERIAL_THREADS, "one thread per row of a k-means workgroup");
static_assert(5 * TIR_MATERIAL_MAX_PALETTE <= TIR_MATERIAL_THREADS, "one thread per (cluster, sum) of the partials");
static_assert(TIR_MATERIAL_EDIT_FLOATS == 32, "the record layout below");

namespace {

// ---- the edit list on one row ---------------------------------------------------------------------------------------------------
struct MatRow {
    float x[3], a[3], r, f[3];          // position, albedo, roughness, Fresnel term as they came
};
struct MatResult {
    float albedo[3], rough, fresnel[3], base[3], metal;
    bool touched;                       // false: every edit had w == 0, the caller keeps the row's bits
};

__device__ __forceinline__ float mat_fall(float d, float r, float f) {
    if (f > 0.f) {
        const float t = fminf(fmaxf((d - r) / f, 0.f), 1.f);
        return 1.f - t * t * (3.f - 2.f * t);
    }
    return d <= r ? 1.f : 0.f;
}
__device__ __forceinline__ float mat_luma(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ __forceinline__ float mat_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

__device__ __forceinline__ MatResult material_row(const MatRow& in, const float* __restrict__ edits, int n_edits,
                                                  const float* __restrict__ palette, int k, float wr) {
    float base[3] = {in.a[0], in.a[1], in.a[2]}, rough = in.r, metal = 0.f;
    bool touched = false;
    int label = -2;                                                    // not yet looked up
    for (int e = 0; e < n_edits; ++e) {
        const float* __restrict__ E = edits + (size_t)e * TIR_MATERIAL_EDIT_FLOATS;
        const int sel = (int)E[0];
        float w = E[1];
        if (sel & 1) {
            const float dx = in.x[0] - E[2], dy = in.x[1] - E[3], dz = in.x[2] - E[4];
            w *= mat_fall(sqrtf(dx * dx + dy * dy + dz * dz), E[5], E[6]);
        }
        if (sel & 2) {
            const float qx = fabsf(in.x[0] - E[7]) - E[10], qy = fabsf(in.x[1] - E[8]) - E[11], qz = fabsf(in.x[2] - E[9]) - E[12];
            w *= mat_fall(fmaxf(fmaxf(qx, qy), qz), 0.f, E[13]);
        }
        if (sel & 4) {
            const float dr = in.a[0] - E[14], dg = in.a[1] - E[15], db = in.a[2] - E[16];
            w *= mat_fall(sqrtf(dr * dr + dg * dg + db * db), E[17], E[18]);
        }
        if (sel & 8) w *= mat_fall(fmaxf(E[19] - in.r, in.r - E[20]), 0.f, E[21]);
        if (sel & 16) {
            if (label == -2) {
                float d2;
                label = k > 0 ? tir::material_label(palette, k, wr, in.a[0], in.a[1], in.a[2], in.r, d2) : -1;
            }
            w *= label == (int)E[22] ? 1.f : 0.f;
        }
        if (w == 0.f) continue;
        touched = true;
        const int mode = (int)E[23];
        float t[3] = {base[0], base[1], base[2]};
        if (mode == 1) {
            t[0] = E[24]; t[1] = E[25]; t[2] = E[26];
        } else if (mode == 2) {
            t[0] = base[0] * E[24]; t[1] = base[1] * E[25]; t[2] = base[2] * E[26];
        } else if (mode == 3) {
            const float s = mat_luma(base[0], base[1], base[2]) / fmaxf(mat_luma(E[24], E[25], E[26]), 1e-6f);
            t[0] = E[24] * s; t[1] = E[25] * s; t[2] = E[26] * s;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) base[c] += w * (mat_clamp(t[c], 0.f, 1.f) - base[c]);
        if (E[27] != 1.f || E[28] != 0.f) rough += w * (mat_clamp(rough * E[27] + E[28], 0.09f, 0.99f) - rough);
        if (E[29] != 0.f) metal += w * (E[30] - metal);
    }
    MatResult o;
    o.touched = touched;
    o.rough = rough;
    o.metal = metal;
    const float dielectric = 1.f - metal;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.base[c] = base[c];
        o.albedo[c] = base[c] * dielectric;
        o.fresnel[c] = in.f[c] * dielectric + base[c] * metal;
    }
    return o;
}

// rows of plain strided arrays -> dense outputs: every row below the count is written, an untouched one as the bits it had
struct MatArrays {
    const float *points, *albedo, *rough, *fresnel;
    float *out_albedo, *out_rough, *out_fresnel, *out_base, *out_metal;
    int ps, as, rs, fs;
    __device__ __forceinline__ bool load(int64_t i, MatRow& r) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            r.x[c] = points[i * ps + c];
            r.a[c] = albedo[i * as + c];
            r.f[c] = fresnel[i * fs + c];
        }
        r.r = rough[i * rs];
        return true;
    }
    __device__ __forceinline__ void store(int64_t i, const MatRow& r, const MatResult& o) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out_albedo[3 * i + c] = o.touched ? o.albedo[c] : r.a[c];
            out_fresnel[3 * i + c] = o.touched ? o.fresnel[c] : r.f[c];
            if (out_base) out_base[3 * i + c] = o.touched ? o.base[c] : r.a[c];
        }
        out_rough[i] = o.touched ? o.rough : r.r;
        if (out_metal) out_metal[i] = o.touched ? o.metal : 0.f;
    }
};

// the [B][20] map rows of a relight chunk, in place: rows at or below the threshold are not read further, untouched rows not written
struct MatMaps {
    float* maps;
    const float* rays;
    float acc_thres;
    __device__ __forceinline__ bool load(int64_t i, MatRow& r) const {
        const float* mp = maps + i * TIR_MAP_STRIDE;
        if (!(mp[14] > acc_thres)) return false;
        const float* ry = rays + i * 6;
        const float depth = mp[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            r.x[c] = tir::surface_point(ry[c], depth, ry[3 + c]);
            r.a[c] = mp[7 + c];
            r.f[c] = mp[11 + c];
        }
        r.r = mp[10];
        return true;
    }
    __device__ __forceinline__ void store(int64_t i, const MatRow&, const MatResult& o) const {
        if (!o.touched) return;
        float* mp = maps + i * TIR_MAP_STRIDE;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mp[7 + c] = o.albedo[c];
            mp[11 + c] = o.fresnel[c];
        }
        mp[10] = o.rough;
    }
};

template <class Rows>
__global__ void __launch_bounds__(TIR_MATERIAL_THREADS)
k_material_edit(Rows R, const float* __restrict__ edits, int n_edits, const float* __restrict__ palette, int k, float wr, int64_t M,
                const int32_t* __restrict__ m_dev) {
    if (m_dev) M = min(M, (int64_t)max(*m_dev, 0));
    const int64_t i = (int64_t)blockIdx.x * TIR_MATERIAL_THREADS + threadIdx.x;
    if (i >= M) return;
    MatRow r;
    if (!R.load(i, r)) return;
    R.store(i, r, material_row(r, edits, n_edits, palette, k, wr));
}

// ---- B of the orm image ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TIR_MATERIAL_THREADS)
k_orm_metal(uint32_t* __restrict__ orm, int size, int cols, int T, int n_cells, const float* __restrict__ metal) {
    const int32_t px = (int32_t)blockIdx.x * TIR_MATERIAL_THREADS + (int32_t)threadIdx.x;
    if (px >= size * size) return;
    const int y = px / size, x = px - y * size;
    const int cx = x / T, cy = y / T, c = cy * cols + cx;
    if (cx >= cols || c >= n_cells) return;                            // an unowned texel keeps its 0
    const int i = x - cx * T, j = y - cy * T;
    const int64_t t = (int64_t)c * T * T + j * T + i;                  // tir_atlas_texels' cell-major order
    orm[px] = (orm[px] & 0xff00ffffu) | (tir::unorm8(metal[t]) << 16);
}

// ---- k-means ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TIR_MATERIAL_THREADS)
k_kmeans_seed_dist(const float* __restrict__ albedo, const float* __restrict__ rough, int64_t N, float wr,
                   const float* __restrict__ last, int first, float* __restrict__ mind, unsigned long long* __restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * TIR_MATERIAL_THREADS + threadIdx.x;
    unsigned long long key = 0ull;
    if (i < N) {
        const float d = tir::material_dist2(last, albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], tir::mul_rn(wr, rough[i]));
        const float m = first ? d : fminf(mind[i], d);
        mind[i] = m;
        key = ((unsigned long long)__float_as_uint(m) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long other = __shfl_xor(key, s, 64);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0 && key != 0ull) atomicMax(best, key);
}

// centroid `out` = the feature of the row `best` names (row 0 when best is null)
__global__ void k_kmeans_seed_pick(const float* __restrict__ albedo, const float* __restrict__ rough, int64_t N, float wr,
                                   const unsigned long long* __restrict__ best, float* __restrict__ out) {
    int64_t i = best ? (int64_t)(0xFFFFFFFFu - (uint32_t)(*best & 0xFFFFFFFFull)) : 0;
    if (i >= N) i = 0;
    out[0] = albedo[3 * i];
    out[1] = albedo[3 * i + 1];
    out[2] = albedo[3 * i + 2];
    out[3] = tir::mul_rn(wr, rough[i]);
}

__global__ void __launch_bounds__(TIR_MATERIAL_THREADS)
k_kmeans_assign(const float* __restrict__ albedo, const float* __restrict__ rough, int64_t N, float wr,
                const float* __restrict__ cent, int k, int first, int32_t* __restrict__ labels, double* __restrict__ part_sums,
                int32_t* __restrict__ part_counts, int32_t* __restrict__ part_changed) {
    __shared__ float s_val[5][TIR_MATERIAL_THREADS];                   // the four features and d2 of the workgroup's rows
    __shared__ int s_lab[TIR_MATERIAL_THREADS];
    __shared__ int s_chg[TIR_MATERIAL_THREADS / 64];
    const int t = threadIdx.x;
    const int64_t g = blockIdx.x, i = g * TIR_MATERIAL_THREADS + t;
    int lab = -1;
    bool changed = false;
    float f[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < N) {
        f[0] = albedo[3 * i]; f[1] = albedo[3 * i + 1]; f[2] = albedo[3 * i + 2];
        const float r0 = rough[i];
        f[3] = tir::mul_rn(wr, r0);
        lab = tir::material_label(cent, k, wr, f[0], f[1], f[2], r0, f[4]);
        changed = first || labels[i] != lab;
        labels[i] = lab;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) s_val[q][t] = f[q];
    s_lab[t] = lab;
    const unsigned long long mask = __ballot(changed);
    if ((t & 63) == 0) s_chg[t >> 6] = __popcll(mask);
    __syncthreads();
    if (t == 0) {
        int n = 0;
        for (int w = 0; w < TIR_MATERIAL_THREADS / 64; ++w) n += s_chg[w];
        part_changed[g] = n;
    }
    if (t < 5 * k) {                                                   // thread (cluster c, sum q): the rows in row order
        const int c = t / 5, q = t - 5 * c;
        double s = 0.0;
        int n = 0;
        for (int r = 0; r < TIR_MATERIAL_THREADS; ++r)
            if (s_lab[r] == c) { s += (double)s_val[q][r]; ++n; }
        part_sums[(g * k + c) * 5 + q] = s;
        if (q == 0) part_counts[g * k + c] = n;
    }
}

__global__ void __launch_bounds__(TIR_MATERIAL_THREADS)
k_kmeans_update(const double* __restrict__ part_sums, const int32_t* __restrict__ part_counts, const int32_t* __restrict__ part_changed,
                int64_t G, float* __restrict__ cent, int k, int64_t* __restrict__ counts, double* __restrict__ inertia,
                int32_t* __restrict__ changed) {
    __shared__ double s_sum[TIR_MATERIAL_MAX_PALETTE][5];
    __shared__ long long s_cnt[TIR_MATERIAL_MAX_PALETTE];
    __shared__ int s_chg[TIR_MATERIAL_THREADS];
    const int t = threadIdx.x;
    int chg = 0;                                                       // an integer sum: any order gives the same number
    for (int64_t g = t; g < G; g += TIR_MATERIAL_THREADS) chg += part_changed[g];
    s_chg[t] = chg;
    if (t < 5 * k) {                                                   // thread (cluster c, sum q): the partials in workgroup order
        const int c = t / 5, q = t - 5 * c;
        double s = 0.0;
        long long n = 0;
        for (int64_t g = 0; g < G; ++g) {
            s += part_sums[(g * k + c) * 5 + q];
            if (q == 0) n += part_counts[g * k + c];
        }
        s_sum[c][q] = s;
        if (q == 0) s_cnt[c] = n;
    }
    __syncthreads();
    if (t < 4 * k) {
        const int c = t / 4, q = t - 4 * c;
        if (s_cnt[c] > 0) cent[4 * c + q] = (float)(s_sum[c][q] / (double)s_cnt[c]);      // an empty cluster keeps its centroid
    }
    if (t < k) counts[t] = s_cnt[t];
    if (t == 0) {
        double s = 0.0;
        for (int c = 0; c < k; ++c) s += s_sum[c][4];
        *inertia = s;
        int n = 0;
        for (int w = 0; w < TIR_MATERIAL_THREADS; ++w) n += s_chg[w];
        *changed = n;
    }
}

bool mat_finite(float v) { return std::isfinite(v); }

// what both edit entries refuse of the list and the palette
int material_list_ok(const float* edits, int32_t n_edits, const float* palette, int32_t k, float wr) {
    if (n_edits < 0 || n_edits > TIR_MATERIAL_MAX_EDITS || k < 0 || k > TIR_MATERIAL_MAX_PALETTE || !mat_finite(wr)) return TIR_ERR_ARG;
    if ((n_edits > 0 && !edits) || (k > 0 && !palette)) return TIR_ERR_ARG;
    return TIR_OK;
}

int kmeans_ok(int64_t N, int32_t k, float wr) {
    if (N <= 0 || k < 1 || k > TIR_MATERIAL_MAX_PALETTE || !mat_finite(wr)) return TIR_ERR_ARG;
    if (N > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    return TIR_OK;
}

unsigned row_blocks(int64_t n) { return (unsigned)((n + TIR_MATERIAL_THREADS - 1) / TIR_MATERIAL_THREADS); }

}  // namespace

extern "C" int tir_material_edit(const float* edits, int32_t n_edits, const float* palette, int32_t k, float wr, const float* points,
                                 int32_t point_stride, const float* albedo, int32_t albedo_stride, const float* rough,
                                 int32_t rough_stride, const float* fresnel, int32_t fresnel_stride, float* out_albedo,
                                 float* out_rough, float* out_fresnel, float* out_base, float* out_metal, int64_t M,
                                 const int32_t* m_dev, void* stream) {
    if (int rc = material_list_ok(edits, n_edits, palette, k, wr)) return rc;
    if (M < 0 || point_stride < 3 || albedo_stride < 3 || rough_stride < 1 || fresnel_stride < 3) return TIR_ERR_ARG;
    if (M > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    if (M == 0) return TIR_OK;
    if (tir_any_null({points, albedo, rough, fresnel, out_albedo, out_rough, out_fresnel})) return TIR_ERR_ARG;
    const MatArrays R{points, albedo, rough, fresnel, out_albedo, out_rough, out_fresnel, out_base, out_metal,
                      point_stride, albedo_stride, rough_stride, fresnel_stride};
    return tir_launch(k_material_edit<MatArrays>, 0, dim3(row_blocks(M)), dim3(TIR_MATERIAL_THREADS), 0, tir_stream(stream), R, edits,
                      (int)n_edits, palette, (int)k, wr, M, m_dev);
}

extern "C" int tir_material_edit_maps(const float* edits, int32_t n_edits, const float* palette, int32_t k, float wr, float* maps,
                                      const float* rays, int64_t B, float acc_thres, void* stream) {
    if (int rc = material_list_ok(edits, n_edits, palette, k, wr)) return rc;
    if (B < 0 || std::isnan(acc_thres)) return TIR_ERR_ARG;
    if (B > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    if (B == 0) return TIR_OK;
    if (!maps || !rays) return TIR_ERR_ARG;
    if (n_edits == 0) return TIR_OK;
    const MatMaps R{maps, rays, acc_thres};
    return tir_launch(k_material_edit<MatMaps>, 0, dim3(row_blocks(B)), dim3(TIR_MATERIAL_THREADS), 0, tir_stream(stream), R, edits,
                      (int)n_edits, palette, (int)k, wr, B, static_cast<const int32_t*>(nullptr));
}

extern "C" int tir_atlas_metal(uint8_t* orm, int32_t size, int32_t cols, int32_t T, int64_t n_faces, const float* metal,
                               void* stream) {
    if (!orm || n_faces < 0 || size < 6 || cols < 1 || (int64_t)cols * T > size) return TIR_ERR_ARG;
    if (T < 6 || size > 8192) return TIR_ERR_UNSUPPORTED;
    const int64_t n_cells = (n_faces + 1) / 2, rows = (n_cells + cols - 1) / cols;
    if (rows * T > size || ((uintptr_t)orm & 3)) return TIR_ERR_ARG;
    if (n_faces == 0) return TIR_OK;
    if (!metal) return TIR_ERR_ARG;
    return tir_launch(k_orm_metal, 0, dim3(row_blocks((int64_t)size * size)), dim3(TIR_MATERIAL_THREADS), 0, tir_stream(stream),
                      reinterpret_cast<uint32_t*>(orm), (int)size, (int)cols, (int)T, (int)n_cells, metal);
}

extern "C" int64_t tir_kmeans_groups(int64_t N) {
    if (N < 0) return TIR_ERR_ARG;
    if (N > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    return (N + TIR_KMEANS_ROWS - 1) / TIR_KMEANS_ROWS;
}

extern "C" int tir_kmeans_seed(const float* albedo, const float* rough, int64_t N, float wr, float* centroids, int32_t k,
                               int32_t n_have, float* mind, uint64_t* best, void* stream) {
    if (int rc = kmeans_ok(N, k, wr)) return rc;
    if (n_have < 0 || n_have >= k || tir_any_null({albedo, rough, centroids, mind, best}) || ((uintptr_t)best & 7)) return TIR_ERR_ARG;
    hipStream_t st = tir_stream(stream);
    unsigned long long* b = reinterpret_cast<unsigned long long*>(best);
    if (n_have > 0) {
        const hipError_t e = hipMemsetAsync(best, 0, sizeof(uint64_t), st);
        if (e != hipSuccess) return -(int)e;
        if (int rc = tir_launch(k_kmeans_seed_dist, 0, dim3(row_blocks(N)), dim3(TIR_MATERIAL_THREADS), 0, st, albedo, rough, N, wr,
                                static_cast<const float*>(centroids + 4 * (n_have - 1)), (int)(n_have == 1), mind, b))
            return rc;
    }
    return tir_launch(k_kmeans_seed_pick, 0, dim3(1), dim3(1), 0, st, albedo, rough, N, wr,
                      static_cast<const unsigned long long*>(n_have > 0 ? b : nullptr), centroids + 4 * n_have);
}

extern "C" int tir_kmeans_assign(const float* albedo, const float* rough, int64_t N, float wr, const float* centroids, int32_t k,
                                 int32_t first, int32_t* labels, double* part_sums, int32_t* part_counts, int32_t* part_changed,
                                 int64_t n_groups, void* stream) {
    if (int rc = kmeans_ok(N, k, wr)) return rc;
    if (tir_any_null({albedo, rough, centroids, labels, part_sums, part_counts, part_changed}) || n_groups != tir_kmeans_groups(N))
        return TIR_ERR_ARG;
    return tir_launch(k_kmeans_assign, 0, dim3((unsigned)n_groups), dim3(TIR_MATERIAL_THREADS), 0, tir_stream(stream), albedo, rough,
                      N, wr, centroids, (int)k, (int)(first != 0), labels, part_sums, part_counts, part_changed);
}

extern "C" int tir_kmeans_update(const double* part_sums, const int32_t* part_counts, const int32_t* part_changed, int64_t n_groups,
                                 float* centroids, int32_t k, int64_t* counts, double* inertia, int32_t* changed, void* stream) {
    if (k < 1 || k > TIR_MATERIAL_MAX_PALETTE || n_groups < 1 || n_groups > INT32_MAX / TIR_KMEANS_ROWS + 1) return TIR_ERR_ARG;
    if (tir_any_null({part_sums, part_counts, part_changed, centroids, counts, inertia, changed})) return TIR_ERR_ARG;
    return tir_launch(k_kmeans_update, 0, dim3(1), dim3(TIR_MATERIAL_THREADS), 0, tir_stream(stream), part_sums, part_counts,
                      part_changed, n_groups, centroids, (int)k, counts, inertia, changed);
}
