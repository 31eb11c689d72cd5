// Image metrics of the evaluation loop (tensoir_amd/metrics.py; contract: include/tensoir_hip.h, tir_ssim / tir_image_error;
// DESIGN 4.11; restated in numpy by tests/metrics_reference.py).
//
// k_ssim        one workgroup (256 threads) per TIR_SSIM_TILE x TIR_SSIM_TILE tile of the output map of one image pair, all
//               channels.  Both images' tile + halo are staged once in LDS (planar, fp32); per channel a row pass writes the
//               five filtered quantities (x, y, x^2, y^2, x y) as doubles to LDS and a column pass finishes them, applies the
//               formula, optionally writes the map and keeps a per-thread sum.  Nothing intermediate goes to memory.
// k_image_error one pass over two images: pixel count, sum of squared differences, sum of angles in degrees.
// Both end in the same tail: per-workgroup double partials, one ticket per image, and the workgroup that draws the last ticket
// adds that image's partials in index order -- no floating-point atomics; a result depends on nothing but its own image.
#include "tir_common.hpp"

#define TIR_METRIC_THREADS TIR_TAIL_THREADS
static_assert(TIR_SSIM_TILE * TIR_SSIM_TILE == TIR_METRIC_THREADS && TIR_SSIM_TILE == 16, "k_ssim: one output per thread, rows of 16");

namespace {

// ---- the deterministic tail: tir_common.hpp (shared with tir_regularise.hip) ------------------------------------------------------
using tir::block_sum;
using tir::last_of_image;

// partial[i * stride] for i in [0, n) added by thread in strides of the workgroup, four loads in flight per wait, then block_sum
__device__ __forceinline__ double sum_partials(const double* partial, int n, int stride, double* s4) {
    double acc = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * TIR_METRIC_THREADS < n; i += 4 * TIR_METRIC_THREADS) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            v[u] = __hip_atomic_load(partial + (size_t)(i + u * TIR_METRIC_THREADS) * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        acc += (v[0] + v[1]) + (v[2] + v[3]);
    }
    for (; i < n; i += TIR_METRIC_THREADS)
        acc += __hip_atomic_load(partial + (size_t)i * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return block_sum(acc, s4);
}

// ---- SSIM ---------------------------------------------------------------------------------------------------------------------
struct SsimTaps { double w[TIR_SSIM_MAX_TAPS]; };

// One value of the map from the five filtered quantities.  Every step rounded on its own, in the reference's order (utils.py:120-137):
// a fused e00 - m0 * m0 would not be the difference of the two rounded numbers the reference subtracts.
__device__ __forceinline__ double ssim_value(double m0, double m1, double e00, double e11, double e01, double c1, double c2) {
#pragma clang fp contract(off)
    const double mu00 = m0 * m0, mu11 = m1 * m1, mu01 = m0 * m1;
    const double s00 = fmax(0.0, e00 - mu00), s11 = fmax(0.0, e11 - mu11);
    double s01 = e01 - mu01;
    const double sgn = (double)((s01 > 0.0) - (s01 < 0.0));
    s01 = sgn * fmin(sqrt(s00 * s11), fabs(s01));
    const double numer = (2.0 * mu01 + c1) * (2.0 * s01 + c2);
    const double denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
    return numer / denom;
}

__global__ void __launch_bounds__(TIR_METRIC_THREADS)
k_ssim(const float* __restrict__ img0, const float* __restrict__ img1, int H, int W, int C, int n, SsimTaps taps, double c1, double c2,
       double* __restrict__ map, double* __restrict__ partial, int32_t* __restrict__ ticket, double* __restrict__ mean, int tiles_x,
       int tiles) {
    constexpr int T = TIR_SSIM_TILE;
    extern __shared__ double s_dyn[];
    __shared__ double s_taps[TIR_SSIM_MAX_TAPS + 1];
    __shared__ double s4[4];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
    const int oy0 = (tile / tiles_x) * T, ox0 = (tile % tiles_x) * T;
    const int TH = T + n - 1, TW = TH, OH = H - n + 1, OW = W - n + 1;
    double* inter = s_dyn;                                        // [5][TH][T]
    float* in = reinterpret_cast<float*>(inter + 5 * TH * T);     // [2][C][TH][TW]
    if (tid < n) s_taps[tid] = taps.w[tid];

    // stage: the tile's rows are contiguous runs of TW * C floats in memory; consecutive threads take consecutive floats of both
    // images (the two loads are independent and leave together), and scatter them to the planar image.  Outside the image: 0,
    // read only by outputs that are not written.
    const int run = TW * C, total = TH * run, plane = TH * TW;
    const size_t base = (size_t)img * H * W * C;
    for (int e0 = tid; e0 < total; e0 += 4 * TIR_METRIC_THREADS) {
        float v0[4], v1[4];
        int dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * TIR_METRIC_THREADS;
            const int r = e / run, j = e - r * run, x = j / C, ch = j - x * C;
            const int gy = oy0 + r, gx = ox0 + x;
            const bool ok = e < total && gy < H && gx < W;
            const size_t off = base + ((size_t)gy * W + gx) * C + ch;
            v0[u] = ok ? img0[off] : 0.0f;
            v1[u] = ok ? img1[off] : 0.0f;
            dst[u] = e < total ? (ch * TH + r) * TW + x : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (dst[u] >= 0) { in[dst[u]] = v0[u]; in[C * plane + dst[u]] = v1[u]; }
    }
    __syncthreads();

    const int oy = tid >> 4, ox = tid & 15;                       // this thread's output of the tile (T = 16: 256 outputs)
    const bool inside = oy0 + oy < OH && ox0 + ox < OW;
    double acc = 0.0;
    for (int ch = 0; ch < C; ++ch) {
        // row pass: (row r of the tile + halo, output column c) -> the five sums over the n taps to the right.  The three products
        // are fp32 multiplies rounded on their own (the reference squares fp32 images in fp32); all sums are double.
        for (int i = tid; i < TH * T; i += TIR_METRIC_THREADS) {
            const int r = i >> 4, c = i & 15;
            const float* p0 = in + (ch * TH + r) * TW + c;
            const float* p1 = p0 + C * plane;
            double a0 = 0.0, a1 = 0.0, a00 = 0.0, a11 = 0.0, a01 = 0.0;
            for (int k = 0; k < n; ++k) {
                const float x = p0[k], y = p1[k];
                const double w = s_taps[k];
                a0 += w * (double)x;
                a1 += w * (double)y;
                a00 += w * (double)tir::mul_rn(x, x);
                a11 += w * (double)tir::mul_rn(y, y);
                a01 += w * (double)tir::mul_rn(x, y);
            }
            double* o = inter + r * T + c;
            o[0] = a0; o[TH * T] = a1; o[2 * TH * T] = a00; o[3 * TH * T] = a11; o[4 * TH * T] = a01;
        }
        __syncthreads();
        // column pass: rows of 16 doubles, a wave reads four whole rows per tap (512 contiguous bytes: no bank is hit twice)
        double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        const double* p = inter + oy * T + ox;
        for (int k = 0; k < n; ++k) {
            const double w = s_taps[k];
#pragma unroll
            for (int s = 0; s < 5; ++s) q[s] += w * p[(s * TH + k) * T];
        }
        if (inside) {
            const double v = ssim_value(q[0], q[1], q[2], q[3], q[4], c1, c2);
            if (map) map[(((size_t)img * OH + (oy0 + oy)) * OW + (ox0 + ox)) * C + ch] = v;
            acc += v;
        }
        __syncthreads();                                          // the next channel's row pass overwrites inter
    }

    const double sum = block_sum(acc, s4);
    if (tid == 0) __hip_atomic_store(partial + blockIdx.x, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!last_of_image(ticket + img, tiles, &s_last)) return;
    const double all = sum_partials(partial + (size_t)img * tiles, tiles, 1, s4);
    if (tid == 0) mean[img] = all / ((double)OH * (double)OW * (double)C);
}

static inline int64_t ssim_tiles(int32_t H, int32_t W, int32_t n, int64_t* tiles_x) {
    const int64_t tx = ((int64_t)W - n + TIR_SSIM_TILE) / TIR_SSIM_TILE, ty = ((int64_t)H - n + TIR_SSIM_TILE) / TIR_SSIM_TILE;
    if (tiles_x) *tiles_x = tx;
    return tx * ty;
}

static inline bool ssim_shape_ok(int64_t N, int32_t H, int32_t W, int32_t n) {
    return N >= 0 && H >= 1 && W >= 1 && n >= 1 && n <= TIR_SSIM_MAX_TAPS && n <= H && n <= W;
}

// ---- PSNR / angular error -----------------------------------------------------------------------------------------------------
// the angle between two stored vectors, in degrees: the products of fp32 values are exact in double, the two additions round in
// the order of a plain sum over the last axis
__device__ __forceinline__ double angle_deg(const float* a, const float* b) {
#pragma clang fp contract(off)
    const double d = ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
    return acos(fmin(fmax(d, -1.0), 1.0)) * 180.0 / 3.14159265358979323846;
}

template <int C>
__global__ void __launch_bounds__(TIR_METRIC_THREADS)
k_image_error(const float* __restrict__ a, const float* __restrict__ b, const uint8_t* __restrict__ mask, int64_t P, int angular,
              double* __restrict__ partial, int32_t* __restrict__ ticket, double* __restrict__ out, int groups) {
    __shared__ double s4[4];
    __shared__ int s_last;
    const int img = blockIdx.x / groups, g = blockIdx.x - img * groups;
    const float* pa = a + (size_t)img * P * C;
    const float* pb = b + (size_t)img * P * C;
    const uint8_t* pm = mask ? mask + (size_t)img * P : nullptr;
    double cnt = 0.0, sq = 0.0, ang = 0.0;
    for (int64_t p = (int64_t)g * TIR_METRIC_THREADS + threadIdx.x; p < P; p += (int64_t)groups * TIR_METRIC_THREADS) {
        float va[C], vb[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { va[c] = pa[p * C + c]; vb[c] = pb[p * C + c]; }
        if (pm && pm[p] == 0) continue;
        cnt += 1.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double d = (double)va[c] - (double)vb[c];
            sq += d * d;
        }
        if (C == 3 && angular) ang += angle_deg(va, vb);
    }
    const double sums[3] = {block_sum(cnt, s4), block_sum(sq, s4), block_sum(ang, s4)};
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k)
            __hip_atomic_store(partial + (size_t)blockIdx.x * 3 + k, sums[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!last_of_image(ticket + img, groups, &s_last)) return;
    for (int k = 0; k < 3; ++k) {
        const double all = sum_partials(partial + (size_t)img * groups * 3 + k, groups, 3, s4);
        if (threadIdx.x == 0) out[(size_t)img * 3 + k] = all;
    }
}

static inline int64_t image_error_groups(int64_t P) {
    int64_t g = (P + TIR_IMAGE_ERROR_SHARE - 1) / TIR_IMAGE_ERROR_SHARE;
    return g < 1 ? 1 : (g > 256 ? 256 : g);
}

// the tickets of N images behind `doubles` partials of a workspace, as a count of doubles
static inline int64_t with_tickets(int64_t doubles, int64_t N) { return doubles + (N + 1) / 2; }

}  // namespace

extern "C" int64_t tir_ssim_workspace(int64_t N, int32_t H, int32_t W, int32_t C, int32_t n_taps) {
    if (!ssim_shape_ok(N, H, W, n_taps)) return TIR_ERR_ARG;
    if (C < 1 || C > 4) return TIR_ERR_UNSUPPORTED;
    return with_tickets(N * ssim_tiles(H, W, n_taps, nullptr), N);
}

extern "C" int tir_ssim(const float* img0, const float* img1, int64_t N, int32_t H, int32_t W, int32_t C, const double* taps,
                        int32_t n_taps, double c1, double c2, double* map, double* workspace, double* mean, void* stream) {
    if (!ssim_shape_ok(N, H, W, n_taps)) return TIR_ERR_ARG;
    if (C < 1 || C > 4) return TIR_ERR_UNSUPPORTED;
    if (N == 0) return TIR_OK;
    if (tir_any_null({img0, img1, taps, workspace, mean})) return TIR_ERR_ARG;
    int64_t tiles_x = 0;
    const int64_t tiles = ssim_tiles(H, W, n_taps, &tiles_x);
    if (N * tiles >= ((int64_t)1 << 31) || tiles >= (1 << 30)) return TIR_ERR_UNSUPPORTED;
    SsimTaps t{};
    for (int k = 0; k < n_taps; ++k) t.w[k] = taps[k];
    const int TH = TIR_SSIM_TILE + n_taps - 1;
    const size_t lds = (size_t)5 * TH * TIR_SSIM_TILE * sizeof(double) + (size_t)2 * C * TH * TH * sizeof(float);
    int32_t* ticket = reinterpret_cast<int32_t*>(workspace + N * tiles);
    hipStream_t s = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(ticket, 0, (size_t)N * sizeof(int32_t), s);      // armed here: a caller's buffer may hold anything
    if (e != hipSuccess) return -(int)e;
    // the dynamic-LDS limit is raised once per device: to what 31 taps of 4 channels need (95 KiB), whatever this call needs
    constexpr int TH_MAX = TIR_SSIM_TILE + TIR_SSIM_MAX_TAPS - 1;
    constexpr int LDS_LIMIT = 5 * TH_MAX * TIR_SSIM_TILE * (int)sizeof(double) + 2 * 4 * TH_MAX * TH_MAX * (int)sizeof(float);
    return tir_launch(k_ssim, LDS_LIMIT, dim3((unsigned)(N * tiles)), dim3(TIR_METRIC_THREADS), lds, s, img0, img1, (int)H, (int)W,
                      (int)C, (int)n_taps, t, c1, c2, map, workspace, ticket, mean, (int)tiles_x, (int)tiles);
}

extern "C" int64_t tir_image_error_workspace(int64_t N, int64_t P) {
    if (N < 0 || P < 0) return TIR_ERR_ARG;
    return with_tickets(N * image_error_groups(P) * 3, N);
}

extern "C" int tir_image_error(const float* a, const float* b, const uint8_t* mask, int64_t N, int64_t P, int32_t C, int32_t angular,
                               double* workspace, double* out, void* stream) {
    if (N < 0 || P < 0) return TIR_ERR_ARG;
    if (C < 1 || C > 4) return TIR_ERR_UNSUPPORTED;
    if (N == 0) return TIR_OK;
    if (tir_any_null({workspace, out}) || (P > 0 && tir_any_null({a, b}))) return TIR_ERR_ARG;
    const int64_t groups = image_error_groups(P);
    if (N * groups >= ((int64_t)1 << 31)) return TIR_ERR_UNSUPPORTED;
    int32_t* ticket = reinterpret_cast<int32_t*>(workspace + N * groups * 3);
    hipStream_t s = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(ticket, 0, (size_t)N * sizeof(int32_t), s);
    if (e != hipSuccess) return -(int)e;
    const dim3 grid((unsigned)(N * groups)), block(TIR_METRIC_THREADS);
    const int ang = angular != 0;
    switch (C) {
        case 1: return tir_launch(k_image_error<1>, 0, grid, block, 0, s, a, b, mask, P, ang, workspace, ticket, out, (int)groups);
        case 2: return tir_launch(k_image_error<2>, 0, grid, block, 0, s, a, b, mask, P, ang, workspace, ticket, out, (int)groups);
        case 3: return tir_launch(k_image_error<3>, 0, grid, block, 0, s, a, b, mask, P, ang, workspace, ticket, out, (int)groups);
        default: return tir_launch(k_image_error<4>, 0, grid, block, 0, s, a, b, mask, P, ang, workspace, ticket, out, (int)groups);
    }
}
