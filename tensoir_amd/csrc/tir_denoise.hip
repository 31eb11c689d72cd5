// Guided a-trous denoiser of relit views (tensoir_amd/denoise.py; contract: include/tensoir_hip.h, tir_denoise_guide /
// tir_atrous_level; restated in float64 by tests/denoise_reference.py).
//
// k_denoise_guide  one thread per ray of a chunk: the twelve guide floats of its pixel from the primary pass's map row and the ray,
//                  written as three 16-byte stores.
// k_atrous_level   one level of the edge-avoiding filter, out of place.  A workgroup (256 threads) owns a 32 x 8 tile of the image,
//                  a thread one pixel: its guide row and its colours stay in registers, the 25 taps are read with plain cached
//                  loads (a tap's 48-byte guide row as three 16-byte loads, its colours as dwords) in the fixed order rows, then
//                  columns, and accumulated with one fused multiply-add per channel -- an order that depends on nothing but the
//                  pixel.  The weighted mean is formed as c_p + sum w (c_q - c_p) / sum w: a pixel with no valid neighbour and a
//                  constant image come out as they went in, to the bit.  A tap outside the image is read at the pixel itself and
//                  dropped.  Instantiated per number of maps (K / 3) and for the colour term on / off; with the colour term off
//                  the weight is shared by the maps (the same bits: |c_p - c_q|^2 * 0 adds nothing to the exponent).  Every
//                  map's arithmetic is written per map, so what a map gets is what a call with that map alone gives.  No LDS,
//                  no atomics.
#include "tir_common.hpp"

#include <cmath>

#define TIR_DENOISE_THREADS 256
#define TIR_ATROUS_TILE_W 32
#define TIR_ATROUS_TILE_H 8
static_assert(TIR_ATROUS_TILE_W * TIR_ATROUS_TILE_H == TIR_DENOISE_THREADS, "one thread per pixel of a tile");
static_assert(TIR_DENOISE_GUIDE == 12 && TIR_ATROUS_MAX_K == 24, "three 16-byte loads per guide row; instantiations for 1..8 maps");

namespace {

// ---- the guide ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TIR_DENOISE_THREADS)
k_denoise_guide(const float* __restrict__ maps, const float* __restrict__ rays, int64_t n, float acc_thres, float* __restrict__ guide) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * TIR_DENOISE_THREADS + threadIdx.x;
    if (r >= n) return;
    const float* m = maps + r * 20;
    const float* ry = rays + r * 6;
    const float depth = m[3], nx = m[4], ny = m[5], nz = m[6];
    // o + depth d with one rounding per component
    const float px = fmaf(depth, ry[3], ry[0]), py = fmaf(depth, ry[4], ry[1]), pz = fmaf(depth, ry[5], ry[2]);
    const float len = fmaxf(sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx))), 1e-6f);
    float4* g = reinterpret_cast<float4*>(guide + r * TIR_DENOISE_GUIDE);
    g[0] = make_float4(px, py, pz, m[14] > acc_thres ? 1.f : 0.f);
    g[1] = make_float4(nx / len, ny / len, nz / len, m[10]);
    g[2] = make_float4(m[7], m[8], m[9], 0.f);
}

// ---- one level ------------------------------------------------------------------------------------------------------------------
struct AtrousArgs {
    int H, W, step, tiles_x;
    float inv_sn, inv_sp, inv_sa2, inv_sr2, inv_sc2;
};

// k[|i|] of the B3 spline (3/8, 1/4, 1/16) without an indexed table
__device__ __forceinline__ float atrous_tap(int i) { return i == 0 ? 0.375f : ((i == 1 || i == -1) ? 0.25f : 0.0625f); }

template <int NM, bool COLOUR>
__global__ void __launch_bounds__(TIR_DENOISE_THREADS)
k_atrous_level(const float* __restrict__ cin, float* __restrict__ cout, const float* __restrict__ guide, AtrousArgs a) {
#pragma clang fp contract(off)
    constexpr int K = 3 * NM;
    const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
    const int x = tile_x * TIR_ATROUS_TILE_W + (int)(threadIdx.x % TIR_ATROUS_TILE_W);
    const int y = tile_y * TIR_ATROUS_TILE_H + (int)(threadIdx.x / TIR_ATROUS_TILE_W);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float4* gp = reinterpret_cast<const float4*>(guide + p * TIR_DENOISE_GUIDE);
    const float4 g0 = gp[0], g1 = gp[1], g2 = gp[2];
    float cp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cp[k] = cin[p * K + k];
    if (!(g0.w > 0.5f)) {                                          // an invalid pixel copies its input
#pragma unroll
        for (int k = 0; k < K; ++k) cout[p * K + k] = cp[k];
        return;
    }
    float sw[NM], sc[K];
#pragma unroll
    for (int m = 0; m < NM; ++m) sw[m] = 0.140625f;                 // the centre tap: h = 9/64, every difference 0
#pragma unroll
    for (int k = 0; k < K; ++k) sc[k] = 0.f;
#pragma unroll 1
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * a.step;                              // < 2^31: the host bounds H, W and the step
        const float hj = atrous_tap(j);
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            if (i == 0 && j == 0) continue;
            const int qx = x + i * a.step;
            const bool inside = qx >= 0 && qx < a.W && qy >= 0 && qy < a.H;
            const size_t q = inside ? (size_t)qy * (size_t)a.W + (size_t)qx : p;
            const float4* gq = reinterpret_cast<const float4*>(guide + q * TIR_DENOISE_GUIDE);
            const float4 q0 = gq[0], q1 = gq[1], q2 = gq[2];
            float cq[K];
#pragma unroll
            for (int k = 0; k < K; ++k) cq[k] = cin[q * K + k];
            if (!(inside && q0.w > 0.5f)) continue;
            const float h = hj * atrous_tap(i);                     // exact: 9, 6, 4, 3/2, 1, 1/4 over 64
            const float ndot = fmaf(g1.z, q1.z, fmaf(g1.y, q1.y, g1.x * q1.x));
            const float dx = q0.x - g0.x, dy = q0.y - g0.y, dz = q0.z - g0.z;
            const float plane = fabsf(fmaf(dz, g1.z, fmaf(dy, g1.y, dx * g1.x)));
            const float ax = g2.x - q2.x, ay = g2.y - q2.y, az = g2.z - q2.z;
            const float alb2 = fmaf(az, az, fmaf(ay, ay, ax * ax));
            const float dr = g1.w - q1.w;
            float e = fmaxf(0.f, 1.f - ndot) * a.inv_sn;
            e = fmaf(plane, a.inv_sp, e);
            e = fmaf(alb2, a.inv_sa2, e);
            e = fmaf(dr * dr, a.inv_sr2, e);
            if (COLOUR) {
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    const float c0 = cp[3 * m] - cq[3 * m], c1 = cp[3 * m + 1] - cq[3 * m + 1], c2 = cp[3 * m + 2] - cq[3 * m + 2];
                    const float d2 = fmaf(c2, c2, fmaf(c1, c1, c0 * c0));
                    const float w = h * expf(-fmaf(d2, a.inv_sc2, e));
                    sw[m] += w;
#pragma unroll
                    for (int c = 0; c < 3; ++c) sc[3 * m + c] = fmaf(w, cq[3 * m + c] - cp[3 * m + c], sc[3 * m + c]);
                }
            } else {
                const float w = h * expf(-e);
                sw[0] += w;
#pragma unroll
                for (int k = 0; k < K; ++k) sc[k] = fmaf(w, cq[k] - cp[k], sc[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) cout[p * K + k] = cp[k] + sc[k] / sw[COLOUR ? k / 3 : 0];
}

template <int NM>
static inline int atrous_launch(bool colour, dim3 grid, hipStream_t s, const float* cin, float* cout, const float* guide, const AtrousArgs& a) {
    if (colour) return tir_launch(k_atrous_level<NM, true>, 0, grid, dim3(TIR_DENOISE_THREADS), 0, s, cin, cout, guide, a);
    return tir_launch(k_atrous_level<NM, false>, 0, grid, dim3(TIR_DENOISE_THREADS), 0, s, cin, cout, guide, a);
}

static inline bool sigma_ok(float v) { return std::isfinite(v) && v >= 0.f; }

}  // namespace

extern "C" int tir_denoise_guide(const float* maps, const float* rays, int64_t n, float acc_thres, float* guide, int64_t row0, void* stream) {
    if (n < 0 || row0 < 0) return TIR_ERR_ARG;
    if (n == 0) return TIR_OK;
    if (tir_any_null({maps, rays, guide}) || !tir_aligned16({guide})) return TIR_ERR_ARG;
    const int64_t groups = (n + TIR_DENOISE_THREADS - 1) / TIR_DENOISE_THREADS;
    if (groups >= ((int64_t)1 << 31) || row0 > INT64_MAX / (4 * TIR_DENOISE_GUIDE) - n) return TIR_ERR_UNSUPPORTED;
    return tir_launch(k_denoise_guide, 0, dim3((unsigned)groups), dim3(TIR_DENOISE_THREADS), 0, tir_stream(stream), maps, rays, n, acc_thres,
                      guide + row0 * TIR_DENOISE_GUIDE);
}

extern "C" int tir_atrous_level(const float* color_in, float* color_out, const float* guide, int32_t H, int32_t W, int32_t K, int32_t step,
                                float inv_sn, float inv_sp, float inv_sa2, float inv_sr2, float inv_sc2, void* stream) {
    if (H < 1 || W < 1 || step < 1) return TIR_ERR_ARG;
    if (K < 3 || K > TIR_ATROUS_MAX_K || K % 3 != 0) return TIR_ERR_ARG;
    if (!sigma_ok(inv_sn) || !sigma_ok(inv_sp) || !sigma_ok(inv_sa2) || !sigma_ok(inv_sr2) || !sigma_ok(inv_sc2)) return TIR_ERR_ARG;
    if (tir_any_null({color_in, color_out, guide}) || color_in == color_out || !tir_aligned16({guide})) return TIR_ERR_ARG;
    // pixel indices and tap coordinates are 32-bit: x + 2 step stays below 2^31 once the step is cut to the image's longer side
    // (a larger step leaves the centre tap alone, whatever it is)
    const int side = H > W ? H : W;
    if (side >= (1 << 29) || (int64_t)H * W >= ((int64_t)1 << 31)) return TIR_ERR_UNSUPPORTED;
    const int64_t tiles_x = (W + TIR_ATROUS_TILE_W - 1) / TIR_ATROUS_TILE_W, tiles_y = (H + TIR_ATROUS_TILE_H - 1) / TIR_ATROUS_TILE_H;
    if (tiles_x * tiles_y >= ((int64_t)1 << 31)) return TIR_ERR_UNSUPPORTED;
    const AtrousArgs a{H, W, step < side ? step : side, (int)tiles_x, inv_sn, inv_sp, inv_sa2, inv_sr2, inv_sc2};
    const dim3 grid((unsigned)(tiles_x * tiles_y));
    hipStream_t s = tir_stream(stream);
    const bool colour = inv_sc2 > 0.f;
    switch (K / 3) {
        case 1: return atrous_launch<1>(colour, grid, s, color_in, color_out, guide, a);
        case 2: return atrous_launch<2>(colour, grid, s, color_in, color_out, guide, a);
        case 3: return atrous_launch<3>(colour, grid, s, color_in, color_out, guide, a);
        case 4: return atrous_launch<4>(colour, grid, s, color_in, color_out, guide, a);
        case 5: return atrous_launch<5>(colour, grid, s, color_in, color_out, guide, a);
        case 6: return atrous_launch<6>(colour, grid, s, color_in, color_out, guide, a);
        case 7: return atrous_launch<7>(colour, grid, s, color_in, color_out, guide, a);
        default: return atrous_launch<8>(colour, grid, s, color_in, color_out, guide, a);
    }
}
