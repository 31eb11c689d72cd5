// Deterministic z-buffer rasteriser of the exported mesh (tensoir_amd/raster.py; contract: include/tensoir_hip.h, tir_raster_*;
// DESIGN 4.8).  Four stages, each one entry:
//   k_raster_project      one thread per corner: camera transform, perspective divide, snap to 1/256 pixel, the face's drop flags
//   k_raster_cover_small  one thread per face: faces whose box of pixel centres holds at most RASTER_SMALL pixels are walked by
//                         their thread; the others are appended to a list
//   k_raster_cover_big    one workgroup per listed face walks the face's box, 256 pixels at a time
//   k_raster_resolve      one thread per pixel: the winning face's perspective-correct barycentrics and camera depth
//   k_raster_shade        one thread per pixel: interpolated attributes, three bilinear RGBA8 lookups, the tangent-space normal
//   k_shadow_maps_*       the same coverage and depth once per light cell, orthographic: one 32-bit z-buffer per cell (tir_shadow_maps,
//                         DESIGN 4.10); k_shadow_lookup reads them back per (point, cell) pair (tir_shadow_lookup)
// Coverage is int64 arithmetic on the snapped corners and the depth test one 64-bit unsigned atomic max per fragment of a key
// (depth bits, inverted face index): neither depends on the order fragments arrive in, so every output repeats bit for bit.
// Every fp32 step of project / cover / resolve is rounded on its own (tir::mul_rn & co.: the numpy restatement's float32 mode
// forms the same numbers); shade is ordinary fp32 with a tolerance.
#include "tir_common.hpp"

namespace {

constexpr int RASTER_THREADS = 256;
constexpr int RASTER_PROJ_THREADS = 192;                 // 64 faces: the three corners of a face always share a block
constexpr int RASTER_GUARD = TIR_RASTER_GUARD * 256;     // largest |snapped coordinate|
constexpr int RASTER_SMALL = 64;                         // a face with more pixel centres in its box goes to the workgroup pass
constexpr int RASTER_BIG_BLOCKS = 1024;

struct RasterCam {
    float r[3][3], o[3];                                 // c2w = [r | o]
    float f, cx, cy, near_;
};

using tir::add_rn;
using tir::mul_rn;
using tir::sub_rn;

__global__ void __launch_bounds__(RASTER_PROJ_THREADS)
k_raster_project(const float* __restrict__ pos, const int32_t* __restrict__ faces, RasterCam C, int64_t n_verts, int64_t n_faces,
                 int4* __restrict__ rows, int32_t* __restrict__ status) {
    __shared__ int s_flags[RASTER_PROJ_THREADS];
    const int64_t q = (int64_t)blockIdx.x * RASTER_PROJ_THREADS + threadIdx.x;
    const bool live = q < 3 * n_faces;
    int flags = 0, sx = 0, sy = 0, k = 0;
    float invz = 0.f;
    if (live) {
        const int64_t f = q / 3;
        k = (int)(q - 3 * f);
        int64_t v = q;
        if (faces) {                                     // all three indices are tested before any vertex of the face is read
            const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
            if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_verts || i1 >= n_verts || i2 >= n_verts) flags = TIR_RASTER_DROP_INDEX;
            v = k == 0 ? i0 : (k == 1 ? i1 : i2);
        }
        if (!flags) {
            const float d0 = sub_rn(pos[3 * v], C.o[0]), d1 = sub_rn(pos[3 * v + 1], C.o[1]), d2 = sub_rn(pos[3 * v + 2], C.o[2]);
            const float X = add_rn(add_rn(mul_rn(C.r[0][0], d0), mul_rn(C.r[1][0], d1)), mul_rn(C.r[2][0], d2));
            const float Y = add_rn(add_rn(mul_rn(C.r[0][1], d0), mul_rn(C.r[1][1], d1)), mul_rn(C.r[2][1], d2));
            const float Z = add_rn(add_rn(mul_rn(C.r[0][2], d0), mul_rn(C.r[1][2], d1)), mul_rn(C.r[2][2], d2));
            if (!(isfinite(X) && isfinite(Y) && isfinite(Z))) {
                flags = TIR_RASTER_DROP_NONFINITE;
            } else if (Z <= C.near_) {
                flags = TIR_RASTER_DROP_NEAR;
            } else {
                const float x = rintf(mul_rn(add_rn(__fdiv_rn(mul_rn(C.f, X), Z), C.cx), 256.f));
                const float y = rintf(mul_rn(add_rn(__fdiv_rn(mul_rn(C.f, Y), Z), C.cy), 256.f));
                if (!(fabsf(x) <= (float)RASTER_GUARD) || !(fabsf(y) <= (float)RASTER_GUARD)) {
                    flags = TIR_RASTER_DROP_GUARD;
                } else {
                    sx = (int)x;
                    sy = (int)y;
                    invz = __fdiv_rn(1.f, Z);
                }
            }
        }
    }
    s_flags[threadIdx.x] = flags;
    __syncthreads();
    if (!live) return;
    const int b = (int)threadIdx.x - k;
    const int all = s_flags[b] | s_flags[b + 1] | s_flags[b + 2];
    if (all) { sx = 0; sy = 0; invz = 0.f; }
    if (k == 0 && all) {                                 // one count per dropped face, under the first reason that applies
        const int slot = (all & TIR_RASTER_DROP_INDEX) ? 0 : (all & TIR_RASTER_DROP_NONFINITE) ? 3 : (all & TIR_RASTER_DROP_NEAR) ? 1 : 2;
        atomicAdd(status + slot, 1);
    }
    rows[q] = make_int4(sx, sy, __float_as_int(invz), all);
}

// A face ready for coverage, in the orientation that makes its doubled area positive: e_k(p) >= 0 inside.
struct RasterFace {
    int x0, y0, x1, y1, x2, y2;
    float w0, w1, w2, area;
    int n;                                               // +1, or -1 when the stored order has a negative doubled area
    int bias0, bias1, bias2;                             // 0 when the edge owns its zero set (top or left), else 1
};

__device__ __forceinline__ int raster_bias(int n, int dx, int dy) {
    dx *= n;
    dy *= n;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
}

// the snapped corners and their depths are in T -> the doubled area's sign (0: no area), orientation, |A| and edge ownership
__device__ __forceinline__ int raster_setup(RasterFace& T) {
    const int64_t A = (int64_t)(T.x1 - T.x0) * (T.y2 - T.y0) - (int64_t)(T.x2 - T.x0) * (T.y1 - T.y0);
    if (A == 0) return 0;
    T.n = A < 0 ? -1 : 1;
    T.area = __ll2float_rn(A < 0 ? -A : A);
    T.bias0 = raster_bias(T.n, T.x2 - T.x1, T.y2 - T.y1);         // edge 0: v1 -> v2, opposite corner 0
    T.bias1 = raster_bias(T.n, T.x0 - T.x2, T.y0 - T.y2);
    T.bias2 = raster_bias(T.n, T.x1 - T.x0, T.y1 - T.y0);
    return T.n;
}

// -> the doubled area's sign (0: nothing to draw, the face is flagged or has no area)
__device__ __forceinline__ int raster_load(const int4* __restrict__ rows, int64_t f, RasterFace& T) {
    const int4 a = rows[3 * f], b = rows[3 * f + 1], c = rows[3 * f + 2];
    if (a.w | b.w | c.w) return 0;
    T.x0 = a.x; T.y0 = a.y; T.x1 = b.x; T.y1 = b.y; T.x2 = c.x; T.y2 = c.y;
    T.w0 = __int_as_float(a.z); T.w1 = __int_as_float(b.z); T.w2 = __int_as_float(c.z);
    return raster_setup(T);
}

// the three edge functions at the centre of pixel (i, j), oriented; -> inside (top-left rule)
__device__ __forceinline__ bool raster_edges(const RasterFace& T, int i, int j, int64_t& e0, int64_t& e1, int64_t& e2) {
    const int px = 256 * i + 128, py = 256 * j + 128;
    const int ax = T.x0 - px, ay = T.y0 - py, bx = T.x1 - px, by = T.y1 - py, cx = T.x2 - px, cy = T.y2 - py;   // |.| < 2^23
    e0 = ((int64_t)bx * cy - (int64_t)cx * by) * T.n;
    e1 = ((int64_t)cx * ay - (int64_t)ax * cy) * T.n;
    e2 = ((int64_t)ax * by - (int64_t)bx * ay) * T.n;
    return e0 >= T.bias0 && e1 >= T.bias1 && e2 >= T.bias2;
}

__device__ __forceinline__ void raster_terms(const RasterFace& T, int64_t e0, int64_t e1, int64_t e2, float& t0, float& t1, float& t2,
                                             float& s) {
    t0 = mul_rn(__ll2float_rn(e0), T.w0);
    t1 = mul_rn(__ll2float_rn(e1), T.w1);
    t2 = mul_rn(__ll2float_rn(e2), T.w2);
    s = add_rn(add_rn(t0, t1), t2);
}

__device__ __forceinline__ void raster_fragment(const RasterFace& T, int i, int j, int W, unsigned low,
                                                unsigned long long* __restrict__ keys) {
    int64_t e0, e1, e2;
    if (!raster_edges(T, i, j, e0, e1, e2)) return;
    float t0, t1, t2, s;
    raster_terms(T, e0, e1, e2, t0, t1, t2, s);
    const float invz = __fdiv_rn(s, T.area);                       // > 0: its bits order as unsigned integers
    const unsigned long long key = ((unsigned long long)__float_as_uint(invz) << 32) | low;
    unsigned long long* p = keys + (int64_t)j * W + i;
    if (*p < key) atomicMax(p, key);                               // the key only grows: a stale read costs an atomic, never a fragment
}

// the pixels whose centres lie in the face's box, clipped to the image -> false when there is none
__device__ __forceinline__ bool raster_box(const RasterFace& T, int W, int H, int& i0, int& i1, int& j0, int& j1) {
    const int xmin = min(T.x0, min(T.x1, T.x2)), xmax = max(T.x0, max(T.x1, T.x2));
    const int ymin = min(T.y0, min(T.y1, T.y2)), ymax = max(T.y0, max(T.y1, T.y2));
    i0 = max((xmin + 127) >> 8, 0);                                // ceil((xmin - 128) / 256)
    i1 = min((xmax - 128) >> 8, W - 1);                            // floor
    j0 = max((ymin + 127) >> 8, 0);
    j1 = min((ymax - 128) >> 8, H - 1);
    return i0 <= i1 && j0 <= j1;
}

__global__ void __launch_bounds__(RASTER_THREADS)
k_raster_cover_small(const int4* __restrict__ rows, int64_t n_faces, int W, int H, int cull, unsigned long long* __restrict__ keys,
                     int32_t* __restrict__ work) {
    const int64_t f = (int64_t)blockIdx.x * RASTER_THREADS + threadIdx.x;
    if (f >= n_faces) return;
    RasterFace T;
    const int sign = raster_load(rows, f, T);
    if (sign == 0 || (cull && sign > 0)) return;
    int i0, i1, j0, j1;
    if (!raster_box(T, W, H, i0, i1, j0, j1)) return;
    if ((int64_t)(i1 - i0 + 1) * (j1 - j0 + 1) > RASTER_SMALL) {
        work[1 + atomicAdd(work, 1)] = (int32_t)f;                 // any order: the max is commutative
        return;
    }
    const unsigned low = 0xFFFFFFFFu - (unsigned)f;
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) raster_fragment(T, i, j, W, low, keys);
}

__global__ void __launch_bounds__(RASTER_THREADS)
k_raster_cover_big(const int4* __restrict__ rows, int W, int H, unsigned long long* __restrict__ keys,
                   const int32_t* __restrict__ work) {
    const int n = work[0];
    for (int b = (int)blockIdx.x; b < n; b += (int)gridDim.x) {
        const int64_t f = work[1 + b];
        RasterFace T;
        int i0, i1, j0, j1;
        if (raster_load(rows, f, T) == 0 || !raster_box(T, W, H, i0, i1, j0, j1)) continue;     // (listed faces pass both)
        const int w = i1 - i0 + 1, npx = w * (j1 - j0 + 1);                                         // <= 8192^2
        const unsigned low = 0xFFFFFFFFu - (unsigned)f;
        for (int p = (int)threadIdx.x; p < npx; p += RASTER_THREADS) {
            const int r = p / w;
            raster_fragment(T, i0 + p - r * w, j0 + r, W, low, keys);
        }
    }
}

// ---- shadow maps of the light cells: the same integer coverage and the same depth formula, one orthographic map
// per cell, a 32-bit atomic max of bits(w) per fragment.  Grid (face block, chunk of cells): a thread keeps its face's corners in
// registers for SHADOW_CELLS cells; the cell is the loop counter, the same in every lane, so its frame arrives by scalar loads.
constexpr int SHADOW_CELLS = 16;

// the face's nine coordinates -> 0, or TIR_RASTER_DROP_INDEX (then nothing was read of pos)
__device__ __forceinline__ int shadow_corners(const float* __restrict__ pos, const int32_t* __restrict__ faces, int64_t n_verts, int64_t f,
                                              float P[9]) {
    int64_t v0 = 3 * f, v1 = 3 * f + 1, v2 = 3 * f + 2;
    if (faces) {
        const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_verts || i1 >= n_verts || i2 >= n_verts) return TIR_RASTER_DROP_INDEX;
        v0 = i0; v1 = i1; v2 = i2;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { P[a] = pos[3 * v0 + a]; P[3 + a] = pos[3 * v1 + a]; P[6 + a] = pos[3 * v2 + a]; }
    return 0;
}

// the face in one cell's frame -> 0 and T (corners snapped, depths w), or the drop flag of the pair
__device__ __forceinline__ int shadow_face(const float P[9], const float* __restrict__ fr, RasterFace& T) {
    float x[3], y[3], w[3];
    bool finite = true, guard = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        tir::shadow_project(fr, P[3 * k], P[3 * k + 1], P[3 * k + 2], x[k], y[k], w[k]);
        finite = finite && isfinite(x[k]) && isfinite(y[k]) && isfinite(w[k]);
        x[k] = rintf(mul_rn(x[k], 256.f));
        y[k] = rintf(mul_rn(y[k], 256.f));
        guard = guard && fabsf(x[k]) <= (float)RASTER_GUARD && fabsf(y[k]) <= (float)RASTER_GUARD;
    }
    if (!finite) return TIR_RASTER_DROP_NONFINITE;
    if (!guard) return TIR_RASTER_DROP_GUARD;
    T.x0 = (int)x[0]; T.y0 = (int)y[0]; T.x1 = (int)x[1]; T.y1 = (int)y[1]; T.x2 = (int)x[2]; T.y2 = (int)y[2];
    T.w0 = w[0]; T.w1 = w[1]; T.w2 = w[2];
    return 0;
}

__device__ __forceinline__ void shadow_fragment(const RasterFace& T, int i, int j, int S, unsigned* __restrict__ map) {
    int64_t e0, e1, e2;
    if (!raster_edges(T, i, j, e0, e1, e2)) return;
    float t0, t1, t2, s;
    raster_terms(T, e0, e1, e2, t0, t1, t2, s);
    const float w = __fdiv_rn(s, T.area);
    if (!(w > 0.f)) return;                                        // behind the frame's range (or NaN): bits would not order
    const unsigned key = __float_as_uint(w);
    unsigned* p = map + (size_t)j * (size_t)S + (size_t)i;         // 0 <= i, j < S: raster_box clips to the map
    if (*p < key) atomicMax(p, key);
}

__global__ void __launch_bounds__(RASTER_THREADS)
k_shadow_maps_small(const float* __restrict__ pos, const int32_t* __restrict__ faces, int64_t n_verts, int64_t n_faces,
                    const float* __restrict__ frames, int D, int S, unsigned* __restrict__ maps, int32_t* __restrict__ work, int work_cap,
                    unsigned long long* __restrict__ status) {
    const int64_t f = (int64_t)blockIdx.x * RASTER_THREADS + threadIdx.x;
    if (f >= n_faces) return;
    float P[9];
    const int bad = shadow_corners(pos, faces, n_verts, f, P);
    for (int d0 = (int)blockIdx.y * SHADOW_CELLS; d0 < D; d0 += (int)gridDim.y * SHADOW_CELLS) {
        const int d1 = min(d0 + SHADOW_CELLS, D);
        for (int d = d0; d < d1; ++d) {
            RasterFace T;
            const int drop = bad ? bad : shadow_face(P, frames + 12 * (size_t)d, T);
            if (drop) {
                atomicAdd(status + ((drop & TIR_RASTER_DROP_INDEX) ? 0 : (drop & TIR_RASTER_DROP_NONFINITE) ? 3 : 2), 1ull);
                continue;
            }
            int i0, i1, j0, j1;
            if (raster_setup(T) == 0 || !raster_box(T, S, S, i0, i1, j0, j1)) continue;
            if ((int64_t)(i1 - i0 + 1) * (j1 - j0 + 1) > RASTER_SMALL && __atomic_load_n(work, __ATOMIC_RELAXED) < work_cap) {
                const int slot = atomicAdd(work, 1);               // the count stays below work_cap + the threads in flight
                if (slot < work_cap) {
                    work[2 + 2 * (size_t)slot] = d;
                    work[3 + 2 * (size_t)slot] = (int32_t)f;
                    continue;
                }
            }
            unsigned* map = maps + (size_t)d * (size_t)S * (size_t)S;
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i) shadow_fragment(T, i, j, S, map);
        }
    }
}

__global__ void __launch_bounds__(RASTER_THREADS)
k_shadow_maps_big(const float* __restrict__ pos, const int32_t* __restrict__ faces, int64_t n_verts, int64_t n_faces,
                  const float* __restrict__ frames, int D, int S, unsigned* __restrict__ maps, const int32_t* __restrict__ work,
                  int work_cap) {
    const int n = min(work[0], work_cap);
    for (int b = (int)blockIdx.x; b < n; b += (int)gridDim.x) {
        const int d = work[2 + 2 * (size_t)b];
        const int64_t f = work[3 + 2 * (size_t)b];
        if (d < 0 || d >= D || f < 0 || f >= n_faces) continue;                              // (listed pairs pass all of these)
        float P[9];
        RasterFace T;
        int i0, i1, j0, j1;
        if (shadow_corners(pos, faces, n_verts, f, P) || shadow_face(P, frames + 12 * (size_t)d, T) || raster_setup(T) == 0 ||
            !raster_box(T, S, S, i0, i1, j0, j1))
            continue;
        const int w = i1 - i0 + 1, npx = w * (j1 - j0 + 1);                                    // <= 4096^2
        unsigned* map = maps + (size_t)d * (size_t)S * (size_t)S;
        for (int p = (int)threadIdx.x; p < npx; p += RASTER_THREADS) {
            const int r = p / w;
            shadow_fragment(T, i0 + p - r * w, j0 + r, S, map);
        }
    }
}

// vis [M][D]: 0 = the pair does not contribute (c <= 1e-6), 1 = shadowed, 2 = lit; one thread per point, the cells in order
__global__ void __launch_bounds__(RASTER_THREADS)
k_shadow_lookup(const float* __restrict__ pts, const float* __restrict__ nrm, const float4* __restrict__ cells,
                const float* __restrict__ frames, const uint32_t* __restrict__ maps, int64_t M, int D, int S, tir::ShadowBias bias,
                uint8_t* __restrict__ vis) {
    const int64_t m = (int64_t)blockIdx.x * RASTER_THREADS + threadIdx.x;
    if (m >= M) return;
    const float p0 = pts[3 * m], p1 = pts[3 * m + 1], p2 = pts[3 * m + 2];
    const float n0 = nrm[3 * m], n1 = nrm[3 * m + 1], n2 = nrm[3 * m + 2];
    for (int d = 0; d < D; ++d) {
        const float4 ca = cells[2 * (size_t)d];
        const float c = tir::light_cosine(n0, n1, n2, ca.x, ca.y, ca.z);
        uint8_t code = 0;
        if (c > 1e-6f)
            code = tir::shadow_lit(frames + 12 * (size_t)d, maps + (size_t)d * (size_t)S * (size_t)S, S, p0, p1, p2, c, bias) ? 2 : 1;
        vis[(size_t)m * (size_t)D + (size_t)d] = code;
    }
}

__global__ void __launch_bounds__(RASTER_THREADS)
k_raster_resolve(const int4* __restrict__ rows, int64_t n_faces, const unsigned long long* __restrict__ keys, int W, int H,
                 int4* __restrict__ out) {
    const int p = (int)blockIdx.x * RASTER_THREADS + (int)threadIdx.x;
    if (p >= W * H) return;
    const unsigned long long key = keys[p];
    int4 o = make_int4(-1, 0, 0, 0);
    const int64_t f = (int64_t)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu));
    RasterFace T;
    if (key != 0 && f < n_faces && raster_load(rows, f, T) != 0) {
        const int j = p / W, i = p - j * W;
        int64_t e0, e1, e2;
        raster_edges(T, i, j, e0, e1, e2);
        float t0, t1, t2, s;
        raster_terms(T, e0, e1, e2, t0, t1, t2, s);
        const float invz = __uint_as_float((unsigned)(key >> 32));
        o = make_int4((int)f, __float_as_int(__fdiv_rn(t1, s)), __float_as_int(__fdiv_rn(t2, s)), __float_as_int(__fdiv_rn(1.f, invz)));
    }
    out[p] = o;
}

struct RasterMesh {
    const float *nrm, *tan, *uv;                         // per corner: [3F][3], [3F][4], [3F][2]; tan and uv null without images
    const uint32_t *base, *orm, *normal;                 // RGBA8 [size][size], or all null
    int size, raw;
};

__device__ __forceinline__ float raster_mix(const float b[3], const float* __restrict__ a, int64_t q, int stride, int c) {
    return fmaf(b[2], a[(q + 2) * stride + c], fmaf(b[1], a[(q + 1) * stride + c], b[0] * a[q * stride + c]));
}

__device__ __forceinline__ void raster_unit(float v[3]) {
    const float l = fmaxf(sqrtf(fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0]))), 1e-20f);
    v[0] /= l; v[1] /= l; v[2] /= l;
}

// LINEAR, CLAMP_TO_EDGE: the four taps and their weights at sample position uv * size - 0.5
struct RasterTaps {
    int o00, o01, o10, o11;
    float w00, w01, w10, w11;
};

__device__ __forceinline__ RasterTaps raster_taps(float u, float v, int S) {
    const float x = fminf(fmaxf(fmaf(u, (float)S, -0.5f), -1.f), (float)S), y = fminf(fmaxf(fmaf(v, (float)S, -0.5f), -1.f), (float)S);
    const float fx0 = floorf(x), fy0 = floorf(y), fx = x - fx0, fy = y - fy0;
    const int i0 = (int)fx0, j0 = (int)fy0;
    const int ia = min(max(i0, 0), S - 1), ib = min(max(i0 + 1, 0), S - 1), ja = min(max(j0, 0), S - 1), jb = min(max(j0 + 1, 0), S - 1);
    RasterTaps t;
    t.o00 = ja * S + ia; t.o01 = ja * S + ib; t.o10 = jb * S + ia; t.o11 = jb * S + ib;
    t.w00 = (1.f - fx) * (1.f - fy); t.w01 = fx * (1.f - fy); t.w10 = (1.f - fx) * fy; t.w11 = fx * fy;
    return t;
}

// channel c of the filtered texel through the decoding table lut (byte -> value)
__device__ __forceinline__ float raster_tex(const uint32_t* __restrict__ img, const RasterTaps& t, int c, const float* lut) {
    const int sh = 8 * c;
    return fmaf(t.w11, lut[(img[t.o11] >> sh) & 255u],
                fmaf(t.w10, lut[(img[t.o10] >> sh) & 255u], fmaf(t.w01, lut[(img[t.o01] >> sh) & 255u], t.w00 * lut[(img[t.o00] >> sh) & 255u])));
}

__global__ void __launch_bounds__(RASTER_THREADS)
k_raster_shade(const int4* __restrict__ pix, int64_t n_faces, RasterMesh M, int W, int H, float4* __restrict__ out) {
    __shared__ float s_lin[256], s_srgb[256];            // byte / 255, and its sRGB -> linear decoding (the inverse of k_atlas_pack's)
    {
        const float s = __fdiv_rn((float)threadIdx.x, 255.f);
        s_lin[threadIdx.x] = s;
        s_srgb[threadIdx.x] = M.raw ? s : (s <= 0.04045f ? s / 12.92f : fmaxf(powf((s + 0.055f) / 1.055f, 2.4f) - 1e-6f, 0.f));
    }
    __syncthreads();
    const int p = (int)blockIdx.x * RASTER_THREADS + (int)threadIdx.x;
    if (p >= W * H) return;
    const int4 r = pix[p];
    float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = o0, o2 = o0;
    if (r.x >= 0 && r.x < n_faces) {
        const float b1 = __int_as_float(r.y), b2 = __int_as_float(r.z);
        const float b[3] = {sub_rn(sub_rn(1.f, b1), b2), b1, b2};
        const int64_t q = 3 * (int64_t)r.x;
        float n[3] = {raster_mix(b, M.nrm, q, 3, 0), raster_mix(b, M.nrm, q, 3, 1), raster_mix(b, M.nrm, q, 3, 2)};
        raster_unit(n);
        float N[3] = {n[0], n[1], n[2]};
        if (M.base) {
            const RasterTaps t = raster_taps(raster_mix(b, M.uv, q, 2, 0), raster_mix(b, M.uv, q, 2, 1), M.size);
            o0 = make_float4(raster_tex(M.base, t, 0, s_srgb), raster_tex(M.base, t, 1, s_srgb), raster_tex(M.base, t, 2, s_srgb),
                             raster_tex(M.orm, t, 1, s_lin));
            o1.x = raster_tex(M.orm, t, 0, s_lin);
            float tg[3] = {raster_mix(b, M.tan, q, 4, 0), raster_mix(b, M.tan, q, 4, 1), raster_mix(b, M.tan, q, 4, 2)};
            raster_unit(tg);
            const float sg = M.tan[4 * q + 3];                             // the handedness of corner 0
            const float bt[3] = {(n[1] * tg[2] - n[2] * tg[1]) * sg, (n[2] * tg[0] - n[0] * tg[2]) * sg, (n[0] * tg[1] - n[1] * tg[0]) * sg};
            const float tx = fmaf(2.f, raster_tex(M.normal, t, 0, s_lin), -1.f), ty = fmaf(2.f, raster_tex(M.normal, t, 1, s_lin), -1.f),
                        tz = fmaf(2.f, raster_tex(M.normal, t, 2, s_lin), -1.f);
#pragma unroll
            for (int a = 0; a < 3; ++a) N[a] = fmaf(tz, n[a], fmaf(ty, bt[a], tx * tg[a]));
            raster_unit(N);
        }
        o1.y = N[0]; o1.z = N[1]; o1.w = N[2];
        o2.x = 1.f;
    }
    out[3 * (int64_t)p] = o0;
    out[3 * (int64_t)p + 1] = o1;
    out[3 * (int64_t)p + 2] = o2;
}

int raster_image(int32_t W, int32_t H) {
    if (W < 1 || H < 1) return TIR_ERR_ARG;
    if (W > TIR_RASTER_MAX_SIDE || H > TIR_RASTER_MAX_SIDE) return TIR_ERR_UNSUPPORTED;
    return TIR_OK;
}

inline unsigned raster_blocks(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace

extern "C" int tir_raster_project(const float* pos, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* c2w,
                                  float focal, int32_t W, int32_t H, float near_z, int32_t* rows, int32_t* status, void* stream) {
    if (!c2w || !status || n_verts < 0 || n_faces < 0 || !(focal > 0.f) || !(near_z >= 0.f)) return TIR_ERR_ARG;
    if (n_faces > 0 && (!pos || !rows)) return TIR_ERR_ARG;
    if (!faces && n_verts < 3 * n_faces) return TIR_ERR_ARG;
    const int rc = raster_image(W, H);
    if (rc) return rc;
    if (n_faces > TIR_RASTER_MAX_FACES || n_verts > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    if ((uintptr_t)rows & 15) return TIR_ERR_ARG;
    hipStream_t st = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(int32_t), st);
    if (e != hipSuccess) return -(int)e;
    if (n_faces == 0) return TIR_OK;
    RasterCam C;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) C.r[r][c] = c2w[4 * r + c];
        C.o[r] = c2w[4 * r + 3];
    }
    C.f = focal; C.cx = 0.5f * (float)W; C.cy = 0.5f * (float)H; C.near_ = near_z;
    hipLaunchKernelGGL(k_raster_project, dim3(raster_blocks(3 * n_faces, RASTER_PROJ_THREADS)), dim3(RASTER_PROJ_THREADS), 0, st, pos,
                       faces, C, n_verts, n_faces, reinterpret_cast<int4*>(rows), status);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_raster_cover(const int32_t* rows, int64_t n_faces, int32_t W, int32_t H, int32_t cull, uint64_t* keys,
                                int32_t* work, void* stream) {
    if (!keys || !work || n_faces < 0 || (n_faces > 0 && !rows)) return TIR_ERR_ARG;
    const int rc = raster_image(W, H);
    if (rc) return rc;
    if (n_faces > TIR_RASTER_MAX_FACES) return TIR_ERR_UNSUPPORTED;
    if (((uintptr_t)rows & 15) || ((uintptr_t)keys & 7)) return TIR_ERR_ARG;
    hipStream_t st = tir_stream(stream);
    hipError_t e = hipMemsetAsync(keys, 0, sizeof(uint64_t) * (size_t)W * (size_t)H, st);
    if (e == hipSuccess) e = hipMemsetAsync(work, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return -(int)e;
    if (n_faces == 0) return TIR_OK;
    auto* k = reinterpret_cast<unsigned long long*>(keys);
    hipLaunchKernelGGL(k_raster_cover_small, dim3(raster_blocks(n_faces, RASTER_THREADS)), dim3(RASTER_THREADS), 0, st,
                       reinterpret_cast<const int4*>(rows), n_faces, (int)W, (int)H, (int)(cull != 0), k, work);
    TIR_CHECK_LAUNCH();
    const unsigned nb = (unsigned)(n_faces < RASTER_BIG_BLOCKS ? n_faces : RASTER_BIG_BLOCKS);
    hipLaunchKernelGGL(k_raster_cover_big, dim3(nb), dim3(RASTER_THREADS), 0, st, reinterpret_cast<const int4*>(rows), (int)W, (int)H, k,
                       work);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_raster_resolve(const int32_t* rows, int64_t n_faces, const uint64_t* keys, int32_t W, int32_t H, int32_t* out,
                                  void* stream) {
    if (!keys || !out || n_faces < 0 || (n_faces > 0 && !rows)) return TIR_ERR_ARG;
    const int rc = raster_image(W, H);
    if (rc) return rc;
    if (n_faces > TIR_RASTER_MAX_FACES) return TIR_ERR_UNSUPPORTED;
    if (((uintptr_t)rows & 15) || ((uintptr_t)keys & 7) || ((uintptr_t)out & 15)) return TIR_ERR_ARG;
    hipLaunchKernelGGL(k_raster_resolve, dim3(raster_blocks((int64_t)W * H, RASTER_THREADS)), dim3(RASTER_THREADS), 0, tir_stream(stream),
                       reinterpret_cast<const int4*>(rows), n_faces, reinterpret_cast<const unsigned long long*>(keys), (int)W, (int)H,
                       reinterpret_cast<int4*>(out));
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_raster_shade(const int32_t* pix, int64_t n_faces, const float* nrm, const float* tan, const float* uv,
                                const uint8_t* base, const uint8_t* orm, const uint8_t* normal, int32_t size, int32_t raw, int32_t W,
                                int32_t H, float* out, void* stream) {
    if (!pix || !out || n_faces < 0 || (n_faces > 0 && !nrm)) return TIR_ERR_ARG;
    const bool textured = base || orm || normal;
    if (textured && (!base || !orm || !normal || size < 1 || (n_faces > 0 && (!tan || !uv)))) return TIR_ERR_ARG;
    const int rc = raster_image(W, H);
    if (rc) return rc;
    if (n_faces > TIR_RASTER_MAX_FACES || (textured && size > TIR_RASTER_MAX_SIDE)) return TIR_ERR_UNSUPPORTED;
    if (((uintptr_t)pix & 15) || ((uintptr_t)out & 15) || (((uintptr_t)base | (uintptr_t)orm | (uintptr_t)normal) & 3)) return TIR_ERR_ARG;
    RasterMesh M{nrm, tan, uv, reinterpret_cast<const uint32_t*>(base), reinterpret_cast<const uint32_t*>(orm),
                 reinterpret_cast<const uint32_t*>(normal), (int)size, (int)(raw != 0)};
    hipLaunchKernelGGL(k_raster_shade, dim3(raster_blocks((int64_t)W * H, RASTER_THREADS)), dim3(RASTER_THREADS), 0, tir_stream(stream),
                       reinterpret_cast<const int4*>(pix), n_faces, M, (int)W, (int)H, reinterpret_cast<float4*>(out));
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

namespace {
int shadow_side(int32_t S) { return S < 1 ? TIR_ERR_ARG : (S > TIR_SHADOW_MAX_SIDE ? TIR_ERR_UNSUPPORTED : TIR_OK); }
}  // namespace

extern "C" int tir_shadow_maps(const float* pos, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* frames, int32_t D,
                               int32_t S, uint32_t* maps, int32_t* work, int32_t work_cap, int64_t* status, void* stream) {
    if (!frames || !maps || !work || !status || D < 1 || n_verts < 0 || n_faces < 0 || work_cap < 0) return TIR_ERR_ARG;
    if (n_faces > 0 && !pos) return TIR_ERR_ARG;
    if (!faces && n_verts < 3 * n_faces) return TIR_ERR_ARG;
    const int rc = shadow_side(S);
    if (rc) return rc;
    if (n_faces > TIR_RASTER_MAX_FACES || n_verts > INT32_MAX || D > (1 << 20)) return TIR_ERR_UNSUPPORTED;
    if (((uintptr_t)frames & 15) || ((uintptr_t)maps & 3) || ((uintptr_t)work & 3) || ((uintptr_t)status & 7)) return TIR_ERR_ARG;
    hipStream_t st = tir_stream(stream);
    hipError_t e = hipMemsetAsync(maps, 0, sizeof(uint32_t) * (size_t)D * (size_t)S * (size_t)S, st);
    if (e == hipSuccess) e = hipMemsetAsync(work, 0, 2 * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, 4 * sizeof(int64_t), st);
    if (e != hipSuccess) return -(int)e;
    if (n_faces == 0) return TIR_OK;
    const unsigned chunks = (unsigned)((D + SHADOW_CELLS - 1) / SHADOW_CELLS);
    hipLaunchKernelGGL(k_shadow_maps_small, dim3(raster_blocks(n_faces, RASTER_THREADS), chunks < 65535u ? chunks : 65535u),
                       dim3(RASTER_THREADS), 0, st, pos, faces, n_verts, n_faces, frames, (int)D, (int)S, maps, work, (int)work_cap,
                       reinterpret_cast<unsigned long long*>(status));
    TIR_CHECK_LAUNCH();
    if (work_cap > 0) {
        hipLaunchKernelGGL(k_shadow_maps_big, dim3((unsigned)(work_cap < RASTER_BIG_BLOCKS ? work_cap : RASTER_BIG_BLOCKS)),
                           dim3(RASTER_THREADS), 0, st, pos, faces, n_verts, n_faces, frames, (int)D, (int)S, maps, work, (int)work_cap);
        TIR_CHECK_LAUNCH();
    }
    return TIR_OK;
}

extern "C" int tir_shadow_lookup(const float* pts, const float* nrm, const float* cells, const float* frames, const uint32_t* maps,
                                 int64_t M, int32_t D, int32_t S, float bias_const, float bias_slope, uint8_t* vis, void* stream) {
    if (M < 0 || D < 1 || !(bias_const >= 0.f && bias_const < INFINITY) || !(bias_slope >= 0.f && bias_slope < INFINITY)) return TIR_ERR_ARG;
    const int rc = shadow_side(S);
    if (rc) return rc;
    if (D > (1 << 20) || M > ((int64_t)1 << 36)) return TIR_ERR_UNSUPPORTED;
    if (M == 0) return TIR_OK;
    if (!pts || !nrm || !cells || !frames || !maps || !vis) return TIR_ERR_ARG;
    if (((uintptr_t)cells & 15) || ((uintptr_t)frames & 15) || ((uintptr_t)maps & 3)) return TIR_ERR_ARG;
    const tir::ShadowBias bias{bias_const, bias_slope, 0.5f / (float)S};
    hipLaunchKernelGGL(k_shadow_lookup, dim3(raster_blocks(M, RASTER_THREADS)), dim3(RASTER_THREADS), 0, tir_stream(stream), pts, nrm,
                       reinterpret_cast<const float4*>(cells), frames, maps, M, (int)D, (int)S, bias, vis);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}
