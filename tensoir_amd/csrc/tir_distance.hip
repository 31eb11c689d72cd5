// Surface distance between meshes (contract: include/tensoir_hip.h, tir_mesh_sample* / tir_face_grid_* / tir_point_mesh_distance;
// DESIGN 4.15).
//   sampling   k_ms_weight        per face: |cross| in fp64 -> the cdf buffer (as its bits), the largest one by an integer atomicMax
//              k_ms_scan<false>   per block of 4096 faces: the sum of the integer weights
//              k_ms_scan_blocks   one workgroup: exclusive scan of the block sums (64-bit)
//              k_ms_scan<true>    the inclusive integer sums, in place over the fp64 weights; total and statistics -> status
//              k_ms_draw          per sample: the counter hash, the stratified position, a binary search, the point
//   grid       k_fg_count         per face: the cells its bounding box overlaps as a product (no loop) -> the 64-bit pair total
//              k_fg_cells<false>  per face and overlapped cell: cursor[cell] += 1
//              k_fg_scan<false/true>  block sums of the cell counts / cursor[cell] = first slot of the cell (tir_exclusive_scan
//                                 of the block sums in between)
//              k_fg_cells<true>   per face and overlapped cell: pairs[cursor[cell]++] = face; cursor[cell] ends as the cell's end
//   query      k_point_mesh_distance  one lane per point: shells of cells of growing Chebyshev radius, fp64 closest point
//              k_ray_mesh<mode>   one lane per ray: slabs of cells along the major axis, fp64 ray-triangle rule (tir_ray_mesh)
//              k_shadow_trace     one lane per surface point, the light cell as the loop counter: the same walk in any-hit mode, the
//                                 64 answers of a wave packed by one ballot (tir_shadow_trace)
// Every sum that crosses lanes is an integer sum, every minimum / maximum is order-independent: no output depends on the order
// the device worked in, the order of the faces inside a cell included (ties go to the smaller face index).
#include "tir_common.hpp"

// nothing in this file may be contracted into an FMA: the integer weights, the stratified positions and the degenerate test are
// discrete functions of fp64 values that the numpy restatement forms with one rounding per operation (profiles/r05_fma_contraction.json)
#pragma clang fp contract(off)

using namespace tir;

namespace {

constexpr int DS_THREADS = 256;
constexpr int DS_ITERS = 16;
constexpr int DS_BLOCK = DS_THREADS * DS_ITERS;            // 4096 faces / cells per scan block
constexpr int64_t DS_MAX_FACES = (int64_t)1 << TIR_DISTANCE_MAX_FACES_LOG2;
constexpr double DS_INF = __builtin_huge_val();

__device__ __forceinline__ double d_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double d_sub(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double d_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double d_div(double a, double b) {
#pragma clang fp contract(off)
    return a / b;
}

constexpr int64_t ds_blocks(int64_t n, int per) { return (n + per - 1) / per; }

// exclusive scan of one 64-bit integer per thread over the block (4 waves); *total = block sum
__device__ __forceinline__ long long ds_block_scan(long long v, long long* wsum, long long* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    long long off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < DS_THREADS / 64; ++q) {
        const long long s = wsum[q];
        off += q < wv ? s : 0;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return off + incl - v;
}

// the corners of face f, or false when an index lies outside [0, V)
__device__ __forceinline__ bool ds_face(const int32_t* __restrict__ faces, int64_t f, int64_t V, int32_t& i0, int32_t& i1, int32_t& i2) {
    i0 = faces[3 * f];
    i1 = faces[3 * f + 1];
    i2 = faces[3 * f + 2];
    return i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
}

struct DsTri {
    double ax, ay, az, bx, by, bz, cx, cy, cz;
};

__device__ __forceinline__ DsTri ds_corners(const float* __restrict__ verts, int32_t i0, int32_t i1, int32_t i2) {
    const float* a = verts + 3 * (int64_t)i0;
    const float* b = verts + 3 * (int64_t)i1;
    const float* c = verts + 3 * (int64_t)i2;
    return DsTri{(double)a[0], (double)a[1], (double)a[2], (double)b[0], (double)b[1], (double)b[2],
                 (double)c[0], (double)c[1], (double)c[2]};
}

// |(b - a) x (c - a)|^2 in fp64, one rounding per operation, summed x, y, z in that order
__device__ __forceinline__ double ds_cross2(const DsTri& t) {
    const double ux = d_sub(t.bx, t.ax), uy = d_sub(t.by, t.ay), uz = d_sub(t.bz, t.az);
    const double vx = d_sub(t.cx, t.ax), vy = d_sub(t.cy, t.ay), vz = d_sub(t.cz, t.az);
    const double nx = d_sub(d_mul(uy, vz), d_mul(uz, vy));
    const double ny = d_sub(d_mul(uz, vx), d_mul(ux, vz));
    const double nz = d_sub(d_mul(ux, vy), d_mul(uy, vx));
    return d_add(d_add(d_mul(nx, nx), d_mul(ny, ny)), d_mul(nz, nz));
}

// ---- sampling -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ds_hash24(uint64_t seed, uint64_t i, uint32_t channel) {
    uint64_t x = seed + 0x9E3779B97F4A7C15ull * (3ull * i + channel + 1ull);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)(x >> 40);
}

// the integer weight of a face whose fp64 weight is w, against the largest weight wmax and the power-of-two scale
__device__ __forceinline__ long long ds_quant(double w, double wmax, double scale) {
    return (w > 0.0 && w <= wmax) ? (long long)d_mul(d_div(w, wmax), scale) : 0ll;       // (false for a NaN; wmax is finite)
}

__global__ void __launch_bounds__(DS_THREADS)
k_ms_weight(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F, double* __restrict__ weight,
            unsigned long long* __restrict__ status) {
    const int64_t f = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    double w = 0.0;
    if (f < F) {
        int32_t i0, i1, i2;
        if (ds_face(faces, f, V, i0, i1, i2)) {
            w = sqrt(ds_cross2(ds_corners(verts, i0, i1, i2)));
            if (!(w < DS_INF)) w = 0.0;                    // a non-finite corner: no weight (NaN compares false)
        } else {
            atomicOr(status + 1, (unsigned long long)TIR_DISTANCE_ERR_FACE_INDEX);
        }
        weight[f] = w;
    }
    // non-negative doubles order as their bit patterns: an integer maximum, exact whatever the order
    unsigned long long bits = (unsigned long long)__double_as_longlong(w);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)bits, d, 64);
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(status + 3, bits);
}

// EMIT = false: sums[block] = the block's integer weight.  EMIT = true: cdf[f] = inclusive sum (in place over the fp64 weights:
// every thread reads its own entry before it writes it), status[0] = total, status[2] += faces of integer weight 0.
template <bool EMIT>
__global__ void __launch_bounds__(DS_THREADS)
k_ms_scan(long long* __restrict__ cdf, int64_t F, int scale_log2, long long* __restrict__ sums, unsigned long long* __restrict__ status) {
    __shared__ long long wsum[DS_THREADS / 64];
    const double wmax = __longlong_as_double((long long)status[3]);
    const double scale = __longlong_as_double((long long)(1023 + scale_log2) << 52);
    const int64_t base = (int64_t)blockIdx.x * DS_BLOCK;
    long long carry = EMIT ? sums[blockIdx.x] : 0, acc = 0;
    int zero = 0;
    for (int it = 0; it < DS_ITERS; ++it) {
        const int64_t f = base + it * DS_THREADS + threadIdx.x;
        const long long q = f < F ? ds_quant(__longlong_as_double(cdf[f]), wmax, scale) : 0;
        if constexpr (EMIT) {
            long long tot;
            const long long o = carry + ds_block_scan(q, wsum, &tot);
            carry += tot;
            if (f < F) {
                cdf[f] = o + q;
                zero += q == 0;
            }
        } else {
            acc += q;
        }
    }
    if constexpr (EMIT) {
        if (zero) atomicAdd(status + 2, (unsigned long long)zero);
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) status[0] = (unsigned long long)carry;
    } else {
        long long tot;
        ds_block_scan(acc, wsum, &tot);
        if (threadIdx.x == 0) sums[blockIdx.x] = tot;
    }
}

// in place: sums[b] = sum of sums[0 .. b)
__global__ void __launch_bounds__(DS_THREADS)
k_ms_scan_blocks(long long* __restrict__ sums, int n) {
    __shared__ long long wsum[DS_THREADS / 64];
    long long carry = 0;
    for (int base = 0; base < n; base += DS_THREADS) {
        const int i = base + threadIdx.x;
        const long long v = i < n ? sums[i] : 0;
        long long tot;
        const long long o = carry + ds_block_scan(v, wsum, &tot);
        carry += tot;
        if (i < n) sums[i] = o;
    }
}

__global__ void __launch_bounds__(DS_THREADS)
k_ms_draw(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F, const long long* __restrict__ cdf,
          int64_t n, uint64_t seed, float* __restrict__ points, int32_t* __restrict__ face) {
    const int64_t i = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long total = cdf[F - 1];
    const uint32_t u0 = ds_hash24(seed, (uint64_t)i, 0), u1 = ds_hash24(seed, (uint64_t)i, 1), u2 = ds_hash24(seed, (uint64_t)i, 2);
    int64_t lo = 0, hi = F - 1;                            // the first face whose inclusive sum exceeds k
    bool ok = total > 0;
    if (ok) {
        const double xi = d_mul((double)u0, 1.0 / 16777216.0);
        const double pos = d_mul(d_div(d_add((double)i, xi), (double)n), (double)total);
        long long k = (long long)pos;
        k = k < total - 1 ? k : total - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (cdf[mid] > k) hi = mid; else lo = mid + 1;
        }
    }
    int32_t i0 = 0, i1 = 0, i2 = 0;
    ok = ok && ds_face(faces, lo, V, i0, i1, i2);          // (a face of weight > 0 has valid indices; never followed otherwise)
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (ok) {
        const float x1 = (float)u1 * (1.0f / 16777216.0f), x2 = (float)u2 * (1.0f / 16777216.0f);
        const float s = sqrtf(x1), b0 = 1.0f - s, b1 = s * (1.0f - x2), b2 = s * x2;
        const float* a = verts + 3 * (int64_t)i0;
        const float* b = verts + 3 * (int64_t)i1;
        const float* c = verts + 3 * (int64_t)i2;
        px = (b0 * a[0] + b1 * b[0]) + b2 * c[0];
        py = (b0 * a[1] + b1 * b[1]) + b2 * c[1];
        pz = (b0 * a[2] + b1 * b[2]) + b2 * c[2];
    }
    points[3 * i] = px;
    points[3 * i + 1] = py;
    points[3 * i + 2] = pz;
    face[i] = ok ? (int32_t)lo : -1;
}

// ---- the uniform grid ------------------------------------------------------------------------------------------------------------
struct DsGrid {
    float cell[3], origin[3];
    int32_t dims[3];
};

// the cell of a coordinate: clamp(floor((x - origin) / cell), 0, dim - 1), fp32 with every operation rounded on its own.  It is
// MONOTONE in x, which is all the search relies on: every point of a face lies in a cell between those of its bounding box.
__device__ __forceinline__ int ds_cell(float x, float origin, float cell, int32_t dim) {
    const float f = fmaxf(floorf(__fdiv_rn(sub_rn(x, origin), cell)), 0.0f);
    return f >= (float)(dim - 1) ? dim - 1 : (int)f;
}

struct DsRange {
    int lo0, lo1, lo2, hi0, hi1, hi2;
    bool listed;
};

// the cells face f is listed in; `bad` receives 1 for a face that is listed nowhere because it is degenerate or not finite
__device__ __forceinline__ DsRange ds_face_range(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t f,
                                                 const DsGrid& G, int& bad, int& bad_index) {
    DsRange r{0, 0, 0, -1, -1, -1, false};
    int32_t i0, i1, i2;
    bad = bad_index = 0;
    if (!ds_face(faces, f, V, i0, i1, i2)) {
        bad_index = 1;
        return r;
    }
    const float* a = verts + 3 * (int64_t)i0;
    const float* b = verts + 3 * (int64_t)i1;
    const float* c = verts + 3 * (int64_t)i2;
    const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
    const bool finite = fabsf(ax) < DS_INF && fabsf(ay) < DS_INF && fabsf(az) < DS_INF && fabsf(bx) < DS_INF && fabsf(by) < DS_INF &&
                        fabsf(bz) < DS_INF && fabsf(cx) < DS_INF && fabsf(cy) < DS_INF && fabsf(cz) < DS_INF;       // (false for a NaN)
    const DsTri t{(double)ax, (double)ay, (double)az, (double)bx, (double)by, (double)bz, (double)cx, (double)cy, (double)cz};
    if (!finite || ds_cross2(t) == 0.0) {
        bad = 1;
        return r;
    }
    r.lo0 = ds_cell(fminf(ax, fminf(bx, cx)), G.origin[0], G.cell[0], G.dims[0]);
    r.hi0 = ds_cell(fmaxf(ax, fmaxf(bx, cx)), G.origin[0], G.cell[0], G.dims[0]);
    r.lo1 = ds_cell(fminf(ay, fminf(by, cy)), G.origin[1], G.cell[1], G.dims[1]);
    r.hi1 = ds_cell(fmaxf(ay, fmaxf(by, cy)), G.origin[1], G.cell[1], G.dims[1]);
    r.lo2 = ds_cell(fminf(az, fminf(bz, cz)), G.origin[2], G.cell[2], G.dims[2]);
    r.hi2 = ds_cell(fmaxf(az, fmaxf(bz, cz)), G.origin[2], G.cell[2], G.dims[2]);
    r.listed = true;
    return r;
}

__device__ __forceinline__ int32_t ds_cell_key(const DsGrid& G, int x, int y, int z) { return (x * G.dims[1] + y) * G.dims[2] + z; }

// status[0] += pairs, status[1] |= error bits, status[2] += degenerate / non-finite faces, status[3] += listed faces
__global__ void __launch_bounds__(DS_THREADS)
k_fg_count(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F, DsGrid G,
           unsigned long long* __restrict__ status) {
    __shared__ long long wsum[DS_THREADS / 64];
    const int64_t f = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    long long pairs = 0;
    int bad = 0, bad_index = 0, listed = 0;
    if (f < F) {
        const DsRange r = ds_face_range(verts, V, faces, f, G, bad, bad_index);
        if (r.listed) {
            pairs = (long long)(r.hi0 - r.lo0 + 1) * (r.hi1 - r.lo1 + 1) * (r.hi2 - r.lo2 + 1);      // <= 2^24 cells
            listed = 1;
        }
    }
    if (bad_index) atomicOr(status + 1, (unsigned long long)TIR_DISTANCE_ERR_FACE_INDEX);
    long long tot;
    ds_block_scan(pairs, wsum, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(status, (unsigned long long)tot);
    if (bad) atomicAdd(status + 2, 1ull);
    if (listed) atomicAdd(status + 3, 1ull);
}

template <bool FILL>
__global__ void __launch_bounds__(DS_THREADS)
k_fg_cells(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F, DsGrid G, int32_t* __restrict__ cursor,
           int32_t* __restrict__ pairs, int64_t n_pairs) {
    const int64_t f = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    if (f >= F) return;
    int bad, bad_index;
    const DsRange r = ds_face_range(verts, V, faces, f, G, bad, bad_index);
    if (!r.listed) return;
    for (int x = r.lo0; x <= r.hi0; ++x)
        for (int y = r.lo1; y <= r.hi1; ++y)
            for (int z = r.lo2; z <= r.hi2; ++z) {
                const int32_t slot = atomicAdd(cursor + ds_cell_key(G, x, y, z), 1);
                if constexpr (FILL) {
                    if (slot >= 0 && slot < n_pairs) pairs[slot] = (int32_t)f;
                }
            }
}

// EMIT = false: counts[block] = faces listed in the block's cells.  EMIT = true: cursor[cell] = the cell's first slot.
template <bool EMIT>
__global__ void __launch_bounds__(DS_THREADS)
k_fg_scan(int32_t* __restrict__ cursor, int64_t n_cells, int32_t* __restrict__ counts, const int32_t* __restrict__ offsets) {
    __shared__ long long wsum[DS_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * DS_BLOCK;
    long long carry = EMIT ? offsets[blockIdx.x] : 0, acc = 0;
    for (int it = 0; it < DS_ITERS; ++it) {
        const int64_t c = base + it * DS_THREADS + threadIdx.x;
        const long long v = c < n_cells ? cursor[c] : 0;
        if constexpr (EMIT) {
            long long tot;
            const long long o = carry + ds_block_scan(v, wsum, &tot);
            carry += tot;
            if (c < n_cells) cursor[c] = (int32_t)o;
        } else {
            acc += v;
        }
    }
    if constexpr (!EMIT) {
        long long tot;
        ds_block_scan(acc, wsum, &tot);
        if (threadIdx.x == 0) counts[blockIdx.x] = (int32_t)tot;        // the pair total is below 2^31 (validated by the caller)
    }
}

// ---- the query ------------------------------------------------------------------------------------------------------------------
struct DsBest {
    double d2, x, y, z;
    int32_t face;
};

// squared distance of p to triangle t, in coordinates relative to corner a; the closest point (relative to a) -> rx, ry, rz.
// The seven regions: corner a, corner b, edge ab, corner c, edge ac, edge bc, interior.
__device__ __forceinline__ double ds_closest(const DsTri& t, double px, double py, double pz, double& rx, double& ry, double& rz) {
    const double abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
    const double acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
    const double apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
    const double d1 = abx * apx + aby * apy + abz * apz, d2 = acx * apx + acy * apy + acz * apz;
    const double bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
    const double d3 = abx * bpx + aby * bpy + abz * bpz, d4 = acx * bpx + acy * bpy + acz * bpz;
    const double cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
    const double d5 = abx * cpx + aby * cpy + abz * cpz, d6 = acx * cpx + acy * cpy + acz * cpz;
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double v, w;                                           // closest = a + v ab + w ac
    if (d1 <= 0.0 && d2 <= 0.0) {
        v = 0.0; w = 0.0;
    } else if (d3 >= 0.0 && d4 <= d3) {
        v = 1.0; w = 0.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        v = d1 / (d1 - d3); w = 0.0;
    } else if (d6 >= 0.0 && d5 <= d6) {
        v = 0.0; w = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        v = 0.0; w = d2 / (d2 - d6);
    } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.0 - w;
    } else {
        const double den = (va + vb) + vc;
        v = vb / den; w = vc / den;
    }
    rx = abx * v + acx * w;
    ry = aby * v + acy * w;
    rz = abz * v + acz * w;
    const double ex = apx - rx, ey = apy - ry, ez = apz - rz;
    return (ex * ex + ey * ey) + ez * ez;
}

// every face listed in cell (x, y, z) against the best so far; returns the number of faces tested
__device__ __forceinline__ int ds_visit(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                                        const DsGrid& G, const int32_t* __restrict__ cursor, const int32_t* __restrict__ pairs,
                                        int64_t n_pairs, int x, int y, int z, double px, double py, double pz, DsBest& B) {
    const int32_t key = ds_cell_key(G, x, y, z);
    int64_t k = key ? cursor[key - 1] : 0, end = cursor[key];
    k = k < 0 ? 0 : k;
    end = end < n_pairs ? end : n_pairs;
    int tested = 0;
    for (; k < end; ++k) {
        const int32_t f = pairs[k];
        int32_t i0, i1, i2;
        if (f < 0 || f >= F || !ds_face(faces, f, V, i0, i1, i2)) continue;
        const DsTri t = ds_corners(verts, i0, i1, i2);
        double rx, ry, rz;
        const double d2 = ds_closest(t, px, py, pz, rx, ry, rz);
        ++tested;
        if (d2 < B.d2 || (d2 == B.d2 && f < B.face)) {
            B.d2 = d2;
            B.face = f;
            B.x = t.ax + rx;
            B.y = t.ay + ry;
            B.z = t.az + rz;
        }
    }
    return tested;
}

// how far p is from every cell beyond radius r on one axis: the nearer of the two planes that still have cells behind them,
// minus the slack that covers the rounding of ds_cell (include/tensoir_hip.h); +inf when the shell has reached both ends
__device__ __forceinline__ double ds_axis_bound(double p, double origin, double cell, int c, int r, int dim) {
    double b = DS_INF;
    const double slack = cell * TIR_DISTANCE_SLACK;
    if (c - r > 0) b = fmin(b, (p - (origin + (double)(c - r) * cell)) - slack);
    if (c + r + 1 < dim) b = fmin(b, ((origin + (double)(c + r + 1) * cell) - p) - slack);
    return b;
}

// how far p is, along one axis, from the slab of cell x, widened by the same slack (the first and the last slab reach to
// infinity): no point of a face listed in the cell is nearer along this axis
__device__ __forceinline__ double ds_slab(double p, double origin, double cell, int x, int dim) {
    const double slack = cell * TIR_DISTANCE_SLACK;
    double d = 0.0;
    if (x > 0) d = fmax(d, ((origin + (double)x * cell) - slack) - p);
    if (x + 1 < dim) d = fmax(d, p - ((origin + (double)(x + 1) * cell) + slack));
    return d;
}

__global__ void __launch_bounds__(DS_THREADS)
k_point_mesh_distance(const float* __restrict__ points, int64_t n, const float* __restrict__ verts, int64_t V,
                      const int32_t* __restrict__ faces, int64_t F, DsGrid G, const int32_t* __restrict__ cursor,
                      const int32_t* __restrict__ pairs, int64_t n_pairs, float* __restrict__ dist, int32_t* __restrict__ face,
                      float* __restrict__ closest, int32_t* __restrict__ tested) {
    const int64_t i = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    if (i >= n) return;
    const float fx = points[3 * i], fy = points[3 * i + 1], fz = points[3 * i + 2];
    const float nan = __builtin_nanf("");
    if (!(fabsf(fx) < DS_INF && fabsf(fy) < DS_INF && fabsf(fz) < DS_INF)) {
        dist[i] = nan;
        face[i] = -1;
        if (closest) closest[3 * i] = closest[3 * i + 1] = closest[3 * i + 2] = nan;
        if (tested) tested[i] = 0;
        return;
    }
    const double px = fx, py = fy, pz = fz;
    const double ox = G.origin[0], oy = G.origin[1], oz = G.origin[2], sx = G.cell[0], sy = G.cell[1], sz = G.cell[2];
    const int d0 = G.dims[0], d1 = G.dims[1], d2 = G.dims[2];
    const int c0 = ds_cell(fx, G.origin[0], G.cell[0], d0), c1 = ds_cell(fy, G.origin[1], G.cell[1], d1),
              c2 = ds_cell(fz, G.origin[2], G.cell[2], d2);
    const int rmax = max(max(max(c0, d0 - 1 - c0), max(c1, d1 - 1 - c1)), max(c2, d2 - 1 - c2));
    DsBest B{DS_INF, 0.0, 0.0, 0.0, 0x7fffffff};
    int nt = 0;
    for (int r = 0; r <= rmax; ++r) {
        const int za = c2 - r, zb = c2 + r;
        for (int x = max(c0 - r, 0); x <= min(c0 + r, d0 - 1); ++x) {
            const double ex = ds_slab(px, ox, sx, x, d0), ex2 = ex * ex;
            if (ex2 > B.d2) continue;                      // no face of this slice of cells can come as close (or tie)
            for (int y = max(c1 - r, 0); y <= min(c1 + r, d1 - 1); ++y) {
                const double ey = ds_slab(py, oy, sy, y, d1), exy2 = ex2 + ey * ey;
                if (exy2 > B.d2) continue;
                // a column on the rim of the shell belongs to it whole; an inner one (r > 0) meets it at its two ends only
                const bool rim = abs(x - c0) == r || abs(y - c1) == r;
                const int step = rim ? 1 : 2 * r;
                for (int z = za; z <= zb; z += step) {
                    if (z < 0 || z >= d2) continue;
                    const double ez = ds_slab(pz, oz, sz, z, d2);
                    if (exy2 + ez * ez > B.d2) continue;
                    nt += ds_visit(verts, V, faces, F, G, cursor, pairs, n_pairs, x, y, z, px, py, pz, B);
                }
            }
        }
        const double b = fmin(fmin(ds_axis_bound(px, ox, sx, c0, r, d0), ds_axis_bound(py, oy, sy, c1, r, d1)),
                              ds_axis_bound(pz, oz, sz, c2, r, d2));
        if (b > 0.0 && b * b > B.d2) break;                // nothing beyond this shell can come as close (or tie)
    }
    const bool found = B.face != 0x7fffffff;
    dist[i] = found ? (float)sqrt(B.d2) : (float)DS_INF;
    face[i] = found ? B.face : -1;
    if (closest) {
        closest[3 * i] = found ? (float)B.x : nan;
        closest[3 * i + 1] = found ? (float)B.y : nan;
        closest[3 * i + 2] = found ? (float)B.z : nan;
    }
    if (tested) tested[i] = nt;
}

// ---- the ray query ---------------------------------------------------------------------------------------------------------------
// e(P, Q) of the header: e(Q, P) == -e(P, Q) bit for bit (every difference of products is the exact negation of the other one)
__device__ __forceinline__ double rm_edge(double dx, double dy, double dz, double px, double py, double pz, double qx, double qy,
                                          double qz) {
    const double x = d_mul(dx, d_sub(d_mul(py, qz), d_mul(pz, qy)));
    const double y = d_mul(dy, d_sub(d_mul(pz, qx), d_mul(px, qz)));
    const double z = d_mul(dz, d_sub(d_mul(px, qy), d_mul(py, qx)));
    return d_add(d_add(x, y), z);
}

// the ray-triangle rule of the header: true when the LINE meets the face and den != 0; the range is the caller's
__device__ __forceinline__ bool rm_test(const DsTri& T, double ox, double oy, double oz, double dx, double dy, double dz, double& t,
                                        double& u, double& v, double& w) {
    const double ax = d_sub(T.ax, ox), ay = d_sub(T.ay, oy), az = d_sub(T.az, oz);
    const double bx = d_sub(T.bx, ox), by = d_sub(T.by, oy), bz = d_sub(T.bz, oz);
    const double cx = d_sub(T.cx, ox), cy = d_sub(T.cy, oy), cz = d_sub(T.cz, oz);
    u = rm_edge(dx, dy, dz, bx, by, bz, cx, cy, cz);
    v = rm_edge(dx, dy, dz, cx, cy, cz, ax, ay, az);
    w = rm_edge(dx, dy, dz, ax, ay, az, bx, by, bz);
    const bool meets = ((u >= 0.0 && v >= 0.0 && w >= 0.0) || (u <= 0.0 && v <= 0.0 && w <= 0.0)) && !(u == 0.0 && v == 0.0 && w == 0.0);
    const double px = d_sub(T.bx, T.ax), py = d_sub(T.by, T.ay), pz = d_sub(T.bz, T.az);
    const double qx = d_sub(T.cx, T.ax), qy = d_sub(T.cy, T.ay), qz = d_sub(T.cz, T.az);
    const double nx = d_sub(d_mul(py, qz), d_mul(pz, qy));
    const double ny = d_sub(d_mul(pz, qx), d_mul(px, qz));
    const double nz = d_sub(d_mul(px, qy), d_mul(py, qx));
    const double den = d_add(d_add(d_mul(dx, nx), d_mul(dy, ny)), d_mul(dz, nz));
    t = d_div(d_add(d_add(d_mul(ax, nx), d_mul(ay, ny)), d_mul(az, nz)), den);
    return meets && den != 0.0;
}

// one of three values by a runtime axis, as conditional moves (an array indexed by it would become a scratch object)
template <typename T>
__device__ __forceinline__ T rm_sel(int axis, T a0, T a1, T a2) {
    return axis == 0 ? a0 : (axis == 1 ? a1 : a2);
}

// the cell of an fp64 coordinate: rounded to fp32 first, as the cell function takes it (NaN -> cell 0, beyond fp32 -> an end cell)
__device__ __forceinline__ int rm_cell(double x, float origin, float cell, int32_t dim) { return ds_cell((float)x, origin, cell, dim); }

struct RmBest {
    double t, u, v, w;
    int32_t face, count, flags;
};

// every face listed in cell (x, y, z) against the ray; returns the number of faces tested.  MODE TIR_RAY_COUNT takes a hit only
// in the cell of its own hit point (clamped into the cells the face is listed in), so that a face listed in several visited
// cells is counted once; the other two modes keep the nearest / the first hit, which a second meeting does not change.
template <int MODE>
__device__ __forceinline__ int rm_visit(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                                        const DsGrid& G, const int32_t* __restrict__ cursor, const int32_t* __restrict__ pairs,
                                        int64_t n_pairs, int x, int y, int z, double ox, double oy, double oz, double dx, double dy,
                                        double dz, double t0, double t1, RmBest& B) {
    const int32_t key = ds_cell_key(G, x, y, z);
    int64_t k = key ? cursor[key - 1] : 0, end = cursor[key];
    k = k < 0 ? 0 : k;
    end = end < n_pairs ? end : n_pairs;
    const int n_list = end > k ? (int)(end - k) : 0;       // an integer bound known before the loop
    int tested = 0;
    for (int j = 0; j < n_list; ++j) {
        const int32_t f = pairs[k + j];
        int32_t i0, i1, i2;
        if (f < 0 || f >= F || !ds_face(faces, f, V, i0, i1, i2)) continue;
        const DsTri T = ds_corners(verts, i0, i1, i2);
        double t, u, v, w;
        const bool meets = rm_test(T, ox, oy, oz, dx, dy, dz, t, u, v, w);
        ++tested;
        if (!(meets && t >= t0 && t <= t1)) continue;      // (false for a NaN)
        const int grazed = (u == 0.0 || v == 0.0 || w == 0.0) ? TIR_RAY_FLAG_GRAZED : 0;
        if constexpr (MODE == TIR_RAY_COUNT) {
            const int hx = rm_cell(d_add(ox, d_mul(t, dx)), G.origin[0], G.cell[0], G.dims[0]);
            const int hy = rm_cell(d_add(oy, d_mul(t, dy)), G.origin[1], G.cell[1], G.dims[1]);
            const int hz = rm_cell(d_add(oz, d_mul(t, dz)), G.origin[2], G.cell[2], G.dims[2]);
            const float fax = (float)T.ax, fbx = (float)T.bx, fcx = (float)T.cx;       // (exact: the corners came from fp32)
            const float fay = (float)T.ay, fby = (float)T.by, fcy = (float)T.cy;
            const float faz = (float)T.az, fbz = (float)T.bz, fcz = (float)T.cz;
            const int lx = ds_cell(fminf(fax, fminf(fbx, fcx)), G.origin[0], G.cell[0], G.dims[0]);
            const int ux = ds_cell(fmaxf(fax, fmaxf(fbx, fcx)), G.origin[0], G.cell[0], G.dims[0]);
            const int ly = ds_cell(fminf(fay, fminf(fby, fcy)), G.origin[1], G.cell[1], G.dims[1]);
            const int uy = ds_cell(fmaxf(fay, fmaxf(fby, fcy)), G.origin[1], G.cell[1], G.dims[1]);
            const int lz = ds_cell(fminf(faz, fminf(fbz, fcz)), G.origin[2], G.cell[2], G.dims[2]);
            const int uz = ds_cell(fmaxf(faz, fmaxf(fbz, fcz)), G.origin[2], G.cell[2], G.dims[2]);
            if (min(max(hx, lx), ux) != x || min(max(hy, ly), uy) != y || min(max(hz, lz), uz) != z) continue;
            B.count += 1;
            B.flags |= grazed;
        }
        if (t < B.t || (t == B.t && f < B.face)) {
            B.t = t;
            B.u = u;
            B.v = v;
            B.w = w;
            B.face = f;
            if constexpr (MODE != TIR_RAY_COUNT) {
                B.count = 1;
                B.flags = grazed;
            }
        }
    }
    return tested;
}

// The walk of one valid ray (header, "Traversal"): clip to the box of the mesh, take the axis of the largest |d| as the major
// axis, walk its slabs of cells from the entry to the exit, and per slab visit the rectangle of cells that the two other
// coordinates cover over the slab's t interval -- every interval and coordinate widened by the slack.  Every loop runs on an
// integer counter whose bound (at most a grid dimension, or a cell's list length) is known before the loop starts.  The one
// walk of the file: k_ray_mesh and k_shadow_trace both call it.  Returns the number of faces tested.
template <int MODE>
__device__ __forceinline__ int rm_walk(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                                       const DsGrid& G, const int32_t* __restrict__ cursor, const int32_t* __restrict__ pairs,
                                       int64_t n_pairs, const float* __restrict__ bounds, double ox, double oy, double oz, double dx,
                                       double dy, double dz, double t0, double t1, RmBest& B) {
    const double lx = bounds[0], ly = bounds[1], lz = bounds[2], hx = bounds[3], hy = bounds[4], hz = bounds[5];
    // 1. the part of [t0, t1] inside the box of the mesh
    double T0 = t0, T1 = t1;
    bool live = true;
    if (dx == 0.0) {
        live = live && !(ox < lx || ox > hx);
    } else {
        const double a = d_div(d_sub(lx, ox), dx), b = d_div(d_sub(hx, ox), dx);
        T0 = fmax(T0, fmin(a, b));
        T1 = fmin(T1, fmax(a, b));
    }
    if (dy == 0.0) {
        live = live && !(oy < ly || oy > hy);
    } else {
        const double a = d_div(d_sub(ly, oy), dy), b = d_div(d_sub(hy, oy), dy);
        T0 = fmax(T0, fmin(a, b));
        T1 = fmin(T1, fmax(a, b));
    }
    if (dz == 0.0) {
        live = live && !(oz < lz || oz > hz);
    } else {
        const double a = d_div(d_sub(lz, oz), dz), b = d_div(d_sub(hz, oz), dz);
        T0 = fmax(T0, fmin(a, b));
        T1 = fmin(T1, fmax(a, b));
    }
    live = live && T0 <= T1;
    int nt = 0;
    if (live) {
        // 2. the major axis m and the two others p = m + 1, q = m + 2 (mod 3), every per-axis value chosen by conditional moves
        const double adx = fabs(dx), ady = fabs(dy), adz = fabs(dz);
        int m = ady > adx ? 1 : 0;
        m = adz > fmax(adx, ady) ? 2 : m;
        const double ex = d_add(d_mul(TIR_DISTANCE_SLACK, (double)G.cell[0]), d_mul(TIR_RAY_COORD_SLACK, fmax(fabs(lx), fabs(hx))));
        const double ey = d_add(d_mul(TIR_DISTANCE_SLACK, (double)G.cell[1]), d_mul(TIR_RAY_COORD_SLACK, fmax(fabs(ly), fabs(hy))));
        const double ez = d_add(d_mul(TIR_DISTANCE_SLACK, (double)G.cell[2]), d_mul(TIR_RAY_COORD_SLACK, fmax(fabs(lz), fabs(hz))));
        const double om = rm_sel(m, ox, oy, oz), op = rm_sel(m, oy, oz, ox), oq = rm_sel(m, oz, ox, oy);
        const double dm = rm_sel(m, dx, dy, dz), dp = rm_sel(m, dy, dz, dx), dq = rm_sel(m, dz, dx, dy);
        const double em = rm_sel(m, ex, ey, ez), ep = rm_sel(m, ey, ez, ex), eq = rm_sel(m, ez, ex, ey);
        const float gom = rm_sel(m, G.origin[0], G.origin[1], G.origin[2]), gop = rm_sel(m, G.origin[1], G.origin[2], G.origin[0]),
                    goq = rm_sel(m, G.origin[2], G.origin[0], G.origin[1]);
        const float gcm = rm_sel(m, G.cell[0], G.cell[1], G.cell[2]), gcp = rm_sel(m, G.cell[1], G.cell[2], G.cell[0]),
                    gcq = rm_sel(m, G.cell[2], G.cell[0], G.cell[1]);
        const int gdm = rm_sel(m, G.dims[0], G.dims[1], G.dims[2]), gdp = rm_sel(m, G.dims[1], G.dims[2], G.dims[0]),
                  gdq = rm_sel(m, G.dims[2], G.dims[0], G.dims[1]);
        const double tw = d_div(fmax(ex, fmax(ey, ez)), fabs(dm));
        const double T0w = d_sub(T0, tw), T1w = d_add(T1, tw);
        const double x0 = d_add(om, d_mul(T0, dm)), x1 = d_add(om, d_mul(T1, dm));
        const int sa = rm_cell(d_sub(fmin(x0, x1), em), gom, gcm, gdm), sb = rm_cell(d_add(fmax(x0, x1), em), gom, gcm, gdm);
        const bool fwd = dm > 0.0;
        const int n_slabs = sb - sa + 1;                   // <= the grid's dimension along the major axis
        bool done = false;
        for (int k = 0; k < n_slabs && !done; ++k) {
            // 3. the slab's t interval: its two planes moved outward by the slack; the first and the last slab are open-ended
            const int s = fwd ? sa + k : sb - k;
            const double L = d_add((double)gom, d_mul((double)s, (double)gcm)), H = d_add((double)gom, d_mul((double)(s + 1), (double)gcm));
            double tl = d_div(d_sub(d_sub(L, em), om), dm), th = d_div(d_sub(d_add(H, em), om), dm);
            if (s == 0) tl = fwd ? -DS_INF : DS_INF;
            if (s == gdm - 1) th = fwd ? DS_INF : -DS_INF;
            double ta = fwd ? tl : th, tb = fwd ? th : tl;
            // 5. no slab from here on holds a hit below its widened entry (strictly: a tie at B.t could still go to a smaller face)
            if (MODE == TIR_RAY_CLOSEST && B.t < ta) break;
            ta = fmax(ta, T0w);
            tb = fmin(tb, T1w);
            if (!(ta <= tb)) continue;
            // 4. the rectangle of cells the two other coordinates cover over [ta, tb]
            const double pa = d_add(op, d_mul(ta, dp)), pb = d_add(op, d_mul(tb, dp));
            const double qa = d_add(oq, d_mul(ta, dq)), qb = d_add(oq, d_mul(tb, dq));
            const int p0 = rm_cell(d_sub(fmin(pa, pb), ep), gop, gcp, gdp), p1 = rm_cell(d_add(fmax(pa, pb), ep), gop, gcp, gdp);
            const int q0 = rm_cell(d_sub(fmin(qa, qb), eq), goq, gcq, gdq), q1 = rm_cell(d_add(fmax(qa, qb), eq), goq, gcq, gdq);
            const int np = p1 - p0 + 1, nq = q1 - q0 + 1;  // <= the two other dimensions
            for (int jp = 0; jp < np && !done; ++jp) {
                for (int jq = 0; jq < nq && !done; ++jq) {
                    const int cp = p0 + jp, cq = q0 + jq;
                    const int x = rm_sel(m, s, cq, cp), y = rm_sel(m, cp, s, cq), z = rm_sel(m, cq, cp, s);
                    nt += rm_visit<MODE>(verts, V, faces, F, G, cursor, pairs, n_pairs, x, y, z, ox, oy, oz, dx, dy, dz, t0, t1, B);
                    if (MODE == TIR_RAY_ANY && B.count) done = true;
                }
            }
        }
    }
    return nt;
}

// One lane per ray.
template <int MODE>
__global__ void __launch_bounds__(DS_THREADS)
k_ray_mesh(const float* __restrict__ origins, const float* __restrict__ dirs, const float* __restrict__ trange, int64_t n,
           const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F, DsGrid G,
           const int32_t* __restrict__ cursor, const int32_t* __restrict__ pairs, int64_t n_pairs, const float* __restrict__ bounds,
           float* __restrict__ out_t, int32_t* __restrict__ out_face, float* __restrict__ out_bary, int32_t* __restrict__ out_count,
           int32_t* __restrict__ out_flags, int32_t* __restrict__ out_tested) {
    const int64_t i = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    if (i >= n) return;
    const float fox = origins[3 * i], foy = origins[3 * i + 1], foz = origins[3 * i + 2];
    const float fdx = dirs[3 * i], fdy = dirs[3 * i + 1], fdz = dirs[3 * i + 2];
    const float ft0 = trange ? trange[2 * i] : 0.0f, ft1 = trange ? trange[2 * i + 1] : (float)DS_INF;
    const float nan = __builtin_nanf("");
    const bool finite = fabsf(fox) < DS_INF && fabsf(foy) < DS_INF && fabsf(foz) < DS_INF && fabsf(fdx) < DS_INF && fabsf(fdy) < DS_INF &&
                        fabsf(fdz) < DS_INF;               // (false for a NaN)
    if (!(finite && (fdx != 0.0f || fdy != 0.0f || fdz != 0.0f) && ft0 <= ft1)) {
        if (out_t) out_t[i] = nan;
        if (out_face) out_face[i] = -1;
        if (out_bary) out_bary[2 * i] = out_bary[2 * i + 1] = nan;
        if (out_count) out_count[i] = 0;
        if (out_flags) out_flags[i] = TIR_RAY_FLAG_INVALID;
        if (out_tested) out_tested[i] = 0;
        return;
    }
    const double ox = fox, oy = foy, oz = foz, dx = fdx, dy = fdy, dz = fdz, t0 = ft0, t1 = ft1;
    RmBest B{DS_INF, 0.0, 0.0, 0.0, 0x7fffffff, 0, 0};
    const int nt = rm_walk<MODE>(verts, V, faces, F, G, cursor, pairs, n_pairs, bounds, ox, oy, oz, dx, dy, dz, t0, t1, B);
    const bool found = B.face != 0x7fffffff;
    if (out_t) out_t[i] = found ? (float)B.t : (float)DS_INF;
    if (out_face) out_face[i] = found ? B.face : -1;
    if (out_bary) {
        const double sum = d_add(d_add(B.u, B.v), B.w);
        out_bary[2 * i] = found ? (float)d_div(B.v, sum) : nan;
        out_bary[2 * i + 1] = found ? (float)d_div(B.w, sum) : nan;
    }
    if (out_count) out_count[i] = B.count;
    if (out_flags) out_flags[i] = MODE == TIR_RAY_ANY ? 0 : B.flags;
    if (out_tested) out_tested[i] = nt;
}

// ---- traced shadows of the light cells (tir_shadow_trace) -------------------------------------------------------------
// One lane per row, one wave per 64 consecutive rows; the cell is the loop counter of a chunk of ST_CELLS cells, the same in
// every lane, so its record arrives by scalar loads while the row's point and normal stay in registers.  A contributing pair
// (c > 1e-6, tir::light_cosine) walks the grid with rm_walk<TIR_RAY_ANY> over [t0, +inf]; the 64 answers are one ballot that the
// wave's first lane stores.  A wave without a contributing lane skips the walk (the branch is empty for it) and stores 0.
constexpr int ST_CELLS = 16;

__global__ void __launch_bounds__(DS_THREADS)
k_shadow_trace(const float* __restrict__ pts, const float* __restrict__ nrm, const float4* __restrict__ cells, int64_t M, int D,
               const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F, DsGrid G,
               const int32_t* __restrict__ cursor, const int32_t* __restrict__ pairs, int64_t n_pairs, const float* __restrict__ bounds,
               float ft0, unsigned long long* __restrict__ occl, int64_t words) {
    const int64_t m = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    const int64_t word = m >> 6;                           // the same in every lane of the wave: blocks start at multiples of 64
    const bool row = m < M;
    float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    if (row) {
        p0 = pts[3 * m]; p1 = pts[3 * m + 1]; p2 = pts[3 * m + 2];
        n0 = nrm[3 * m]; n1 = nrm[3 * m + 1]; n2 = nrm[3 * m + 2];
    }
    const bool valid = row && fabsf(p0) < DS_INF && fabsf(p1) < DS_INF && fabsf(p2) < DS_INF;      // (false for a NaN)
    const double ox = p0, oy = p1, oz = p2, t0 = ft0;
    for (int d0 = (int)blockIdx.y * ST_CELLS; d0 < D; d0 += (int)gridDim.y * ST_CELLS) {
        const int d1 = min(d0 + ST_CELLS, D);
        for (int d = d0; d < d1; ++d) {
            const float4 ca = cells[2 * (size_t)d];
            const float c = tir::light_cosine(n0, n1, n2, ca.x, ca.y, ca.z);
            const bool ray = fabsf(ca.x) < DS_INF && fabsf(ca.y) < DS_INF && fabsf(ca.z) < DS_INF &&
                             (ca.x != 0.0f || ca.y != 0.0f || ca.z != 0.0f);
            bool hit = false;
            if (valid && ray && c > 1e-6f) {
                RmBest B{DS_INF, 0.0, 0.0, 0.0, 0x7fffffff, 0, 0};
                rm_walk<TIR_RAY_ANY>(verts, V, faces, F, G, cursor, pairs, n_pairs, bounds, ox, oy, oz, (double)ca.x, (double)ca.y,
                                     (double)ca.z, t0, DS_INF, B);
                hit = B.count != 0;
            }
            const unsigned long long bits = __ballot(hit);
            if ((threadIdx.x & 63) == 0 && word < words) occl[(size_t)d * (size_t)words + (size_t)word] = bits;
        }
    }
}

// host-side validation shared by the grid entries and the query: 0, or a negative TIR_ERR_*; fills the grid and the cell count
int ds_validate_grid(int64_t V, int64_t F, const float* cell, const float* origin, const int32_t* dims, DsGrid* G, int64_t* cells) {
    if (!cell || !origin || !dims || V < 0 || F < 0) return TIR_ERR_ARG;
    int64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (!(cell[a] > 0.0f) || !(cell[a] < DS_INF) || !(origin[a] - origin[a] == 0.0f) || dims[a] < 1) return TIR_ERR_ARG;
        G->cell[a] = cell[a];
        G->origin[a] = origin[a];
        G->dims[a] = dims[a];
    }
    for (int a = 0; a < 3; ++a) {
        if (dims[a] > TIR_DISTANCE_MAX_DIM) return TIR_ERR_UNSUPPORTED;
        n *= dims[a];
    }
    if (V > INT32_MAX || F > DS_MAX_FACES) return TIR_ERR_UNSUPPORTED;
    *cells = n;
    return TIR_OK;
}

}  // namespace

extern "C" int64_t tir_distance_blocks(int64_t n) { return n < 0 ? TIR_ERR_ARG : ds_blocks(n, DS_BLOCK); }

extern "C" int tir_mesh_sample_cdf(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int64_t* cdf,
                                   int64_t* sums, int64_t* status, void* stream) {
    if (n_verts < 0 || n_faces < 0) return TIR_ERR_ARG;
    if (n_verts > INT32_MAX || n_faces > DS_MAX_FACES) return TIR_ERR_UNSUPPORTED;
    if (!status) return TIR_ERR_ARG;
    if (n_faces > 0 && (!faces || !cdf || !sums || (n_verts > 0 && !verts))) return TIR_ERR_ARG;
    if (n_faces == 0) return TIR_OK;                       // nothing to do: status is left as the caller zeroed it
    hipStream_t st = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(int64_t), st);
    if (e != hipSuccess) return -(int)e;
    int scale_log2 = 52;                                   // F * 2^scale <= 2^52: the total stays below 2^53
    while (scale_log2 > 0 && ((int64_t)1 << (52 - scale_log2)) < n_faces) --scale_log2;
    const int64_t nb = ds_blocks(n_faces, DS_BLOCK);
    unsigned long long* s = reinterpret_cast<unsigned long long*>(status);
    hipLaunchKernelGGL(k_ms_weight, dim3((unsigned)ds_blocks(n_faces, DS_THREADS)), dim3(DS_THREADS), 0, st, verts, n_verts, faces,
                       n_faces, reinterpret_cast<double*>(cdf), s);
    TIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ms_scan<false>, dim3((unsigned)nb), dim3(DS_THREADS), 0, st, reinterpret_cast<long long*>(cdf), n_faces,
                       scale_log2, reinterpret_cast<long long*>(sums), s);
    TIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ms_scan_blocks, dim3(1), dim3(DS_THREADS), 0, st, reinterpret_cast<long long*>(sums), (int)nb);
    TIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ms_scan<true>, dim3((unsigned)nb), dim3(DS_THREADS), 0, st, reinterpret_cast<long long*>(cdf), n_faces,
                       scale_log2, reinterpret_cast<long long*>(sums), s);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_mesh_sample(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int64_t* cdf,
                               int64_t n, uint64_t seed, float* points, int32_t* face, void* stream) {
    if (n_verts < 0 || n_faces < 0 || n < 0) return TIR_ERR_ARG;
    if (n_verts > INT32_MAX || n_faces > DS_MAX_FACES || n > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    if (n == 0) return TIR_OK;
    if (n_faces == 0 || n_verts == 0 || !verts || !faces || !cdf || !points || !face) return TIR_ERR_ARG;
    hipLaunchKernelGGL(k_ms_draw, dim3((unsigned)ds_blocks(n, DS_THREADS)), dim3(DS_THREADS), 0, tir_stream(stream), verts, n_verts,
                       faces, n_faces, reinterpret_cast<const long long*>(cdf), n, seed, points, face);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_face_grid_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell,
                                   const float* origin, const int32_t* dims, int64_t* status, void* stream) {
    DsGrid G;
    int64_t n_cells = 0;
    const int rc = ds_validate_grid(n_verts, n_faces, cell, origin, dims, &G, &n_cells);
    if (rc) return rc;
    if (!status) return TIR_ERR_ARG;
    if (n_faces > 0 && (!faces || (n_verts > 0 && !verts))) return TIR_ERR_ARG;
    if (n_faces == 0) return TIR_OK;                       // nothing to do: status is left as the caller zeroed it
    hipStream_t st = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(int64_t), st);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(k_fg_count, dim3((unsigned)ds_blocks(n_faces, DS_THREADS)), dim3(DS_THREADS), 0, st, verts, n_verts, faces,
                       n_faces, G, reinterpret_cast<unsigned long long*>(status));
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_face_grid_fill(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell,
                                  const float* origin, const int32_t* dims, int64_t n_pairs, int32_t* cursor, int32_t* counts,
                                  int32_t* offsets, int32_t* pairs, void* stream) {
    DsGrid G;
    int64_t n_cells = 0;
    const int rc = ds_validate_grid(n_verts, n_faces, cell, origin, dims, &G, &n_cells);
    if (rc) return rc;
    if (n_pairs < 0 || !cursor || !counts || !offsets) return TIR_ERR_ARG;
    if (n_pairs > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    if (n_pairs > 0 && (!pairs || !faces || !verts || n_faces == 0)) return TIR_ERR_ARG;
    if (n_pairs == 0) return TIR_OK;                       // no face is listed: the caller's zeroed cursor says every cell is empty
    hipStream_t st = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(cursor, 0, (size_t)n_cells * sizeof(int32_t), st);
    if (e != hipSuccess) return -(int)e;
    const int64_t nbc = ds_blocks(n_cells, DS_BLOCK);
    const unsigned fb = (unsigned)ds_blocks(n_faces, DS_THREADS);
    hipLaunchKernelGGL(k_fg_cells<false>, dim3(fb), dim3(DS_THREADS), 0, st, verts, n_verts, faces, n_faces, G, cursor,
                       (int32_t*)nullptr, n_pairs);
    TIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fg_scan<false>, dim3((unsigned)nbc), dim3(DS_THREADS), 0, st, cursor, n_cells, counts, (const int32_t*)nullptr);
    TIR_CHECK_LAUNCH();
    const int src = tir_exclusive_scan(counts, offsets, (int32_t)nbc, stream);
    if (src) return src;
    hipLaunchKernelGGL(k_fg_scan<true>, dim3((unsigned)nbc), dim3(DS_THREADS), 0, st, cursor, n_cells, (int32_t*)nullptr,
                       (const int32_t*)offsets);
    TIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fg_cells<true>, dim3(fb), dim3(DS_THREADS), 0, st, verts, n_verts, faces, n_faces, G, cursor, pairs, n_pairs);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_point_mesh_distance(const float* points, int64_t n, const float* verts, int64_t n_verts, const int32_t* faces,
                                       int64_t n_faces, const float* cell, const float* origin, const int32_t* dims,
                                       const int32_t* cursor, const int32_t* pairs, int64_t n_pairs, float* dist, int32_t* face,
                                       float* closest, int32_t* tested, void* stream) {
    DsGrid G;
    int64_t n_cells = 0;
    const int rc = ds_validate_grid(n_verts, n_faces, cell, origin, dims, &G, &n_cells);
    if (rc) return rc;
    if (n < 0 || n_pairs < 0) return TIR_ERR_ARG;
    if (n > INT32_MAX || n_pairs > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    if (n == 0) return TIR_OK;
    if (!points || !cursor || !dist || !face) return TIR_ERR_ARG;
    if (n_pairs > 0 && (!pairs || !faces || !verts)) return TIR_ERR_ARG;
    hipLaunchKernelGGL(k_point_mesh_distance, dim3((unsigned)ds_blocks(n, DS_THREADS)), dim3(DS_THREADS), 0, tir_stream(stream), points,
                       n, verts, n_verts, faces, n_faces, G, cursor, pairs, n_pairs, dist, face, closest, tested);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_ray_mesh(const float* origins, const float* dirs, const float* trange, int64_t n, const float* verts, int64_t n_verts,
                            const int32_t* faces, int64_t n_faces, const float* cell, const float* origin, const int32_t* dims,
                            const int32_t* cursor, const int32_t* pairs, int64_t n_pairs, const float* bounds, int mode, float* t,
                            int32_t* face, float* bary, int32_t* count, int32_t* flags, int32_t* tested, void* stream) {
    DsGrid G;
    int64_t n_cells = 0;
    const int rc = ds_validate_grid(n_verts, n_faces, cell, origin, dims, &G, &n_cells);
    if (rc) return rc;
    if (n < 0 || n_pairs < 0) return TIR_ERR_ARG;
    if (mode != TIR_RAY_CLOSEST && mode != TIR_RAY_COUNT && mode != TIR_RAY_ANY) return TIR_ERR_ARG;
    if (mode == TIR_RAY_ANY && (t || face || bary)) return TIR_ERR_ARG;      // which face is met first depends on the grid
    if (n > INT32_MAX || n_pairs > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    if (n == 0) return TIR_OK;
    if (!origins || !dirs || !cursor || !bounds) return TIR_ERR_ARG;
    if (mode == TIR_RAY_ANY ? !count : (!t || !face)) return TIR_ERR_ARG;
    if (n_pairs > 0 && (!pairs || !faces || !verts)) return TIR_ERR_ARG;
    const dim3 grid((unsigned)ds_blocks(n, DS_THREADS)), block(DS_THREADS);
    hipStream_t st = tir_stream(stream);
#define TIR_RAY_LAUNCH(M)                                                                                                         \
    hipLaunchKernelGGL(k_ray_mesh<M>, grid, block, 0, st, origins, dirs, trange, n, verts, n_verts, faces, n_faces, G, cursor, pairs, \
                       n_pairs, bounds, t, face, bary, count, flags, tested)
    if (mode == TIR_RAY_CLOSEST) TIR_RAY_LAUNCH(TIR_RAY_CLOSEST);
    else if (mode == TIR_RAY_COUNT) TIR_RAY_LAUNCH(TIR_RAY_COUNT);
    else TIR_RAY_LAUNCH(TIR_RAY_ANY);
#undef TIR_RAY_LAUNCH
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_shadow_trace(const float* pts, const float* nrm, const float* cells, int64_t M, int32_t D, const float* verts,
                                int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell, const float* origin,
                                const int32_t* dims, const int32_t* cursor, const int32_t* pairs, int64_t n_pairs, const float* bounds,
                                float t0, uint64_t* occl, void* stream) {
    DsGrid G;
    int64_t n_cells = 0;
    const int rc = ds_validate_grid(n_verts, n_faces, cell, origin, dims, &G, &n_cells);
    if (rc) return rc;
    if (M < 0 || n_pairs < 0 || D < 1 || !(t0 >= 0.0f && t0 < (float)DS_INF)) return TIR_ERR_ARG;
    if (D > (1 << 20) || M > INT32_MAX || n_pairs > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    if (M == 0) return TIR_OK;
    if (!pts || !nrm || !cells || !cursor || !bounds || !occl) return TIR_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(cells) % 16 != 0 || reinterpret_cast<uintptr_t>(occl) % 8 != 0) return TIR_ERR_ARG;
    if (n_pairs > 0 && (!pairs || !faces || !verts)) return TIR_ERR_ARG;
    const unsigned chunks = (unsigned)((D + ST_CELLS - 1) / ST_CELLS);
    hipLaunchKernelGGL(k_shadow_trace, dim3((unsigned)ds_blocks(M, DS_THREADS), chunks < 65535u ? chunks : 65535u), dim3(DS_THREADS), 0,
                       tir_stream(stream), pts, nrm, reinterpret_cast<const float4*>(cells), M, (int)D, verts, n_verts, faces, n_faces, G,
                       cursor, pairs, n_pairs, bounds, t0, reinterpret_cast<unsigned long long*>(occl), (M + 63) / 64);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}
