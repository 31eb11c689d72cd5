// Marching-cubes surface extraction of a dense lattice (scripts/export_mesh.py:15-24 -> utils.py:164-226 call
// skimage.measure.marching_cubes on getDenseAlpha's output).  Contract: include/tensoir_hip.h (tir_mc_*).
//
// Three launches plus two single-workgroup scans, no atomics, so the output order is fixed:
//   k_mc_count   per block of MC_BLOCK_POINTS lattice points: crossing edges (= vertices) and triangles
//   scans        tir_exclusive_scan of both count arrays -> per-block vertex / face offsets and the two totals
//   k_mc_verts   block-local scan of the per-point crossing counts: vertices + normals in (point, axis) order, vbase[p]
//   k_mc_faces   block-local scan of the per-cell triangle counts: faces in (cell, table) order; a corner's vertex on the
//                edge along `axis` is vbase[corner] + the number of its crossing edges along lower axes
#define TIR_MC_CONSTANT __constant__
#include "tir_common.hpp"
#include "tir_mc_table.hpp"

using namespace tir;

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_ITERS = 16;
constexpr int MC_BLOCK_POINTS = MC_THREADS * MC_ITERS;   // 4096: 32 K blocks at 512^3, one scan workgroup walks them in 32 chunks

struct McLattice {
    const float* vol;
    int32_t gx, gy, gz;
    int64_t n;        // gx * gy * gz
    float level;
};

__device__ __forceinline__ bool mc_in(const McLattice& L, int64_t p) { return L.vol[p] > L.level; }

// crossing bits of the +x / +y / +z lattice edges of point (x, y, z) whose own inside flag is `in`
__device__ __forceinline__ unsigned mc_cross_bits(const McLattice& L, int64_t p, int x, int y, int z, bool in) {
    const int64_t sy = L.gz, sx = (int64_t)L.gy * L.gz;
    unsigned b = 0;
    if (x + 1 < L.gx && mc_in(L, p + sx) != in) b |= 1u;
    if (y + 1 < L.gy && mc_in(L, p + sy) != in) b |= 2u;
    if (z + 1 < L.gz && mc_in(L, p + 1) != in) b |= 4u;
    return b;
}

// case index of the cell whose lowest corner is point p (caller checks x+1 < gx, y+1 < gy, z+1 < gz)
__device__ __forceinline__ unsigned mc_case(const McLattice& L, int64_t p) {
    const int64_t sy = L.gz, sx = (int64_t)L.gy * L.gz;
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int64_t q = p + ((k & 1) ? sx : 0) + ((k & 2) ? sy : 0) + ((k & 4) ? 1 : 0);
        c |= (unsigned)mc_in(L, q) << k;
    }
    return c;
}

// 32-bit divisions: the lattice has at most 2^31 - 1 points (mc_validate), and a 64-bit division is a long software sequence
__device__ __forceinline__ void mc_coords(const McLattice& L, int64_t p, int& x, int& y, int& z) {
    const uint32_t q = (uint32_t)p, r = q / (uint32_t)L.gz;
    z = (int)(q - r * (uint32_t)L.gz);
    x = (int)(r / (uint32_t)L.gy);
    y = (int)(r - (uint32_t)x * (uint32_t)L.gy);
}

__device__ __forceinline__ bool mc_has_cell(const McLattice& L, int x, int y, int z) {
    return x + 1 < L.gx && y + 1 < L.gy && z + 1 < L.gz;
}

// exclusive scan of one int per thread over the block (4 waves); *total = block sum
__device__ __forceinline__ int mc_block_scan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < MC_THREADS / 64; ++q) {
        int s = wsum[q];
        off += q < wv ? s : 0;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return off + incl - v;
}

__device__ __forceinline__ int mc_block_sum(int v, int* wsum) {
    int t;
    mc_block_scan(v, wsum, &t);
    return t;
}

__global__ void __launch_bounds__(MC_THREADS)
k_mc_count(McLattice L, int32_t* __restrict__ vcount, int32_t* __restrict__ fcount) {
    __shared__ int wsum[MC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * MC_BLOCK_POINTS;
    int nv = 0, nf = 0;
    for (int it = 0; it < MC_ITERS; ++it) {
        const int64_t p = base + it * MC_THREADS + threadIdx.x;
        if (p < L.n) {
            int x, y, z;
            mc_coords(L, p, x, y, z);
            nv += __popc(mc_cross_bits(L, p, x, y, z, mc_in(L, p)));
            if (mc_has_cell(L, x, y, z)) nf += tir_mc_ntri[mc_case(L, p)];
        }
    }
    nv = mc_block_sum(nv, wsum);
    nf = mc_block_sum(nf, wsum);
    if (threadIdx.x == 0) {
        vcount[blockIdx.x] = nv;
        fcount[blockIdx.x] = nf;
    }
}

// one gradient component along an axis of stride s at index i of n: central difference inside, one-sided on the boundary
__device__ __forceinline__ float mc_grad1(const float* vol, int64_t p, int64_t s, int i, int n) {
    if (i > 0 && i + 1 < n) return (vol[p + s] - vol[p - s]) * 0.5f;
    if (i == 0) return vol[p + s] - vol[p];
    return vol[p] - vol[p - s];
}

__device__ __forceinline__ void mc_grad(const McLattice& L, int64_t p, int x, int y, int z, float g[3]) {
    const int64_t sy = L.gz, sx = (int64_t)L.gy * L.gz;
    g[0] = mc_grad1(L.vol, p, sx, x, L.gx);
    g[1] = mc_grad1(L.vol, p, sy, y, L.gy);
    g[2] = mc_grad1(L.vol, p, 1, z, L.gz);
}

struct McPlace {
    float spacing[3];
    float origin[3];
};

__global__ void __launch_bounds__(MC_THREADS)
k_mc_verts(McLattice L, McPlace P, const int32_t* __restrict__ voff, int32_t n_verts, int32_t* __restrict__ vbase,
           float* __restrict__ verts, float* __restrict__ normals) {
    __shared__ int wsum[MC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * MC_BLOCK_POINTS;
    const int64_t sy = L.gz, sx = (int64_t)L.gy * L.gz;
    int carry = voff[blockIdx.x];
    for (int it = 0; it < MC_ITERS; ++it) {
        const int64_t p = base + it * MC_THREADS + threadIdx.x;
        int x = 0, y = 0, z = 0;
        unsigned bits = 0;
        float v0 = 0.f;
        if (p < L.n) {
            mc_coords(L, p, x, y, z);
            v0 = L.vol[p];
            bits = mc_cross_bits(L, p, x, y, z, v0 > L.level);
        }
        int tot;
        int o = carry + mc_block_scan(__popc(bits), wsum, &tot);
        carry += tot;
        if (p >= L.n) continue;
        vbase[p] = o;
        if (!bits) continue;
        const int idx[3] = {x, y, z};
        float g0[3];
        mc_grad(L, p, x, y, z, g0);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(bits & (1u << a))) continue;
            const int64_t q = p + (a == 0 ? sx : a == 1 ? sy : 1);
            const float v1 = L.vol[q];
            // t and the position with every fp32 operation rounded on its own (no contraction): tests/mesh_reference.py
            // restates it bit for bit
            const float t = __fdiv_rn(sub_rn(L.level, v0), sub_rn(v1, v0));
            float g1[3];
            mc_grad(L, q, x + (a == 0), y + (a == 1), z + (a == 2), g1);
            float nrm[3], ss = 0.f;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                nrm[b] = -(g0[b] + t * (g1[b] - g0[b]));
                ss += nrm[b] * nrm[b];
            }
            const float inv = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
            if (o < n_verts) {
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    float c = b == a ? add_rn((float)idx[b], t) : (float)idx[b];
                    verts[(int64_t)o * 3 + b] = add_rn(P.origin[b], mul_rn(c, P.spacing[b]));
                    normals[(int64_t)o * 3 + b] = nrm[b] * inv;
                }
            }
            ++o;
        }
    }
}

// vertex index of the crossing lattice edge that leaves corner point (x, y, z) along `axis`
__device__ __forceinline__ int mc_edge_vertex(const McLattice& L, const int32_t* __restrict__ vbase, int x, int y, int z,
                                              int axis) {
    const int64_t sy = L.gz, sx = (int64_t)L.gy * L.gz;
    const int64_t p = (int64_t)x * sx + (int64_t)y * sy + z;
    int v = vbase[p];
    if (axis > 0) {
        const bool in = mc_in(L, p);
        if (x + 1 < L.gx && mc_in(L, p + sx) != in) ++v;
        if (axis > 1 && y + 1 < L.gy && mc_in(L, p + sy) != in) ++v;
    }
    return v;
}

__global__ void __launch_bounds__(MC_THREADS)
k_mc_faces(McLattice L, const int32_t* __restrict__ foff, int32_t n_faces, const int32_t* __restrict__ vbase,
           int32_t* __restrict__ faces) {
    __shared__ int wsum[MC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * MC_BLOCK_POINTS;
    int carry = foff[blockIdx.x];
    for (int it = 0; it < MC_ITERS; ++it) {
        const int64_t p = base + it * MC_THREADS + threadIdx.x;
        int x = 0, y = 0, z = 0;
        unsigned c = 0, nt = 0;
        if (p < L.n) {
            mc_coords(L, p, x, y, z);
            if (mc_has_cell(L, x, y, z)) {
                c = mc_case(L, p);
                nt = tir_mc_ntri[c];
            }
        }
        int tot;
        int o = carry + mc_block_scan((int)nt, wsum, &tot);
        carry += tot;
        for (unsigned j = 0; j < nt; ++j, ++o) {
            if (o >= n_faces) break;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = tir_mc_tri[c][3 * j + k];
                const int axis = e >> 2, kk = e & 3;
                // the two other axes take the bits of kk, lower axis first
                const int lo = axis == 0 ? 1 : 0, hi = axis == 2 ? 1 : 2;
                int d[3] = {0, 0, 0};
                d[lo] = kk & 1;
                d[hi] = (kk >> 1) & 1;
                faces[(int64_t)o * 3 + k] = mc_edge_vertex(L, vbase, x + d[0], y + d[1], z + d[2], axis);
            }
        }
    }
}

// host-side validation shared by the entry points: blocks of the lattice, or a negative TIR_ERR_*
int64_t mc_validate(int32_t gx, int32_t gy, int32_t gz) {
    if (gx < 2 || gy < 2 || gz < 2) return TIR_ERR_ARG;
    const int64_t n = (int64_t)gx * gy * gz;
    if (n > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    // worst-case totals must fit the int32 offsets / indices: every lattice edge crossing, every cell at TIR_MC_MAX_TRI
    const int64_t edges = (int64_t)(gx - 1) * gy * gz + (int64_t)gx * (gy - 1) * gz + (int64_t)gx * gy * (gz - 1);
    const int64_t cells = (int64_t)(gx - 1) * (gy - 1) * (gz - 1);
    if (edges > INT32_MAX || cells * TIR_MC_MAX_TRI > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    return (n + MC_BLOCK_POINTS - 1) / MC_BLOCK_POINTS;
}

}  // namespace

extern "C" int64_t tir_mc_blocks(int32_t gx, int32_t gy, int32_t gz) { return mc_validate(gx, gy, gz); }

extern "C" int tir_mc_count(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, int32_t* counts,
                            int32_t* offsets, void* stream) {
    const int64_t nb = mc_validate(gx, gy, gz);
    if (nb < 0) return (int)nb;
    if (!vol || !counts || !offsets) return TIR_ERR_ARG;
    const McLattice L{vol, gx, gy, gz, (int64_t)gx * gy * gz, level};
    hipLaunchKernelGGL(k_mc_count, dim3((unsigned)nb), dim3(MC_THREADS), 0, tir_stream(stream), L, counts, counts + nb);
    TIR_CHECK_LAUNCH();
    int rc = tir_exclusive_scan(counts, offsets, (int32_t)nb, stream);
    if (rc) return rc;
    return tir_exclusive_scan(counts + nb, offsets + nb + 1, (int32_t)nb, stream);
}

extern "C" int tir_mc_emit(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, float sx, float sy, float sz,
                           float ox, float oy, float oz, const int32_t* offsets, int32_t n_verts, int32_t n_faces,
                           int32_t* vbase, float* verts, float* normals, int32_t* faces, void* stream) {
    const int64_t nb = mc_validate(gx, gy, gz);
    if (nb < 0) return (int)nb;
    if (!vol || !offsets || n_verts < 0 || n_faces < 0) return TIR_ERR_ARG;
    if (n_verts > 0 && (!vbase || !verts || !normals)) return TIR_ERR_ARG;
    if (n_faces > 0 && (!vbase || !faces || n_verts == 0)) return TIR_ERR_ARG;
    if (n_verts == 0) return TIR_OK;
    const McLattice L{vol, gx, gy, gz, (int64_t)gx * gy * gz, level};
    const McPlace P{{sx, sy, sz}, {ox, oy, oz}};
    hipLaunchKernelGGL(k_mc_verts, dim3((unsigned)nb), dim3(MC_THREADS), 0, tir_stream(stream), L, P, offsets, n_verts,
                       vbase, verts, normals);
    TIR_CHECK_LAUNCH();
    if (n_faces == 0) return TIR_OK;
    hipLaunchKernelGGL(k_mc_faces, dim3((unsigned)nb), dim3(MC_THREADS), 0, tir_stream(stream), L, offsets + nb + 1, n_faces,
                       vbase, faces);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}
