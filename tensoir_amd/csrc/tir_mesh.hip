// Marching-cubes surface extraction of a dense lattice (scripts/export_mesh.py:15-24 -> utils.py:164-226 call
// skimage.measure.marching_cubes on getDenseAlpha's output).  Contract: include/tensoir_hip.h (tir_mc_*).
//
// Three launches plus two single-workgroup scans, no atomics, so the output order is fixed:
//   k_mc_count   per block of MC_BLOCK_POINTS lattice points: crossing edges (= vertices) and triangles
//   scans        tir_exclusive_scan of both count arrays -> per-block vertex / face offsets and the two totals
//   k_mc_verts   block-local scan of the per-point crossing counts: vertices + normals in (point, axis) order, vbase[p]
//   k_mc_faces   block-local scan of the per-cell triangle counts: faces in (cell, table) order; a corner's vertex on the
//                edge along `axis` is vbase[corner] + the number of its crossing edges along lower axes
//
// Connected components of the same lattice (contract: include/tensoir_hip.h, tir_ccl_*): the kernels and their union-find are
// described where they start below ("connected components of {vol > level}").
//
// Per-vertex bake of the exported mesh (tensoir_amd/bake.py; contract: include/tensoir_hip.h, tir_bake_composite and
// tir_irradiance_integrate): two reductions without atomics, every point summed in a fixed order.
//   k_bake_composite        BAKE_LANES lanes per point walk its contiguous record segment of the short inward march
//   k_irradiance_integrate  one wave64 per point walks its contiguous visibility row
//
// Texture atlas of the exported mesh (tensoir_amd/mesh.py, bake_atlas; contract: include/tensoir_hip.h, tir_atlas_*): three
// streaming kernels, described where they start below ("per-triangle texture atlas").
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

// ---- connected components of {vol > level} (contract: include/tensoir_hip.h, tir_ccl_*) ---------------------------
// Union-find whose parent links always point to a SMALLER linear index (atomicMin on the root's own slot), so a tree's root is
// the smallest index of its set and the flattened labels do not depend on the order the unions happened in.
//   k_ccl_local    one workgroup per CCL_TX x CCL_TY x CCL_TZ tile: union-find in LDS over the tile's own links; labels[p] =
//                  the tile-local root as a global index (a tile index and a global index order the tile's points alike)
//   k_ccl_merge    the links that cross a tile face / edge / corner: device-scope atomicMin union-find on labels
//   k_ccl_flatten  labels[p] = root of p
//   k_ccl_roots<false/true>  count per block of MC_BLOCK_POINTS points / emit in ascending order the points with labels[p] == p
//   k_ccl_stats    voxel count and index bounding box per component: integer atomics, one set per run of equal labels per wave
//   k_ccl_filter   out = vol where outside or kept, else fill
// Kernel boundaries are the only global synchronisation; no workgroup waits on another.
constexpr int CCL_TX = 4, CCL_TY = 8, CCL_TZ = 32;
constexpr int CCL_TILE = CCL_TX * CCL_TY * CCL_TZ;        // 1024 points = 4 KB of LDS labels; z fastest as in the lattice
constexpr int CCL_THREADS = 256;                          // thread t owns (lx = 0..3, ly = t >> 5, lz = t & 31)

struct CclGrid {
    int32_t gx, gy, gz;
    int32_t ntx, nty, ntz;    // tiles per axis
    int64_t n;
};

// the 13 neighbours with a smaller linear index, faces first (x, y, z): connectivity 6 takes the first three
__constant__ int8_t ccl_back[13][3] = {{-1, 0, 0}, {0, -1, 0}, {0, 0, -1},
                                       {-1, -1, 0}, {-1, 1, 0}, {-1, 0, -1}, {-1, 0, 1}, {0, -1, -1}, {0, -1, 1},
                                       {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

__device__ __forceinline__ int ccl_lds_find(const volatile int* L, int a) {
    int q = L[a];
    while (q != a) { a = q; q = L[a]; }
    return a;
}

__device__ __forceinline__ void ccl_lds_union(int* L, int a, int b) {
    for (;;) {
        a = ccl_lds_find(L, a);
        b = ccl_lds_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }     // a > b: hang a below b, if a is still a root
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;                                          // a had already been hung below `old`: unite that with b
    }
}

__global__ void __launch_bounds__(CCL_THREADS)
k_ccl_local(const float* __restrict__ vol, float level, CclGrid G, int n_back, int32_t* __restrict__ labels) {
    __shared__ int L[CCL_TILE];
    const uint32_t b = blockIdx.x, bz = b % (uint32_t)G.ntz, br = b / (uint32_t)G.ntz;
    const int x0 = (int)(br / (uint32_t)G.nty) * CCL_TX, y0 = (int)(br % (uint32_t)G.nty) * CCL_TY, z0 = (int)bz * CCL_TZ;
    const int ly = threadIdx.x >> 5, lz = threadIdx.x & 31;
    const int y = y0 + ly, z = z0 + lz;
    const bool col = y < G.gy && z < G.gz;
#pragma unroll
    for (int lx = 0; lx < CCL_TX; ++lx) {
        const int t = lx * (CCL_TY * CCL_TZ) + threadIdx.x;
        bool in = false;
        if (col && x0 + lx < G.gx) in = vol[((int64_t)(x0 + lx) * G.gy + y) * G.gz + z] > level;
        L[t] = in ? t : -1;
    }
    __syncthreads();
#pragma unroll
    for (int lx = 0; lx < CCL_TX; ++lx) {
        const int t = lx * (CCL_TY * CCL_TZ) + threadIdx.x;
        if (L[t] < 0) continue;
        for (int k = 0; k < n_back; ++k) {
            const int qx = lx + ccl_back[k][0], qy = ly + ccl_back[k][1], qz = lz + ccl_back[k][2];
            if (qx < 0 || qy < 0 || qy >= CCL_TY || qz < 0 || qz >= CCL_TZ) continue;
            const int q = (qx * CCL_TY + qy) * CCL_TZ + qz;
            if (L[q] >= 0) ccl_lds_union(L, t, q);        // (never written to or from -1: outside slots stay outside)
        }
    }
    __syncthreads();
    int root[CCL_TX];
#pragma unroll
    for (int lx = 0; lx < CCL_TX; ++lx) {
        const int t = lx * (CCL_TY * CCL_TZ) + threadIdx.x;
        root[lx] = L[t] < 0 ? -1 : ccl_lds_find(L, t);
    }
#pragma unroll
    for (int lx = 0; lx < CCL_TX; ++lx) {
        if (!(col && x0 + lx < G.gx)) continue;
        const int r = root[lx];
        int32_t out = -1;
        if (r >= 0) {
            const int rx = r / (CCL_TY * CCL_TZ), ry = (r / CCL_TZ) % CCL_TY, rz = r % CCL_TZ;
            out = (int32_t)(((int64_t)(x0 + rx) * G.gy + (y0 + ry)) * G.gz + (z0 + rz));
        }
        labels[((int64_t)(x0 + lx) * G.gy + y) * G.gz + z] = out;
    }
}

// Device-scope reads of the forest: served by L2 / memory, where the atomics of other compute units land.  (A stale parent
// would still be an ancestor -- links only ever move to smaller members of the same set -- so this is for progress, not safety.)
__device__ __forceinline__ int32_t ccl_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t ccl_find(const int32_t* L, int32_t a) {
    int32_t q = ccl_load(L + a);
    while (q != a) { a = q; q = ccl_load(L + a); }
    return a;
}

__device__ __forceinline__ void ccl_union(int32_t* L, int32_t a, int32_t b) {
    for (;;) {
        a = ccl_find(L, a);
        b = ccl_find(L, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ void ccl_coords(const CclGrid& G, int64_t p, int& x, int& y, int& z) {
    const uint32_t q = (uint32_t)p, r = q / (uint32_t)G.gz;
    z = (int)(q - r * (uint32_t)G.gz);
    x = (int)(r / (uint32_t)G.gy);
    y = (int)(r - (uint32_t)x * (uint32_t)G.gy);
}

__global__ void __launch_bounds__(CCL_THREADS)
k_ccl_merge(CclGrid G, int n_back, int32_t* labels) {
    const int64_t p = (int64_t)blockIdx.x * CCL_THREADS + threadIdx.x;
    if (p >= G.n) return;
    int x, y, z;
    ccl_coords(G, p, x, y, z);
    const int lx = x % CCL_TX, ly = y % CCL_TY, lz = z % CCL_TZ;
    // a point away from the low faces of its tile (and, with diagonal links, from the high y / z faces) has no link that
    // leaves the tile toward a smaller index
    if (lx > 0 && ly > 0 && lz > 0 && (n_back == 3 || (ly < CCL_TY - 1 && lz < CCL_TZ - 1))) return;
    if (labels[p] < 0) return;
    for (int k = 0; k < n_back; ++k) {
        const int dx = ccl_back[k][0], dy = ccl_back[k][1], dz = ccl_back[k][2];
        const int qx = x + dx, qy = y + dy, qz = z + dz;
        if (qx < 0 || qy < 0 || qy >= G.gy || qz < 0 || qz >= G.gz) continue;
        const bool same_tile = lx + dx >= 0 && ly + dy >= 0 && ly + dy < CCL_TY && lz + dz >= 0 && lz + dz < CCL_TZ;
        if (same_tile) continue;
        const int64_t q = ((int64_t)qx * G.gy + qy) * G.gz + qz;
        if (ccl_load(labels + q) >= 0) ccl_union(labels, (int32_t)p, (int32_t)q);
    }
}

// Concurrent flattening is safe: a slot is only ever overwritten by an ancestor of its point, and roots are never written.
__global__ void __launch_bounds__(CCL_THREADS)
k_ccl_flatten(int64_t n, int32_t* labels) {
    const int64_t p = (int64_t)blockIdx.x * CCL_THREADS + threadIdx.x;
    if (p >= n) return;
    const int32_t l = labels[p];
    if (l < 0 || l == (int32_t)p) return;
    const int32_t r = ccl_find(labels, l);
    if (r != l) labels[p] = r;
}

constexpr int32_t CCL_BOX_EMPTY_LO = 0x7fffffff;

template <bool EMIT>
__global__ void __launch_bounds__(MC_THREADS)
k_ccl_roots(const int32_t* __restrict__ labels, int64_t n, int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
            int32_t K, int32_t* __restrict__ roots, int32_t* __restrict__ sizes, int32_t* __restrict__ boxes) {
    __shared__ int wsum[MC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * MC_BLOCK_POINTS;
    int carry = EMIT ? offsets[blockIdx.x] : 0, nr = 0;
    for (int it = 0; it < MC_ITERS; ++it) {
        const int64_t p = base + it * MC_THREADS + threadIdx.x;
        const int is_root = p < n && labels[p] == (int32_t)p;
        if constexpr (EMIT) {
            int tot;
            const int o = carry + mc_block_scan(is_root, wsum, &tot);
            carry += tot;
            if (is_root && o < K) {
                roots[o] = (int32_t)p;
                sizes[o] = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    boxes[(int64_t)o * 6 + a] = CCL_BOX_EMPTY_LO;
                    boxes[(int64_t)o * 6 + 3 + a] = -1;
                }
            }
        } else {
            nr += is_root;
        }
    }
    if constexpr (!EMIT) {
        nr = mc_block_sum(nr, wsum);
        if (threadIdx.x == 0) counts[blockIdx.x] = nr;
    }
}

// index of `label` in the ascending roots[K], or -1
__device__ __forceinline__ int ccl_component(const int32_t* __restrict__ roots, int32_t K, int32_t label) {
    int lo = 0, hi = K - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (roots[mid] < label) lo = mid + 1; else hi = mid;
    }
    return (K > 0 && roots[lo] == label) ? lo : -1;
}

struct CclAcc {
    int32_t label, count, lo[3], hi[3];
};

// Every lane of the wave calls this together.  Lanes with `flush` hand in their run; each distinct label among them costs the
// wave one table look-up and seven integer atomics (size, three minima, three maxima), issued by its first seven lanes.
__device__ __forceinline__ void ccl_wave_flush(bool flush, const CclAcc& A, const int32_t* __restrict__ roots, int32_t K,
                                               int32_t* __restrict__ sizes, int32_t* __restrict__ boxes) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(flush);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t lab = __shfl(A.label, leader, 64);
        const bool mine = flush && A.label == lab;
        todo &= ~__ballot(mine);
        int32_t v[7];
        v[0] = mine ? A.count : 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[1 + a] = mine ? A.lo[a] : CCL_BOX_EMPTY_LO;
            v[4 + a] = mine ? A.hi[a] : -1;
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            v[0] += __shfl_xor(v[0], s, 64);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[1 + a] = min(v[1 + a], __shfl_xor(v[1 + a], s, 64));
                v[4 + a] = max(v[4 + a], __shfl_xor(v[4 + a], s, 64));
            }
        }
        const int k = ccl_component(roots, K, lab);       // wave-uniform
        if (k < 0) continue;
        if (lane == 0) atomicAdd(&sizes[k], v[0]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (lane == 1 + a) atomicMin(&boxes[(int64_t)k * 6 + a], v[1 + a]);
            if (lane == 4 + a) atomicMax(&boxes[(int64_t)k * 6 + 3 + a], v[4 + a]);
        }
    }
}

__global__ void __launch_bounds__(MC_THREADS)
k_ccl_stats(const int32_t* __restrict__ labels, CclGrid G, const int32_t* __restrict__ roots, int32_t K,
            int32_t* __restrict__ sizes, int32_t* __restrict__ boxes) {
    // a wave walks 64 * MC_ITERS consecutive points, a lane every 64th of them, and keeps the run of equal labels it is in
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * MC_BLOCK_POINTS + (int64_t)wv * (64 * MC_ITERS);
    CclAcc A;
    A.label = -1;
    A.count = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { A.lo[a] = CCL_BOX_EMPTY_LO; A.hi[a] = -1; }
    for (int it = 0; it < MC_ITERS; ++it) {
        const int64_t p = base + it * 64 + lane;
        const int32_t l = p < G.n ? labels[p] : -1;
        const bool change = l >= 0 && A.label >= 0 && l != A.label;
        if (__any(change)) {
            ccl_wave_flush(change, A, roots, K, sizes, boxes);
            if (change) {
                A.label = -1;
                A.count = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a) { A.lo[a] = CCL_BOX_EMPTY_LO; A.hi[a] = -1; }
            }
        }
        if (l >= 0) {
            int c[3];
            ccl_coords(G, p, c[0], c[1], c[2]);
            A.label = l;
            A.count += 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) { A.lo[a] = min(A.lo[a], c[a]); A.hi[a] = max(A.hi[a], c[a]); }
        }
    }
    ccl_wave_flush(A.label >= 0, A, roots, K, sizes, boxes);
}

__global__ void __launch_bounds__(CCL_THREADS)
k_ccl_filter(const float* __restrict__ vol, const int32_t* __restrict__ labels, int64_t n, const int32_t* __restrict__ roots,
             const uint8_t* __restrict__ keep, int32_t K, float fill, float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * CCL_THREADS + threadIdx.x;
    if (p >= n) return;
    const int32_t l = labels[p];
    float v = vol[p];
    if (l >= 0) {
        const int k = ccl_component(roots, K, l);
        if (k < 0 || !keep[k]) v = fill;
    }
    out[p] = v;
}

// host-side validation of the tir_ccl_* entries: 0, or a negative TIR_ERR_*; fills the tile grid
int ccl_validate(int32_t gx, int32_t gy, int32_t gz, CclGrid* G) {
    if (gx <= 0 || gy <= 0 || gz <= 0) return TIR_ERR_ARG;
    const int64_t n = (int64_t)gx * gy * gz;
    if (n > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    G->gx = gx; G->gy = gy; G->gz = gz;
    G->ntx = (gx + CCL_TX - 1) / CCL_TX;
    G->nty = (gy + CCL_TY - 1) / CCL_TY;
    G->ntz = (gz + CCL_TZ - 1) / CCL_TZ;
    G->n = n;
    // one workgroup per tile in a one-dimensional grid (a 1 x N x 1 lattice has N / CCL_TY tiles: always below 2^31)
    if ((int64_t)G->ntx * G->nty * G->ntz > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    return TIR_OK;
}

// ---- simplification by quadric vertex clustering (contract: include/tensoir_hip.h, tir_simplify_*) -----------------
//   k_simplify_key            per vertex: cell key (fp32, every operation rounded on its own) -> cell_of_vertex, slots[key] = 1
//   k_simplify_slots<false/true>  count per block of MC_BLOCK_POINTS slots / rewrite slots[key] = compact id (ascending keys), -1
//   k_simplify_map            cell_of_vertex[v] = slots[key of v]
//   k_simplify_faces<false/true>  per block of MC_BLOCK_POINTS faces: count the faces that survive the remap (and check indices
//                             and extents) / write them at their scanned offsets, in input order
//   k_simplify_status         {V', F'} next to the error word: one read-back
//   k_simplify_accum_verts / _faces  the sums of a cell as integer fixed point, integer atomics whose value is never read back;
//                             a face term takes two 64-bit words (the fixed-point value split at its low 32 bits), which gives
//                             it 32 more fraction bits than one word could hold under the worst-case bound
//   k_simplify_solve          per output vertex: the regularised 3 x 3 system in fp64, position and normal
// The only order-dependent operations are integer additions, so the outputs do not depend on the order the device worked in.
constexpr double SIMP_EXTENT = TIR_SIMPLIFY_EXTENT;
constexpr int SIMP_ACC = TIR_SIMPLIFY_ACC;                 // m, s[3], then (high, low) word pairs of A[6] (00 01 02 11 12 22), b[3], N[3]
constexpr int SIMP_A = 4, SIMP_B = 16, SIMP_N = 22;        // first word of each group
constexpr int64_t SIMP_MAX_FACES = (int64_t)1 << 28;
// fraction bits: |u| <= 4 over < 2^31 vertices; |n_i| <= 2 * 4^2 = 32 >= |A_ij|, |b_i| <= 32 * 8 sqrt(3) < 2^9 over < 2^30 corners
constexpr double SIMP_S_SCALE = (double)(1 << 30), SIMP_A_SCALE = (double)(1 << 28), SIMP_B_SCALE = (double)(1 << 24),
                 SIMP_N_SCALE = (double)(1 << 28);

struct SimpGrid {
    float cell[3], origin[3];
    int32_t dims[3];
};

__device__ __forceinline__ void simp_q(const SimpGrid& G, const float* __restrict__ v, float q[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = __fdiv_rn(sub_rn(v[a], G.origin[a]), G.cell[a]);
}

// clamp(floor(q), 0, dim - 1); fmaxf returns its other operand for a NaN, and the comparison is made before the conversion
__device__ __forceinline__ int simp_index(float q, int32_t dim) {
    const float f = fmaxf(floorf(q), 0.0f);
    return f >= (float)(dim - 1) ? dim - 1 : (int)f;
}

__device__ __forceinline__ int32_t simp_key(const SimpGrid& G, const int i[3]) {
    return (int32_t)(((int64_t)i[0] * G.dims[1] + i[1]) * G.dims[2] + i[2]);       // < 2^31 (simp_validate)
}

__device__ __forceinline__ void simp_add(int64_t* p, double v, double scale, int mult) {
    const long long w = __double2ll_rn(v * scale) * mult;
    if (w) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)w);
}

// v with 32 fraction bits more than `scale` gives one word: p[0] += floor(v scale), p[1] += round((v scale - floor) 2^32), the
// latter in [0, 2^32] and so below 2^62 over 2^30 corners.  Every step before the rounding is exact (a power-of-two scale, the
// difference of a value and its own floor), so the pair is the value rounded once at 2^-32 / scale.
__device__ __forceinline__ void simp_add2(int64_t* p, double v, double scale, int mult) {
    const double y = v * scale, h = floor(y);
    const long long hi = (long long)h * mult;
    const unsigned long long lo = (unsigned long long)__double2ll_rn((y - h) * 4294967296.0) * (unsigned)mult;
    if (hi) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)hi);
    if (lo) atomicAdd(reinterpret_cast<unsigned long long*>(p + 1), lo);
}

// the value of a word pair: the whole part of the low word is carried into the high one first, so that sums whose terms cancel
// come out exactly
__device__ __forceinline__ double simp_value(const int64_t* p, double scale) {
    const unsigned long long lo = (unsigned long long)p[1];
    const long long hi = p[0] + (long long)(lo >> 32);
    return ((double)hi + (double)(lo & 0xffffffffull) * (1.0 / 4294967296.0)) / scale;
}

__global__ void __launch_bounds__(MC_THREADS)
k_simplify_key(const float* __restrict__ verts, int64_t V, SimpGrid G, int32_t* __restrict__ vkey, int32_t* __restrict__ slots,
               int32_t* __restrict__ status) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= V) return;
    float q[3];
    simp_q(G, verts + 3 * v, q);
    int i[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        i[a] = simp_index(q[a], G.dims[a]);
        ok = ok && fabs((double)q[a] - ((double)i[a] + 0.5)) <= SIMP_EXTENT;
    }
    const int32_t key = simp_key(G, i);
    vkey[v] = key;
    slots[key] = 1;                                        // (every writer of a slot writes the same value)
    if (!ok) atomicOr(status + 2, TIR_SIMPLIFY_ERR_VERTEX);
}

template <bool EMIT>
__global__ void __launch_bounds__(MC_THREADS)
k_simplify_slots(int32_t* __restrict__ slots, int64_t n, int32_t* __restrict__ counts, const int32_t* __restrict__ offsets) {
    __shared__ int wsum[MC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * MC_BLOCK_POINTS;
    int carry = EMIT ? offsets[blockIdx.x] : 0, nr = 0;
    for (int it = 0; it < MC_ITERS; ++it) {
        const int64_t p = base + it * MC_THREADS + threadIdx.x;
        const int used = p < n && slots[p] != 0;
        if constexpr (EMIT) {
            int tot;
            const int o = carry + mc_block_scan(used, wsum, &tot);
            carry += tot;
            if (p < n) slots[p] = used ? o : -1;
        } else {
            nr += used;
        }
    }
    if constexpr (!EMIT) {
        nr = mc_block_sum(nr, wsum);
        if (threadIdx.x == 0) counts[blockIdx.x] = nr;
    }
}

__global__ void __launch_bounds__(MC_THREADS)
k_simplify_map(int32_t* __restrict__ cell_of_vertex, int64_t V, const int32_t* __restrict__ slots) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v < V) cell_of_vertex[v] = slots[cell_of_vertex[v]];      // (holds the key, which k_simplify_key formed inside the slots)
}

// the corners of face f, or false when an index lies outside [0, V)
__device__ __forceinline__ bool simp_face(const int32_t* __restrict__ faces, int64_t f, int64_t V, int32_t idx[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        idx[k] = faces[3 * f + k];
        ok = ok && idx[k] >= 0 && idx[k] < V;
    }
    return ok;
}

// the edges q1 - q0 and q2 - q0 in fp64 (differences of fp32 values: exact), or false beyond the extent the scales assume
__device__ __forceinline__ bool simp_edges(const float q[3][3], double e1[3], double e2[3]) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = (double)q[1][a] - (double)q[0][a];
        e2[a] = (double)q[2][a] - (double)q[0][a];
        ok = ok && fabs(e1[a]) <= SIMP_EXTENT && fabs(e2[a]) <= SIMP_EXTENT;       // (false for a NaN)
    }
    return ok;
}

template <bool EMIT>
__global__ void __launch_bounds__(MC_THREADS)
k_simplify_faces(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t F, int64_t V, SimpGrid G,
                 const int32_t* __restrict__ cell_of_vertex, int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
                 int32_t n_out_faces, int32_t* __restrict__ out_faces, int32_t* __restrict__ status) {
    __shared__ int wsum[MC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * MC_BLOCK_POINTS;
    int carry = EMIT ? offsets[blockIdx.x] : 0, nk = 0;
    for (int it = 0; it < MC_ITERS; ++it) {
        const int64_t f = base + it * MC_THREADS + threadIdx.x;
        int32_t idx[3], c[3] = {0, 0, 0};
        int keep = 0;
        if (f < F) {
            if (simp_face(faces, f, V, idx)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = cell_of_vertex[idx[k]];
                keep = c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
                if constexpr (!EMIT) {
                    float q[3][3];
                    double e1[3], e2[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) simp_q(G, verts + 3 * (int64_t)idx[k], q[k]);
                    if (!simp_edges(q, e1, e2)) atomicOr(status + 2, TIR_SIMPLIFY_ERR_FACE_EXTENT);
                }
            } else if constexpr (!EMIT) {
                atomicOr(status + 2, TIR_SIMPLIFY_ERR_FACE_INDEX);
            }
        }
        if constexpr (EMIT) {
            int tot;
            const int o = carry + mc_block_scan(keep, wsum, &tot);
            carry += tot;
            if (keep && o < n_out_faces) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out_faces[(int64_t)o * 3 + k] = c[k];
            }
        } else {
            nk += keep;
        }
    }
    if constexpr (!EMIT) {
        nk = mc_block_sum(nk, wsum);
        if (threadIdx.x == 0) counts[blockIdx.x] = nk;
    }
}

__global__ void k_simplify_status(const int32_t* __restrict__ slot_total, const int32_t* __restrict__ face_total,
                                  int32_t* __restrict__ status) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    status[0] = *slot_total;
    status[1] = *face_total;
}

__global__ void __launch_bounds__(MC_THREADS)
k_simplify_accum_verts(const float* __restrict__ verts, int64_t V, SimpGrid G, const int32_t* __restrict__ cell_of_vertex,
                       int32_t n_out, int64_t* __restrict__ acc, int32_t* __restrict__ keys) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= V) return;
    const int32_t c = cell_of_vertex[v];
    if (c < 0 || c >= n_out) return;
    float q[3];
    simp_q(G, verts + 3 * v, q);
    int i[3];
    double u[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        i[a] = simp_index(q[a], G.dims[a]);
        u[a] = (double)q[a] - ((double)i[a] + 0.5);
        ok = ok && fabs(u[a]) <= SIMP_EXTENT;
    }
    keys[c] = simp_key(G, i);                              // (every vertex of a cell writes the same key)
    if (!ok) return;                                       // reported by k_simplify_key; never added, so no sum can overflow
    int64_t* A = acc + (int64_t)c * SIMP_ACC;
    atomicAdd(reinterpret_cast<unsigned long long*>(A), 1ull);
#pragma unroll
    for (int a = 0; a < 3; ++a) simp_add(A + 1 + a, u[a], SIMP_S_SCALE, 1);
}

__global__ void __launch_bounds__(MC_THREADS)
k_simplify_accum_faces(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t F, int64_t V, SimpGrid G,
                       const int32_t* __restrict__ cell_of_vertex, int32_t n_out, int64_t* __restrict__ acc) {
    const int64_t f = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= F) return;
    int32_t idx[3];
    if (!simp_face(faces, f, V, idx)) return;
    float q[3][3];
    double e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) simp_q(G, verts + 3 * (int64_t)idx[k], q[k]);
    if (!simp_edges(q, e1, e2)) return;
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double l = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(l > 0.0)) return;
    const double inv = 1.0 / l;
    int32_t c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = cell_of_vertex[idx[k]];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // corners that share a cell share every term (the same centre): the first of them adds the integer terms for all
        int mult = 1;
        bool first = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j < k && c[j] == c[k]) first = false;
            if (j > k && c[j] == c[k]) ++mult;
        }
        if (!first || c[k] < 0 || c[k] >= n_out) continue;
        double dn = 0.0;
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double ctr = (double)simp_index(q[k][a], G.dims[a]) + 0.5;
            ok = ok && fabs((double)q[k][a] - ctr) <= SIMP_EXTENT;
            dn += n[a] * ((double)q[0][a] - ctr);
        }
        if (!ok) continue;
        int64_t* A = acc + (int64_t)c[k] * SIMP_ACC;
        simp_add2(A + SIMP_A, n[0] * n[0] * inv, SIMP_A_SCALE, mult);
        simp_add2(A + SIMP_A + 2, n[0] * n[1] * inv, SIMP_A_SCALE, mult);
        simp_add2(A + SIMP_A + 4, n[0] * n[2] * inv, SIMP_A_SCALE, mult);
        simp_add2(A + SIMP_A + 6, n[1] * n[1] * inv, SIMP_A_SCALE, mult);
        simp_add2(A + SIMP_A + 8, n[1] * n[2] * inv, SIMP_A_SCALE, mult);
        simp_add2(A + SIMP_A + 10, n[2] * n[2] * inv, SIMP_A_SCALE, mult);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            simp_add2(A + SIMP_B + 2 * a, n[a] * dn * inv, SIMP_B_SCALE, mult);
            simp_add2(A + SIMP_N + 2 * a, n[a], SIMP_N_SCALE, mult);
        }
    }
}

__global__ void __launch_bounds__(MC_THREADS)
k_simplify_solve(const int64_t* __restrict__ acc, const int32_t* __restrict__ keys, int32_t n_out, SimpGrid G, double reg,
                 float* __restrict__ out_verts, float* __restrict__ out_normals) {
    const int64_t c = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (c >= n_out) return;
    const int64_t* A = acc + c * SIMP_ACC;
    const double m = (double)A[0];
    double mu[3], b[3], N[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mu[a] = m > 0.0 ? (double)A[1 + a] / SIMP_S_SCALE / m : 0.0;
        b[a] = simp_value(A + SIMP_B + 2 * a, SIMP_B_SCALE);
        N[a] = simp_value(A + SIMP_N + 2 * a, SIMP_N_SCALE);
    }
    const double a00 = simp_value(A + SIMP_A, SIMP_A_SCALE), a01 = simp_value(A + SIMP_A + 2, SIMP_A_SCALE),
                 a02 = simp_value(A + SIMP_A + 4, SIMP_A_SCALE), a11 = simp_value(A + SIMP_A + 6, SIMP_A_SCALE),
                 a12 = simp_value(A + SIMP_A + 8, SIMP_A_SCALE), a22 = simp_value(A + SIMP_A + 10, SIMP_A_SCALE);
    const double t = a00 + a11 + a22;
    double x[3] = {mu[0], mu[1], mu[2]};
    if (t > 0.0) {
        const double r = reg * t;
        const double p = a00 + r, d = a11 + r, g = a22 + r;
        const double r0 = b[0] + r * mu[0], r1 = b[1] + r * mu[1], r2 = b[2] + r * mu[2];
        // symmetric positive definite with condition <= about 1 / reg: the cofactor form in fp64 is ample
        const double c00 = d * g - a12 * a12, c01 = a02 * a12 - a01 * g, c02 = a01 * a12 - a02 * d;
        const double c11 = p * g - a02 * a02, c12 = a01 * a02 - p * a12, c22 = p * d - a01 * a01;
        const double idet = 1.0 / (p * c00 + a01 * c01 + a02 * c02);
        const double s0 = (c00 * r0 + c01 * r1 + c02 * r2) * idet, s1 = (c01 * r0 + c11 * r1 + c12 * r2) * idet,
                     s2 = (c02 * r0 + c12 * r1 + c22 * r2) * idet;
        if (fabs(s0) < INFINITY && fabs(s1) < INFINITY && fabs(s2) < INFINITY) { x[0] = s0; x[1] = s1; x[2] = s2; }
    }
    // the cell's index from its key: 32-bit divisions (the key is below 2^31)
    const uint32_t key = (uint32_t)keys[c], kr = key / (uint32_t)G.dims[2];
    const uint32_t ix = kr / (uint32_t)G.dims[1];
    const int i[3] = {(int)ix, (int)(kr - ix * (uint32_t)G.dims[1]), (int)(key - kr * (uint32_t)G.dims[2])};
    double nw[3], ss = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double xa = fmin(fmax(x[a], -0.5), 0.5);
        out_verts[3 * c + a] = (float)((double)G.origin[a] + ((double)i[a] + 0.5 + xa) * (double)G.cell[a]);
        nw[a] = N[a] / (double)G.cell[a];
        ss += nw[a] * nw[a];
    }
    const bool flat = N[0] == 0.0 && N[1] == 0.0 && N[2] == 0.0;         // exact: opposite terms cancel in the integer sums
    const double inv = flat ? 0.0 : 1.0 / sqrt(ss);
    out_normals[3 * c] = (float)(nw[0] * inv);
    out_normals[3 * c + 1] = (float)(nw[1] * inv);
    out_normals[3 * c + 2] = flat ? 1.0f : (float)(nw[2] * inv);
}

// host-side validation shared by the tir_simplify_* entries: 0, or a negative TIR_ERR_*; fills the grid and the slot count
int simp_validate(int64_t V, int64_t F, const float* cell, const float* origin, const int32_t* dims, SimpGrid* G, int64_t* slots) {
    if (!cell || !origin || !dims || V < 0 || F < 0) return TIR_ERR_ARG;
    int64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (!(cell[a] > 0.0f) || dims[a] < 1) return TIR_ERR_ARG;
        G->cell[a] = cell[a];
        G->origin[a] = origin[a];
        G->dims[a] = dims[a];
    }
    for (int a = 0; a < 3; ++a) {
        n *= dims[a];                                      // each factor is below 2^31 and n is checked after every one
        if (n > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    }
    if (V > INT32_MAX || F > SIMP_MAX_FACES) return TIR_ERR_UNSUPPORTED;
    *slots = n;
    return TIR_OK;
}

constexpr int64_t simp_blocks(int64_t n, int per) { return (n + per - 1) / per; }

// ---- per-vertex bake -------------------------------------------------------------------------------------------------------
constexpr int BAKE_LANES = 8;        // a trained surface leaves 5-30 records per ray: 1-4 strides of the segment per lane
constexpr int BAKE_THREADS = 256;
constexpr int BAKE_ROW = 16;           // floats per output row (TIR_BAKE_ROW)

struct BakeBox {
    float mn[3];
    float half[3];                     // (aabb_max - aabb_min) / 2: world = mn + (normalised + 1) * half
};

__global__ void __launch_bounds__(BAKE_THREADS)
k_bake_composite(const int32_t* __restrict__ off, const int32_t* __restrict__ cnt, const float* __restrict__ rec_w,
                 const float* __restrict__ rec_xyz, const float* __restrict__ rec_brdf, const float* __restrict__ rec_normal,
                 const float* __restrict__ origins, const float* __restrict__ dirs, const float* __restrict__ fallback,
                 BakeBox box, int64_t n_points, int64_t n_rec, float* __restrict__ rows) {
    const int64_t p = ((int64_t)blockIdx.x * BAKE_THREADS + threadIdx.x) / BAKE_LANES;
    const int gl = threadIdx.x & (BAKE_LANES - 1);
    // a whole lane group leaves together (BAKE_LANES divides the wave), so the shuffles below never meet a retired lane
    if (p >= n_points) return;
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { o[a] = origins[3 * p + a]; d[a] = dirs[3 * p + a]; }
    // the segment, clipped to the rows that exist (a dropped ray has cnt 0; nothing outside [0, n_rec) is ever read)
    const int c = cnt[p];
    int64_t b = off[p], e = b + c;
    if (c <= 0 || b < 0) { b = 0; e = 0; }
    if (e > n_rec) e = n_rec;
    float acc = 0.f, alb[3] = {0.f, 0.f, 0.f}, rough = 0.f, nv[3] = {0.f, 0.f, 0.f}, depth = 0.f;
    for (int64_t i = b + gl; i < e; i += BAKE_LANES) {
        const float w = rec_w[i];
        const float4 br = *reinterpret_cast<const float4*>(rec_brdf + 4 * i);
        float z = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float world = fmaf(rec_xyz[3 * i + a] + 1.0f, box.half[a], box.mn[a]);
            z = fmaf(world - o[a], d[a], z);
            nv[a] = fmaf(w, rec_normal[3 * i + a], nv[a]);
        }
        acc += w;
        alb[0] = fmaf(w, br.x, alb[0]);
        alb[1] = fmaf(w, br.y, alb[1]);
        alb[2] = fmaf(w, br.z, alb[2]);
        rough = fmaf(w, fmaf(br.w, 0.9f, 0.09f), rough);
        depth = fmaf(w, z, depth);
    }
    // butterfly inside the lane group: every lane ends with the same sums, added in the same order on every call
#pragma unroll
    for (int s = BAKE_LANES / 2; s > 0; s >>= 1) {
        acc += __shfl_xor(acc, s, BAKE_LANES);
        rough += __shfl_xor(rough, s, BAKE_LANES);
        depth += __shfl_xor(depth, s, BAKE_LANES);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            alb[a] += __shfl_xor(alb[a], s, BAKE_LANES);
            nv[a] += __shfl_xor(nv[a], s, BAKE_LANES);
        }
    }
    if (gl >= 4) return;
    const float den = fmaxf(acc, 1e-6f);
    float4 out;
    if (gl == 0) {
        out = make_float4(fminf(fmaxf(alb[0] / den, 0.f), 1.f), fminf(fmaxf(alb[1] / den, 0.f), 1.f),
                          fminf(fmaxf(alb[2] / den, 0.f), 1.f), fminf(fmaxf(rough / den, 0.f), 1.f));
    } else if (gl == 1) {
        const float len = sqrtf(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
        if (acc <= 0.5f || !(len > 1e-6f)) {
            out = make_float4(fallback[3 * p], fallback[3 * p + 1], fallback[3 * p + 2], fminf(acc, 1.0f));
        } else {
            // (the fp32 sum of an opaque ray's weights can end one ulp above 1: the coverage is reported within [0, 1])
            out = make_float4(nv[0] / len, nv[1] / len, nv[2] / len, fminf(acc, 1.0f));
        }
    } else if (gl == 2) {
        const float t = depth / den;
        out = make_float4(fmaf(d[0], t, o[0]), fmaf(d[1], t, o[1]), fmaf(d[2], t, o[2]), depth);
    } else {
        out = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    *reinterpret_cast<float4*>(rows + BAKE_ROW * p + 4 * gl) = out;    // 4 x 16 bytes: one 64-byte row per lane group
}

// VEC4: D % 4 == 0 and a 16-byte aligned vis -- a lane takes four neighbouring directions per 16-byte load.
// The direction / weight / radiance tables (28 bytes per direction, 14 KB at D = 512) are read straight from global memory:
// every wave reads the same few KB, which stay in the vector L1 / L2; staging them in LDS would cost a workgroup of four
// points more bytes than its four visibility rows.
template <bool VEC4>
__global__ void __launch_bounds__(BAKE_THREADS)
k_irradiance_integrate(const float* __restrict__ rows, const float* __restrict__ dirs, const float* __restrict__ vis,
                       const float* __restrict__ env, const float* __restrict__ weight_d, const int32_t* __restrict__ light_idx,
                       int64_t M, int D, int n_lights, float* __restrict__ out) {
    const int64_t m = (int64_t)blockIdx.x * (BAKE_THREADS / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;                                           // wave-uniform
    const float4 r1 = *reinterpret_cast<const float4*>(rows + BAKE_ROW * m + 4);      // normal, coverage
    if (!(r1.w > 0.5f)) {                                         // no surface here: unoccluded, unlit
        if (lane == 0) *reinterpret_cast<float4*>(out + 4 * m) = make_float4(1.f, 0.f, 0.f, 0.f);
        return;
    }
    int li = light_idx[m];
    li = li < 0 ? 0 : (li >= n_lights ? n_lights - 1 : li);
    const float* __restrict__ e = env + (size_t)li * D * 3;
    const float* __restrict__ v = vis + (size_t)m * D;
    float num = 0.f, den = 0.f, irr[3] = {0.f, 0.f, 0.f};
    constexpr int PER = VEC4 ? 4 : 1;
    for (int d0 = lane * PER; d0 < D; d0 += 64 * PER) {
        float vv[PER];
        if constexpr (VEC4) {
            const float4 q = *reinterpret_cast<const float4*>(v + d0);
            vv[0] = q.x; vv[1] = q.y; vv[2] = q.z; vv[3] = q.w;
        } else {
            vv[0] = v[d0];
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int d = d0 + j;
            // the cosine exactly as the caller's activity mask forms it: three products, two sums, each rounded on its own
            const float c = add_rn(add_rn(mul_rn(dirs[3 * d], r1.x), mul_rn(dirs[3 * d + 1], r1.y)), mul_rn(dirs[3 * d + 2], r1.z));
            if (!(c > 1e-6f)) continue;
            const float cw = c * weight_d[d];
            const float vc = vv[j] * cw;
            den += cw;
            num += vc;
            irr[0] = fmaf(vc, e[3 * d], irr[0]);
            irr[1] = fmaf(vc, e[3 * d + 1], irr[1]);
            irr[2] = fmaf(vc, e[3 * d + 2], irr[2]);
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        num += __shfl_xor(num, s, 64);
        den += __shfl_xor(den, s, 64);
#pragma unroll
        for (int a = 0; a < 3; ++a) irr[a] += __shfl_xor(irr[a], s, 64);
    }
    if (lane == 0) *reinterpret_cast<float4*>(out + 4 * m) = make_float4(den > 0.f ? num / den : 1.f, irr[0], irr[1], irr[2]);
}

// ---- per-triangle texture atlas (contract: include/tensoir_hip.h, tir_atlas_*) ---------------------------------------
//   k_atlas_corners  one thread per face corner: the unwelded vertex, its uv and its tangent
//   k_atlas_texels   one thread per texel of the used cells (cell-major): the surface point and unit normal the bake is run at
//   k_atlas_pack     one thread per texel of the image: the three RGBA8 images from the per-texel bake results
// A texel's owner and its clamped barycentrics are integer arithmetic (quarter texels) followed by three fp32 divisions of exact
// numbers, so all three kernels -- and the numpy restatement -- derive the same fp32 barycentrics for a texel.
constexpr int ATLAS_THREADS = 256;

struct AtlasLayout {
    int32_t size, cols, T;
    int32_t n_cells;
    int64_t n_faces, n_verts;
};

// nearest point of the triangle (0, 0), (L, 0), (0, L) to (X, Y), all in quarter texels -> (qx, qy)
__device__ __forceinline__ void atlas_nearest(int X, int Y, int L, int& qx, int& qy) {
    if (X >= 0 && Y >= 0 && X + Y <= L) { qx = X; qy = Y; return; }
    const int ax = min(max(X, 0), L), by = min(max(Y, 0), L), u = min(max((L - X + Y) / 2, 0), L);   // L - X + Y is even
    const int64_t d0 = (int64_t)(X - ax) * (X - ax) + (int64_t)Y * Y;
    const int64_t d1 = (int64_t)X * X + (int64_t)(Y - by) * (Y - by);
    const int64_t d2 = (int64_t)(X - (L - u)) * (X - (L - u)) + (int64_t)(Y - u) * (Y - u);
    qx = ax; qy = 0;
    int64_t d = d0;
    if (d1 < d) { d = d1; qx = 0; qy = by; }
    if (d2 < d) { qx = L - u; qy = u; }
}

// cell-local texel (i, j) of cell c -> owning face, and the barycentrics of the texel centre clamped to the owner's UV triangle
__device__ __forceinline__ int64_t atlas_owner(const AtlasLayout& A, int c, int i, int j, float b[3]) {
    const int T = A.T;
    const bool upper = i + j >= T && 2 * (int64_t)c + 1 < A.n_faces;
    // centre minus corner 0, in quarter texels: (i + 0.5) - 1, or T - (i + 0.5) - 1 for the upper face (the cell turned by 180 degrees)
    const int X = upper ? 4 * (T - i) - 6 : 4 * i - 2, Y = upper ? 4 * (T - j) - 6 : 4 * j - 2, L = 4 * (T - 4);
    int qx, qy;
    atlas_nearest(X, Y, L, qx, qy);
    b[0] = __fdiv_rn((float)(L - qx - qy), (float)L);
    b[1] = __fdiv_rn((float)qx, (float)L);
    b[2] = __fdiv_rn((float)qy, (float)L);
    return 2 * (int64_t)c + (upper ? 1 : 0);
}

struct AtlasFace {
    float v[3][3], n[3][3];
};

// the face's three vertices and vertex normals; false (nothing read) when an index lies outside [0, V)
__device__ __forceinline__ bool atlas_load_face(const float* __restrict__ verts, const float* __restrict__ normals,
                                                const int32_t* __restrict__ faces, int64_t f, int64_t n_verts, AtlasFace& F) {
    int32_t id[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) id[k] = faces[3 * f + k];
    if (id[0] < 0 || id[1] < 0 || id[2] < 0 || id[0] >= n_verts || id[1] >= n_verts || id[2] >= n_verts) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            F.v[k][a] = verts[3 * (int64_t)id[k] + a];
            F.n[k][a] = normals[3 * (int64_t)id[k] + a];
        }
    return true;
}

__device__ __forceinline__ float atlas_len(const float x[3]) { return sqrtf(fmaf(x[2], x[2], fmaf(x[1], x[1], x[0] * x[0]))); }

// normalize(sum b_k n_k); the face normal when that sum is shorter than 1e-20 (or not a number), then (0, 0, 1)
__device__ __forceinline__ void atlas_normal(const AtlasFace& F, const float b[3], float n[3]) {
    float s[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] = fmaf(b[2], F.n[2][a], fmaf(b[1], F.n[1][a], b[0] * F.n[0][a]));
    float l = atlas_len(s);
    if (!(l >= 1e-20f)) {
        float e1[3], e2[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { e1[a] = F.v[1][a] - F.v[0][a]; e2[a] = F.v[2][a] - F.v[0][a]; }
        s[0] = e1[1] * e2[2] - e1[2] * e2[1];
        s[1] = e1[2] * e2[0] - e1[0] * e2[2];
        s[2] = e1[0] * e2[1] - e1[1] * e2[0];
        l = atlas_len(s);
        if (!(l >= 1e-20f)) { s[0] = 0.f; s[1] = 0.f; s[2] = 1.f; l = 1.f; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a] = s[a] / l;
}

// t = normalize(e - n (n . e)) with e the world direction of +u on the face; when that is shorter than 1e-20 the same with the
// coordinate axis of n's smallest |component| (the first of equals) in place of e, which is never short for a unit n
__device__ __forceinline__ void atlas_tangent(const AtlasFace& F, bool upper, const float n[3], float t[3]) {
    float e[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) e[a] = upper ? F.v[0][a] - F.v[1][a] : F.v[1][a] - F.v[0][a];
    float d = fmaf(n[2], e[2], fmaf(n[1], e[1], n[0] * e[0]));
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = fmaf(-n[a], d, e[a]);
    float l = atlas_len(t);
    if (!(l >= 1e-20f)) {
        const float a0 = fabsf(n[0]), a1 = fabsf(n[1]), a2 = fabsf(n[2]);
        const int ax = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
        d = ax == 0 ? n[0] : (ax == 1 ? n[1] : n[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) t[a] = fmaf(-n[a], d, a == ax ? 1.f : 0.f);
        l = atlas_len(t);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = t[a] / l;
}

// The corner's tangent (steps 4 and 5 at the corner, where sum b_k n_k is the vertex normal) in double, rounded once.  On the thin
// triangles of a simplified mesh the vertex normal can lie almost along the edge: e - n (n . e) then cancels to a small part of
// |e|, and float32 arithmetic -- the restatement's as well as the kernel's -- is several 1e-6 from the exact unit vector (2e-6 to
// 4e-6 on simplified trained fields).  The tangent goes into the asset, 3 F values per export: the double form costs nothing.
__device__ __forceinline__ double atlas_len_d(const double x[3]) { return sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]); }

__device__ __forceinline__ void atlas_corner_tangent(const AtlasFace& F, int k, bool upper, float t_out[3]) {
    double s[3], e[3], t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)          // sum b_k n_k with b the corner's unit vector (a NaN in another vertex normal still counts)
        s[a] = (k == 0 ? 1.0 : 0.0) * (double)F.n[0][a] + (k == 1 ? 1.0 : 0.0) * (double)F.n[1][a] + (k == 2 ? 1.0 : 0.0) * (double)F.n[2][a];
    double l = atlas_len_d(s);
    if (!(l >= 1e-20)) {
        double e1[3], e2[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { e1[a] = (double)F.v[1][a] - (double)F.v[0][a]; e2[a] = (double)F.v[2][a] - (double)F.v[0][a]; }
        s[0] = e1[1] * e2[2] - e1[2] * e2[1];
        s[1] = e1[2] * e2[0] - e1[0] * e2[2];
        s[2] = e1[0] * e2[1] - e1[1] * e2[0];
        l = atlas_len_d(s);
        if (!(l >= 1e-20)) { s[0] = 0.0; s[1] = 0.0; s[2] = 1.0; l = 1.0; }
    }
    const double n[3] = {s[0] / l, s[1] / l, s[2] / l};
#pragma unroll
    for (int a = 0; a < 3; ++a) e[a] = upper ? (double)F.v[0][a] - (double)F.v[1][a] : (double)F.v[1][a] - (double)F.v[0][a];
    double d = n[0] * e[0] + n[1] * e[1] + n[2] * e[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = e[a] - n[a] * d;
    l = atlas_len_d(t);
    if (!(l >= 1e-20)) {
        const double a0 = fabs(n[0]), a1 = fabs(n[1]), a2 = fabs(n[2]);
        const int ax = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
        d = ax == 0 ? n[0] : (ax == 1 ? n[1] : n[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) t[a] = (a == ax ? 1.0 : 0.0) - n[a] * d;
        l = atlas_len_d(t);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) t_out[a] = (float)(t[a] / l);
}

__global__ void __launch_bounds__(ATLAS_THREADS)
k_atlas_corners(const float* __restrict__ verts, const float* __restrict__ normals, const int32_t* __restrict__ faces,
                AtlasLayout A, float* __restrict__ pos, float* __restrict__ nrm, float* __restrict__ tan, float* __restrict__ uv,
                int32_t* __restrict__ status) {
    const int64_t q = (int64_t)blockIdx.x * ATLAS_THREADS + threadIdx.x;
    if (q >= 3 * A.n_faces) return;
    const int64_t f = q / 3;
    const int k = (int)(q - 3 * f);
    const bool upper = f & 1;
    const int c = (int)(f >> 1), T = A.T;
    const int cx = k == 1 ? T - 3 : 1, cy = k == 2 ? T - 3 : 1;                     // the lower face's corner, cell-local
    const int x = (c % A.cols) * T + (upper ? T - cx : cx), y = (c / A.cols) * T + (upper ? T - cy : cy);
    uv[2 * q] = __fdiv_rn((float)x, (float)A.size);
    uv[2 * q + 1] = __fdiv_rn((float)y, (float)A.size);
    AtlasFace F;
    float t[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f}, m[3] = {0.f, 0.f, 0.f};
    if (atlas_load_face(verts, normals, faces, f, A.n_verts, F)) {
        atlas_corner_tangent(F, k, upper, t);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = k == 0 ? F.v[0][a] : (k == 1 ? F.v[1][a] : F.v[2][a]);
            m[a] = k == 0 ? F.n[0][a] : (k == 1 ? F.n[1][a] : F.n[2][a]);
        }
    } else {
        *status = 1;                                   // every writer stores the same word: no atomic needed
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { pos[3 * q + a] = p[a]; nrm[3 * q + a] = m[a]; }
    *reinterpret_cast<float4*>(tan + 4 * q) = make_float4(t[0], t[1], t[2], 1.f);
}

// VEC: point and outward are 16-byte aligned -- a block's 256 x 3 floats go through LDS and leave as 192 16-byte stores
template <bool VEC>
__global__ void __launch_bounds__(ATLAS_THREADS)
k_atlas_texels(const float* __restrict__ verts, const float* __restrict__ normals, const int32_t* __restrict__ faces,
               AtlasLayout A, int32_t n_texels, float* __restrict__ point, float* __restrict__ outward,
               int32_t* __restrict__ face, int32_t* __restrict__ status) {
    __shared__ __align__(16) float s_p[VEC ? 3 * ATLAS_THREADS : 4], s_o[VEC ? 3 * ATLAS_THREADS : 4];      // read back 16 bytes at a time
    const int32_t base = (int32_t)blockIdx.x * ATLAS_THREADS, idx = base + (int32_t)threadIdx.x;
    float p[3] = {0.f, 0.f, 0.f}, o[3] = {0.f, 0.f, 1.f};
    if (idx < n_texels) {
        const int tt = A.T * A.T, c = idx / tt, r = idx - c * tt, j = r / A.T, i = r - j * A.T;
        float b[3];
        const int64_t f = atlas_owner(A, c, i, j, b);
        face[idx] = (int32_t)f;
        AtlasFace F;
        if (atlas_load_face(verts, normals, faces, f, A.n_verts, F)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = fmaf(b[2], F.v[2][a], fmaf(b[1], F.v[1][a], b[0] * F.v[0][a]));
            atlas_normal(F, b, o);
        } else {
            *status = 1;
        }
    }
    if constexpr (VEC) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_p[3 * threadIdx.x + a] = p[a]; s_o[3 * threadIdx.x + a] = o[a]; }
        __syncthreads();
        const int n_fl = 3 * min(ATLAS_THREADS, n_texels - base), o4 = 4 * (int)threadIdx.x;      // floats this block owns
        if (o4 >= n_fl) return;
        float* gp = point + 3 * (int64_t)base + o4;
        float* go = outward + 3 * (int64_t)base + o4;
        if (o4 + 4 <= n_fl) {
            *reinterpret_cast<float4*>(gp) = *reinterpret_cast<const float4*>(s_p + o4);
            *reinterpret_cast<float4*>(go) = *reinterpret_cast<const float4*>(s_o + o4);
        } else {
            for (int k = 0; o4 + k < n_fl; ++k) { gp[k] = s_p[o4 + k]; go[k] = s_o[o4 + k]; }
        }
    } else {
        if (idx >= n_texels) return;
#pragma unroll
        for (int a = 0; a < 3; ++a) { point[3 * (int64_t)idx + a] = p[a]; outward[3 * (int64_t)idx + a] = o[a]; }
    }
}

// round(255 x) of a value in [0, 1] (a NaN counts as 0)
__device__ __forceinline__ unsigned atlas_u8(float x) { return tir::unorm8(x); }

// relight.linear2srgb_torch, its + 1e-6 included
__device__ __forceinline__ float atlas_srgb(float c) {
    const float x = fminf(fmaxf(c, 0.f), 1.f);
    return x <= 0.0031308f ? x * 12.92f : 1.055f * powf(x + 1e-6f, 1.0f / 2.4f) - 0.055f;
}

__device__ __forceinline__ uint32_t atlas_rgba(unsigned r, unsigned g, unsigned b) { return r | (g << 8) | (b << 16) | 0xff000000u; }

struct AtlasBake {
    const float *albedo, *irradiance, *roughness, *ao, *normal, *coverage;     // cell-major; irradiance and ao may be null
};

__global__ void __launch_bounds__(ATLAS_THREADS)
k_atlas_pack(const float* __restrict__ verts, const float* __restrict__ normals, const int32_t* __restrict__ faces, AtlasLayout A,
             AtlasBake B, uint32_t* __restrict__ base, uint32_t* __restrict__ orm, uint32_t* __restrict__ nimg,
             int32_t* __restrict__ status) {
    const int32_t px = (int32_t)blockIdx.x * ATLAS_THREADS + (int32_t)threadIdx.x;
    if (px >= A.size * A.size) return;
    const int y = px / A.size, x = px - y * A.size, T = A.T;
    const int cx = x / T, cy = y / T, c = cy * A.cols + cx;
    uint32_t o_base = atlas_rgba(0, 0, 0), o_orm = o_base, o_n = atlas_rgba(128, 128, 255);       // an unowned texel
    AtlasFace F;
    float b[3];
    if (cx < A.cols && c < A.n_cells) {
        const int i = x - cx * T, j = y - cy * T;
        const int64_t f = atlas_owner(A, c, i, j, b);
        if (atlas_load_face(verts, normals, faces, f, A.n_verts, F)) {
            const int64_t k = (int64_t)c * T * T + j * T + i;
            float col[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                col[a] = B.albedo[3 * k + a];
                if (B.irradiance) col[a] = fminf(fmaxf(col[a] / 3.14159265358979323846f * B.irradiance[3 * k + a], 0.f), 1.f);
            }
            o_base = atlas_rgba(atlas_u8(atlas_srgb(col[0])), atlas_u8(atlas_srgb(col[1])), atlas_u8(atlas_srgb(col[2])));
            o_orm = atlas_rgba(B.ao ? atlas_u8(B.ao[k]) : 255u, atlas_u8(B.roughness[k]), 0);
            if (B.coverage[k] > 0.5f) {
                float n[3], t[3];
                atlas_normal(F, b, n);
                atlas_tangent(F, f & 1, n, t);
                const float bt[3] = {n[1] * t[2] - n[2] * t[1], n[2] * t[0] - n[0] * t[2], n[0] * t[1] - n[1] * t[0]};
                const float N[3] = {B.normal[3 * k], B.normal[3 * k + 1], B.normal[3 * k + 2]};
                const float dt = fmaf(N[2], t[2], fmaf(N[1], t[1], N[0] * t[0]));
                const float db = fmaf(N[2], bt[2], fmaf(N[1], bt[1], N[0] * bt[0]));
                const float dn = fmaf(N[2], n[2], fmaf(N[1], n[1], N[0] * n[0]));
                o_n = atlas_rgba(atlas_u8(fmaf(0.5f, dt, 0.5f)), atlas_u8(fmaf(0.5f, db, 0.5f)), atlas_u8(fmaf(0.5f, dn, 0.5f)));
            }
        } else {
            *status = 1;
        }
    }
    base[px] = o_base;
    orm[px] = o_orm;
    nimg[px] = o_n;
}

// host-side validation shared by the tir_atlas_* entries: 0, or a negative TIR_ERR_*; fills the layout
int atlas_validate(int64_t V, int64_t F, int32_t size, int32_t cols, int32_t T, AtlasLayout* A) {
    if (V < 0 || F < 0 || size < 6 || cols < 1 || (int64_t)cols * T > size) return TIR_ERR_ARG;
    if (T < 6 || size > 8192 || V > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    const int64_t n_cells = (F + 1) / 2, rows = (n_cells + cols - 1) / cols;
    if (rows * T > size) return TIR_ERR_ARG;
    A->size = size; A->cols = cols; A->T = T;
    A->n_cells = (int32_t)n_cells;
    A->n_faces = F; A->n_verts = V;
    return TIR_OK;
}

}  // namespace

extern "C" int tir_bake_composite(const int32_t* ray_rec_off, const int32_t* ray_rec_cnt, const float* rec_w, const float* rec_xyz,
                                  const float* rec_brdf, const float* rec_normal, const float* origins, const float* dirs,
                                  const float* fallback_normal, const float* aabb, int64_t n_points, int64_t n_rec, float* rows,
                                  void* stream) {
    if (n_points < 0 || n_rec < 0 || !aabb) return TIR_ERR_ARG;
    if (n_points == 0) return TIR_OK;
    if (!ray_rec_off || !ray_rec_cnt || !origins || !dirs || !fallback_normal || !rows) return TIR_ERR_ARG;
    if (n_rec > 0 && (!rec_w || !rec_xyz || !rec_brdf || !rec_normal)) return TIR_ERR_ARG;
    if (((uintptr_t)rows | (uintptr_t)rec_brdf) & 15) return TIR_ERR_ARG;
    const int64_t nblk = (n_points * BAKE_LANES + BAKE_THREADS - 1) / BAKE_THREADS;
    if (nblk > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    BakeBox box;
    for (int a = 0; a < 3; ++a) {
        box.mn[a] = aabb[a];
        box.half[a] = (aabb[3 + a] - aabb[a]) * 0.5f;
    }
    hipLaunchKernelGGL(k_bake_composite, dim3((unsigned)nblk), dim3(BAKE_THREADS), 0, tir_stream(stream), ray_rec_off,
                       ray_rec_cnt, rec_w, rec_xyz, rec_brdf, rec_normal, origins, dirs, fallback_normal, box, n_points, n_rec,
                       rows);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_irradiance_integrate(const float* rows, const float* dirs, const float* vis, const float* env,
                                        const float* weight_d, const int32_t* light_idx, int64_t M, int32_t D, int32_t n_lights,
                                        float* out, void* stream) {
    if (M < 0 || D <= 0 || n_lights <= 0) return TIR_ERR_ARG;
    if (M == 0) return TIR_OK;
    if (!rows || !dirs || !vis || !env || !weight_d || !light_idx || !out) return TIR_ERR_ARG;
    if (((uintptr_t)rows | (uintptr_t)out) & 15) return TIR_ERR_ARG;
    const int64_t nblk = (M + BAKE_THREADS / 64 - 1) / (BAKE_THREADS / 64);
    if (nblk > INT32_MAX) return TIR_ERR_UNSUPPORTED;
    if (D % 4 == 0 && ((uintptr_t)vis & 15) == 0)
        hipLaunchKernelGGL(k_irradiance_integrate<true>, dim3((unsigned)nblk), dim3(BAKE_THREADS), 0, tir_stream(stream), rows,
                           dirs, vis, env, weight_d, light_idx, M, (int)D, (int)n_lights, out);
    else
        hipLaunchKernelGGL(k_irradiance_integrate<false>, dim3((unsigned)nblk), dim3(BAKE_THREADS), 0, tir_stream(stream), rows,
                           dirs, vis, env, weight_d, light_idx, M, (int)D, (int)n_lights, out);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_atlas_corners(const float* verts, int64_t n_verts, const float* normals, const int32_t* faces, int64_t n_faces,
                                 int32_t size, int32_t cols, int32_t T, float* pos, float* nrm, float* tan, float* uv,
                                 int32_t* status, void* stream) {
    AtlasLayout A;
    if (!status || (n_faces > 0 && (!verts || !normals || !faces || !pos || !nrm || !tan || !uv))) return TIR_ERR_ARG;
    const int rc = atlas_validate(n_verts, n_faces, size, cols, T, &A);
    if (rc) return rc;
    if ((uintptr_t)tan & 15) return TIR_ERR_ARG;
    if (n_faces == 0) return TIR_OK;
    hipStream_t st = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(k_atlas_corners, dim3((unsigned)((3 * n_faces + ATLAS_THREADS - 1) / ATLAS_THREADS)), dim3(ATLAS_THREADS), 0,
                       st, verts, normals, faces, A, pos, nrm, tan, uv, status);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_atlas_texels(const float* verts, int64_t n_verts, const float* normals, const int32_t* faces, int64_t n_faces,
                                int32_t size, int32_t cols, int32_t T, float* point, float* outward, int32_t* face,
                                int32_t* status, void* stream) {
    AtlasLayout A;
    if (!status || (n_faces > 0 && (!verts || !normals || !faces || !point || !outward || !face))) return TIR_ERR_ARG;
    const int rc = atlas_validate(n_verts, n_faces, size, cols, T, &A);
    if (rc) return rc;
    if (n_faces == 0) return TIR_OK;
    hipStream_t st = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return -(int)e;
    const int32_t n = A.n_cells * T * T;                               // at most size^2 <= 2^26
    const dim3 grid((unsigned)((n + ATLAS_THREADS - 1) / ATLAS_THREADS)), block(ATLAS_THREADS);
    if ((((uintptr_t)point | (uintptr_t)outward) & 15) == 0)
        hipLaunchKernelGGL(k_atlas_texels<true>, grid, block, 0, st, verts, normals, faces, A, n, point, outward, face, status);
    else
        hipLaunchKernelGGL(k_atlas_texels<false>, grid, block, 0, st, verts, normals, faces, A, n, point, outward, face, status);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_atlas_pack(const float* verts, int64_t n_verts, const float* normals, const int32_t* faces, int64_t n_faces,
                              int32_t size, int32_t cols, int32_t T, const float* albedo, const float* irradiance,
                              const float* roughness, const float* ao, const float* normal, const float* coverage, uint8_t* base,
                              uint8_t* orm, uint8_t* normal_image, int32_t* status, void* stream) {
    AtlasLayout A;
    if (!status || !base || !orm || !normal_image) return TIR_ERR_ARG;
    if (n_faces > 0 && (!verts || !normals || !faces || !albedo || !roughness || !normal || !coverage)) return TIR_ERR_ARG;
    const int rc = atlas_validate(n_verts, n_faces, size, cols, T, &A);
    if (rc) return rc;
    if (((uintptr_t)base | (uintptr_t)orm | (uintptr_t)normal_image) & 3) return TIR_ERR_ARG;
    if (n_faces == 0) return TIR_OK;
    hipStream_t st = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return -(int)e;
    const AtlasBake B{albedo, irradiance, roughness, ao, normal, coverage};
    hipLaunchKernelGGL(k_atlas_pack, dim3((unsigned)((size * size + ATLAS_THREADS - 1) / ATLAS_THREADS)), dim3(ATLAS_THREADS), 0, st,
                       verts, normals, faces, A, B, reinterpret_cast<uint32_t*>(base), reinterpret_cast<uint32_t*>(orm),
                       reinterpret_cast<uint32_t*>(normal_image), status);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int64_t tir_simplify_blocks(int64_t n) { return n < 0 ? TIR_ERR_ARG : simp_blocks(n, MC_BLOCK_POINTS); }

extern "C" int tir_simplify_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell,
                                  const float* origin, const int32_t* dims, int32_t* slots, int32_t* cell_of_vertex,
                                  int32_t* counts, int32_t* offsets, int32_t* status, void* stream) {
    SimpGrid G;
    int64_t n_slots = 0;
    const int rc = simp_validate(n_verts, n_faces, cell, origin, dims, &G, &n_slots);
    if (rc) return rc;
    if (!slots || !counts || !offsets || !status) return TIR_ERR_ARG;
    if ((n_verts > 0 && (!verts || !cell_of_vertex)) || (n_faces > 0 && !faces)) return TIR_ERR_ARG;
    const int64_t nbs = simp_blocks(n_slots, MC_BLOCK_POINTS), nbf = simp_blocks(n_faces, MC_BLOCK_POINTS);
    hipStream_t st = tir_stream(stream);
    hipError_t e = hipMemsetAsync(slots, 0, (size_t)n_slots * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, 4 * sizeof(int32_t), st);
    if (e != hipSuccess) return -(int)e;
    if (n_verts > 0) {
        hipLaunchKernelGGL(k_simplify_key, dim3((unsigned)simp_blocks(n_verts, MC_THREADS)), dim3(MC_THREADS), 0, st, verts, n_verts,
                           G, cell_of_vertex, slots, status);
        TIR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_simplify_slots<false>, dim3((unsigned)nbs), dim3(MC_THREADS), 0, st, slots, n_slots, counts,
                       (const int32_t*)nullptr);
    TIR_CHECK_LAUNCH();
    int src = tir_exclusive_scan(counts, offsets, (int32_t)nbs, stream);
    if (src) return src;
    hipLaunchKernelGGL(k_simplify_slots<true>, dim3((unsigned)nbs), dim3(MC_THREADS), 0, st, slots, n_slots, (int32_t*)nullptr,
                       (const int32_t*)offsets);
    TIR_CHECK_LAUNCH();
    if (n_verts > 0) {
        hipLaunchKernelGGL(k_simplify_map, dim3((unsigned)simp_blocks(n_verts, MC_THREADS)), dim3(MC_THREADS), 0, st,
                           cell_of_vertex, n_verts, (const int32_t*)slots);
        TIR_CHECK_LAUNCH();
    }
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_simplify_faces<false>, dim3((unsigned)nbf), dim3(MC_THREADS), 0, st, verts, faces, n_faces, n_verts, G,
                           (const int32_t*)cell_of_vertex, counts + nbs, (const int32_t*)nullptr, 0, (int32_t*)nullptr, status);
        TIR_CHECK_LAUNCH();
    }
    src = tir_exclusive_scan(counts + nbs, offsets + nbs + 1, (int32_t)nbf, stream);
    if (src) return src;
    hipLaunchKernelGGL(k_simplify_status, dim3(1), dim3(64), 0, st, (const int32_t*)(offsets + nbs),
                       (const int32_t*)(offsets + nbs + 1 + nbf), status);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_simplify_emit(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cell,
                                 const float* origin, const int32_t* dims, double reg, const int32_t* cell_of_vertex,
                                 const int32_t* offsets, int32_t n_out_verts, int32_t n_out_faces, int64_t* acc, int32_t* keys,
                                 float* out_verts, float* out_normals, int32_t* out_faces, void* stream) {
    SimpGrid G;
    int64_t n_slots = 0;
    const int rc = simp_validate(n_verts, n_faces, cell, origin, dims, &G, &n_slots);
    if (rc) return rc;
    if (!(reg >= 0.0) || n_out_verts < 0 || n_out_faces < 0 || n_out_verts > n_verts || n_out_faces > n_faces) return TIR_ERR_ARG;
    if (n_out_verts == 0) return n_out_faces == 0 ? TIR_OK : TIR_ERR_ARG;
    if (!verts || !cell_of_vertex || !acc || !keys || !out_verts || !out_normals) return TIR_ERR_ARG;
    if (n_faces > 0 && !faces) return TIR_ERR_ARG;
    if (n_out_faces > 0 && (!offsets || !out_faces)) return TIR_ERR_ARG;
    const int64_t nbs = simp_blocks(n_slots, MC_BLOCK_POINTS), nbf = simp_blocks(n_faces, MC_BLOCK_POINTS);
    hipStream_t st = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(acc, 0, (size_t)n_out_verts * SIMP_ACC * sizeof(int64_t), st);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(k_simplify_accum_verts, dim3((unsigned)simp_blocks(n_verts, MC_THREADS)), dim3(MC_THREADS), 0, st, verts,
                       n_verts, G, cell_of_vertex, n_out_verts, acc, keys);
    TIR_CHECK_LAUNCH();
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_simplify_accum_faces, dim3((unsigned)simp_blocks(n_faces, MC_THREADS)), dim3(MC_THREADS), 0, st, verts,
                           faces, n_faces, n_verts, G, cell_of_vertex, n_out_verts, acc);
        TIR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_simplify_solve, dim3((unsigned)simp_blocks(n_out_verts, MC_THREADS)), dim3(MC_THREADS), 0, st,
                       (const int64_t*)acc, (const int32_t*)keys, n_out_verts, G, reg, out_verts, out_normals);
    TIR_CHECK_LAUNCH();
    if (n_out_faces > 0) {
        hipLaunchKernelGGL(k_simplify_faces<true>, dim3((unsigned)nbf), dim3(MC_THREADS), 0, st, verts, faces, n_faces, n_verts, G,
                           cell_of_vertex, (int32_t*)nullptr, offsets + nbs + 1, n_out_faces, out_faces, (int32_t*)nullptr);
        TIR_CHECK_LAUNCH();
    }
    return TIR_OK;
}

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

extern "C" int64_t tir_ccl_blocks(int32_t gx, int32_t gy, int32_t gz) {
    CclGrid G;
    const int rc = ccl_validate(gx, gy, gz, &G);
    return rc ? rc : (G.n + MC_BLOCK_POINTS - 1) / MC_BLOCK_POINTS;
}

extern "C" int tir_ccl_label(const float* vol, int32_t gx, int32_t gy, int32_t gz, float level, int32_t connectivity,
                             int32_t* labels, int32_t* counts, int32_t* offsets, void* stream) {
    CclGrid G;
    if (connectivity != 6 && connectivity != 26) return TIR_ERR_ARG;
    const int rc = ccl_validate(gx, gy, gz, &G);
    if (rc) return rc;
    if (!vol || !labels || !counts || !offsets) return TIR_ERR_ARG;
    const int n_back = connectivity == 6 ? 3 : 13;
    const unsigned tiles = (unsigned)((int64_t)G.ntx * G.nty * G.ntz);
    const unsigned pblk = (unsigned)((G.n + CCL_THREADS - 1) / CCL_THREADS);
    const int64_t nb = (G.n + MC_BLOCK_POINTS - 1) / MC_BLOCK_POINTS;
    hipStream_t st = tir_stream(stream);
    hipLaunchKernelGGL(k_ccl_local, dim3(tiles), dim3(CCL_THREADS), 0, st, vol, level, G, n_back, labels);
    TIR_CHECK_LAUNCH();
    if (tiles > 1) {
        hipLaunchKernelGGL(k_ccl_merge, dim3(pblk), dim3(CCL_THREADS), 0, st, G, n_back, labels);
        TIR_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ccl_flatten, dim3(pblk), dim3(CCL_THREADS), 0, st, G.n, labels);
        TIR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_ccl_roots<false>, dim3((unsigned)nb), dim3(MC_THREADS), 0, st, (const int32_t*)labels, G.n, counts,
                       (const int32_t*)nullptr, 0, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    TIR_CHECK_LAUNCH();
    return tir_exclusive_scan(counts, offsets, (int32_t)nb, stream);
}

extern "C" int tir_ccl_table(const int32_t* labels, int32_t gx, int32_t gy, int32_t gz, const int32_t* offsets, int32_t n_comp,
                             int32_t* roots, int32_t* sizes, int32_t* boxes, void* stream) {
    CclGrid G;
    const int rc = ccl_validate(gx, gy, gz, &G);
    if (rc) return rc;
    if (!labels || !offsets || n_comp < 0) return TIR_ERR_ARG;
    if (n_comp == 0) return TIR_OK;
    if (!roots || !sizes || !boxes) return TIR_ERR_ARG;
    const int64_t nb = (G.n + MC_BLOCK_POINTS - 1) / MC_BLOCK_POINTS;
    hipStream_t st = tir_stream(stream);
    hipLaunchKernelGGL(k_ccl_roots<true>, dim3((unsigned)nb), dim3(MC_THREADS), 0, st, labels, G.n, (int32_t*)nullptr, offsets,
                       n_comp, roots, sizes, boxes);
    TIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ccl_stats, dim3((unsigned)nb), dim3(MC_THREADS), 0, st, labels, G, (const int32_t*)roots, n_comp, sizes,
                       boxes);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}

extern "C" int tir_ccl_filter(const float* vol, const int32_t* labels, int32_t gx, int32_t gy, int32_t gz, float level,
                              const int32_t* roots, const uint8_t* keep, int32_t n_comp, float fill, float* out, void* stream) {
    CclGrid G;
    if (!(fill <= level)) return TIR_ERR_ARG;             // a removed point must become an outside point (a NaN fill is one,
    const int rc = ccl_validate(gx, gy, gz, &G);          // but a NaN here is far more likely a mistake: refused as well)
    if (rc) return rc;
    if (!vol || !labels || !out || n_comp < 0) return TIR_ERR_ARG;
    if (n_comp > 0 && (!roots || !keep)) return TIR_ERR_ARG;
    hipLaunchKernelGGL(k_ccl_filter, dim3((unsigned)((G.n + CCL_THREADS - 1) / CCL_THREADS)), dim3(CCL_THREADS), 0,
                       tir_stream(stream), vol, labels, G.n, roots, keep, n_comp, fill, out);
    TIR_CHECK_LAUNCH();
    return TIR_OK;
}
