// Total-variation regulariser of the VM planes (tensoir_amd/regularisers.py; contract: include/tensoir_hip.h, tir_tv_fwd / tir_tv_bwd;
// DESIGN 4.12; restated in float64 by tests/regulariser_reference.py).
//
// k_tv_fwd  one launch for all planes of a call.  A workgroup (256 threads) owns a contiguous share of one plane's [H][W][C]
//           storage (tv_fwd_share: at least TIR_TV_SHARE floats, at most TIR_TV_FWD_GROUPS workgroups per plane -- a function of
//           the plane alone); per element it forms the forward differences along W (C floats ahead) and along H (W C floats
//           ahead) -- fp32 subtraction and fp32 square, each rounded on its own -- and adds them as doubles.  The neighbours were
//           or will be read as some thread's own element: they come from cache.  The tail is tir_metrics.hip's: two double
//           partials per workgroup, one ticket per launch, and in the workgroup that draws the last ticket wave w adds the
//           partials of planes w and w + 4 in workgroup order; thread 0 then forms the loss.  (Every workgroup draws the one
//           ticket: the cap on workgroups per plane keeps that word far below the rate at which it saturates.)
// k_tv_bwd  one launch for all planes whose gradient is wanted, TIR_TV_SHARE floats per workgroup: the two-sided stencil recomputed
//           from the plane, every element of the gradient written once.  The upstream gradient is read from a device scalar.
// Both take 16-byte loads and stores when C % 4 == 0 (and the tensors are 16-byte aligned) and a scalar path otherwise; the plane
// table travels by value in the kernel arguments, with the two divisors of the index arithmetic as multiply-and-shift pairs.
#include "tir_common.hpp"

#define TIR_TV_THREADS TIR_TAIL_THREADS
static_assert(TIR_TV_MAX_PLANES <= 8 && TIR_TV_FWD_GROUPS <= 128, "k_tv_fwd's tail: wave w adds planes w and w + 4, two partials per lane");
static_assert(TIR_TV_SHARE % (4 * TIR_TV_THREADS) == 0, "a share is whole 16-byte rounds of the workgroup");

namespace {

using tir::block_sum;
using tir::last_of_image;
using tir::sub_rn;
using tir::mul_rn;

// n / d for n < 2^31 and a divisor known on the host: (n * m) >> (32 + s) with m = ceil(2^(32 + s) / d), s = ceil(log2 d) - 1
// (m d = 2^(32 + s) + e with 0 <= e < d, so the quotient's error n e / (d 2^(32 + s)) stays below 1 / d: the floor is exact).
struct TvDiv { unsigned m, s; };                      // m == 0: d == 1
static inline TvDiv tv_div(unsigned d) {
    if (d <= 1) return {0u, 0u};
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    return {(unsigned)((((unsigned long long)1 << (31 + l)) + d - 1) / d), l - 1};
}
__device__ __forceinline__ unsigned div_by(unsigned n, TvDiv d) { return d.m ? __umulhi(n, d.m) >> d.s : n; }

struct TvPlane {
    const float* x;
    float* grad;            // backward only
    int C, H, W;
    int first;              // the plane's first workgroup
    unsigned share;         // floats per workgroup
    int vec;                // 16-byte path
    TvDiv by_cu, by_w;      // / (C / 4 or C), / W
    float ah, aw;           // backward: fp32(4 coef / nh), fp32(4 coef / nw)
    double coef, nh, nw;    // forward
};

struct TvTable {
    TvPlane p[TIR_TV_MAX_PLANES];
    int n;
};

// The plane of workgroup `wg`: the last one whose first workgroup is not behind it.  Selected field by field (no indexed copy of a
// kernel argument: that would become a scratch object).
__device__ __forceinline__ TvPlane plane_of(const TvTable& t, int wg) {
    TvPlane r = t.p[0];
#pragma unroll
    for (int i = 1; i < TIR_TV_MAX_PLANES; ++i)
        if (i < t.n && wg >= t.p[i].first) r = t.p[i];
    return r;
}

// unit u of a plane: VW consecutive floats of one texel; its texel's column and row
struct TvUnit { unsigned w, h; };
__device__ __forceinline__ TvUnit unit_of(unsigned u, const TvPlane& pl) {
    const unsigned pix = div_by(u, pl.by_cu), h = div_by(pix, pl.by_w);
    return {pix - h * (unsigned)pl.W, h};
}

template <int VW> struct TvVec;
template <> struct TvVec<1> {
    float v[1];
    __device__ __forceinline__ static TvVec ld(const float* p) { return {{*p}}; }
    __device__ __forceinline__ void st(float* p) const { *p = v[0]; }
};
template <> struct TvVec<4> {
    float v[4];
    __device__ __forceinline__ static TvVec ld(const float* p) { const float4 q = *reinterpret_cast<const float4*>(p); return {{q.x, q.y, q.z, q.w}}; }
    __device__ __forceinline__ void st(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// ---- forward ------------------------------------------------------------------------------------------------------------------
// units [u0, u1) of the plane, by thread in strides of the workgroup.  A unit on the last column / row reads itself instead of the
// missing neighbour (always loadable) and its term is dropped.
template <int VW>
__device__ __forceinline__ void tv_fwd_units(const TvPlane& pl, unsigned u0, unsigned u1, double& sh, double& sw) {
    const unsigned cu = (unsigned)pl.C / VW, W = (unsigned)pl.W, H = (unsigned)pl.H, row = W * cu;
#pragma unroll 4
    for (unsigned u = u0 + threadIdx.x; u < u1; u += TIR_TV_THREADS) {
        const TvUnit t = unit_of(u, pl);
        const bool in_w = t.w + 1 < W, in_h = t.h + 1 < H;
        const float* p = pl.x + (size_t)u * VW;
        const TvVec<VW> x = TvVec<VW>::ld(p), xw = TvVec<VW>::ld(p + (in_w ? (size_t)cu * VW : 0)),
                        xh = TvVec<VW>::ld(p + (in_h ? (size_t)row * VW : 0));
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float dw = sub_rn(xw.v[k], x.v[k]), dh = sub_rn(xh.v[k], x.v[k]);
            sw += (double)(in_w ? mul_rn(dw, dw) : 0.f);
            sh += (double)(in_h ? mul_rn(dh, dh) : 0.f);
        }
    }
}

__global__ void __launch_bounds__(TIR_TV_THREADS)
k_tv_fwd(TvTable tab, double* __restrict__ partial, int32_t* __restrict__ ticket, double* __restrict__ sums, float* __restrict__ loss) {
    __shared__ double s4[4];
    __shared__ double s_sum[TIR_TV_MAX_PLANES][2];
    __shared__ int s_last;
    const TvPlane pl = plane_of(tab, (int)blockIdx.x);
    const unsigned total = (unsigned)pl.C * (unsigned)pl.H * (unsigned)pl.W;               // < 2^31 (checked on the host)
    const unsigned e0 = (unsigned)((int)blockIdx.x - pl.first) * pl.share;                 // < total: the plane has ceil(total / share) workgroups
    const unsigned e1 = min(e0 + pl.share, total);
    double sh = 0.0, sw = 0.0;
    if (pl.vec) tv_fwd_units<4>(pl, e0 / 4, e1 / 4, sh, sw);        // C % 4 == 0: total and the share are multiples of 4
    else tv_fwd_units<1>(pl, e0, e1, sh, sw);
    const double bh = block_sum(sh, s4), bw = block_sum(sw, s4);
    if (threadIdx.x == 0) {
        __hip_atomic_store(partial + 2 * (size_t)blockIdx.x, bh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(partial + 2 * (size_t)blockIdx.x + 1, bw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!last_of_image(ticket, (int)gridDim.x, &s_last)) return;
    // The last workgroup of the launch.  Wave w adds the partials of planes w and w + 4: lane l those of the plane's workgroups l
    // and l + 64 (a plane has at most TIR_TV_FWD_GROUPS = 128), then the xor tree -- an order that depends on the plane's own
    // workgroup count only.  All loads of a wave leave together.
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double v[2][2][2];                                              // [plane of the wave][partial of the lane][h, w]
    int first[2] = {0, 0}, count[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < TIR_TV_MAX_PLANES; ++i) {
        const int f = tab.p[i].first;
        const int next = (i + 1 < TIR_TV_MAX_PLANES && i + 1 < tab.n) ? tab.p[(i + 1) % TIR_TV_MAX_PLANES].first : (int)gridDim.x;
        if (i < tab.n && i == wave) { first[0] = f; count[0] = next - f; }
        if (i < tab.n && i == wave + 4) { first[1] = f; count[1] = next - f; }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int i = lane + 64 * r;
                v[j][r][k] = i < count[j] ? __hip_atomic_load(partial + 2 * (size_t)(first[j] + i) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            double a = v[j][0][k] + v[j][1][k];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) a += __shfl_xor(a, d, 64);
            if (lane == 0 && wave + 4 * j < tab.n) {
                s_sum[wave + 4 * j][k] = a;
                sums[2 * (wave + 4 * j) + k] = a;
            }
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        // the loss in double, plane by plane in the order of the contract, rounded once
        double acc = 0.0;
#pragma unroll
        for (int p = 0; p < TIR_TV_MAX_PLANES; ++p) {
#pragma clang fp contract(off)
            if (p < tab.n) acc += tab.p[p].coef * 2.0 * (s_sum[p][0] / tab.p[p].nh + s_sum[p][1] / tab.p[p].nw);
        }
        *loss = (float)acc;
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
template <int VW>
__device__ __forceinline__ void tv_bwd_units(const TvPlane& pl, unsigned u0, unsigned u1, float sh, float sw) {
    const unsigned cu = (unsigned)pl.C / VW, W = (unsigned)pl.W, H = (unsigned)pl.H, row = W * cu;
#pragma unroll 2
    for (unsigned u = u0 + threadIdx.x; u < u1; u += TIR_TV_THREADS) {
        const TvUnit t = unit_of(u, pl);
        const bool w_hi = t.w + 1 < W, w_lo = t.w > 0, h_hi = t.h + 1 < H, h_lo = t.h > 0;
        const float* p = pl.x + (size_t)u * VW;
        const TvVec<VW> x = TvVec<VW>::ld(p);
        const TvVec<VW> xwp = TvVec<VW>::ld(p + (w_hi ? (size_t)cu * VW : 0)), xwm = TvVec<VW>::ld(p - (w_lo ? (size_t)cu * VW : 0));
        const TvVec<VW> xhp = TvVec<VW>::ld(p + (h_hi ? (size_t)row * VW : 0)), xhm = TvVec<VW>::ld(p - (h_lo ? (size_t)row * VW : 0));
        TvVec<VW> g;
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float dwp = w_hi ? sub_rn(xwp.v[k], x.v[k]) : 0.f, dwm = w_lo ? sub_rn(x.v[k], xwm.v[k]) : 0.f;
            const float dhp = h_hi ? sub_rn(xhp.v[k], x.v[k]) : 0.f, dhm = h_lo ? sub_rn(x.v[k], xhm.v[k]) : 0.f;
            g.v[k] = sh * (dhm - dhp) + sw * (dwm - dwp);
        }
        g.st(pl.grad + (size_t)u * VW);
    }
}

__global__ void __launch_bounds__(TIR_TV_THREADS)
k_tv_bwd(TvTable tab, const float* __restrict__ g_up) {
    const TvPlane pl = plane_of(tab, (int)blockIdx.x);
    const unsigned total = (unsigned)pl.C * (unsigned)pl.H * (unsigned)pl.W;
    const unsigned e0 = (unsigned)((int)blockIdx.x - pl.first) * pl.share;
    const unsigned e1 = min(e0 + pl.share, total);
    const float g = *g_up;
    const float sh = mul_rn(g, pl.ah), sw = mul_rn(g, pl.aw);
    if (pl.vec) tv_bwd_units<4>(pl, e0 / 4, e1 / 4, sh, sw);
    else tv_bwd_units<1>(pl, e0, e1, sh, sw);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// floats per workgroup of a plane of `elements` floats.  Forward: TIR_TV_SHARE, or what leaves the plane TIR_TV_FWD_GROUPS
// workgroups, rounded up to whole 16-byte rounds of the workgroup.  Backward: TIR_TV_SHARE.
static inline int64_t tv_fwd_share(int64_t elements) {
    constexpr int64_t round = 4 * TIR_TV_THREADS;
    const int64_t even = (elements + TIR_TV_FWD_GROUPS - 1) / TIR_TV_FWD_GROUPS;
    const int64_t share = (even + round - 1) / round * round;
    return share < TIR_TV_SHARE ? TIR_TV_SHARE : share;
}
static inline int64_t tv_groups(int64_t elements, int64_t share) { return (elements + share - 1) / share; }

// the shapes of a call -> TIR_OK and, where asked for, the forward's workgroups over all planes; or the refusal
static inline int tv_shapes(int32_t n_planes, const int32_t* C, const int32_t* H, const int32_t* W, int64_t* groups) {
    if (n_planes < 0 || n_planes > TIR_TV_MAX_PLANES) return TIR_ERR_ARG;
    if (groups) *groups = 0;
    if (n_planes == 0) return TIR_OK;
    if (tir_any_null({C, H, W})) return TIR_ERR_ARG;
    for (int p = 0; p < n_planes; ++p)
        if (C[p] < 1 || H[p] < 2 || W[p] < 2) return TIR_ERR_ARG;
    for (int p = 0; p < n_planes; ++p) {
        // elements are indexed with 32 bits; (2^31)^2 fits an int64, the third factor is applied once that product is known small
        const int64_t hw = (int64_t)H[p] * W[p];
        if (hw >= ((int64_t)1 << 31) || hw * C[p] >= ((int64_t)1 << 31)) return TIR_ERR_UNSUPPORTED;
        if (groups) *groups += tv_groups(hw * C[p], tv_fwd_share(hw * C[p]));
    }
    return TIR_OK;
}

// What both entries refuse, in the one order the contract states: a bad shape (TIR_ERR_ARG), then a missing pointer (`need`, every
// planes[p]) -> TIR_ERR_ARG, then a plane too large -> TIR_ERR_UNSUPPORTED.  n_planes == 0 is TIR_OK with *empty set: nothing to do.
static inline int tv_check(int32_t n_planes, const int32_t* C, const int32_t* H, const int32_t* W, const float* const* planes,
                           std::initializer_list<const void*> need, int64_t* fwd_groups, bool* empty) {
    const int shape = tv_shapes(n_planes, C, H, W, fwd_groups);
    *empty = shape == TIR_OK && n_planes == 0;
    if (shape == TIR_ERR_ARG || *empty) return shape;
    if (!planes || tir_any_null(need)) return TIR_ERR_ARG;
    for (int p = 0; p < n_planes; ++p)
        if (!planes[p]) return TIR_ERR_ARG;
    return shape;
}

// what both kernels read of plane p; -> its workgroups
static inline int tv_plane(TvPlane& t, const float* x, float* grad, int C, int H, int W, int first, int64_t share) {
    const int64_t elements = (int64_t)C * H * W;
    t.x = x; t.grad = grad; t.C = C; t.H = H; t.W = W;
    t.first = first;
    t.share = (unsigned)share;
    t.vec = C % 4 == 0 && tir_aligned16({x, grad});
    t.by_cu = tv_div((unsigned)(t.vec ? C / 4 : C));
    t.by_w = tv_div((unsigned)W);
    t.nh = (double)C * (double)(H - 1) * (double)W;
    t.nw = (double)C * (double)H * (double)(W - 1);
    return (int)tv_groups(elements, share);
}

}  // namespace

extern "C" int64_t tir_tv_workspace(int32_t n_planes, const int32_t* C, const int32_t* H, const int32_t* W) {
    int64_t groups = 0;
    if (int rc = tv_shapes(n_planes, C, H, W, &groups)) return rc;
    return 2 * groups + 1;                                 // two partials per workgroup, and the ticket
}

extern "C" int tir_tv_fwd(const float* const* planes, const int32_t* C, const int32_t* H, const int32_t* W, const double* coef,
                          int32_t n_planes, double* workspace, double* sums, float* loss, void* stream) {
    int64_t groups = 0;
    bool empty = false;
    if (int rc = tv_check(n_planes, C, H, W, planes, {coef, workspace, sums, loss}, &groups, &empty)) return rc;
    if (empty) return TIR_OK;
    TvTable tab{};
    tab.n = n_planes;
    int first = 0;
    for (int p = 0; p < n_planes; ++p) {
        tab.p[p].coef = coef[p];
        first += tv_plane(tab.p[p], planes[p], nullptr, C[p], H[p], W[p], first, tv_fwd_share((int64_t)C[p] * H[p] * W[p]));
    }
    int32_t* ticket = reinterpret_cast<int32_t*>(workspace + 2 * groups);
    hipStream_t s = tir_stream(stream);
    const hipError_t e = hipMemsetAsync(ticket, 0, sizeof(int32_t), s);         // armed here: a caller's buffer may hold anything
    if (e != hipSuccess) return -(int)e;
    return tir_launch(k_tv_fwd, 0, dim3((unsigned)groups), dim3(TIR_TV_THREADS), 0, s, tab, workspace, ticket, sums, loss);
}

extern "C" int tir_tv_bwd(const float* const* planes, const int32_t* C, const int32_t* H, const int32_t* W, const double* coef,
                          int32_t n_planes, const float* g, float* const* grads, void* stream) {
    bool empty = false;
    if (int rc = tv_check(n_planes, C, H, W, planes, {coef, g, grads}, nullptr, &empty)) return rc;
    if (empty) return TIR_OK;
    TvTable tab{};
    int first = 0;
    for (int p = 0; p < n_planes; ++p) {
        if (!grads[p]) continue;                           // a plane whose gradient nobody wants gets no workgroup
        TvPlane& t = tab.p[tab.n++];
        first += tv_plane(t, planes[p], grads[p], C[p], H[p], W[p], first, TIR_TV_SHARE);     // at most 8 * 2^18 workgroups
        t.ah = (float)(4.0 * coef[p] / t.nh);
        t.aw = (float)(4.0 * coef[p] / t.nw);
    }
    if (tab.n == 0) return TIR_OK;
    return tir_launch(k_tv_bwd, 0, dim3((unsigned)first), dim3(TIR_TV_THREADS), 0, tir_stream(stream), tab, g);
}
