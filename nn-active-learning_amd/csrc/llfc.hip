// Closed forms of the last fully connected layer (NN.LLFC_grads / LLFC_hess, NN.py:874-955) and the stochastic influence
// recursion built on them (PW_NNAL.stoch_approx_IF, PW_NNAL.py:851-881).
//
// Notation: u [d] = a sample's feature vector, u~ = (u, 1), p [c] = its posterior, P = (d+1) c.  A parameter vector is ordered
// like the reference's: W class-major (entry j*d + i = class j, feature i), then the c biases.
//     gradient   g[j*d+i] = ([j == y] - p_j) u_i,  g[c*d+j] = [j == y] - p_j
//     Hessian    H = A (x) (u~ u~^T),  A_jk = p_j (p_k - [j == k])
//     recursion  V_0 = G;  V <- G + V + H_r V / scale  for the drawn training sample r.  H_r has rank c, so per column
//                s_k = Vw[k,:] . u_r + vb[k],  q_j = p_j (s_j - sum_k p_k s_k),  Vw[j,:] += Gw[j,:] - (q_j / scale) u_r,
//                vb[j] += gb[j] - q_j / scale.   Columns never interact and G = e (x) u~_pool is regenerated, never read.
// The reference forms H with np.kron ((d+1)c squared doubles: 537 MB for NET-B) and multiplies it into V every iteration.
//
// llfc_if_resident_kernel keeps the columns of V in LDS (fp32) over all T iterations: a workgroup of 512 threads owns up to 4
// columns, every thread the same elements of them in the dot products and in the update, so V needs no barrier of its own; one
// barrier per iteration orders the per-wave partial sums (double-buffered by the iteration's parity, like the biases).  The dot
// products and the update arithmetic are fp64; an element is rounded to fp32 once per iteration.  V leaves the chip once.
// Columns that do not fit in LDS run llfc_if_dot_kernel + llfc_if_update_kernel per iteration over V in HBM, with the same
// element-to-thread map and the same summation tree: both paths give the same bits, and neither uses atomics.
// Stores are 4 or 8 bytes wide (alq_internal.h, the 16-byte-store hazard does not arise).
#include <algorithm>

#include "alq_internal.h"

#pragma clang fp contract(off)

namespace alq {

namespace {

constexpr int LF_THREADS = 512;                       // 8 waves: 2 per SIMD
constexpr int LF_WAVES = LF_THREADS / 64;
constexpr int LF_NC = 4;                              // columns of V a resident workgroup holds at most
constexpr int LF_MAXC_RES = 4;                        // class counts the resident kernel is instantiated for: 2, 3, 4
constexpr int LF_MAXC = 16;                           // class counts the streaming kernels take
constexpr size_t LF_LDS_DYN_MAX = 160 * 1024 - 4096;  // dynamic LDS of the resident kernel (its static part is below 4 KiB)
constexpr size_t LF_HESS_MAX_BYTES = (size_t)256 << 20;

template <int W>
struct LfVec;
template <>
struct LfVec<1> {
    float v[1];
    __device__ static LfVec ld(const float *p) { return LfVec{{p[0]}}; }
    __device__ void st(float *p) const { p[0] = v[0]; }
};
template <>
struct LfVec<2> {
    float v[2];
    __device__ static LfVec ld(const float *p) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        return LfVec{{t.x, t.y}};
    }
    __device__ void st(float *p) const { *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]); }
};

// sum over the 64 lanes, the same tree in every kernel (xor 32, 16, 8, 4, 2, 1); every lane gets the sum
__device__ inline double lf_wave_sum(double a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m, 64);
    return a;
}

// the wave partials of one dot product in wave order, then the bias: s_k
__device__ inline double lf_fold(const double *red, int stride, float vb) {
    double s = red[0];
#pragma unroll
    for (int w = 1; w < LF_WAVES; ++w) s += red[w * stride];
    return s + (double)vb;
}

// q_j / scale from the c values s_k and the drawn sample's posterior
template <typename PF>
__device__ inline double lf_qs(const double *s, PF p, int c, int j, double scale) {
    double ps = 0.0;
    for (int k = 0; k < c; ++k) ps += (double)p(k) * s[k];
    return ((double)p(j) * (s[j] - ps)) / scale;
}

__device__ inline float lf_init(double e, float up) { return (float)(e * (double)up); }
__device__ inline float lf_step(float v, double e, float up, double qs, float u) {
    return (float)fma(-qs, (double)u, fma(e, (double)up, (double)v));
}
__device__ inline int lf_clamp(int r, int n) { return r < 0 ? 0 : (r >= n ? n - 1 : r); }

// ---------------------------------------------------------------------------------------------- gradients
__global__ __launch_bounds__(256) void llfc_grads_kernel(const float *__restrict__ feat, const float *__restrict__ post,
                                                         const int *__restrict__ labels, int n, int d, int c,
                                                         float *__restrict__ out) {
    const int s = blockIdx.y;
    const long long P = (long long)(d + 1) * c;
    const int y = labels[s];
    const float *u = feat + (long long)s * d;
    float *o = out + (long long)s * P;
    for (int j = 0; j < c; ++j) {
        const float e = (j == y ? 1.f : 0.f) - post[(long long)j * n + s];
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d; i += gridDim.x * blockDim.x) o[(long long)j * d + i] = e * u[i];
        if (blockIdx.x == 0 && threadIdx.x == 0) o[(long long)c * d + j] = e;
    }
}

// ---------------------------------------------------------------------------------------------- explicit Hessian of one sample
__global__ __launch_bounds__(256) void llfc_hess_kernel(const float *__restrict__ u, const float *__restrict__ p, int d, int c,
                                                        double *__restrict__ H) {
    const int P = (d + 1) * c;
    const int a = blockIdx.y;
    const int j = a < c * d ? a / d : a - c * d;
    const double ua = a < c * d ? (double)u[a - j * d] : 1.0;
    const double pj = (double)p[j];
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < P; b += gridDim.x * blockDim.x) {
        const int k = b < c * d ? b / d : b - c * d;
        const double ub = b < c * d ? (double)u[b - k * d] : 1.0;
        const double A = j == k ? pj * ((double)p[k] - 1.0) : pj * (double)p[k];
        H[(long long)a * P + b] = A * (ua * ub);      // ua * ub is exact (two fp32 factors): H is symmetric bit for bit
    }
}

// ---------------------------------------------------------------------------------------------- resident recursion
template <int CT, int W>
__global__ __launch_bounds__(LF_THREADS) void llfc_if_resident_kernel(
    const float *__restrict__ pool_feat, const float *__restrict__ pool_post, const int *__restrict__ pool_labels, int n_pool,
    const float *__restrict__ tr_feat, const float *__restrict__ tr_post, int n_tr, const int *__restrict__ draws, int T,
    double scale, int d, int nc_max, float *__restrict__ V) {
    extern __shared__ __attribute__((aligned(16))) float lf_v[];      // [nc][CT][d]
    __shared__ double red[2][LF_WAVES][LF_NC][LF_MAXC_RES];
    __shared__ float vb[2][LF_NC][LF_MAXC_RES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col0 = blockIdx.x * nc_max;
    const int nc = min(nc_max, n_pool - col0);
    const int ngrp = d / W;
    const long long P = (long long)(d + 1) * CT;

    double e[LF_NC][CT];
#pragma unroll
    for (int col = 0; col < LF_NC; ++col)
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            e[col][j] = 0.0;
            if (col < nc)
                e[col][j] = (j == pool_labels[col0 + col] ? 1.0 : 0.0) - (double)pool_post[(long long)j * n_pool + col0 + col];
        }
    // V_0 = G
    for (int g = tid; g < ngrp; g += LF_THREADS)
#pragma unroll
        for (int col = 0; col < LF_NC; ++col)
            if (col < nc) {
                const LfVec<W> up = LfVec<W>::ld(pool_feat + (long long)(col0 + col) * d + (long long)g * W);
#pragma unroll
                for (int j = 0; j < CT; ++j) {
                    LfVec<W> v;
#pragma unroll
                    for (int x = 0; x < W; ++x) v.v[x] = lf_init(e[col][j], up.v[x]);
                    v.st(lf_v + ((long long)col * CT + j) * d + (long long)g * W);
                }
            }
    if (tid < LF_NC * CT) {
        const int col = tid / CT, j = tid - col * CT;
        if (col < nc) vb[0][col][j] = (float)((j == pool_labels[col0 + col] ? 1.0 : 0.0) - (double)pool_post[(long long)j * n_pool + col0 + col]);
    }

    for (int t = 0; t < T; ++t) {
        const int par = t & 1;
        const int r = lf_clamp(draws[t], n_tr);
        const float *u = tr_feat + (long long)r * d;
        // the c dot products of every column: each thread over its own elements, ascending
        double acc[LF_NC][CT];
#pragma unroll
        for (int col = 0; col < LF_NC; ++col)
#pragma unroll
            for (int k = 0; k < CT; ++k) acc[col][k] = 0.0;
        for (int g = tid; g < ngrp; g += LF_THREADS) {
            const LfVec<W> uu = LfVec<W>::ld(u + (long long)g * W);
#pragma unroll
            for (int col = 0; col < LF_NC; ++col)
                if (col < nc)
#pragma unroll
                    for (int k = 0; k < CT; ++k) {
                        const LfVec<W> v = LfVec<W>::ld(lf_v + ((long long)col * CT + k) * d + (long long)g * W);
#pragma unroll
                        for (int x = 0; x < W; ++x) acc[col][k] = fma((double)v.v[x], (double)uu.v[x], acc[col][k]);
                    }
        }
#pragma unroll
        for (int col = 0; col < LF_NC; ++col)
            if (col < nc)
#pragma unroll
                for (int k = 0; k < CT; ++k) {
                    const double w = lf_wave_sum(acc[col][k]);
                    if (lane == 0) red[par][wave][col][k] = w;
                }
        __syncthreads();
        double qs[LF_NC][CT];
#pragma unroll
        for (int col = 0; col < LF_NC; ++col) {
#pragma unroll
            for (int j = 0; j < CT; ++j) qs[col][j] = 0.0;
            if (col < nc) {
                double s[CT];
#pragma unroll
                for (int k = 0; k < CT; ++k) s[k] = lf_fold(&red[par][0][col][k], LF_NC * LF_MAXC_RES, vb[par][col][k]);
#pragma unroll
                for (int j = 0; j < CT; ++j)
                    qs[col][j] = lf_qs(s, [&](int k) { return tr_post[(long long)k * n_tr + r]; }, CT, j, scale);
            }
        }
        if (tid < LF_NC * CT) {
            const int col = tid / CT, j = tid - col * CT;
            if (col < nc) {
                double ee = 0.0, qq = 0.0;      // (a register array indexed by col / j would go to scratch)
#pragma unroll
                for (int a = 0; a < LF_NC; ++a)
#pragma unroll
                    for (int b = 0; b < CT; ++b)
                        if (a == col && b == j) {
                            ee = e[a][b];
                            qq = qs[a][b];
                        }
                vb[par ^ 1][col][j] = (float)(((double)vb[par][col][j] + ee) - qq);
            }
        }
        for (int g = tid; g < ngrp; g += LF_THREADS) {
            const LfVec<W> uu = LfVec<W>::ld(u + (long long)g * W);
#pragma unroll
            for (int col = 0; col < LF_NC; ++col)
                if (col < nc) {
                    const LfVec<W> up = LfVec<W>::ld(pool_feat + (long long)(col0 + col) * d + (long long)g * W);
#pragma unroll
                    for (int j = 0; j < CT; ++j) {
                        float *at = lf_v + ((long long)col * CT + j) * d + (long long)g * W;
                        LfVec<W> v = LfVec<W>::ld(at);
#pragma unroll
                        for (int x = 0; x < W; ++x) v.v[x] = lf_step(v.v[x], e[col][j], up.v[x], qs[col][j], uu.v[x]);
                        v.st(at);
                    }
                }
        }
    }
    __syncthreads();      // the biases of the last iteration (or of V_0)
    for (int col = 0; col < nc; ++col) {
        float *o = V + (long long)(col0 + col) * P;
        for (int j = 0; j < CT; ++j)
            for (int g = tid; g < ngrp; g += LF_THREADS)
                LfVec<W>::ld(lf_v + ((long long)col * CT + j) * d + (long long)g * W).st(o + (long long)j * d + (long long)g * W);
        if (tid < CT) o[(long long)CT * d + tid] = vb[T & 1][col][tid];
    }
}

// ---------------------------------------------------------------------------------------------- streaming recursion
// s[col][k] of one column per workgroup: the element-to-thread map and the tree of the resident kernel
template <int W>
__global__ __launch_bounds__(LF_THREADS) void llfc_if_dot_kernel(const float *__restrict__ V, const float *__restrict__ tr_feat,
                                                                const int *__restrict__ draws, int t, int n_tr, int d, int c,
                                                                double *__restrict__ s) {
    __shared__ double red[LF_WAVES][LF_MAXC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ngrp = d / W;
    const long long P = (long long)(d + 1) * c;
    const float *v0 = V + (long long)blockIdx.x * P;
    const float *u = tr_feat + (long long)lf_clamp(draws[t], n_tr) * d;
    for (int k = 0; k < c; ++k) {
        double acc = 0.0;
        for (int g = tid; g < ngrp; g += LF_THREADS) {
            const LfVec<W> uu = LfVec<W>::ld(u + (long long)g * W);
            const LfVec<W> v = LfVec<W>::ld(v0 + (long long)k * d + (long long)g * W);
#pragma unroll
            for (int x = 0; x < W; ++x) acc = fma((double)v.v[x], (double)uu.v[x], acc);
        }
        const double w = lf_wave_sum(acc);
        if (lane == 0) red[wave][k] = w;
    }
    __syncthreads();
    if (tid < c) s[(long long)blockIdx.x * c + tid] = lf_fold(&red[0][tid], LF_MAXC, v0[(long long)c * d + tid]);
}

// INIT: V = G.  Else one iteration's update from s.  grid (chunks of a row, columns)
template <int W, bool INIT>
__global__ __launch_bounds__(256) void llfc_if_update_kernel(const float *__restrict__ pool_feat, const float *__restrict__ pool_post,
                                                             const int *__restrict__ pool_labels, int n_pool,
                                                             const float *__restrict__ tr_feat, const float *__restrict__ tr_post,
                                                             int n_tr, const int *__restrict__ draws, int t, double scale, int d, int c,
                                                             const double *__restrict__ s, float *__restrict__ V) {
    const int col = blockIdx.y;
    const int ngrp = d / W;
    const long long P = (long long)(d + 1) * c;
    float *v0 = V + (long long)col * P;
    const float *up0 = pool_feat + (long long)col * d;
    const int y = pool_labels[col];
    int r = 0;
    const float *u = tr_feat;
    if (!INIT) {
        r = lf_clamp(draws[t], n_tr);
        u = tr_feat + (long long)r * d;
    }
    for (int j = 0; j < c; ++j) {
        const double e = (j == y ? 1.0 : 0.0) - (double)pool_post[(long long)j * n_pool + col];
        double qs = 0.0;
        if (!INIT) qs = lf_qs(s + (long long)col * c, [&](int k) { return tr_post[(long long)k * n_tr + r]; }, c, j, scale);
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < ngrp; g += gridDim.x * blockDim.x) {
            const LfVec<W> up = LfVec<W>::ld(up0 + (long long)g * W);
            float *at = v0 + (long long)j * d + (long long)g * W;
            LfVec<W> v;
            if (INIT) {
#pragma unroll
                for (int x = 0; x < W; ++x) v.v[x] = lf_init(e, up.v[x]);
            } else {
                const LfVec<W> uu = LfVec<W>::ld(u + (long long)g * W);
                v = LfVec<W>::ld(at);
#pragma unroll
                for (int x = 0; x < W; ++x) v.v[x] = lf_step(v.v[x], e, up.v[x], qs, uu.v[x]);
            }
            v.st(at);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            float *b = v0 + (long long)c * d + j;
            *b = INIT ? (float)e : (float)(((double)*b + e) - qs);
        }
    }
}

bool lf_resident_ok(int d, int c) { return c >= 2 && c <= LF_MAXC_RES && (size_t)c * d * sizeof(float) <= LF_LDS_DYN_MAX; }

template <int CT, int W>
int lf_launch_resident(alq_ctx *ctx, const float *pf, const float *pp, const int *pl, int n_pool, const float *tf, const float *tp,
                       int n_tr, const int *draws, int T, double scale, int d, float *V) {
    const size_t colb = (size_t)CT * d * sizeof(float);
    // as many columns per workgroup as LDS holds, but no more than leaves every CU a workgroup
    const int nc = (int)std::max<size_t>(1, std::min<size_t>({(size_t)LF_NC, LF_LDS_DYN_MAX / colb,
                                                              (size_t)((n_pool + ctx->num_cus - 1) / ctx->num_cus)}));
    auto kfn = llfc_if_resident_kernel<CT, W>;
    const size_t lds = colb * nc;
    ALQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LF_LDS_DYN_MAX));
    hipLaunchKernelGGL(kfn, dim3((unsigned)((n_pool + nc - 1) / nc)), dim3(LF_THREADS), lds, ctx->stream, pf, pp, pl, n_pool, tf, tp,
                       n_tr, draws, T, scale, d, nc, V);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

template <int W>
int lf_launch_streaming(alq_ctx *ctx, const float *pf, const float *pp, const int *pl, int n_pool, const float *tf, const float *tp,
                        int n_tr, const int *draws, int T, double scale, int d, int c, float *V, double *s) {
    const int ngrp = d / W;
    const dim3 ugrid((unsigned)std::max(1, std::min((ngrp + 255) / 256, 64)), (unsigned)n_pool);
    hipLaunchKernelGGL((llfc_if_update_kernel<W, true>), ugrid, dim3(256), 0, ctx->stream, pf, pp, pl, n_pool, tf, tp, n_tr, draws, 0,
                       scale, d, c, (const double *)nullptr, V);
    for (int t = 0; t < T; ++t) {
        hipLaunchKernelGGL((llfc_if_dot_kernel<W>), dim3((unsigned)n_pool), dim3(LF_THREADS), 0, ctx->stream, (const float *)V, tf, draws, t,
                           n_tr, d, c, s);
        hipLaunchKernelGGL((llfc_if_update_kernel<W, false>), ugrid, dim3(256), 0, ctx->stream, pf, pp, pl, n_pool, tf, tp, n_tr, draws, t,
                           scale, d, c, (const double *)s, V);
    }
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // namespace

}  // namespace alq

using namespace alq;

extern "C" {

int alq_llfc_grads(alq_ctx *ctx, const float *d_feat, const float *d_post, const int32_t *d_labels, int n, int d, int c, float *d_out) {
    ALQ_REQUIRE(ctx && d_feat && d_post && d_labels && d_out, ALQ_EINVAL, "alq_llfc_grads: null argument");
    ALQ_REQUIRE(n >= 1 && n <= 65535 && d >= 1 && c >= 2, ALQ_EINVAL, "alq_llfc_grads: n=%d (1..65535) d=%d c=%d", n, d, c);
    const dim3 grid((unsigned)std::max(1, std::min((d + 255) / 256, 64)), (unsigned)n);
    hipLaunchKernelGGL(llfc_grads_kernel, grid, dim3(256), 0, ctx->stream, d_feat, d_post, d_labels, n, d, c, d_out);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

size_t alq_llfc_hess_max_bytes(void) { return LF_HESS_MAX_BYTES; }

int alq_llfc_hess(alq_ctx *ctx, const float *d_feat_one, const float *d_post_one, int d, int c, double *d_H) {
    ALQ_REQUIRE(ctx && d_feat_one && d_post_one && d_H, ALQ_EINVAL, "alq_llfc_hess: null argument");
    ALQ_REQUIRE(d >= 1 && c >= 2, ALQ_EINVAL, "alq_llfc_hess: d=%d c=%d", d, c);
    const unsigned long long P = (unsigned long long)(d + 1) * c;
    ALQ_REQUIRE(P <= 65535 && P * P * sizeof(double) <= LF_HESS_MAX_BYTES, ALQ_EUNSUPPORTED,
                "alq_llfc_hess: the explicit matrix of (d+1)c = %llu parameters exceeds %zu bytes; use alq_llfc_stoch_if (implicit)", P,
                LF_HESS_MAX_BYTES);
    const dim3 grid((unsigned)std::min<unsigned long long>((P + 255) / 256, 64), (unsigned)P);
    hipLaunchKernelGGL(llfc_hess_kernel, grid, dim3(256), 0, ctx->stream, d_feat_one, d_post_one, d, c, d_H);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int alq_llfc_if_path(int d, int c) { return lf_resident_ok(d, c) ? 1 : 2; }

size_t alq_llfc_if_work_bytes(int n_pool, int c) { return (size_t)std::max(n_pool, 0) * (size_t)std::max(c, 0) * sizeof(double); }

int alq_llfc_stoch_if(alq_ctx *ctx, const float *d_pool_feat, const float *d_pool_post, const int32_t *d_pool_labels, int n_pool,
                      const float *d_tr_feat, const float *d_tr_post, int n_tr, const int32_t *d_draws, int T, double scale, int d, int c,
                      int path, float *d_V, void *d_work) {
    ALQ_REQUIRE(ctx && d_pool_feat && d_pool_post && d_pool_labels && d_V, ALQ_EINVAL, "alq_llfc_stoch_if: null argument");
    ALQ_REQUIRE(n_pool >= 1 && n_pool <= 65535 && d >= 1 && c >= 2 && c <= LF_MAXC && T >= 0 && path >= 0 && path <= 2, ALQ_EINVAL,
                "alq_llfc_stoch_if: n_pool=%d (1..65535) d=%d c=%d (2..%d) T=%d path=%d", n_pool, d, c, LF_MAXC, T, path);
    ALQ_REQUIRE(T == 0 || (d_tr_feat && d_tr_post && d_draws && n_tr >= 1), ALQ_EINVAL, "alq_llfc_stoch_if: T=%d needs training samples and draws", T);
    ALQ_REQUIRE(scale != 0.0, ALQ_EINVAL, "alq_llfc_stoch_if: scale = 0");
    if (path == 0) path = alq_llfc_if_path(d, c);
    ALQ_REQUIRE(path == 2 || lf_resident_ok(d, c), ALQ_EUNSUPPORTED,
                "alq_llfc_stoch_if: a column of c=%d x d=%d does not fit the resident kernel (c <= %d, c d 4 <= %zu bytes)", c, d, LF_MAXC_RES,
                LF_LDS_DYN_MAX);
    // 8-byte accesses: the feature rows (d even) and, for V in HBM, its rows ((d+1)c even) must keep the alignment of their bases
    auto al8 = [](const void *p) { return ((uintptr_t)p & 7) == 0; };
    const bool w2 = d % 2 == 0 && c % 2 == 0 && al8(d_pool_feat) && al8(d_V) && (T == 0 || al8(d_tr_feat));
    if (path == 1) {
#define LF_RES(CT)                                                                                                                     \
    return w2 ? lf_launch_resident<CT, 2>(ctx, d_pool_feat, d_pool_post, d_pool_labels, n_pool, d_tr_feat, d_tr_post, n_tr, d_draws, T, \
                                          scale, d, d_V)                                                                               \
              : lf_launch_resident<CT, 1>(ctx, d_pool_feat, d_pool_post, d_pool_labels, n_pool, d_tr_feat, d_tr_post, n_tr, d_draws, T, \
                                          scale, d, d_V)
        if (c == 2) LF_RES(2);
        if (c == 3) LF_RES(3);
        LF_RES(4);
#undef LF_RES
    }
    ALQ_REQUIRE(T == 0 || d_work, ALQ_EINVAL, "alq_llfc_stoch_if: the streaming path needs d_work (alq_llfc_if_work_bytes)");
    return w2 ? lf_launch_streaming<2>(ctx, d_pool_feat, d_pool_post, d_pool_labels, n_pool, d_tr_feat, d_tr_post, n_tr, d_draws, T, scale,
                                       d, c, d_V, (double *)d_work)
              : lf_launch_streaming<1>(ctx, d_pool_feat, d_pool_post, d_pool_labels, n_pool, d_tr_feat, d_tr_post, n_tr, d_draws, T, scale,
                                       d, c, d_V, (double *)d_work);
}

}  // extern "C"
