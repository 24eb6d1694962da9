// Fully-connected CRF on a two-class posterior map (the reference's PW_analyze_results.DCRF_postprocess_2D: pydensecrf's
// DenseCRF2D with a smoothness and an appearance kernel, NORMALIZE_SYMMETRIC, Potts compatibilities, mean-field inference, arg-max)
// with the two Gaussian filters computed exactly on a window instead of on a permutohedral lattice.
//
//   alq_dcrf2d   S independent slices [H, W]: class-1 marginal after `niter` mean-field iterations and / or its arg-max
//
// Per pixel i of a slice, with p the posterior read (0 -> 1e-10):  nl = -log p,  U = float32(1 - nl, nl)  (the reference's unary,
// quirk included: label 0 gets 1 + log p),  dU = U_0 - U_1.  Per kernel  k(i, j) = exp(-|f_i - f_j|^2 / 2)  with
// f = (row / sd[0], column / sd[1]) (smoothness) or (row / sd[0], column / sd[1], img / schan) (appearance), evaluated on the
// window |d row| <= R_0, |d column| <= R_1, R = ceil(sd sqrt(48 ln 2)) (what is dropped is below 2^-24 of the peak), clipped
// to the slice;  n_i = 1 / sqrt(sum_j k(i, j) + 1e-20)  over the same window.  Only the class-1 plane q is carried (Q_0 = 1 - q):
//   q <- sigmoid(dU)                                                                                  (= softmax(-U)_1)
//   q <- sigmoid(b_i + 2 w_s n^s_i sum_j k_s n^s_j q_j + 2 w_a n^a_i sum_j k_a n^a_j q_j),   b_i = dU_i - w_s n^s_i sum_j k_s n^s_j
//                                                                                                  - w_a n^a_i sum_j k_a n^a_j
// which is softmax(-U + w_s K~_s Q + w_a K~_a Q)_1 with K~ = diag(n) K diag(n).
//
// One kernel body does every windowed sum  (sum_j k_s(i, j) v^s_j, sum_j k_a(i, j) v^a_j);  what is staged as v tells the launches
// apart:  NORM  v = [j inside the slice] -> n^s, n^a (and the unaries: dU, q_0);  BIAS  v = n_j -> b;  ITER  v = n_j q_j -> q.
// Every iteration needs the whole previous q, so the launch boundaries are the grid-wide dependency: 2 + niter launches.
// A 512-thread workgroup owns a tile of 32 rows x 64 columns.  It stages (img sqrt(log2 e / 2) / schan, v^a) of the tile plus
// the appearance halo as float2 and v^s of the tile plus the smoothness halo in LDS once.  Lanes run along the columns, so a
// wave reads 64 consecutive float2 (conflict-free); a wave owns 4 rows and every staged value it reads feeds its 4 outputs from
// registers.  A tap is  d = a_i - a_j,  e = exp2(-d d + lx[|dx|]),  acc += e v_j :  the column weight sits in the exponent
// (lx = -dx^2 log2 e / (2 sd_1^2), a table held in the lanes of one register and read with v_readlane), the row weight
// exp(-dy^2 / (2 sd_0^2)) multiplies the finished row sum.  The smoothness kernel is separable (13 x 13) and runs in the same
// launch on the rows already staged.  Sums run in one fixed order and no atomics are used: the same input gives the same bits.
// Work buffer: 5 floats per pixel (n^s, n^a, b, two q planes).
#include <algorithm>
#include <cmath>

#include "alq_internal.h"

namespace alq {

namespace {

constexpr int DC_LANES = 64;                      // tile columns = lanes of a wave
// (measured at 32 x 256 x 256 and 8 x 512 x 512, same bits: 16 waves x 4 rows takes 10 % less time per launch and 8 waves x 8 rows 4 %
// less, but a single 256 x 256 slice - 16 tiles instead of 32 - takes 1.8 x and 1.9 x as long)
constexpr int DC_WAVES = 8;
constexpr int DC_RPT = 4;                         // output rows per wave
constexpr int DC_TH = DC_WAVES * DC_RPT;          // tile rows
constexpr int DC_THREADS = DC_WAVES * 64;
constexpr int DC_MAXR = 31;                       // window radii: a weight table (2 R + 1 entries) lives in the 64 lanes of one register
constexpr size_t DC_MAX_LDS = 160 * 1024;

enum { DC_NORM = 0, DC_BIAS = 1, DC_ITER = 2 };

struct DcGeo {
    int S, H, W;
    int ray, rax;          // appearance window radii (rows, columns)
    int rsy, rsx;          // smoothness window radii
    float isy2a, isx2a;    // appearance: 1 / (2 sd_0^2), log2 e / (2 sd_1^2)
    float isy2s, isx2s;    // smoothness: 1 / (2 sd_0^2), 1 / (2 sd_1^2)
    float cscale;          // sqrt(log2 e / 2) / schan
    float ws, wa;          // compatibilities
};

// dU = U_0 - U_1 of the reference's unary: nl = -log p in double as NumPy takes it, U = float32(1 - nl, nl)
__device__ inline float dc_unary(float p) {
    const double pd = p == 0.f ? 1e-10 : (double)p;
    const double nl = -log(pd);
    return (float)(1.0 - nl) - (float)nl;
}

// pitch of the staged appearance image: the tile, the halo and the columns that round the window up to whole steps of four
__host__ __device__ inline int dc_pitch_a(int rax) { return DC_LANES + 4 * ((2 * rax + 4) >> 2); }

__device__ inline float dc_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

__device__ inline float dc_lane(float table, int idx) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(table), idx)); }

// q_0 = softmax(-U)_1 alone (niter = 0)
__global__ __launch_bounds__(256) void dcrf_unary_kernel(const float *__restrict__ post, long long n, float *__restrict__ q1,
                                                         unsigned char *__restrict__ map) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float q = dc_sigmoid(dc_unary(post[i]));
        if (q1) q1[i] = q;
        if (map) map[i] = (unsigned char)(q > 0.5f);
    }
}

template <int MODE>
__global__ __launch_bounds__(DC_THREADS) void dcrf_filter_kernel(DcGeo g, const float *__restrict__ post, const float *__restrict__ img,
                                                                 float *__restrict__ ns, float *__restrict__ na, float *bias,
                                                                 const float *__restrict__ qin, float *__restrict__ qout,
                                                                 unsigned char *__restrict__ map) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dc_lds[];
    const int pa = dc_pitch_a(g.rax), rows_a = DC_TH + 2 * g.ray;      // appearance image: pitch, rows
    const int ps = DC_LANES + 2 * g.rsx, rows_s = DC_TH + 2 * g.rsy;      // smoothness image
    float2 *sa = reinterpret_cast<float2 *>(dc_lds);
    float *ss = reinterpret_cast<float *>(dc_lds + (size_t)pa * rows_a * sizeof(float2));
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = blockIdx.x * DC_LANES, y0 = blockIdx.y * DC_TH;
    const long long plane = (long long)blockIdx.z * g.H * g.W;
    img += plane;
    ns += plane;
    na += plane;
    bias += plane;

    // ---- stage (a_j, v^a_j) and v^s_j; outside the slice v = 0: the window is clipped
    for (int t = threadIdx.x; t < pa * rows_a; t += DC_THREADS) {
        const int r = t / pa, c = t - r * pa;
        const int y = y0 - g.ray + r, x = x0 - g.rax + c;
        float2 v = make_float2(0.f, 0.f);
        if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
            const long long j = (long long)y * g.W + x;
            v.x = img[j] * g.cscale;
            v.y = MODE == DC_NORM ? 1.f : MODE == DC_BIAS ? na[j] : na[j] * qin[plane + j];
        }
        sa[t] = v;
    }
    for (int t = threadIdx.x; t < ps * rows_s; t += DC_THREADS) {
        const int r = t / ps, c = t - r * ps;
        const int y = y0 - g.rsy + r, x = x0 - g.rsx + c;
        float v = 0.f;
        if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
            const long long j = (long long)y * g.W + x;
            v = MODE == DC_NORM ? 1.f : MODE == DC_BIAS ? ns[j] : ns[j] * qin[plane + j];
        }
        ss[t] = v;
    }
    // weight tables, the entry of window column (row) k = d + R in lane k: the column weights of the appearance kernel as
    // exponents, the other three as factors
    const float dxa = (float)(lane - g.rax), dya = (float)(lane - g.ray), dxs = (float)(lane - g.rsx), dys = (float)(lane - g.rsy);
    const float lxa = lane <= 2 * g.rax ? -dxa * dxa * g.isx2a : -INFINITY;
    const float wya = expf(-dya * dya * g.isy2a);
    const float wxs = expf(-dxs * dxs * g.isx2s);
    const float wys = expf(-dys * dys * g.isy2s);
    __syncthreads();

    // ---- appearance kernel: rows [wave * RPT, wave * RPT + RPT - 1 + 2 ray] of the staged image feed this wave's RPT output rows
    float ai[DC_RPT], acc_a[DC_RPT], acc_s[DC_RPT];
#pragma unroll
    for (int p = 0; p < DC_RPT; ++p) {
        ai[p] = sa[(wave * DC_RPT + p + g.ray) * pa + lane + g.rax].x;
        acc_a[p] = 0.f;
        acc_s[p] = 0.f;
    }
    const int ngrp = (2 * g.rax + 4) >> 2;      // steps of four window columns; the columns past the window weigh exp2(-inf) = 0
    for (int rr = 0; rr < DC_RPT + 2 * g.ray; ++rr) {
        const float2 *row = sa + (wave * DC_RPT + rr) * pa + lane;
        float racc[DC_RPT];
#pragma unroll
        for (int p = 0; p < DC_RPT; ++p) racc[p] = 0.f;
        // four taps per step; the next step's reads are in flight under this step's arithmetic
        float2 t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = row[u];
        for (int gq = 0; gq < ngrp; ++gq) {
            const int nx = 4 * min(gq + 1, ngrp - 1);
            float2 tn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) tn[u] = row[nx + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float lx = dc_lane(lxa, 4 * gq + u);
#pragma unroll
                for (int p = 0; p < DC_RPT; ++p) {
                    const float d = ai[p] - t[u].x;
                    const float e = __builtin_amdgcn_exp2f(fmaf(-d, d, lx));
                    racc[p] = fmaf(e, t[u].y, racc[p]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = tn[u];
        }
        // output row p sees this row at dy = rr - p - ray; outside the window the row weight is 0
#pragma unroll
        for (int p = 0; p < DC_RPT; ++p) {
            const int k = rr - p;
            const float wy = k >= 0 && k <= 2 * g.ray ? dc_lane(wya, k) : 0.f;
            acc_a[p] = fmaf(wy, racc[p], acc_a[p]);
        }
    }
    // ---- smoothness kernel: separable, one row sum serves the RPT outputs
    const int nds = 2 * g.rsx + 1;
    for (int rr = 0; rr < DC_RPT + 2 * g.rsy; ++rr) {
        const float *row = ss + (wave * DC_RPT + rr) * ps + lane;
        float rs = 0.f;
        for (int dxi = 0; dxi < nds; ++dxi) rs = fmaf(dc_lane(wxs, dxi), row[dxi], rs);
#pragma unroll
        for (int p = 0; p < DC_RPT; ++p) {
            const int k = rr - p;
            const float wy = k >= 0 && k <= 2 * g.rsy ? dc_lane(wys, k) : 0.f;
            acc_s[p] = fmaf(wy, rs, acc_s[p]);
        }
    }

    // ---- epilogue: every thread touches its own pixels only
    const int x = x0 + lane;
#pragma unroll
    for (int p = 0; p < DC_RPT; ++p) {
        const int y = y0 + wave * DC_RPT + p;
        if (y >= g.H || x >= g.W) continue;
        const long long i = (long long)y * g.W + x;
        if (MODE == DC_NORM) {
            ns[i] = 1.f / sqrtf(acc_s[p] + 1e-20f);
            na[i] = 1.f / sqrtf(acc_a[p] + 1e-20f);
            const float du = dc_unary(post[plane + i]);
            bias[i] = du;
            qout[plane + i] = dc_sigmoid(du);
        } else if (MODE == DC_BIAS) {
            bias[i] = bias[i] - g.ws * (ns[i] * acc_s[p]) - g.wa * (na[i] * acc_a[p]);
        } else {
            const float q = dc_sigmoid(bias[i] + 2.f * g.ws * (ns[i] * acc_s[p]) + 2.f * g.wa * (na[i] * acc_a[p]));
            if (qout) qout[plane + i] = q;
            if (map) map[plane + i] = (unsigned char)(q > 0.5f);
        }
    }
}

const alq_dcrf_params kDcDefaults = {{1.f, 1.f}, {5.f, 5.f}, 1.f, 20.f, 30.f, 5};

// window radius of a kernel axis: what lies beyond carries less than 2^-24 of the peak weight
int dc_radius(float sd) { return (int)std::ceil((double)sd * std::sqrt(48.0 * std::log(2.0))); }

// dims -> S, H, W; false: an axis below 1 or 2^31 pixels and more
bool dc_dims(const int64_t dims[3], DcGeo *g) {
    const int64_t lim = (int64_t)1 << 31;
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 1 || dims[a] >= lim) return false;
    if (dims[1] * dims[2] >= lim || dims[0] * dims[1] * dims[2] >= lim) return false;
    g->S = (int)dims[0];
    g->H = (int)dims[1];
    g->W = (int)dims[2];
    return true;
}

size_t dc_lds_bytes(const DcGeo &g) {
    return (size_t)dc_pitch_a(g.rax) * (DC_TH + 2 * g.ray) * sizeof(float2) + (size_t)(DC_LANES + 2 * g.rsx) * (DC_TH + 2 * g.rsy) * sizeof(float);
}

template <int MODE>
int dc_launch(alq_ctx *ctx, const DcGeo &g, const float *post, const float *img, float *ns, float *na, float *bias, const float *qin,
              float *qout, unsigned char *map) {
    const size_t lds = dc_lds_bytes(g);
    auto kfn = dcrf_filter_kernel<MODE>;
    ALQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((g.W + DC_LANES - 1) / DC_LANES, (g.H + DC_TH - 1) / DC_TH, g.S);
    // taps the launch evaluates: 2 flops (multiply, add) each on the accumulate side
    ProfScope ps(ctx, PROF_REDUCE, 2.0 * g.S * g.H * g.W * ((2.0 * g.ray + 1) * (2.0 * g.rax + 1) + (2.0 * g.rsy + 1) * (2.0 * g.rsx + 1)));
    hipLaunchKernelGGL(kfn, grid, dim3(DC_THREADS), lds, ctx->stream, g, post, img, ns, na, bias, qin, qout, map);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // namespace

}  // namespace alq

using namespace alq;

extern "C" {

size_t alq_dcrf_work_bytes(const int64_t dims[3]) {
    DcGeo g;
    if (!dims || !dc_dims(dims, &g)) return 0;
    return (size_t)5 * sizeof(float) * g.S * g.H * g.W;
}

int alq_dcrf2d(alq_ctx *ctx, const float *d_post, const float *d_img, const int64_t dims[3], const alq_dcrf_params *par, float *d_q1,
               uint8_t *d_map, void *d_work) {
    ALQ_REQUIRE(ctx && d_post && d_img && dims && d_work, ALQ_EINVAL, "alq_dcrf2d: null argument");
    ALQ_REQUIRE(d_q1 || d_map, ALQ_EINVAL, "alq_dcrf2d: neither d_q1 nor d_map");
    DcGeo g;
    ALQ_REQUIRE(dc_dims(dims, &g), ALQ_EINVAL, "alq_dcrf2d: dims %lld x %lld x %lld (each >= 1, below 2^31 pixels)", (long long)dims[0],
                (long long)dims[1], (long long)dims[2]);
    const alq_dcrf_params P = par ? *par : kDcDefaults;
    ALQ_REQUIRE(P.niter >= 0 && P.niter <= 64, ALQ_EINVAL, "alq_dcrf2d: niter %d outside [0, 64]", P.niter);
    const float vals[7] = {P.sdims_smooth[0], P.sdims_smooth[1], P.sdims_app[0], P.sdims_app[1], P.schan, P.compat_smooth, P.compat_app};
    for (int k = 0; k < 7; ++k) ALQ_REQUIRE(std::isfinite(vals[k]), ALQ_EINVAL, "alq_dcrf2d: parameter %d is not finite", k);
    for (int k = 0; k < 5; ++k) ALQ_REQUIRE(vals[k] > 0.f, ALQ_EINVAL, "alq_dcrf2d: sdims / schan must be positive (parameter %d = %g)", k, vals[k]);
    ALQ_REQUIRE(((uintptr_t)d_work & 3) == 0, ALQ_EINVAL, "alq_dcrf2d: d_work not 4-byte aligned");
    g.rsy = dc_radius(P.sdims_smooth[0]);
    g.rsx = dc_radius(P.sdims_smooth[1]);
    g.ray = dc_radius(P.sdims_app[0]);
    g.rax = dc_radius(P.sdims_app[1]);
    ALQ_REQUIRE(g.S <= 65535, ALQ_EUNSUPPORTED, "alq_dcrf2d: %d slices in one call (at most 65535)", g.S);
    ALQ_REQUIRE(std::max(std::max(g.rsy, g.rsx), std::max(g.ray, g.rax)) <= DC_MAXR && dc_lds_bytes(g) <= DC_MAX_LDS, ALQ_EUNSUPPORTED,
                "alq_dcrf2d: windows %d x %d and %d x %d do not fit a workgroup's LDS", 2 * g.rsy + 1, 2 * g.rsx + 1, 2 * g.ray + 1, 2 * g.rax + 1);
    const double log2e = 1.4426950408889634;
    g.isy2s = (float)(1.0 / (2.0 * P.sdims_smooth[0] * P.sdims_smooth[0]));
    g.isx2s = (float)(1.0 / (2.0 * P.sdims_smooth[1] * P.sdims_smooth[1]));
    g.isy2a = (float)(1.0 / (2.0 * P.sdims_app[0] * P.sdims_app[0]));
    g.isx2a = (float)(log2e / (2.0 * P.sdims_app[1] * P.sdims_app[1]));
    g.cscale = (float)(std::sqrt(log2e / 2.0) / P.schan);
    g.ws = P.compat_smooth;
    g.wa = P.compat_app;
    ALQ_HIP(hipSetDevice(ctx->device));
    const long long n = (long long)g.S * g.H * g.W;
    if (P.niter == 0) {
        ProfScope ps(ctx, PROF_ELEMWISE, 0);
        const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)ctx->num_cus * 8));
        hipLaunchKernelGGL(dcrf_unary_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_post, n, d_q1, d_map);
        ALQ_HIP(hipGetLastError());
        return ALQ_OK;
    }
    float *w = static_cast<float *>(d_work);
    float *ns = w, *na = w + n, *bias = w + 2 * n, *q[2] = {w + 3 * n, w + 4 * n};
    ALQ_TRY(dc_launch<DC_NORM>(ctx, g, d_post, d_img, ns, na, bias, nullptr, q[0], nullptr));
    ALQ_TRY(dc_launch<DC_BIAS>(ctx, g, d_post, d_img, ns, na, bias, nullptr, nullptr, nullptr));
    for (int it = 0; it < P.niter; ++it) {
        const bool last = it == P.niter - 1;
        ALQ_TRY(dc_launch<DC_ITER>(ctx, g, d_post, d_img, ns, na, bias, q[it & 1], last ? d_q1 : q[(it + 1) & 1], last ? d_map : nullptr));
    }
    return ALQ_OK;
}

}  // extern "C"
