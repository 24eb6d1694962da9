// Mean-teacher consistency training of a fully-convolutional model (NN_extended.py:913-926, :1337-1396, :1535-1560).
//   * mt_cotangent_kernel<C>: one streaming pass over the student's and the teacher's posterior planes [c, R] (R = N V voxels),
//     the labels and the voxel weights: the cotangent rows [R, c] of  s * sum_v l_v + k' * sum_v div_v  (l: get_FCN_loss's
//     weighted / focal cross-entropy, exactly loss_cotangent_kernel's CE branch; div: the output-perturbation measure between
//     student p and teacher q, 'L2' = mean_j (p_j - q_j)^2 with row_k += k p_k (d_k - sum_j p_j d_j), d = p - q, k = 2 k' / c;
//     'CE' = -sum_j p_j log q_j, which TF does not differentiate: no row term) and per-workgroup fp64 partials of
//     (sum l, number of non-zero weights, sum div).  A lane owns 4 consecutive voxels: every plane, the labels and the weights
//     come in as 16-byte pieces, the 4 c floats of its rows go out as c plain 16-byte stores (global stores through a pointer:
//     not the register-offset buffer stores of alq_internal.h's hazard note).  R % 4 != 0 or an unaligned base: every voxel
//     takes the guarded one-voxel path, as in dense_head_fwd_kernel.  At most ALQ_MT_MAX_BLOCKS workgroups, grid-stride beyond.
//   * mt_cotangent_au_kernel<C>: the same pass for a head of c + 1 channels whose last one, through a ReLU, is a per-voxel
//     log-variance a (AU_4U, NN_extended.py:265-288, :1376-1383, :1551-1554): one plane more comes in (a [R]), the consistency
//     value of a voxel is div e + kappa a / 2 with e = exp(-a), its rows [R, c + 1] are
//         k < c:  [labelled row] + k e p_k (d_k - sum_j p_j d_j)  (L2; CE: the labelled row alone)
//         c:      a > 0 ? k_au (kappa / 2 - div e) : 0            (TF's ReluGrad; both measures)
//     and go out as c + 1 16-byte stores a lane.  Both kernels are one body (mt_body<C, AU>): with a = 0 and kappa = 0 the
//     columns below c and the statistics are mt_cotangent_kernel's, operation for operation.
//   * mt_finish_kernel: the partials into the three statistics: lane t adds partials t, t + 256, ... in that order, the lanes
//     fold in a fixed tree.  No atomics anywhere: bit-identical from run to run.
//   * ema_step_kernel: tf.train.ExponentialMovingAverage's update, shadow -= (shadow - theta) * (1 - decay), in fp32.
//   * perturb_input_kernel: perturb_input (:1337-1351): Gaussian noise, then tf.contrib.image.rotate (nearest neighbour about
//     the centre, zero outside), as one gather.
// This file is compiled without contraction into fused multiply-adds (build.sh): the EMA and the rotation's coordinates are
// stated operation by operation (mteach.py) and must round the same way on the host and on the device.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "alq_internal.h"

namespace alq {

#define ALQ_LAUNCH_CHECK() ALQ_HIP(hipGetLastError())

constexpr int MT_BLOCK = 256;
constexpr int MT_VOX = 4;      // voxels of a lane on the 16-byte path

struct MtArgs {
    const float *p, *q;       // student / teacher posteriors [c, R]
    const int *labels;        // [R]
    const float *sw;          // [R] or null
    const float *cw;          // [c] or null
    float *dl;                // [R, c] or null (statistics only)
    double *part;             // [gridDim.x][3]
    long long R, groups;      // groups of 4 voxels on the 16-byte path
    float gamma, s, k;
    int measure;
    const float *au;          // aleatoric kernel: the student's log-variances [R], >= 0
    float kau, kappa;         // ... the scale of their column and AU_log_rel_coeff
};

__device__ inline double mt_logp(float p) { return log((double)fmaxf(p, 1e-38f)); }

// One voxel: its row (when wanted) and its three statistics.  The labelled part is loss_cotangent_kernel's CE branch operation
// for operation; with a.k == 0 the row is that kernel's, bit for bit.
// AU: `av` is the voxel's log-variance, row has the column C of it, and the third statistic is the consistency value div e + kappa av / 2.
template <int C, int AU>
__device__ inline void mt_voxel(const MtArgs &a, const float (&p)[C], const float (&q)[C], int y, float swv, float av, float (&row)[C + AU],
                                double &sl, double &sc, double &sd) {
    const bool lab = y >= 0 && y < C;
    double mul = 0;
    if (lab) {
        float pt = p[0];
#pragma unroll
        for (int j = 1; j < C; ++j) pt = j == y ? p[j] : pt;
        const double w = (a.cw ? (double)a.cw[y] : 1.0) * (double)swv;
        double f = 1.0, fac = 1.0;
        const double lp = mt_logp(pt);
        if (a.gamma > 0.f) {
            const float om = 1.f - pt;
            const double g = (double)a.gamma;
            if (pt == 1.0f) { f = 0.0; fac = 0.0; }
            else { f = pow((double)om, g); fac = f - g * pow((double)om, g - 1.0) * (double)pt * lp; }
        }
        const double wf = w * f;
        sl -= wf * lp;
        if (wf != 0.0) sc += 1.0;
        mul = w * fac;
    }
    double dot = 0, div = 0;
    if (a.measure == ALQ_MT_L2) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const double dj = (double)p[j] - (double)q[j];
            dot += (double)p[j] * dj;
            div += dj * dj;
        }
        div = div / (double)C;
    } else {
#pragma unroll
        for (int j = 0; j < C; ++j) div -= (double)p[j] * mt_logp(q[j]);
    }
    const double e = AU ? exp(-(double)av) : 1.0;
    sd += AU ? div * e + (0.5 * (double)a.kappa) * (double)av : div;
    if (!a.dl) return;
    const bool cons = a.k != 0.f && a.measure == ALQ_MT_L2;
    const double ke = AU ? (double)a.k * e : (double)a.k;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const float base = lab ? (p[j] - (j == y ? 1.f : 0.f)) * a.s : 0.f;
        float d;
        if (cons) d = (float)((double)base * mul + ke * (double)p[j] * (((double)p[j] - (double)q[j]) - dot));      // one rounding of both terms
        else d = (lab && mul != 1.0) ? (float)((double)base * mul) : base;
        row[j] = d;
    }
    if constexpr (AU != 0) row[C] = av > 0.f ? (float)((double)a.kau * (0.5 * (double)a.kappa - div * e)) : 0.f;      // ReluGrad: g * (x > 0)
}

template <int C, int AU>
__device__ __forceinline__ void mt_body(const MtArgs &a) {
    constexpr int CT = C + AU;      // floats of a row
    __shared__ double sh[3][MT_BLOCK];
    const long long R = a.R, stride = (long long)gridDim.x * MT_BLOCK, t0 = blockIdx.x * (long long)MT_BLOCK + threadIdx.x;
    double sl = 0, sc = 0, sd = 0;
    for (long long g = t0; g < a.groups; g += stride) {
        const long long r0 = MT_VOX * g;
        float4 pv[C], qv[C];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            pv[j] = *reinterpret_cast<const float4 *>(a.p + (long long)j * R + r0);
            qv[j] = *reinterpret_cast<const float4 *>(a.q + (long long)j * R + r0);
        }
        const int4 yv = *reinterpret_cast<const int4 *>(a.labels + r0);
        const float4 wv = a.sw ? *reinterpret_cast<const float4 *>(a.sw + r0) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 uv = AU ? *reinterpret_cast<const float4 *>(a.au + r0) : make_float4(0.f, 0.f, 0.f, 0.f);
        const int ys[MT_VOX] = {yv.x, yv.y, yv.z, yv.w};
        const float ws[MT_VOX] = {wv.x, wv.y, wv.z, wv.w};
        const float us[MT_VOX] = {uv.x, uv.y, uv.z, uv.w};
        float rows[MT_VOX][CT];
#pragma unroll
        for (int v = 0; v < MT_VOX; ++v) {
            float p[C], q[C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                p[j] = v == 0 ? pv[j].x : (v == 1 ? pv[j].y : (v == 2 ? pv[j].z : pv[j].w));
                q[j] = v == 0 ? qv[j].x : (v == 1 ? qv[j].y : (v == 2 ? qv[j].z : qv[j].w));
            }
            mt_voxel<C, AU>(a, p, q, ys[v], ws[v], us[v], rows[v], sl, sc, sd);
        }
        if (a.dl) {      // the rows of voxels r0 .. r0 + 3 are 4 CT consecutive floats
            float4 *out = reinterpret_cast<float4 *>(a.dl + r0 * CT);
#pragma unroll
            for (int i = 0; i < CT; ++i)      // flat element f = v CT + j of the lane's 4 rows
                out[i] = make_float4(rows[(4 * i) / CT][(4 * i) % CT], rows[(4 * i + 1) / CT][(4 * i + 1) % CT],
                                     rows[(4 * i + 2) / CT][(4 * i + 2) % CT], rows[(4 * i + 3) / CT][(4 * i + 3) % CT]);
        }
    }
    // the voxels the groups do not cover, one per lane
    for (long long r = MT_VOX * a.groups + t0; r < R; r += stride) {
        float p[C], q[C], row[CT];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            p[j] = a.p[(long long)j * R + r];
            q[j] = a.q[(long long)j * R + r];
        }
        mt_voxel<C, AU>(a, p, q, a.labels[r], a.sw ? a.sw[r] : 1.f, AU ? a.au[r] : 0.f, row, sl, sc, sd);
        if (a.dl) {
#pragma unroll
            for (int j = 0; j < CT; ++j) a.dl[r * CT + j] = row[j];
        }
    }
    sh[0][threadIdx.x] = sl; sh[1][threadIdx.x] = sc; sh[2][threadIdx.x] = sd;
    __syncthreads();
    for (int o = MT_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
            sh[2][threadIdx.x] += sh[2][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) a.part[blockIdx.x * 3 + threadIdx.x] = sh[threadIdx.x][0];
}

template <int C>
__global__ __launch_bounds__(MT_BLOCK) void mt_cotangent_kernel(MtArgs a) { mt_body<C, 0>(a); }

template <int C>
__global__ __launch_bounds__(MT_BLOCK) void mt_cotangent_au_kernel(MtArgs a) { mt_body<C, 1>(a); }

__global__ __launch_bounds__(MT_BLOCK) void mt_finish_kernel(const double *part, int nblk, double *stats) {
    __shared__ double sh[3][MT_BLOCK];
    double s[3] = {0, 0, 0};
    for (int b = threadIdx.x; b < nblk; b += MT_BLOCK) {
        s[0] += part[b * 3]; s[1] += part[b * 3 + 1]; s[2] += part[b * 3 + 2];
    }
    sh[0][threadIdx.x] = s[0]; sh[1][threadIdx.x] = s[1]; sh[2][threadIdx.x] = s[2];
    __syncthreads();
    for (int o = MT_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
            sh[2][threadIdx.x] += sh[2][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) stats[threadIdx.x] = sh[threadIdx.x][0];
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int mt_check(const char *who, const float *post, const float *tpost, int c, long long R, const int32_t *labels, const alq_loss_t *loss,
             int measure) {
    ALQ_REQUIRE(post && labels && loss, ALQ_EINVAL, "%s: null argument", who);
    ALQ_REQUIRE(tpost, ALQ_EINVAL, "%s: the teacher's posterior planes are missing", who);
    ALQ_REQUIRE(c >= 2 && c <= 8, ALQ_EINVAL, "%s: %d classes (2 .. 8)", who, c);
    ALQ_REQUIRE(R >= 1, ALQ_EINVAL, "%s: R=%lld", who, R);
    ALQ_REQUIRE(measure == ALQ_MT_L2 || measure == ALQ_MT_CE, ALQ_EINVAL, "%s: output-perturbation measure %d", who, measure);
    ALQ_REQUIRE(loss->kind == ALQ_LOSS_CE && !loss->d_targets && !loss->d_old_logits, ALQ_EINVAL,
                "%s: the labelled objective is the weighted / focal cross-entropy (no targets, no old logits)", who);
    return ALQ_OK;
}

// au null: mt_cotangent_kernel, rows [R, c]; else mt_cotangent_au_kernel, rows [R, c + 1] (c <= 7)
static int mt_launch(alq_ctx *ctx, const float *post_cR, const float *tpost_cR, const float *au, int c, long long R, const int *labels,
                     const alq_loss_t *loss, float loss_scale, float cons_scale, float au_scale, float kappa, int measure, float *dlogits,
                     double *d_stats3) {
    if (!ctx->mt_part) ALQ_HIP(hipMalloc(&ctx->mt_part, (size_t)ALQ_MT_MAX_BLOCKS * 3 * sizeof(double)));
    MtArgs a;
    a.p = post_cR; a.q = tpost_cR; a.labels = labels; a.sw = loss->d_sample_w; a.cw = loss->d_class_w; a.dl = dlogits;
    a.part = ctx->mt_part; a.R = R; a.gamma = loss->focal_gamma; a.s = loss_scale; a.k = cons_scale; a.measure = measure;
    a.au = au; a.kau = au_scale; a.kappa = kappa;
    const bool vec = R % MT_VOX == 0 && aligned16(post_cR) && aligned16(tpost_cR) && aligned16(labels) && aligned16(loss->d_sample_w) &&
                     aligned16(dlogits) && aligned16(au);
    a.groups = vec ? R / MT_VOX : 0;
    const long long lanes = std::max(a.groups, R - MT_VOX * a.groups);
    const int nblk = (int)std::max(1LL, std::min((lanes + MT_BLOCK - 1) / MT_BLOCK, (long long)ALQ_MT_MAX_BLOCKS));
    {
        ProfScope ps(ctx, PROF_ELEMWISE, 0);
#define CALL(CC) hipLaunchKernelGGL(mt_cotangent_kernel<CC>, dim3((unsigned)nblk), dim3(MT_BLOCK), 0, ctx->stream, a)
#define CALL_AU(CC) hipLaunchKernelGGL(mt_cotangent_au_kernel<CC>, dim3((unsigned)nblk), dim3(MT_BLOCK), 0, ctx->stream, a)
        if (au) {
            switch (c) {
                case 2: CALL_AU(2); break;
                case 3: CALL_AU(3); break;
                case 4: CALL_AU(4); break;
                case 5: CALL_AU(5); break;
                case 6: CALL_AU(6); break;
                default: CALL_AU(7); break;
            }
        } else {
            switch (c) {
                case 2: CALL(2); break;
                case 3: CALL(3); break;
                case 4: CALL(4); break;
                case 5: CALL(5); break;
                case 6: CALL(6); break;
                case 7: CALL(7); break;
                default: CALL(8); break;
            }
        }
#undef CALL
#undef CALL_AU
        ALQ_LAUNCH_CHECK();
    }
    if (d_stats3) {
        ProfScope ps(ctx, PROF_REDUCE, 0);
        hipLaunchKernelGGL(mt_finish_kernel, dim3(1), dim3(MT_BLOCK), 0, ctx->stream, ctx->mt_part, nblk, d_stats3);
        ALQ_LAUNCH_CHECK();
    }
    return ALQ_OK;
}

int k_mt_cotangent(alq_ctx *ctx, const float *post_cR, const float *tpost_cR, int c, long long R, const int *labels,
                   const alq_loss_t *loss, float loss_scale, float cons_scale, int measure, float *dlogits, double *d_stats3) {
    return mt_launch(ctx, post_cR, tpost_cR, nullptr, c, R, labels, loss, loss_scale, cons_scale, 0.f, 0.f, measure, dlogits, d_stats3);
}

int mt_check_au(const char *who, const float *post, const float *tpost, const float *au, int c, long long R, const int32_t *labels,
                const alq_loss_t *loss, int measure) {
    ALQ_REQUIRE(au, ALQ_EINVAL, "%s: the log-variance plane is missing", who);
    ALQ_REQUIRE(c >= 2 && c <= 7, ALQ_EINVAL, "%s: %d classes beside the log-variance channel (2 .. 7)", who, c);
    return mt_check(who, post, tpost, c, R, labels, loss, measure);
}

int k_mt_cotangent_au(alq_ctx *ctx, const float *post_cR, const float *tpost_cR, const float *au, int c, long long R, const int *labels,
                      const alq_loss_t *loss, float loss_scale, float cons_scale, float au_scale, float kappa, int measure, float *dlogits,
                      double *d_stats3) {
    return mt_launch(ctx, post_cR, tpost_cR, au, c, R, labels, loss, loss_scale, cons_scale, au_scale, kappa, measure, dlogits, d_stats3);
}

// ------------------------------------------------------------------------------------------ the teacher's weights
__device__ inline float ema_one(float sh, float th, float omd) { return sh - (sh - th) * omd; }

__global__ void ema_step_kernel(float *shadow, const float *theta, long long n, long long n4, float omd) {
    const long long stride = (long long)gridDim.x * blockDim.x, i0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    float4 *s4 = reinterpret_cast<float4 *>(shadow);
    const float4 *t4 = reinterpret_cast<const float4 *>(theta);
    for (long long i = i0; i < n4; i += stride) {
        float4 s = s4[i];
        const float4 t = t4[i];
        s.x = ema_one(s.x, t.x, omd); s.y = ema_one(s.y, t.y, omd); s.z = ema_one(s.z, t.z, omd); s.w = ema_one(s.w, t.w, omd);
        s4[i] = s;
    }
    for (long long i = 4 * n4 + i0; i < n; i += stride) shadow[i] = ema_one(shadow[i], theta[i], omd);
}

// ------------------------------------------------------------------------------------------ the teacher's input
struct PerturbArgs {
    const float *x;
    float *out;
    long long total;      // N H W C
    int H, W, C, rotate;
    float std, ca, sa, xo, yo;
    unsigned long long seed;
    long long first_sample;
};

// the layers' dropout masks carry their layer index (< 64) in the top byte of the key: no layer has this one
constexpr unsigned long long MT_NOISE_TAG = 0xFFull << 56;

__device__ inline float mt_noise(unsigned long long seed, long long sample, long long e) {
    const unsigned long long h = tr_splitmix64(tr_splitmix64(seed ^ ((unsigned long long)sample * 0xD1B54A32D192ED03ull) ^ MT_NOISE_TAG) +
                                               (unsigned long long)e);
    const float u1 = (float)((unsigned)(h >> 40) + 1u) * (1.0f / 16777216.0f);             // (0, 1]
    const float u2 = (float)((unsigned)(h >> 16) & 0xFFFFFFu) * (1.0f / 16777216.0f);      // [0, 1)
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

__global__ void perturb_input_kernel(PerturbArgs a) {
    const long long per = (long long)a.H * a.W * a.C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < a.total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / per, e = i - n * per;
        long long src = e;
        bool inside = true;
        if (a.rotate) {
            const long long pix = e / a.C;
            const int ch = (int)(e - pix * a.C), y = (int)(pix / a.W), x = (int)(pix - (long long)y * a.W);
            const float fx = (float)x, fy = (float)y;
            const float ys = roundf((a.sa * fx + a.ca * fy) + a.yo), xs = roundf((a.ca * fx - a.sa * fy) + a.xo);
            inside = ys >= 0.f && ys <= (float)(a.H - 1) && xs >= 0.f && xs <= (float)(a.W - 1);
            src = inside ? ((long long)ys * a.W + (long long)xs) * a.C + ch : 0;
        }
        float v = 0.f;
        if (inside) {
            v = a.x[n * per + src];
            if (a.std > 0.f) v = v + a.std * mt_noise(a.seed, a.first_sample + n, src);
        }
        a.out[i] = v;
    }
}

}  // namespace alq

extern "C" {

int64_t alq_mt_trip_voxels(void) { return (int64_t)alq::MT_VOX * alq::MT_BLOCK * ALQ_MT_MAX_BLOCKS; }

int alq_mt_cotangent(alq_ctx *ctx, const float *d_post, const float *d_teacher_post, int c, int64_t R, const int32_t *d_labels,
                     const alq_loss_t *loss, float loss_scale, float cons_scale, int measure, float *d_rows, double *d_stats3) {
    ALQ_REQUIRE(ctx && d_rows && d_stats3, ALQ_EINVAL, "alq_mt_cotangent: null argument");
    ALQ_TRY(alq::mt_check("alq_mt_cotangent", d_post, d_teacher_post, c, R, d_labels, loss, measure));
    ALQ_HIP(hipSetDevice(ctx->device));
    return alq::k_mt_cotangent(ctx, d_post, d_teacher_post, c, R, d_labels, loss, loss_scale, cons_scale, measure, d_rows, d_stats3);
}

int alq_mt_stats(alq_ctx *ctx, const float *d_post, const float *d_teacher_post, int c, int64_t R, const int32_t *d_labels,
                 const alq_loss_t *loss, int measure, double *d_stats3) {
    ALQ_REQUIRE(ctx && d_stats3, ALQ_EINVAL, "alq_mt_stats: null argument");
    ALQ_TRY(alq::mt_check("alq_mt_stats", d_post, d_teacher_post, c, R, d_labels, loss, measure));
    ALQ_HIP(hipSetDevice(ctx->device));
    return alq::k_mt_cotangent(ctx, d_post, d_teacher_post, c, R, d_labels, loss, 1.f, 0.f, measure, nullptr, d_stats3);
}

int64_t alq_mt_au_trip_voxels(void) { return alq_mt_trip_voxels(); }

int alq_mt_cotangent_au(alq_ctx *ctx, const float *d_post, const float *d_teacher_post, const float *d_au, int c, int64_t R,
                        const int32_t *d_labels, const alq_loss_t *loss, float loss_scale, float cons_scale, float au_scale,
                        float au_log_rel_coeff, int measure, float *d_rows, double *d_stats3) {
    ALQ_REQUIRE(ctx && d_rows && d_stats3, ALQ_EINVAL, "alq_mt_cotangent_au: null argument");
    ALQ_TRY(alq::mt_check_au("alq_mt_cotangent_au", d_post, d_teacher_post, d_au, c, R, d_labels, loss, measure));
    ALQ_HIP(hipSetDevice(ctx->device));
    return alq::k_mt_cotangent_au(ctx, d_post, d_teacher_post, d_au, c, R, d_labels, loss, loss_scale, cons_scale, au_scale, au_log_rel_coeff,
                                  measure, d_rows, d_stats3);
}

int alq_mt_stats_au(alq_ctx *ctx, const float *d_post, const float *d_teacher_post, const float *d_au, int c, int64_t R,
                    const int32_t *d_labels, const alq_loss_t *loss, float au_log_rel_coeff, int measure, double *d_stats3) {
    ALQ_REQUIRE(ctx && d_stats3, ALQ_EINVAL, "alq_mt_stats_au: null argument");
    ALQ_TRY(alq::mt_check_au("alq_mt_stats_au", d_post, d_teacher_post, d_au, c, R, d_labels, loss, measure));
    ALQ_HIP(hipSetDevice(ctx->device));
    return alq::k_mt_cotangent_au(ctx, d_post, d_teacher_post, d_au, c, R, d_labels, loss, 1.f, 0.f, 0.f, au_log_rel_coeff, measure, nullptr,
                                  d_stats3);
}

int alq_ema_step(alq_ctx *ctx, float *d_shadow, const float *d_theta, int64_t n, float decay) {
    ALQ_REQUIRE(ctx && n >= 0 && (n == 0 || (d_shadow && d_theta)), ALQ_EINVAL, "alq_ema_step: bad argument");
    ALQ_REQUIRE(decay >= 0.f && decay <= 1.f, ALQ_EINVAL, "alq_ema_step: decay %g outside [0, 1]", (double)decay);
    if (n == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(ctx->device));
    const uintptr_t bits = reinterpret_cast<uintptr_t>(d_shadow) | reinterpret_cast<uintptr_t>(d_theta);
    const long long n4 = (bits & 15) ? 0 : n / 4;          // a vector that does not start on 16 bytes takes the scalar loop
    long long blocks = ((n4 ? n4 : n) + 255) / 256;
    blocks = std::max(1LL, std::min(blocks, 65535LL * 16));
    hipLaunchKernelGGL(alq::ema_step_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_shadow, d_theta, (long long)n, n4,
                       1.f - decay);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

int alq_perturb_input(alq_ctx *ctx, const float *d_x, float *d_out, int N, int H, int W, int C, float noise_std, uint64_t seed,
                      int64_t first_sample, int rotate, float angle) {
    ALQ_REQUIRE(ctx && d_x && d_out, ALQ_EINVAL, "alq_perturb_input: null argument");
    ALQ_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1, ALQ_EINVAL, "alq_perturb_input: N=%d H=%d W=%d C=%d", N, H, W, C);
    ALQ_REQUIRE(noise_std >= 0.f, ALQ_EINVAL, "alq_perturb_input: noise_std %g", (double)noise_std);
    ALQ_REQUIRE(!rotate || d_x != d_out, ALQ_EINVAL, "alq_perturb_input: a rotation cannot run in place");
    ALQ_HIP(hipSetDevice(ctx->device));
    alq::PerturbArgs a;
    a.x = d_x; a.out = d_out; a.total = (long long)N * H * W * C; a.H = H; a.W = W; a.C = C; a.rotate = rotate ? 1 : 0;
    a.std = noise_std; a.seed = seed; a.first_sample = first_sample;
    // tf.contrib.image.angles_to_projective_transforms in fp32, one operation at a time (mteach.rotation_offsets)
    const float w1 = (float)(W - 1), h1 = (float)(H - 1);
    a.ca = cosf(angle); a.sa = sinf(angle);
    a.xo = (w1 - (a.ca * w1 - a.sa * h1)) / 2.f;
    a.yo = (h1 - (a.sa * w1 + a.ca * h1)) / 2.f;
    const long long blocks = std::max(1LL, std::min((a.total + 255) / 256, 65535LL * 16));
    alq::ProfScope ps(ctx, alq::PROF_ELEMWISE, 0);
    hipLaunchKernelGGL(alq::perturb_input_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

}  // extern "C"
