// Training objectives of NN_extended.CNN at the logits and the RMSProp step.
//   * loss_cotangent_kernel: the cotangent rows dlogits [N, c] and the loss statistics of weighted / focal cross-entropy
//     (NN_extended.get_loss, NN_extended.py:1221-1259, focal term as get_FCN_loss applies it, :1296-1335), CE_softclasses
//     (:1261-1271), GCE (:1273-1277, compute_Lq :1530-1533) and the learning-without-forgetting term of model_utils.get_LwF
//     (model_utils.py:98-135) - everything these objectives change about a training step; the backward sweep and the weight
//     products are those of alq_param_grads.
//   * rmsprop_step_kernel: tf.train.RMSPropOptimizer (not centred) on flat device vectors.
// Nothing here is on the scoring path.  One thread per sample (c is a handful), per-sample arithmetic in fp64 on the fp32
// posteriors, per-workgroup partials of the three statistics folded in a fixed tree and summed in workgroup order by a second
// launch: no atomics, bit-identical from run to run.
#include <algorithm>
#include <cstdint>

#include "alq_internal.h"

namespace alq {

#define ALQ_LAUNCH_CHECK() ALQ_HIP(hipGetLastError())

constexpr int LOSS_BLOCK = 256;

struct LossArgs {
    const float *post;        // [c, N]
    const int *labels;        // [N] or null (soft kinds)
    const float *class_w;     // [c] or null
    const float *sample_w;    // [N] or null
    const float *targets;     // [c, N] or null
    const float *old_logits;  // [c, N] or null
    int c, N, kind;
    float gamma, q, T;
    float s, s2;              // loss_scale, lwf_scale
    float *dl;                // [N, c] or null (statistics only)
    double *part;             // [gridDim.x][3]
};

__device__ inline double loss_logp(float p) { return log((double)fmaxf(p, 1e-38f)); }

__global__ __launch_bounds__(LOSS_BLOCK) void loss_cotangent_kernel(LossArgs a) {
    __shared__ double sh[3][LOSS_BLOCK];
    const int c = a.c, N = a.N;
    double sl = 0, sc = 0, s2 = 0;
    for (int n = blockIdx.x * LOSS_BLOCK + threadIdx.x; n < N; n += gridDim.x * LOSS_BLOCK) {
        const float *p = a.post + n;                 // p[j * N] = posterior of class j
        // ---- the learning-without-forgetting term: pi = softmax(log p / T) (from the fp32 posteriors), tau = softmax(o / T)
        double amax = 0, alse = 0, omax = 0, olse = 0;
        const bool lwf = a.old_logits != nullptr;
        if (lwf) {
            const double iT = 1.0 / (double)a.T;
            amax = -1e300; omax = -1e300;
            for (int j = 0; j < c; ++j) {
                amax = fmax(amax, loss_logp(p[(long long)j * N]) * iT);
                omax = fmax(omax, (double)a.old_logits[(long long)j * N + n] * iT);
            }
            double as = 0, os = 0;
            for (int j = 0; j < c; ++j) {
                as += exp(loss_logp(p[(long long)j * N]) * iT - amax);
                os += exp((double)a.old_logits[(long long)j * N + n] * iT - omax);
            }
            alse = log(as); olse = log(os);
            double l2 = 0;
            for (int j = 0; j < c; ++j) {
                const double lpi = loss_logp(p[(long long)j * N]) * iT - amax - alse;
                const double tau = exp((double)a.old_logits[(long long)j * N + n] * iT - omax - olse);
                l2 -= tau * lpi;
            }
            s2 += l2;
        }
        // ---- the main objective: per-sample loss, weight, and what the row needs
        int y = -1;
        double mul = 0;        // CE: w * (f - gamma (1 - pt)^(gamma - 1) pt log pt), applied to the fp32 row (p - e_y) s
        double tsum = 0;       // CE_SOFT: sum_k t_k;  GCE: sum_j t_j [in range] p_j^q
        if (a.kind == ALQ_LOSS_CE) {
            y = a.labels[n];
            if (y >= 0 && y < c) {
                const float pt = p[(long long)y * N];
                double w = (a.class_w ? (double)a.class_w[y] : 1.0) * (a.sample_w ? (double)a.sample_w[n] : 1.0);
                double f = 1.0, fac = 1.0;
                const double lp = loss_logp(pt);
                if (a.gamma > 0.f) {
                    const float om = 1.f - pt;               // fp32, like tf.pow(1. - model.pt, gamma)
                    const double g = (double)a.gamma;
                    if (pt == 1.0f) { f = 0.0; fac = 0.0; }
                    else { f = pow((double)om, g); fac = f - g * pow((double)om, g - 1.0) * (double)pt * lp; }
                }
                const double wf = w * f;
                sl -= wf * lp;
                if (wf != 0.0) sc += 1.0;
                mul = w * fac;
            } else {
                y = -1;
            }
        } else if (a.kind == ALQ_LOSS_CE_SOFT) {
            double l = 0;
            for (int j = 0; j < c; ++j) {
                const double t = (double)a.targets[(long long)j * N + n];
                tsum += t;
                l -= t * loss_logp(p[(long long)j * N]);
            }
            sl += l; sc += 1.0;
        } else {
            const double q = (double)a.q;
            double l = 0;
            for (int j = 0; j < c; ++j) {
                const double t = (double)a.targets[(long long)j * N + n];
                const float pj = p[(long long)j * N];
                const float pc = fminf(fmaxf(pj, 1e-4f), 1.f - 1e-4f);
                l += t * (1.0 - pow((double)pc, q)) / q;
                if (pj >= 1e-4f && pj <= 1.f - 1e-4f) tsum += t * pow((double)pj, q);
            }
            sl += l / (double)c; sc += 1.0;
        }
        if (!a.dl) continue;
        for (int j = 0; j < c; ++j) {
            const float pj = p[(long long)j * N];
            float d;
            if (a.kind == ALQ_LOSS_CE) {
                // the row of logit_cotangent_kernel mode 1 in its own fp32 arithmetic, times the weight: with unit weights
                // and no focal term the two kernels write the same bits
                const float base = y >= 0 ? (pj - (j == y ? 1.f : 0.f)) * a.s : 0.f;
                d = (y >= 0 && mul != 1.0) ? (float)((double)base * mul) : base;
            } else if (a.kind == ALQ_LOSS_CE_SOFT) {
                d = (float)((double)a.s * ((double)pj * tsum - (double)a.targets[(long long)j * N + n]));
            } else {
                const double t = (double)a.targets[(long long)j * N + n];
                const double own = (pj >= 1e-4f && pj <= 1.f - 1e-4f) ? t * pow((double)pj, (double)a.q) : 0.0;
                d = (float)(-((double)a.s / (double)c) * (own - (double)pj * tsum));
            }
            if (lwf) {
                const double iT = 1.0 / (double)a.T;
                const double pi = exp(loss_logp(pj) * iT - amax - alse);
                const double tau = exp((double)a.old_logits[(long long)j * N + n] * iT - omax - olse);
                d = (float)((double)d + (double)a.s2 * (pi - tau) * iT);
            }
            a.dl[(long long)n * c + j] = d;
        }
    }
    sh[0][threadIdx.x] = sl; sh[1][threadIdx.x] = sc; sh[2][threadIdx.x] = s2;
    __syncthreads();
    for (int o = LOSS_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
            sh[2][threadIdx.x] += sh[2][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) a.part[blockIdx.x * 3 + threadIdx.x] = sh[threadIdx.x][0];
}

// stats[k] = sum over workgroups, in workgroup order
__global__ void loss_finish_kernel(const double *part, int nblk, double *stats) {
    const int k = threadIdx.x;
    if (k >= 3) return;
    double s = 0;
    for (int b = 0; b < nblk; ++b) s += part[b * 3 + k];
    stats[k] = s;
}

int k_loss_cotangent(alq_ctx *ctx, const float *post_cN, int c, int N, const int *labels, const alq_loss_t *loss, float loss_scale,
                     float lwf_scale, float *dlogits, double *d_stats3) {
    if (!ctx->loss_part) ALQ_HIP(hipMalloc(&ctx->loss_part, (size_t)ALQ_LOSS_MAX_BLOCKS * 3 * sizeof(double)));
    LossArgs a;
    a.post = post_cN; a.labels = labels; a.class_w = loss->d_class_w; a.sample_w = loss->d_sample_w; a.targets = loss->d_targets;
    a.old_logits = loss->d_old_logits; a.c = c; a.N = N; a.kind = loss->kind; a.gamma = loss->focal_gamma; a.q = loss->gce_q;
    a.T = loss->lwf_T; a.s = loss_scale; a.s2 = lwf_scale; a.dl = dlogits; a.part = ctx->loss_part;
    const int nblk = std::min(ALQ_LOSS_MAX_BLOCKS, (N + LOSS_BLOCK - 1) / LOSS_BLOCK);
    {
        ProfScope ps(ctx, PROF_ELEMWISE, 0);
        hipLaunchKernelGGL(loss_cotangent_kernel, dim3(nblk), dim3(LOSS_BLOCK), 0, ctx->stream, a);
        ALQ_LAUNCH_CHECK();
    }
    if (d_stats3) {
        ProfScope ps(ctx, PROF_REDUCE, 0);
        hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->loss_part, nblk, d_stats3);
        ALQ_LAUNCH_CHECK();
    }
    return ALQ_OK;
}

// ------------------------------------------------------------------------------------------ RMSProp
// tf.train.RMSPropOptimizer, not centred: ms = decay ms + (1 - decay) g^2; mom = momentum mom + lr g / sqrt(ms + eps);
// theta -= mom.  16-byte loads and stores over the aligned body, a scalar tail.
__device__ inline void rmsprop_one(float &th, float g, float &ms, float &mom, float lr, float decay, float momentum, float eps) {
    ms = decay * ms + (1.f - decay) * g * g;
    mom = momentum * mom + lr * g / sqrtf(ms + eps);
    th -= mom;
}

__global__ void rmsprop_step_kernel(float *theta, const float *g, float *ms, float *mom, long long n, long long n4, float lr,
                                    float decay, float momentum, float eps) {
    const long long stride = (long long)gridDim.x * blockDim.x, i0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    float4 *t4 = reinterpret_cast<float4 *>(theta), *s4 = reinterpret_cast<float4 *>(ms), *m4 = reinterpret_cast<float4 *>(mom);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    for (long long i = i0; i < n4; i += stride) {
        float4 t = t4[i], s = s4[i], m = m4[i];
        const float4 gg = g4[i];
        rmsprop_one(t.x, gg.x, s.x, m.x, lr, decay, momentum, eps);
        rmsprop_one(t.y, gg.y, s.y, m.y, lr, decay, momentum, eps);
        rmsprop_one(t.z, gg.z, s.z, m.z, lr, decay, momentum, eps);
        rmsprop_one(t.w, gg.w, s.w, m.w, lr, decay, momentum, eps);
        s4[i] = s; m4[i] = m; t4[i] = t;
    }
    for (long long i = 4 * n4 + i0; i < n; i += stride) rmsprop_one(theta[i], g[i], ms[i], mom[i], lr, decay, momentum, eps);
}

int k_rmsprop(alq_ctx *ctx, float *theta, const float *g, float *ms, float *mom, long long n, float lr, float decay, float momentum,
              float eps) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(ms) |
                           reinterpret_cast<uintptr_t>(mom);
    const long long n4 = (bits & 15) ? 0 : n / 4;          // a vector that does not start on 16 bytes takes the scalar loop
    long long blocks = ((n4 ? n4 : n) + 255) / 256;
    blocks = std::max(1LL, std::min(blocks, 65535LL * 16));
    hipLaunchKernelGGL(rmsprop_step_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, theta, g, ms, mom, n, n4, lr, decay,
                       momentum, eps);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

}  // namespace alq
