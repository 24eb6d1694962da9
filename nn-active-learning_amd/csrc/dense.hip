// The 1x1 conv head of a fully-convolutional ("dense") model: per voxel z = b + x W, softmax over c <= 8 classes.
//   * dense_head_fwd_kernel: x [R, Ci] (R = N * V voxels, channels last) -> posteriors as class-major planes [c, R], optionally
//     the first maximal class [R] (int64) and the logits [R, c].  A lane owns 4 consecutive voxels: x comes in as 16-byte
//     pieces, every plane goes out as 16-byte stores; W / b sit in LDS, read as broadcasts.  Voxels past the last whole group
//     of 4 - or all of them when the planes cannot be stored 16 bytes at a time (R % 4 != 0 or an unaligned buffer: plane j
//     starts at float j R) - take the guarded one-voxel path.
//   * dense_head_fwd_au_kernel: the same body for a head of c + 1 channels whose last one is a log-variance (AU_4U,
//     NN_extended.py:265-288): softmax and first maximum over the first c accumulators, au [R] = max(z_c, 0) as one more plane,
//     logits [R, c + 1].  Every channel keeps its own chain of fused multiply-adds: the posterior planes carry the bits
//     dense_head_fwd_kernel writes for W[:, :c], b[:c].
//   * dense_head_bwd_kernel: one pass over delta [R, c] and x [R, Ci]: dX = delta W^T (16-byte stores, optionally added to
//     what a skip consumer wrote) and per-workgroup partials of dW = x^T delta, db = sum delta.  A lane owns one 4-channel
//     piece of a row (consecutive lanes = consecutive 16-byte pieces of x and dX); it takes 4 rows per trip (their loads issued together), sums 64 of its rows in fp32, folds
//     those into fp64, and the workgroup folds its lanes in a fixed fp64 tree.
//   * dense_head_reduce_kernel: the partials into the flat gradient vector, one workgroup per element, a fixed order of additions.
// Streaming kernels: nothing is read or written twice but the c floats of a cotangent row.  No atomics, the launch geometry
// depends on the sizes alone: bit-identical from run to run.  Not on the scoring path of fc-head models.
#include <algorithm>
#include <cstdint>

#include "alq_internal.h"

namespace alq {

#define ALQ_LAUNCH_CHECK() ALQ_HIP(hipGetLastError())

constexpr int DENSE_BLOCK = 256;
constexpr int DENSE_MAX_CI = 64, DENSE_MAX_C = 8;
constexpr int DENSE_FLUSH = 64;      // rows a lane sums in fp32 before they go into its fp64 sums

struct DenseFwdArgs {
    const float *x;      // [R, Ci]
    const float *W;      // [Ci, c]
    const float *b;      // [c]
    float *post;         // [c, R]
    long long *pred;     // [R] or null
    float *z;            // [R, c] (aleatoric: [R, c + 1]) or null
    float *au;           // aleatoric: [R] or null
    long long R, groups; // groups of 4 voxels on the 16-byte path
    int Ci;
};

// softmax and first maximum over the first C of the CT logits of a voxel
template <int C, int CT>
__device__ inline void dense_softmax(const float (&zv)[CT], float (&p)[C], int *best) {
    float mx = zv[0];
#pragma unroll
    for (int j = 1; j < C; ++j) mx = fmaxf(mx, zv[j]);
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) { p[j] = expf(zv[j] - mx); den += p[j]; }
    int bj = 0;
    float bp = -1.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        p[j] = p[j] / den;
        if (p[j] > bp) { bp = p[j]; bj = j; }      // first maximum, like tf.argmax
    }
    *best = bj;
}

// AU = 1: one accumulator more a voxel, the log-variance channel; W [Ci, CT], b [CT]
template <int C, int AU>
__device__ __forceinline__ void dense_head_fwd_body(const DenseFwdArgs &a) {
    constexpr int CT = C + AU;
    __shared__ float sW[DENSE_MAX_CI * CT + CT];
    const int Ci = a.Ci, nq = Ci / 4;
    for (int i = threadIdx.x; i < Ci * CT + CT; i += DENSE_BLOCK) sW[i] = i < Ci * CT ? a.W[i] : a.b[i - Ci * CT];
    __syncthreads();
    const float *sb = sW + Ci * CT;
    const long long R = a.R, stride = (long long)gridDim.x * DENSE_BLOCK, t0 = blockIdx.x * (long long)DENSE_BLOCK + threadIdx.x;
    const float4 *x4 = reinterpret_cast<const float4 *>(a.x);
    for (long long g = t0; g < a.groups; g += stride) {
        const long long r0 = 4 * g;
        float acc[4][CT];
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int j = 0; j < CT; ++j) acc[v][j] = sb[j];
        for (int q = 0; q < nq; ++q) {
            float4 xv[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) xv[v] = x4[(r0 + v) * nq + q];
            const float *w = sW + 4 * q * CT;
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                const float w0 = w[j], w1 = w[CT + j], w2 = w[2 * CT + j], w3 = w[3 * CT + j];
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    acc[v][j] = fmaf(xv[v].w, w3, fmaf(xv[v].z, w2, fmaf(xv[v].y, w1, fmaf(xv[v].x, w0, acc[v][j]))));
            }
        }
        float p[4][C];
        int best[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) dense_softmax<C, CT>(acc[v], p[v], &best[v]);
#pragma unroll
        for (int j = 0; j < C; ++j)
            *reinterpret_cast<float4 *>(a.post + (long long)j * R + r0) = make_float4(p[0][j], p[1][j], p[2][j], p[3][j]);
        if constexpr (AU != 0)
            if (a.au)
                *reinterpret_cast<float4 *>(a.au + r0) = make_float4(fmaxf(acc[0][C], 0.f), fmaxf(acc[1][C], 0.f), fmaxf(acc[2][C], 0.f),
                                                                     fmaxf(acc[3][C], 0.f));
        if (a.pred) {
            longlong2 *pp = reinterpret_cast<longlong2 *>(a.pred + r0);
            pp[0] = make_longlong2(best[0], best[1]);
            pp[1] = make_longlong2(best[2], best[3]);
        }
        if (a.z) {
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int j = 0; j < CT; ++j) a.z[(r0 + v) * CT + j] = acc[v][j];
        }
    }
    // the voxels the groups do not cover, one per lane
    for (long long r = 4 * a.groups + t0; r < R; r += stride) {
        float zv[CT], p[C];
#pragma unroll
        for (int j = 0; j < CT; ++j) zv[j] = sb[j];
        for (int q = 0; q < nq; ++q) {
            const float4 xv = x4[r * nq + q];
            const float *w = sW + 4 * q * CT;
#pragma unroll
            for (int j = 0; j < CT; ++j)
                zv[j] = fmaf(xv.w, w[3 * CT + j], fmaf(xv.z, w[2 * CT + j], fmaf(xv.y, w[CT + j], fmaf(xv.x, w[j], zv[j]))));
        }
        int best;
        dense_softmax<C, CT>(zv, p, &best);
#pragma unroll
        for (int j = 0; j < C; ++j) a.post[(long long)j * R + r] = p[j];
        if constexpr (AU != 0)
            if (a.au) a.au[r] = fmaxf(zv[C], 0.f);
        if (a.pred) a.pred[r] = best;
        if (a.z) {
#pragma unroll
            for (int j = 0; j < CT; ++j) a.z[r * CT + j] = zv[j];
        }
    }
}

template <int C>
__global__ __launch_bounds__(DENSE_BLOCK) void dense_head_fwd_kernel(DenseFwdArgs a) { dense_head_fwd_body<C, 0>(a); }

template <int C>
__global__ __launch_bounds__(DENSE_BLOCK) void dense_head_fwd_au_kernel(DenseFwdArgs a) { dense_head_fwd_body<C, 1>(a); }

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#define DENSE_DISPATCH(c, CALL)                                                  \
    switch (c) {                                                                 \
        case 2: CALL(2); break;                                                  \
        case 3: CALL(3); break;                                                  \
        case 4: CALL(4); break;                                                  \
        case 5: CALL(5); break;                                                  \
        case 6: CALL(6); break;                                                  \
        case 7: CALL(7); break;                                                  \
        default: CALL(8); break;                                                 \
    }

static int dense_check(const char *who, const float *x, long long R, int Ci, int c) {
    ALQ_REQUIRE(x && R >= 1, ALQ_EINVAL, "%s: null input or no voxels", who);
    ALQ_REQUIRE(Ci >= 4 && Ci <= DENSE_MAX_CI && Ci % 4 == 0, ALQ_EUNSUPPORTED, "%s: %d input channels (a multiple of 4, at most %d)", who, Ci,
                DENSE_MAX_CI);
    ALQ_REQUIRE(c >= 2 && c <= DENSE_MAX_C, ALQ_EUNSUPPORTED, "%s: %d classes (2 .. %d)", who, c, DENSE_MAX_C);
    ALQ_REQUIRE(R * std::max(Ci, c) < (1LL << 31), ALQ_EUNSUPPORTED, "%s: %lld voxels x %d channels pass 32-bit offsets", who, R, std::max(Ci, c));
    ALQ_REQUIRE(aligned16(x), ALQ_EINVAL, "%s: the input is not 16-byte aligned", who);
    return ALQ_OK;
}

// au_head: W [Ci, c + 1], b [c + 1], the log-variance channel behind the c classes (c <= 7): au [R] or null, z [R, c + 1] or null
static int dense_fwd_launch(alq_ctx *ctx, bool au_head, const float *x, long long R, int Ci, int c, const float *W, const float *b,
                            float *post_cR, int64_t *pred, float *au, float *z) {
    const char *who = au_head ? "dense_head_fwd_au" : "dense_head_fwd";
    ALQ_TRY(dense_check(who, x, R, Ci, c + (au_head ? 1 : 0)));
    ALQ_REQUIRE(!au_head || c >= 2, ALQ_EUNSUPPORTED, "%s: %d classes beside the log-variance channel (2 .. %d)", who, c, DENSE_MAX_C - 1);
    ALQ_REQUIRE(W && b && post_cR, ALQ_EINVAL, "%s: null argument", who);
    DenseFwdArgs a;
    a.x = x; a.W = W; a.b = b; a.post = post_cR; a.pred = reinterpret_cast<long long *>(pred); a.z = z; a.au = au; a.R = R; a.Ci = Ci;
    const bool vec = R % 4 == 0 && aligned16(post_cR) && (!pred || aligned16(pred)) && aligned16(au);
    a.groups = vec ? R / 4 : 0;
    const long long lanes = std::max(a.groups, R - 4 * a.groups);
    const unsigned nblk = (unsigned)std::max(1LL, std::min((lanes + DENSE_BLOCK - 1) / DENSE_BLOCK, 65535LL * 16));
    ProfScope ps(ctx, PROF_ELEMWISE, 2.0 * R * Ci * (c + (au_head ? 1 : 0)));
    if (au_head) {
#define CALL(CC) hipLaunchKernelGGL(dense_head_fwd_au_kernel<CC>, dim3(nblk), dim3(DENSE_BLOCK), 0, ctx->stream, a)
        switch (c) {
            case 2: CALL(2); break;
            case 3: CALL(3); break;
            case 4: CALL(4); break;
            case 5: CALL(5); break;
            case 6: CALL(6); break;
            default: CALL(7); break;
        }
#undef CALL
    } else {
#define CALL(CC) hipLaunchKernelGGL(dense_head_fwd_kernel<CC>, dim3(nblk), dim3(DENSE_BLOCK), 0, ctx->stream, a)
        DENSE_DISPATCH(c, CALL)
#undef CALL
    }
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

int k_dense_head_fwd(alq_ctx *ctx, const float *x, long long R, int Ci, int c, const float *W, const float *b, float *post_cR,
                     int64_t *pred, float *z) {
    return dense_fwd_launch(ctx, false, x, R, Ci, c, W, b, post_cR, pred, nullptr, z);
}

int k_dense_head_fwd_au(alq_ctx *ctx, const float *x, long long R, int Ci, int c, const float *W, const float *b, float *post_cR,
                        int64_t *pred, float *au, float *z) {
    return dense_fwd_launch(ctx, true, x, R, Ci, c, W, b, post_cR, pred, au, z);
}

// ------------------------------------------------------------------------------------------ backward
struct DenseBwdArgs {
    const float *delta;  // [R, c]
    const float *x;      // [R, Ci]
    const float *W;      // [Ci, c]
    float *dx;           // [R, Ci] or null
    double *part;        // [gridDim.x][Ci * c + c]
    long long R, per;    // rows per workgroup
    int Ci, accumulate;
};

template <int C>
__global__ __launch_bounds__(DENSE_BLOCK) void dense_head_bwd_kernel(DenseBwdArgs a) {
    constexpr int NV = 5 * C;      // a lane's sums: 4 channels x C classes of dW, C of db
    constexpr int KB = 8;          // sums folded per round of the workgroup tree
    __shared__ double sh[KB][DENSE_BLOCK];
    const int Ci = a.Ci, nq = Ci / 4;
    const int rpi = DENSE_BLOCK / nq;                 // rows per sweep of the workgroup; lanes >= rpi * nq idle
    const int tid = threadIdx.x;
    const bool active = tid < rpi * nq;
    const int q = tid % nq, rl = tid / nq;
    float w[4][C];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < C; ++j) w[k][j] = a.W[(4 * q + k) * C + j];
    double sum[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) sum[v] = 0.0;
    const long long rb = blockIdx.x * a.per, re = std::min(a.R, rb + a.per);
    const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(a.x);
    float4 *__restrict__ dx4 = reinterpret_cast<float4 *>(a.dx);
    // U rows of the lane per trip: their loads are issued together, ahead of the arithmetic and the stores of the trip
    constexpr int U = 4;
    const float *__restrict__ dl = a.delta;
    long long r = rb + rl;
    while (active && r < re) {
        float acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = 0.f;
        for (int it = 0; it < DENSE_FLUSH && r < re; it += U, r += (long long)U * rpi) {
            float d[U][C];
            float4 xv[U], old[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long rr = r + (long long)u * rpi;
                const bool ok = rr < re;
                const long long rc = ok ? rr : r;          // (a row past the end: the trip's first row again, weight 0)
                xv[u] = x4[rc * nq + q];
#pragma unroll
                for (int j = 0; j < C; ++j) d[u][j] = ok ? dl[rc * C + j] : 0.f;
                if (dx4 && a.accumulate) old[u] = dx4[rc * nq + q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long rr = r + (long long)u * rpi;
                if (dx4 && rr < re) {
                    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int j = 0; j < C; ++j) {
                        o.x = fmaf(d[u][j], w[0][j], o.x); o.y = fmaf(d[u][j], w[1][j], o.y);
                        o.z = fmaf(d[u][j], w[2][j], o.z); o.w = fmaf(d[u][j], w[3][j], o.w);
                    }
                    if (a.accumulate) { o.x += old[u].x; o.y += old[u].y; o.z += old[u].z; o.w += old[u].w; }
                    dx4[rr * nq + q] = o;
                }
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    acc[j] = fmaf(xv[u].x, d[u][j], acc[j]);
                    acc[C + j] = fmaf(xv[u].y, d[u][j], acc[C + j]);
                    acc[2 * C + j] = fmaf(xv[u].z, d[u][j], acc[2 * C + j]);
                    acc[3 * C + j] = fmaf(xv[u].w, d[u][j], acc[3 * C + j]);
                    acc[4 * C + j] += d[u][j];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) sum[v] += (double)acc[v];
    }
    // lanes of one 4-channel piece q sit at tid = rl * nq + q: a fixed tree over rl, KB sums per round
    int top = 1;
    while (top < rpi) top <<= 1;
    double *out = a.part + (long long)blockIdx.x * (Ci * C + C);
#pragma unroll
    for (int v0 = 0; v0 < NV; v0 += KB) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (v0 + k < NV) sh[k][tid] = active ? sum[v0 + k] : 0.0;
        __syncthreads();
        for (int o = top >> 1; o > 0; o >>= 1) {
            if (active && rl < o && rl + o < rpi) {
#pragma unroll
                for (int k = 0; k < KB; ++k)
                    if (v0 + k < NV) sh[k][tid] += sh[k][tid + o * nq];
            }
            __syncthreads();
        }
        if (tid < nq) {      // rl = 0, q = tid
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const int v = v0 + k;
                if (v >= NV) continue;
                if (v < 4 * C) out[(4 * q + v / C) * C + v % C] = sh[k][tid];
                else if (q == 0) out[Ci * C + (v - 4 * C)] = sh[k][tid];
            }
        }
        __syncthreads();
    }
}

// out[e] = sum of the workgroups' partials, one workgroup per element: lane t adds partials t, t + 256, ... in that order, the
// lanes fold in a fixed tree.  e < Ci c: the weights [Ci][c] (the TF layout of a 1x1 filter), then the bias.
// (One lane per element walking all partials is a chain of dependent loads: 2048 partials took ~500 us.)
__global__ __launch_bounds__(DENSE_BLOCK) void dense_head_reduce_kernel(const double *part, int nblk, int len, float *out) {
    __shared__ double sh[DENSE_BLOCK];
    const int e = blockIdx.x;
    double s = 0;
    for (int b = threadIdx.x; b < nblk; b += DENSE_BLOCK) s += part[(long long)b * len + e];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = DENSE_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[e] = (float)sh[0];
}

// Workgroups of a backward launch over R rows: enough rows each to amortise the closing tree, never more than the partials hold
static int dense_head_bwd_rpi(int Ci) { return DENSE_BLOCK / (Ci / 4); }      // the kernel's `rpi`

int dense_head_bwd_blocks(long long R, int Ci) {
    const int rpi = dense_head_bwd_rpi(Ci);
    const long long want = (R + (long long)rpi * 8 - 1) / ((long long)rpi * 8);
    return (int)std::max(1LL, std::min(want, (long long)ALQ_DENSE_MAX_BLOCKS));
}

// Rows per workgroup of that launch (the kernel's `per`)
static long long dense_head_bwd_rows(long long R, int nblk) { return (R + nblk - 1) / nblk; }

int k_dense_head_bwd(alq_ctx *ctx, const float *delta, const float *x, long long R, int Ci, int c, const float *W, float *dx,
                     int accumulate, double *part, float *d_dW_db) {
    ALQ_TRY(dense_check("dense_head_bwd", x, R, Ci, c));
    ALQ_REQUIRE(delta && W && part && d_dW_db, ALQ_EINVAL, "dense_head_bwd: null argument");
    ALQ_REQUIRE(!dx || aligned16(dx), ALQ_EINVAL, "dense_head_bwd: the input cotangent is not 16-byte aligned");
    DenseBwdArgs a;
    a.delta = delta; a.x = x; a.W = W; a.dx = dx; a.part = part; a.R = R; a.Ci = Ci; a.accumulate = accumulate;
    const int nblk = dense_head_bwd_blocks(R, Ci);
    a.per = dense_head_bwd_rows(R, nblk);
    {
        ProfScope ps(ctx, PROF_ELEMWISE, 4.0 * R * Ci * c);
#define CALL(CC) hipLaunchKernelGGL(dense_head_bwd_kernel<CC>, dim3((unsigned)nblk), dim3(DENSE_BLOCK), 0, ctx->stream, a)
        DENSE_DISPATCH(c, CALL)
#undef CALL
        ALQ_LAUNCH_CHECK();
    }
    const int len = Ci * c + c;
    ProfScope ps(ctx, PROF_REDUCE, 0);
    hipLaunchKernelGGL(dense_head_reduce_kernel, dim3((unsigned)len), dim3(DENSE_BLOCK), 0, ctx->stream, part, nblk, len, d_dW_db);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

}  // namespace alq

// ---- the kernels on their own (model-free, like alq_loss_stats): kernel-level checks and timing
extern "C" {

size_t alq_dense_head_work_bytes(int Ci, int c) {
    return (Ci > 0 && c > 0) ? (size_t)ALQ_DENSE_MAX_BLOCKS * ((size_t)Ci * c + c) * sizeof(double) : 0;
}

int alq_dense_head_bwd_geometry(int64_t R, int Ci, int *blocks, int64_t *rows_per_block, int *rows_per_sweep, int *flush_rows) {
    ALQ_REQUIRE(blocks && rows_per_block && rows_per_sweep && flush_rows && R >= 1, ALQ_EINVAL,
                "alq_dense_head_bwd_geometry: null argument or no voxels");
    ALQ_REQUIRE(Ci >= 4 && Ci <= alq::DENSE_MAX_CI && Ci % 4 == 0, ALQ_EUNSUPPORTED,
                "alq_dense_head_bwd_geometry: %d input channels (a multiple of 4, at most %d)", Ci, alq::DENSE_MAX_CI);
    *blocks = alq::dense_head_bwd_blocks(R, Ci);
    *rows_per_block = alq::dense_head_bwd_rows(R, *blocks);
    *rows_per_sweep = alq::dense_head_bwd_rpi(Ci);
    *flush_rows = alq::DENSE_FLUSH;
    return ALQ_OK;
}

int alq_dense_head_fwd(alq_ctx *ctx, const float *d_x, int64_t R, int Ci, int c, const float *d_W, const float *d_b, float *d_post,
                       int64_t *d_pred) {
    ALQ_REQUIRE(ctx, ALQ_EINVAL, "alq_dense_head_fwd: null context");
    ALQ_HIP(hipSetDevice(ctx->device));
    return alq::k_dense_head_fwd(ctx, d_x, R, Ci, c, d_W, d_b, d_post, d_pred, nullptr);
}

int alq_dense_head_fwd_au(alq_ctx *ctx, const float *d_x, int64_t R, int Ci, int c, const float *d_W, const float *d_b, float *d_post,
                          int64_t *d_pred, float *d_au, float *d_logits) {
    ALQ_REQUIRE(ctx && d_au, ALQ_EINVAL, "alq_dense_head_fwd_au: null context or log-variance plane");
    ALQ_HIP(hipSetDevice(ctx->device));
    return alq::k_dense_head_fwd_au(ctx, d_x, R, Ci, c, d_W, d_b, d_post, d_pred, d_au, d_logits);
}

int alq_dense_head_bwd(alq_ctx *ctx, const float *d_delta, const float *d_x, int64_t R, int Ci, int c, const float *d_W, float *d_dx,
                       void *d_work, float *d_dW_db) {
    ALQ_REQUIRE(ctx, ALQ_EINVAL, "alq_dense_head_bwd: null context");
    ALQ_HIP(hipSetDevice(ctx->device));
    return alq::k_dense_head_bwd(ctx, d_delta, d_x, R, Ci, c, d_W, d_dx, 0, static_cast<double *>(d_work), d_dW_db);
}

}  // extern "C"
