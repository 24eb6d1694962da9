// Diagonal Fisher without per-sample gradient rows (alq_diag_fisher; model_utils.diagonal_Fisher, model_utils.py:294-330) and
// the masks of partial fine-tuning built from it (alq_topk_mask / alq_threshold_mask; model_utils.keep_k_largest_from_LoV,
// threshold_LoV, model_utils.py:54-96).
//   acc[i] += sum_n (d log posteriors[cls_n, n] / d theta_i)^2 from the tensors a general backward pass left behind:
//   * conv / conv_transpose weights: the per-sample gradient G[tap][v][u] = sum_q U[q, u] V[s q + tap - lo, v] is the sweep
//     of gnorm.hip (gnorm_sweep.h: 16 x 16 tiles on v_mfma_f32_16x16x4_f32, in registers for the whole voxel sweep of a
//     sample, boxes folded in two fp32 levels).  Where the norm kernel sums the squares of a sample's tile, this one keeps
//     them apart: after a sample's sweep every entry is squared in fp64 and added to an fp64 accumulator of its own, the
//     workgroup goes on to its next sample, and after the last one the accumulators go to the entry's position in the TF
//     layout ([tap][v][u]: conv [tap][ci][co], conv_transpose [tap][co][ci]).  The mirrored form of a narrow stride-1 conv
//     has the tile's rows and columns the other way round (rows (tap, u), columns v); the store maps them back.
//     Work is split over (column tile, row-tile group) and over groups of consecutive samples, never over the voxels of a
//     sample; the sample groups write partials that dfisher_fold_kernel adds in group order.
//   * conv biases: (sum_q U[q, c])^2 from fp64 channel sums, summed over the samples in order.
//   * fc: acc[o][f] += sum_n delta[n, o]^2 a[n, f]^2 and acc_b[o] += sum_n delta[n, o]^2, squares, products and sums in
//     fp64, samples in ascending order; a thread owns one input feature f (in the reference's flatten order) and a block of
//     outputs, so the stream of |W| doubles is read and written once per call in rows contiguous in f (the much smaller
//     input is gathered with a stride and re-read per output block, out of L2: see dfisher_fcw_kernel).
//   No atomics on any floating-point value and no buffer of N x P: every sum has a fixed order, so a call is bit-identical
//   from run to run.
//   * masks: a radix select on the order-preserving bit patterns of the doubles (8 passes of 8 bits; per-workgroup
//     histograms, integer counts) finds the k-th largest value and how many entries equal to it are still to be taken; one
//     ordered pass then hands those out by ascending index.  Nothing is sorted.
#include <algorithm>

#include "alq_internal.h"
#include "gnorm_sweep.h"

namespace alq {

using namespace gn;

namespace {

constexpr int DF_TARGET_WG = 1024;        // workgroups a weight launch aims for before it stops splitting the samples
constexpr int DF_OB = 16;                 // outputs per thread of the fc kernel

// grid (NT * groups, sample groups); sample group sgi sweeps the samples [sgi * per, min(N, (sgi + 1) * per)) in order and
// writes part[sgi * Pl + TF position] = sum over its samples of G^2
template <int TPW>
__global__ __launch_bounds__(GN_THREADS) void dfisher_w_kernel(GnView X, GnView Y, GnGeom g, int N, int per, int mirror,
                                                               double *part, long long Pl) {
    const int ct = blockIdx.x / g.groups, rg = blockIdx.x - ct * g.groups;
    const int sgi = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int toff[TPW];
    const int ntile = gn_tile_rows<TPW>(g, rg, toff);
    double dacc[TPW][4];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) dacc[j][r] = 0.0;
    const int n1 = min(N, (sgi + 1) * per);
    for (int n = sgi * per; n < n1; ++n) {
        gn_f32x4 tot[TPW];
        gn_sweep_sample<TPW>(X, Y, g, n, ct * 16, toff, ntile, tot);
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const double v = (double)tot[j][r]; dacc[j][r] += v * v; }
    }
    // C/D layout: register r of lane l = tile row 4 * (l >> 4) + r, tile column l & 15
    const int rows = g.T * g.Cb;
    const int a = ct * 16 + (lane & 15);
    double *dst = part + (long long)sgi * Pl;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int rt = rg * (GN_WAVES * TPW) + w + GN_WAVES * j;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = rt * 16 + 4 * (lane >> 4) + r;
            if (rt < g.MT && m < rows && a < g.Ca) {
                long long pos;
                if (mirror) {                 // rows (tap, u), columns v  ->  [tap][v][u]
                    const int tap = m / g.Cb, u = m - tap * g.Cb;
                    pos = ((long long)tap * g.Ca + a) * g.Cb + u;
                } else {                      // rows (tap, v), columns u  ->  [tap][v][u]
                    pos = (long long)m * g.Ca + a;
                }
                dst[pos] = dacc[j][r];
            }
        }
    }
}

// acc[i] += sum_g part[g * Pl + i], in g order
__global__ void dfisher_fold_kernel(const double *part, int G, long long Pl, double *acc) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= Pl) return;
    double s = 0.0;
    for (int gi = 0; gi < G; ++gi) s += part[(long long)gi * Pl + i];
    acc[i] += s;
}

// channel sums of a conv cotangent: cs[n * C + c] = sum_x D[n, x, c], fp64; one workgroup per sample (the summation order
// of gnorm.hip's bias kernel: thread t sums channel t % C over the rows t / C, t / C + R, ..., the R partials fold in order)
__global__ __launch_bounds__(256) void dfisher_chansum_kernel(GnView D, long long vox, int C, double *cs) {
    __shared__ double sh[256];
    const int n = blockIdx.x;
    const int R = 256 / C;
    const int t = threadIdx.x;
    double s = 0.0;
    if (t < R * C) {
        const int c = t % C;
        for (long long r = t / C; r < vox; r += R) s += (double)D.at((long long)n * vox + r, c);
    }
    sh[t] = s;
    __syncthreads();
    if (t < C) {
        double tot = 0.0;
        for (int i = 0; i < R; ++i) tot += sh[i * C + t];
        cs[(long long)n * C + t] = tot;
    }
}

// acc[c] += sum_n cs[n * C + c]^2, n ascending
__global__ void dfisher_bias_fold_kernel(const double *cs, int N, int C, double *acc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int n = 0; n < N; ++n) { const double v = cs[(long long)n * C + c]; s += v * v; }
    acc[c] += s;
}

// fc bias: d2[n * nout + o] = delta[n, o]^2 (kept for the weight kernel), acc_b[o] += sum_n d2[n, o]
__global__ void dfisher_fcb_kernel(const float *delta, int nout, int N, double *d2, double *acc_b) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nout) return;
    double s = 0.0;
    for (int n = 0; n < N; ++n) {
        const double v = (double)delta[(long long)n * nout + o];
        const double q = v * v;
        d2[(long long)n * nout + o] = q;
        s += q;
    }
    acc_b[o] += s;
}

// fc weights: grid (ceil(F / 256), ceil(nout / DF_OB)); thread = one f_tf = ((c * W + w) * H + h) * D + d and DF_OB outputs.
// The d2 reads are uniform over the workgroup; rows of acc are contiguous in f_tf, and acc is the only stream read and written
// once.  The input a is NOT: f_tf runs fastest in d while memory runs slowest in it, so neighbouring lanes read a H * W * cs
// floats apart (contiguous only behind another fc layer), and every one of the nout / DF_OB output blocks reads a sample's
// features again.  a is N * F floats (1.6 MB at 64 samples of NET-B's fc1) and stays in L2; staging it through LDS in memory
// order would be the next step if this kernel came to set the time.
__global__ __launch_bounds__(256) void dfisher_fcw_kernel(const double *__restrict__ d2, GnView A, int D, int H, int W, int C,
                                                          int nout, int N, double *__restrict__ acc) {
    const long long vox = (long long)D * H * W, F = vox * C;
    const long long f = blockIdx.x * 256LL + threadIdx.x;
    const int o0 = blockIdx.y * DF_OB;
    if (f >= F) return;
    long long ft = f;
    const int d = (int)(ft % D); ft /= D;
    const int h = (int)(ft % H); ft /= H;
    const int w = (int)(ft % W); ft /= W;
    const int c = (int)ft;
    const long long vrow = ((long long)d * H + h) * W + w;
    double s[DF_OB];
#pragma unroll
    for (int j = 0; j < DF_OB; ++j) s[j] = 0.0;
    for (int n = 0; n < N; ++n) {
        const double av = (double)A.at((long long)n * vox + vrow, c);
        const double a2 = av * av;
        const double *dn = d2 + (long long)n * nout + o0;
#pragma unroll
        for (int j = 0; j < DF_OB; ++j)
            if (o0 + j < nout) s[j] += dn[j] * a2;
    }
#pragma unroll
    for (int j = 0; j < DF_OB; ++j)
        if (o0 + j < nout) acc[(long long)(o0 + j) * F + f] += s[j];
}

int df_tpw(int MT) { return std::min(gn_tpw(MT), 8); }      // 8 tiles: 32 fp64 accumulators per lane beside the fp32 ones

struct DfPlan {
    GnGeom g;
    bool mirror;
    int tpw, G;
    long long Pl;
};
DfPlan df_plan(const View &U, const View &V, const int k[3], const int s[3], const int lo[3]) {
    DfPlan p;
    p.g = make_geom(U, V, k, s, lo, &p.mirror);
    p.tpw = df_tpw(p.g.MT);
    p.g.groups = (p.g.MT + GN_WAVES * p.tpw - 1) / (GN_WAVES * p.tpw);
    p.G = p.g.NT * p.g.groups;
    p.Pl = (long long)p.g.T * U.C * V.C;
    return p;
}
int df_sample_groups_max(int G) { return std::max(1, (DF_TARGET_WG + G - 1) / G); }

}  // namespace

long long dfisher_weight_scratch(const View &U, const View &V, const int k[3], const int s[3], const int lo[3], int max_batch) {
    const DfPlan p = df_plan(U, V, k, s, lo);
    return (long long)std::min(max_batch, df_sample_groups_max(p.G)) * p.Pl;
}

int k_dfisher_weight(alq_ctx *ctx, const View &U, const View &V, const int k[3], const int s[3], const int lo[3], int N,
                     double *scratch, double *d_acc) {
    const DfPlan p = df_plan(U, V, k, s, lo);
    ALQ_REQUIRE((long long)p.g.halo_fl <= GN_HALO_MAX, ALQ_EUNSUPPORTED,
                "alq_diag_fisher: %d channels x %d taps do not fit the staged halo", p.g.Cb, p.g.T);
    const int per = (N + std::min(N, df_sample_groups_max(p.G)) - 1) / std::min(N, df_sample_groups_max(p.G));
    const int SG = (N + per - 1) / per;
    const View &X = p.mirror ? V : U, &Y = p.mirror ? U : V;
    const GnView gx = gview(X), gy = gview(Y);
    const size_t lds = gnorm_dyn_lds_bytes(p.g);
    {
        ProfScope ps(ctx, PROF_GNORM, 2.0 * (double)N * X.vox() * p.g.T * p.g.Cb * p.g.Ca);
        dim3 grid((unsigned)p.G, (unsigned)SG);
#define ALQ_DF(TP)                                                                                                          \
    hipLaunchKernelGGL(dfisher_w_kernel<TP>, grid, dim3(GN_THREADS), lds, ctx->stream, gx, gy, p.g, N, per, p.mirror ? 1 : 0, \
                       scratch, p.Pl)
        switch (p.tpw) {
            case 1: ALQ_DF(1); break;
            case 2: ALQ_DF(2); break;
            case 4: ALQ_DF(4); break;
            default: ALQ_DF(8); break;
        }
#undef ALQ_DF
        ALQ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(dfisher_fold_kernel, dim3((unsigned)((p.Pl + 255) / 256)), dim3(256), 0, ctx->stream, scratch, SG, p.Pl, d_acc);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int k_dfisher_bias(alq_ctx *ctx, const View &delta, int N, double *scratch /*[N * C]*/, double *d_acc) {
    ALQ_REQUIRE(delta.C >= 1 && delta.C <= 256, ALQ_EUNSUPPORTED, "alq_diag_fisher: bias of %d channels", delta.C);
    hipLaunchKernelGGL(dfisher_chansum_kernel, dim3((unsigned)N), dim3(256), 0, ctx->stream, gview(delta), (long long)delta.vox(),
                       delta.C, scratch);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(dfisher_bias_fold_kernel, dim3((delta.C + 255) / 256), dim3(256), 0, ctx->stream, scratch, N, delta.C, d_acc);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int k_dfisher_fc(alq_ctx *ctx, const float *delta, int nout, const View &a, int N, double *scratch /*[N * nout]*/, double *d_acc_w,
                 double *d_acc_b) {
    hipLaunchKernelGGL(dfisher_fcb_kernel, dim3((nout + 255) / 256), dim3(256), 0, ctx->stream, delta, nout, N, scratch, d_acc_b);
    ALQ_HIP(hipGetLastError());
    const long long F = (long long)a.vox() * a.C;
    ProfScope ps(ctx, PROF_REDUCE, 2.0 * (double)N * F * nout);
    dim3 grid((unsigned)((F + 255) / 256), (unsigned)((nout + DF_OB - 1) / DF_OB));
    hipLaunchKernelGGL(dfisher_fcw_kernel, grid, dim3(256), 0, ctx->stream, scratch, gview(a), a.D, a.H, a.W, a.C, nout, N, d_acc_w);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

// ------------------------------------------------------------------------------------------ masks
namespace {

constexpr int MK_CHUNK = 4096;            // entries per workgroup of the ordered pass (256 threads x 16 consecutive)
constexpr int MK_HB = 1024;               // most workgroups of a histogram pass
constexpr size_t MK_HIST_OFF = 256, MK_CNT_OFF = MK_HIST_OFF + (size_t)MK_HB * 256 * sizeof(unsigned);

struct MkState {
    unsigned long long prefix;            // the digits of the k-th largest key found so far (high bits)
    long long krem;                       // entries still to take among those that share the prefix
};

// numeric order as unsigned bits (topk.hip's key), with -0.0 taken as +0.0: the two compare equal
__device__ inline unsigned long long mk_key(double v) {
    const unsigned long long u = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

__global__ void mk_init_kernel(MkState *st, long long k) {
    st->prefix = 0;
    st->krem = k;
}

// pass p (0 = the top 8 bits): counts of digit p among the keys whose higher digits equal the prefix; hist[block][256].
// The shared-memory adds are integer counts: their order does not change the result.
__global__ __launch_bounds__(256) void mk_hist_kernel(const double *v, long long n, int pass, const MkState *st, unsigned *hist) {
    __shared__ unsigned lh[256];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long prefix = st->prefix;
    const int shift = 56 - 8 * pass;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned long long key = mk_key(v[i]);
        if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&lh[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(long long)blockIdx.x * 256 + threadIdx.x] = lh[threadIdx.x];
}

// one workgroup: the digit in which the krem-th largest of the candidates lies
__global__ __launch_bounds__(256) void mk_select_kernel(const unsigned *hist, int nb, MkState *st) {
    __shared__ unsigned long long tot[256];
    unsigned long long s = 0;
    for (int b = 0; b < nb; ++b) s += hist[(long long)b * 256 + threadIdx.x];
    tot[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long krem = (unsigned long long)st->krem;
        unsigned long long cum = 0;
        int d = 0;
        for (int b = 255; b >= 0; --b) {
            if (cum + tot[b] >= krem) { d = b; break; }
            cum += tot[b];
        }
        st->prefix = (st->prefix << 8) | (unsigned long long)d;
        st->krem = (long long)(krem - cum);
    }
}

// entries equal to the threshold key per chunk of MK_CHUNK consecutive entries
__global__ __launch_bounds__(256) void mk_count_kernel(const double *v, long long n, const MkState *st, unsigned long long *cnt) {
    __shared__ unsigned sh[256];
    const unsigned long long T = st->prefix;
    const long long i0 = blockIdx.x * (long long)MK_CHUNK;
    unsigned c = 0;
    for (int j = threadIdx.x; j < MK_CHUNK; j += 256)
        if (i0 + j < n && mk_key(v[i0 + j]) == T) ++c;
    sh[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[blockIdx.x] = sh[0];
}

// one workgroup: cnt -> exclusive prefix sums, in place
__global__ __launch_bounds__(256) void mk_scan_kernel(unsigned long long *cnt, long long nchunks) {
    __shared__ unsigned long long seg[256];
    const long long per = (nchunks + 255) / 256;
    const long long a = threadIdx.x * per, b = a + per < nchunks ? a + per : nchunks;
    unsigned long long s = 0;
    for (long long i = a; i < b; ++i) s += cnt[i];
    seg[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 256; ++t) { const unsigned long long x = seg[t]; seg[t] = run; run += x; }
    }
    __syncthreads();
    unsigned long long run = seg[threadIdx.x];
    for (long long i = a; i < b; ++i) { const unsigned long long x = cnt[i]; cnt[i] = run; run += x; }
}

// mask[i] = key > T, or key == T and fewer than krem equal entries lie before i; a thread owns 16 consecutive entries
__global__ __launch_bounds__(256) void mk_emit_kernel(const double *v, long long n, const MkState *st, const unsigned long long *off,
                                                      float *mask) {
    __shared__ unsigned sh[256];
    const unsigned long long T = st->prefix;
    const unsigned long long krem = (unsigned long long)st->krem;
    const int t = threadIdx.x;
    const long long i0 = blockIdx.x * (long long)MK_CHUNK + t * 16;
    unsigned long long key[16];
    unsigned ce = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        key[j] = i0 + j < n ? mk_key(v[i0 + j]) : 0ull;
        if (i0 + j < n && key[j] == T) ++ce;
    }
    sh[t] = ce;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned x = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    unsigned long long rank = off[blockIdx.x] + (sh[t] - ce);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (i0 + j >= n) break;
        float m = 0.f;
        if (key[j] > T) m = 1.f;
        else if (key[j] == T) { m = rank < krem ? 1.f : 0.f; ++rank; }
        mask[i0 + j] = m;
    }
}

__global__ void mk_threshold_kernel(const double *v, long long n, double thr, float *mask) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        mask[i] = v[i] >= thr ? 1.f : 0.f;
}

}  // namespace

size_t topk_mask_work_bytes_impl(int64_t n) {
    const long long nchunks = n > 0 ? (n + MK_CHUNK - 1) / MK_CHUNK : 1;
    return MK_CNT_OFF + (size_t)nchunks * sizeof(unsigned long long);
}

int topk_mask_impl(alq_ctx *ctx, const double *d_v, int64_t n, int64_t k, float *d_mask, void *d_work) {
    ALQ_REQUIRE(n >= 0 && k >= 0 && k <= n, ALQ_EINVAL, "alq_topk_mask: need 0 <= k <= n (k=%lld n=%lld)", (long long)k, (long long)n);
    if (n == 0) return ALQ_OK;
    if (k == 0) {
        ALQ_HIP(hipMemsetAsync(d_mask, 0, (size_t)n * sizeof(float), ctx->stream));
        return ALQ_OK;
    }
    char *wb = static_cast<char *>(d_work);
    MkState *st = reinterpret_cast<MkState *>(wb);
    unsigned *hist = reinterpret_cast<unsigned *>(wb + MK_HIST_OFF);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(wb + MK_CNT_OFF);
    const long long nchunks = (n + MK_CHUNK - 1) / MK_CHUNK;
    const int nb = (int)std::min<long long>(nchunks, MK_HB);
    ProfScope ps(ctx, PROF_REDUCE, 0);
    hipLaunchKernelGGL(mk_init_kernel, dim3(1), dim3(1), 0, ctx->stream, st, (long long)k);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(mk_hist_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_v, (long long)n, pass, st, hist);
        hipLaunchKernelGGL(mk_select_kernel, dim3(1), dim3(256), 0, ctx->stream, hist, nb, st);
    }
    hipLaunchKernelGGL(mk_count_kernel, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, d_v, (long long)n, st, cnt);
    hipLaunchKernelGGL(mk_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, cnt, nchunks);
    hipLaunchKernelGGL(mk_emit_kernel, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, d_v, (long long)n, st, cnt, d_mask);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int threshold_mask_impl(alq_ctx *ctx, const double *d_v, int64_t n, double thr, float *d_mask) {
    if (n == 0) return ALQ_OK;
    const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 65535LL * 16);
    hipLaunchKernelGGL(mk_threshold_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_v, (long long)n, thr, d_mask);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // namespace alq
