// Per-sample squared norms of parameter gradients without materialising them (alq_grad_sqnorms): what the expected-
// gradient-length query (NNAL.py:234-285) sums, ||d log p_j / d theta_t||^2 per variable.
//   * conv / conv_transpose weights: the per-sample weight gradient of one layer is
//         G[tap][v][u] = sum_q U[q, u] V[s q + tap - lo, v]          (the indexing of train.hip's wgrad_kernel)
//     a GEMM over the voxels q of one sample.  It runs on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32), every
//     16 x 16 tile of G lives in registers for the whole voxel sweep, and only sum(G^2) leaves the workgroup.
//     Generic form: H[tap][b][a] = sum_r X[r, a] Y[s r + o(tap), b] with X the UNSHIFTED operand (the MFMA's B, columns a),
//     Y the SHIFTED one (the MFMA's A, rows (tap, b)) and o(tap) = sg * tap + base per dimension.  The squared norm does
//     not care how the entries of G are laid out, so a stride-1 conv whose output side is narrower than 16 channels
//     (NET-C's dec2: 8 output, 16 input channels) runs in the mirrored form p = q + tap - lo,
//         G[tap][v][u] = sum_p V[p, v] U[p - tap + lo, u]            (X = V, Y = U, sg = -1),
//     which fills the 16 columns of the tile instead of half of them.
//     The voxels are swept in boxes of 1 x RY x RX points of X's grid; each box stages its X rows and the halo of Y it
//     touches (zero outside the grid) in LDS, then every wave runs its row tiles over the box in k-steps of 4 points.
//     Work is split across workgroups by (sample, column tile, row-tile group) only - never over the voxels - and the
//     fp32 accumulators are folded into a second fp32 set after every box (a two-level sum: the error of one entry grows
//     with sqrt(box) + sqrt(boxes), not with sqrt(voxels)).  Squares and folds are fp64 in a fixed order, so a sample's
//     result is bit-identical whatever the batch and whichever run.
//   * biases: ||sum_q U[q, :]||^2 from fp64 channel sums.
//   * fc: the per-sample gradient is rank one, ||dW||^2 = ||delta||^2 ||a||^2, ||db||^2 = ||delta||^2
//     (NNAL_tools.FC_gradnorms_batch, NNAL_tools.py:725-775): O(F + out) per sample.
#include <algorithm>

#include "alq_internal.h"
#include "gnorm_sweep.h"

namespace alq {

using namespace gn;

namespace {

// grid (NT * groups, N); writes part[n * gridDim.x + blockIdx.x] = sum of the squares of this workgroup's tiles
template <int TPW>
__global__ __launch_bounds__(GN_THREADS) void gnorm_wsq_kernel(GnView X, GnView Y, GnGeom g, double *part) {
    __shared__ double red[GN_THREADS];

    const int n = blockIdx.y;
    const int ct = blockIdx.x / g.groups, rg = blockIdx.x - ct * g.groups;
    int toff[TPW];
    const int ntile = gn_tile_rows<TPW>(g, rg, toff);
    gn_f32x4 tot[TPW];
    gn_sweep_sample<TPW>(X, Y, g, n, ct * 16, toff, ntile, tot);
    // squares in fp64, fixed order: tiles, registers, then a fixed tree over the lanes and waves
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const double v = (double)tot[j][r]; s += v * v; }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = GN_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long long)n * gridDim.x + blockIdx.x] = red[0];
}

// sq[n * ld + col] = sum_g part[n * G + g], in g order
__global__ void gnorm_fold_kernel(const double *part, int G, int N, double *sq, int ld, int col) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int i = 0; i < G; ++i) s += part[(long long)n * G + i];
    sq[(long long)n * ld + col] = s;
}

// bias of a conv / conv_transpose: sq[n * ld + col] = sum_c (sum_x D[n, x, c])^2, fp64; one workgroup per sample.
// Thread t sums channel t % C over the rows t / C, t / C + R, ... (R = 256 / C), the R partials of a channel fold in order.
__global__ __launch_bounds__(256) void gnorm_bias_kernel(GnView D, long long vox, int C, double *sq, int ld, int col) {
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
    if (t == 0) {
        double tot = 0.0;
        for (int c = 0; c < C; ++c) {
            double cs = 0.0;
            for (int i = 0; i < R; ++i) cs += sh[i * C + c];
            tot += cs * cs;
        }
        sq[(long long)n * ld + col] = tot;
    }
}

// fc: sq[n * ld + col] = ||delta_n||^2 ||a_n||^2, sq[n * ld + col + 1] = ||delta_n||^2 (fp64, fixed trees); one workgroup per sample
__global__ __launch_bounds__(256) void gnorm_fc_kernel(const float *delta, int nout, GnView A, long long avox, int aC, double *sq,
                                                       int ld, int col) {
    __shared__ double sd[256], sa[256];
    const int n = blockIdx.x, t = threadIdx.x;
    double d = 0.0, a = 0.0;
    for (int o = t; o < nout; o += 256) { const double v = (double)delta[(long long)n * nout + o]; d += v * v; }
    const long long F = avox * aC;
    for (long long f = t; f < F; f += 256) {
        const long long r = f / aC;
        const double v = (double)A.at((long long)n * avox + r, (int)(f - r * aC));
        a += v * v;
    }
    sd[t] = d; sa[t] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { sd[t] += sd[t + o]; sa[t] += sa[t + o]; }
        __syncthreads();
    }
    if (t == 0) {
        sq[(long long)n * ld + col] = sd[0] * sa[0];
        sq[(long long)n * ld + col + 1] = sd[0];
    }
}

}  // namespace

long long gnorm_partials(const View &U, const View &V, const int k[3], const int s[3], const int lo[3]) {     // per sample
    bool mirror;
    const GnGeom g = make_geom(U, V, k, s, lo, &mirror);
    const int tpw = gn_tpw(g.MT);
    const int groups = (g.MT + GN_WAVES * tpw - 1) / (GN_WAVES * tpw);
    return (long long)g.NT * groups;
}

int k_gnorm_weight(alq_ctx *ctx, const View &U, const View &V, const int k[3], const int s[3], const int lo[3], int N, double *part,
                   double *d_sq, int ld, int col) {
    bool mirror;
    GnGeom g = make_geom(U, V, k, s, lo, &mirror);
    ALQ_REQUIRE((long long)g.halo_fl <= GN_HALO_MAX, ALQ_EUNSUPPORTED,
                "alq_grad_sqnorms: %d channels x %d taps do not fit the staged halo", g.Cb, g.T);
    const int tpw = gn_tpw(g.MT);
    g.groups = (g.MT + GN_WAVES * tpw - 1) / (GN_WAVES * tpw);
    const int G = g.NT * g.groups;
    const View &X = mirror ? V : U, &Y = mirror ? U : V;
    const GnView gx = gview(X), gy = gview(Y);
    const size_t lds = gnorm_dyn_lds_bytes(g);
    {
        ProfScope ps(ctx, PROF_GNORM, 2.0 * (double)N * X.vox() * g.T * g.Cb * g.Ca);
        dim3 grid((unsigned)G, (unsigned)N);
#define ALQ_GN(TP) hipLaunchKernelGGL(gnorm_wsq_kernel<TP>, grid, dim3(GN_THREADS), lds, ctx->stream, gx, gy, g, part)
        switch (tpw) {
            case 1: ALQ_GN(1); break;
            case 2: ALQ_GN(2); break;
            case 4: ALQ_GN(4); break;
            case 8: ALQ_GN(8); break;
            default: ALQ_GN(16); break;
        }
#undef ALQ_GN
        ALQ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(gnorm_fold_kernel, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, part, G, N, d_sq, ld, col);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int k_gnorm_bias(alq_ctx *ctx, const View &delta, int N, double *d_sq, int ld, int col) {
    ALQ_REQUIRE(delta.C >= 1 && delta.C <= 256, ALQ_EUNSUPPORTED, "alq_grad_sqnorms: bias of %d channels", delta.C);
    hipLaunchKernelGGL(gnorm_bias_kernel, dim3((unsigned)N), dim3(256), 0, ctx->stream, gview(delta), (long long)delta.vox(), delta.C,
                       d_sq, ld, col);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int k_gnorm_fc(alq_ctx *ctx, const float *delta, int nout, const View &a, int N, double *d_sq, int ld, int col) {
    hipLaunchKernelGGL(gnorm_fc_kernel, dim3((unsigned)N), dim3(256), 0, ctx->stream, delta, nout, gview(a), (long long)a.vox(), a.C,
                       d_sq, ld, col);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // namespace alq
