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

namespace alq {

namespace {

typedef float gn_f32x4 __attribute__((ext_vector_type(4)));

constexpr int GN_WAVES = 4;
constexpr int GN_THREADS = GN_WAVES * 64;
constexpr int GN_KC_MAX = 128;            // points per box
constexpr int GN_HALO_MAX = 13312;        // floats of the staged Y halo (52 KiB; with X rows + table: < 64 KiB LDS)

// element (voxel row r of the N-patch tensor, channel c) of a View, split concat included
struct GnView {
    const float *p;
    int cs, c0, split;
    long long delta;
    __device__ inline float at(long long row, int c) const {
        if (split && c >= split) return p[delta + row * cs + (c - split)];
        return p[row * cs + c0 + c];
    }
};
GnView gview(const View &v) {
    GnView d;
    d.p = v.p; d.cs = v.cs; d.c0 = v.c0; d.split = v.split; d.delta = v.delta;
    return d;
}

struct GnGeom {
    int XD, XH, XW, Ca;          // unshifted operand: grid of the swept points r, channels a (tile columns)
    int YD, YH, YW, Cb;          // shifted operand: grid, channels b (tile rows (tap, b))
    int k[3], s[3], sg, base[3];
    int omin[3], span[3];        // tap offsets o = sg * t + base: minimum and extent per dimension
    int RY, RX, hy, hx;          // box of X points (1 x RY x RX); halo extent in y and x (z: span[0])
    int T, MT, NT, groups;       // taps, row tiles, column tiles, row-tile groups per column tile
    int halo_fl;                 // floats of the staged halo (the X rows and the offset table follow it in LDS)
};

// grid (NT * groups, N); writes part[n * gridDim.x + blockIdx.x] = sum of the squares of this workgroup's tiles
template <int TPW>
__global__ __launch_bounds__(GN_THREADS) void gnorm_wsq_kernel(GnView X, GnView Y, GnGeom g, double *part) {
    extern __shared__ float gn_lds[];
    float *Ys = gn_lds;                                   // [span0][hy][hx][Cb]
    float *Xs = gn_lds + g.halo_fl;                       // [ksteps * 4][16]
    int *hb = (int *)(Xs + ((g.RY * g.RX + 3) & ~3) * 16);   // [ksteps * 4] halo offset of box point kk
    __shared__ double red[GN_THREADS];

    const int n = blockIdx.y;
    const int ct = blockIdx.x / g.groups, rg = blockIdx.x - ct * g.groups;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long xvox = (long long)g.XD * g.XH * g.XW, yvox = (long long)g.YD * g.YH * g.YW;
    const int rows = g.T * g.Cb;

    // per tile j of this wave: the halo offset of row (tap, b) = lane & 15, or -1 for a row past the end
    int toff[TPW];
    int ntile = 0;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int rt = rg * (GN_WAVES * TPW) + w + GN_WAVES * j;
        if (rt < g.MT) ntile = j + 1;
        const int m = rt * 16 + (lane & 15);
        if (rt < g.MT && m < rows) {
            const int tap = m / g.Cb, b = m - tap * g.Cb;
            const int tz = tap / (g.k[1] * g.k[2]), ty = (tap / g.k[2]) % g.k[1], tx = tap % g.k[2];
            const int oz = g.sg * tz + g.base[0] - g.omin[0];
            const int oy = g.sg * ty + g.base[1] - g.omin[1];
            const int ox = g.sg * tx + g.base[2] - g.omin[2];
            toff[j] = ((oz * g.hy + oy) * g.hx + ox) * g.Cb + b;
        } else {
            toff[j] = -1;
        }
    }
    gn_f32x4 acc[TPW], tot[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) { acc[j] = gn_f32x4{0.f, 0.f, 0.f, 0.f}; tot[j] = acc[j]; }

    const int KC = g.RY * g.RX;
    const int ksteps = (KC + 3) / 4;
    const int halo = g.halo_fl;
    const int col0 = ct * 16;
    for (int z = 0; z < g.XD; ++z) {
        for (int y0 = 0; y0 < g.XH; y0 += g.RY) {
            for (int x0 = 0; x0 < g.XW; x0 += g.RX) {
                __syncthreads();
                // X rows of the box: Xs[kk][a], zero outside the grid and past the channels
                for (int i = threadIdx.x; i < ksteps * 4 * 16; i += GN_THREADS) {
                    const int kk = i >> 4, a = i & 15;
                    const int ry = kk / g.RX, rx = kk - ry * g.RX;
                    const int y = y0 + ry, x = x0 + rx;
                    float v = 0.f;
                    if (kk < KC && y < g.XH && x < g.XW && col0 + a < g.Ca)
                        v = X.at((long long)n * xvox + ((long long)z * g.XH + y) * g.XW + x, col0 + a);
                    Xs[i] = v;
                }
                for (int kk = threadIdx.x; kk < ksteps * 4; kk += GN_THREADS) {
                    const int ry = kk / g.RX, rx = kk - ry * g.RX;
                    hb[kk] = kk < KC ? (g.s[1] * ry * g.hx + g.s[2] * rx) * g.Cb : 0;
                }
                // Y halo: Ys[hz][hy][hx][b] = Y[origin + (hz, hy, hx), b]
                const int oz = g.s[0] * z + g.omin[0], oy = g.s[1] * y0 + g.omin[1], ox = g.s[2] * x0 + g.omin[2];
                for (int i = threadIdx.x; i < halo; i += GN_THREADS) {
                    int r = i / g.Cb;
                    const int b = i - r * g.Cb;
                    const int hx_ = r % g.hx; r /= g.hx;
                    const int hy_ = r % g.hy;
                    const int hz_ = r / g.hy;
                    const int pz = oz + hz_, py = oy + hy_, px = ox + hx_;
                    float v = 0.f;
                    if ((unsigned)pz < (unsigned)g.YD && (unsigned)py < (unsigned)g.YH && (unsigned)px < (unsigned)g.YW)
                        v = Y.at((long long)n * yvox + ((long long)pz * g.YH + py) * g.YW + px, b);
                    Ys[i] = v;
                }
                __syncthreads();
                for (int ks = 0; ks < ksteps; ++ks) {
                    const int kk = ks * 4 + (lane >> 4);
                    const float bv = Xs[kk * 16 + (lane & 15)];
                    const int h = hb[kk];
#pragma unroll
                    for (int j = 0; j < TPW; ++j) {
                        if (j < ntile) {
                            const float av = toff[j] >= 0 ? Ys[h + toff[j]] : 0.f;
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < TPW; ++j) { tot[j] += acc[j]; acc[j] = gn_f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
        }
    }
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

int span_of(int s, int n_pts, int span) { return s * (n_pts - 1) + span; }

// the kernel's geometry for U / V of a layer (see the header comment); mirrored form for a narrow stride-1 conv
GnGeom make_geom(const View &U, const View &V, const int k[3], const int s[3], const int lo[3], bool *mirror) {
    GnGeom g{};
    const bool stride1 = s[0] == 1 && s[1] == 1 && s[2] == 1;
    *mirror = stride1 && U.C < 16 && V.C > U.C;
    const View &X = *mirror ? V : U, &Y = *mirror ? U : V;
    g.XD = X.D; g.XH = X.H; g.XW = X.W; g.Ca = X.C;
    g.YD = Y.D; g.YH = Y.H; g.YW = Y.W; g.Cb = Y.C;
    g.sg = *mirror ? -1 : 1;
    for (int d = 0; d < 3; ++d) {
        g.k[d] = k[d];
        g.s[d] = s[d];
        g.base[d] = *mirror ? lo[d] : -lo[d];
        g.omin[d] = *mirror ? lo[d] - (k[d] - 1) : -lo[d];
        g.span[d] = k[d];
    }
    g.T = k[0] * k[1] * k[2];
    g.MT = (g.T * g.Cb + 15) / 16;
    g.NT = (g.Ca + 15) / 16;
    // box: whole x rows where they fit, as many rows as the point and halo budgets allow
    g.RX = std::min(g.XW, GN_KC_MAX);
    g.RY = std::max(1, std::min(g.XH, GN_KC_MAX / g.RX));
    for (;;) {
        g.hy = span_of(g.s[1], g.RY, g.span[1]);
        g.hx = span_of(g.s[2], g.RX, g.span[2]);
        if ((long long)g.span[0] * g.hy * g.hx * g.Cb <= GN_HALO_MAX) break;
        if (g.RY > 1) --g.RY;
        else if (g.RX > 1) --g.RX;
        else break;
    }
    g.halo_fl = g.span[0] * g.hy * g.hx * g.Cb;
    return g;
}

int gn_tpw(int MT) {
    const int need = (MT + GN_WAVES - 1) / GN_WAVES;
    return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
}

// LDS of one workgroup: only what the layer's box needs (more workgroups share a CU when the halo is small)
size_t gnorm_dyn_lds_bytes(const GnGeom &g) {
    const int kc = (g.RY * g.RX + 3) & ~3;
    return (size_t)(g.halo_fl + kc * 16) * 4 + (size_t)kc * 4;
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
