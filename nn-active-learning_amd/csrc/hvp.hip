// Exact Hessian-vector products (alq_hess_vecp): the kernels of the R-operator pass.
//   Replaces: the Pearlmutter double-backward of Influence.get_hess_vec_product / hessian_vector_product (Influence.py:64-166)
//   that PW_sample_influence (Influence.py:369-453) hands to scipy's Newton-CG.
// The driver (grads.hip) runs the ordinary forward pass with everything kept, which fixes every ReLU and max-pool decision
// (the stored activation's sign, the stored arg-max), and then evaluates on those decisions, in fp64 throughout:
//   activations        a_l = mask . (op(a_{l-1}; W_l) + b_l), max-pool at the stored arg-max, a 'con' skip as a two-part source;
//   logits             p = softmax(z), delta = loss_scale (p - y) (hvp_softmax64);
//   cotangents         delta_{l-1} = mask . op^T(delta_l; W_l);
//   tangent forward    Rz_l = op(a_{l-1}; V_l) + c_l + op(Ra_{l-1}; W_l), same routing (hvp_contract / hvp_fc_fwd / hvp_pool_fwd);
//   logits             Rdelta = loss_scale (diag(p) - p p^T) Rz (hvp_softmax2);
//   backward           Rdelta_{l-1} = mask . (op^T(delta_l; V_l) + op^T(Rdelta_l; W_l)) (hvp_contract with the transposed geometry /
//                      hvp_fc_bwd / hvp_pool_bwd / hvp_mask), the two channel groups of a concat routed to their producers;
//   products           (Hv)_W = wgrad(Rdelta_l, a_{l-1}) + wgrad(delta_l, Ra_{l-1}), (Hv)_b = sum Rdelta_l (hvp_wgrad / hvp_fc_wgrad /
//                      hvp_bias) into the caller's fp64 vector.
// Why fp64 tensors and not the fp32 ones the scoring engines leave: the second-order term multiplies differences of large
// tangents (|Rz| is 100 x Rz_j - Rz_k for a vector with a component along the head's weights) by p_j p_k; fp32 activations (3e-6 on
// values of 6) put 1.5e-6 on a head-bias entry of 0.4 - above what an fp32 double-backward reaches.  What fp64 costs in
// arithmetic rate has not been measured apart from the rest; DESIGN.md has the measured cost of a whole product.
// Not on the scored path: plain VALU kernels, one thread (or one workgroup) per output element,
// every store a single dword or qword without a register offset (the 16-byte store hazard of alq_internal.h does not arise);
// fixed summation orders and no atomics: results are bit-identical from run to run, and every operation is linear in v, so
// scaling v by a power of two scales the result exactly.
#include <algorithm>

#include "alq_internal.h"

namespace alq {

#define ALQ_LAUNCH_CHECK() ALQ_HIP(hipGetLastError())

static inline unsigned hgrid(long long n, int block = 256) {
    long long g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 65535LL * 16) g = 65535LL * 16;
    return (unsigned)g;
}

__device__ inline double hs_at(const HSrc &s, long long row, int c) {
    if (c < s.Ca) {
        const long long o = row * s.csa + s.c0a + c;
        return s.da ? s.da[o] : (double)s.pa[o];
    }
    const long long o = row * s.csb + s.c0b + (c - s.Ca);
    return s.db ? s.db[o] : (double)s.pb[o];
}
__device__ inline bool hs_on(const HSrc &s) { return s.pa != nullptr || s.da != nullptr; }
__device__ inline void hd_put(const HDst &d, long long row, int c, double v) {
    if (c < d.Ca) {
        double *q = d.pa + row * d.Ca + c;
        *q = d.acca ? *q + v : v;
    } else {
        double *q = d.pb + row * d.Cb + (c - d.Ca);
        *q = d.accb ? *q + v : v;
    }
}

HSrc hsrc_view(const View &v) {
    HSrc s;
    if (v.split) {
        s.pa = v.p; s.csa = v.cs; s.c0a = v.c0; s.Ca = v.split;
        s.pb = v.p + v.delta; s.csb = v.cs; s.c0b = 0; s.Cb = v.C - v.split;
    } else {
        s.pa = v.p; s.csa = v.cs; s.c0a = v.c0; s.Ca = v.C;
    }
    return s;
}
HSrc hsrc_dense(const double *pa, int Ca, const double *pb, int Cb) {
    HSrc s;
    s.da = pa; s.csa = Ca; s.Ca = Ca;
    s.db = pb; s.csb = Cb; s.Cb = Cb;
    return s;
}

// ------------------------------------------------------------------------------------------ two-term contraction
// out[n, p, j] = cb[j] + sum_t sum_i s1[n, pos(p, t), i] W1[t, i, j] + s2[n, pos(p, t), i] W2[t, i, j], per dimension
// pos = (p a + b t + c) / d where that is an integer inside the source grid.  With the four (a, b, c, d) sets and weight strides
// of hvp_geometry this is a conv or a conv_transpose, forward or backward-data, on the TF filter layouts as they are.
// A term whose source is null is skipped (its weights are never read: the entries of v of a layer that is switched off).
__global__ __launch_bounds__(256) void hvp_contract_kernel(HSrc s1, const float *W1, HSrc s2, const float *W2, const float *cb, HSrc mask,
                                                           HDst dst, HGeo g, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int j = (int)(r % g.Cj); r /= g.Cj;
        const long long orow = r;
        const int px = (int)(r % g.OW); r /= g.OW;
        const int py = (int)(r % g.OH); r /= g.OH;
        const int pz = (int)(r % g.OD); r /= g.OD;
        const long long n = r;
        double acc = cb ? (double)cb[j] : 0.0;
        for (int tz = 0; tz < g.kz; ++tz) {
            const int nz = pz * g.a[0] + g.b[0] * tz + g.c[0];
            if (nz < 0 || nz % g.d[0]) continue;
            const int qz = nz / g.d[0];
            if (qz >= g.ID) continue;
            for (int ty = 0; ty < g.ky; ++ty) {
                const int ny = py * g.a[1] + g.b[1] * ty + g.c[1];
                if (ny < 0 || ny % g.d[1]) continue;
                const int qy = ny / g.d[1];
                if (qy >= g.IH) continue;
                for (int tx = 0; tx < g.kx; ++tx) {
                    const int nx = px * g.a[2] + g.b[2] * tx + g.c[2];
                    if (nx < 0 || nx % g.d[2]) continue;
                    const int qx = nx / g.d[2];
                    if (qx >= g.IW) continue;
                    const long long row = ((n * g.ID + qz) * g.IH + qy) * g.IW + qx;
                    const long long wo = (long long)((tz * g.ky + ty) * g.kx + tx) * g.wt + (long long)j * g.wj;
                    if (hs_on(s1))
                        for (int ii = 0; ii < g.Ci; ++ii) acc = fma(hs_at(s1, row, ii), (double)W1[wo + (long long)ii * g.wi], acc);
                    if (hs_on(s2))
                        for (int ii = 0; ii < g.Ci; ++ii) acc = fma(hs_at(s2, row, ii), (double)W2[wo + (long long)ii * g.wi], acc);
                }
            }
        }
        if (hs_on(mask) && !(hs_at(mask, orow, j) > 0.0)) acc = 0.0;
        hd_put(dst, orow, j, acc);
    }
}

int hvp_geometry(int type, int backward, const View &in, const View &out, const int k[3], const int s[3], const int lo[3], HGeo *g) {
    const int Cin = in.C, Cout = out.C;
    const int dims_in[3] = {in.D, in.H, in.W}, dims_out[3] = {out.D, out.H, out.W};
    g->kz = k[0]; g->ky = k[1]; g->kx = k[2];
    g->wt = (long long)Cin * Cout;
    const int *src = backward ? dims_out : dims_in, *dstd = backward ? dims_in : dims_out;
    g->ID = src[0]; g->IH = src[1]; g->IW = src[2];
    g->OD = dstd[0]; g->OH = dstd[1]; g->OW = dstd[2];
    g->Ci = backward ? Cout : Cin;
    g->Cj = backward ? Cin : Cout;
    for (int d = 0; d < 3; ++d) {
        if (type == ALQ_CONV) {
            g->a[d] = 1; g->d[d] = 1;
            g->b[d] = backward ? -1 : 1;
            g->c[d] = backward ? lo[d] : -lo[d];
        } else {
            g->a[d] = backward ? s[d] : 1;
            g->d[d] = backward ? 1 : s[d];
            g->b[d] = backward ? 1 : -1;
            g->c[d] = backward ? -lo[d] : lo[d];
        }
    }
    if (type == ALQ_CONV) {          // W[t][ci][co]
        g->wi = backward ? 1 : Cout;
        g->wj = backward ? Cout : 1;
    } else if (type == ALQ_CONVT) {  // W[t][co][ci]
        g->wi = backward ? Cin : 1;
        g->wj = backward ? 1 : Cin;
    } else {
        set_error("hvp_geometry: layer type %d", type);
        return ALQ_EINVAL;
    }
    return ALQ_OK;
}

int k_hvp_contract(alq_ctx *ctx, const HSrc &s1, const float *W1, const HSrc &s2, const float *W2, const float *cb, const HSrc &mask,
                   const HDst &dst, const HGeo &g, int N) {
    const long long total = (long long)N * g.OD * g.OH * g.OW * g.Cj;
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    hipLaunchKernelGGL(hvp_contract_kernel, dim3(hgrid(total)), dim3(256), 0, ctx->stream, s1, W1, s2, W2, cb, mask, dst, g, total);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// ------------------------------------------------------------------------------------------ fully connected layers
// The weights stay in the TF layout [out][f_tf], f_tf = ((c W + w) H + h) D + d (the reference's flatten order, NN.py:296-301);
// the activations are [n][(d, h, w)][c].
__device__ inline long long hvp_ftf(long long v, int c, int D, int H, int W) {
    const int w = (int)(v % W);
    const long long t = v / W;
    const int h = (int)(t % H), d = (int)(t / H);
    return (((long long)c * W + w) * H + h) * D + d;
}

// tangent of the pre-activation, one workgroup per (unit, sample): threads stride over the features, fixed tree
__global__ __launch_bounds__(256) void hvp_fc_fwd_kernel(HSrc a, const float *V, HSrc Ra, const float *W, const float *cb, HSrc mask,
                                                         double *out, int D, int H, int Wd, int C, int nout) {
    __shared__ double sh[256];
    const int o = blockIdx.x, n = blockIdx.y;
    const long long vox = (long long)D * H * Wd, F = vox * C;
    double acc = 0.0;
    for (long long f = threadIdx.x; f < F; f += 256) {
        const long long v = f / C;
        const int c = (int)(f - v * C);
        const long long wi = (long long)o * F + hvp_ftf(v, c, D, H, Wd);
        const long long row = (long long)n * vox + v;
        if (hs_on(a)) acc = fma(hs_at(a, row, c), (double)V[wi], acc);
        if (hs_on(Ra)) acc = fma(hs_at(Ra, row, c), (double)W[wi], acc);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double r = sh[0] + (cb ? (double)cb[o] : 0.0);
        if (hs_on(mask) && !(hs_at(mask, n, o) > 0.0)) r = 0.0;      // an fc output has one row per sample
        out[(long long)n * nout + o] = r;
    }
}

int k_hvp_fc_fwd(alq_ctx *ctx, const HSrc &a, const float *V, const HSrc &Ra, const float *W, const float *cb, const HSrc &mask,
                 double *out, const View &in, int nout, int N) {
    ALQ_REQUIRE(nout <= 65535 && N <= 65535, ALQ_EUNSUPPORTED, "hvp: fc layer of %d units / batch %d", nout, N);
    ProfScope ps(ctx, PROF_FC_SMALL, 0);
    hipLaunchKernelGGL(hvp_fc_fwd_kernel, dim3((unsigned)nout, (unsigned)N), dim3(256), 0, ctx->stream, a, V, Ra, W, cb, mask, out,
                       in.D, in.H, in.W, in.C, nout);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// tangent of the input cotangent: one thread per (sample, feature)
__global__ __launch_bounds__(256) void hvp_fc_bwd_kernel(const double *delta, const float *V, const double *Rdelta, const float *W, HDst dst, int D,
                                                         int H, int Wd, int C, int nout, long long total) {
    const long long vox = (long long)D * H * Wd, F = vox * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / F, f = i - n * F;
        const long long v = f / C;
        const int c = (int)(f - v * C);
        const long long ft = hvp_ftf(v, c, D, H, Wd);
        double acc = 0.0;
        if (V)
            for (int o = 0; o < nout; ++o) acc = fma(delta[n * nout + o], (double)V[(long long)o * F + ft], acc);
        for (int o = 0; o < nout; ++o) acc = fma(Rdelta[n * nout + o], (double)W[(long long)o * F + ft], acc);
        hd_put(dst, n * vox + v, c, acc);
    }
}

int k_hvp_fc_bwd(alq_ctx *ctx, const double *delta, const float *V, const double *Rdelta, const float *W, const HDst &dst, const View &in,
                 int nout, int N) {
    const long long total = (long long)N * in.vox() * in.C;
    ProfScope ps(ctx, PROF_FC_SMALL, 0);
    hipLaunchKernelGGL(hvp_fc_bwd_kernel, dim3(hgrid(total)), dim3(256), 0, ctx->stream, delta, V, Rdelta, W, dst, in.D, in.H, in.W, in.C,
                       nout, total);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// (Hv)_W[o][f_tf] (+)= sum_n Rdelta[n, o] a[n, f] + delta[n, o] Ra[n, f], samples in order
__global__ __launch_bounds__(256) void hvp_fc_wgrad_kernel(const double *Rdelta, HSrc a, const double *delta, HSrc Ra, int D, int H, int Wd, int C,
                                                           int nout, int N, int accumulate, double *hv) {
    const long long vox = (long long)D * H * Wd, F = vox * C, total = F * nout;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int o = (int)(i / F);
        long long ft = i - (long long)o * F;
        const int d = (int)(ft % D); ft /= D;
        const int h = (int)(ft % H); ft /= H;
        const int w = (int)(ft % Wd); ft /= Wd;
        const int c = (int)ft;
        const long long v = ((long long)d * H + h) * Wd + w;
        double s = 0.0;
        for (int n = 0; n < N; ++n) {
            s = fma(Rdelta[(long long)n * nout + o], hs_at(a, n * vox + v, c), s);
            if (hs_on(Ra)) s = fma(delta[(long long)n * nout + o], hs_at(Ra, n * vox + v, c), s);
        }
        hv[i] = accumulate ? hv[i] + s : s;
    }
}

int k_hvp_fc_wgrad(alq_ctx *ctx, const double *Rdelta, const HSrc &a, const double *delta, const HSrc &Ra, const View &in, int nout, int N,
                   int accumulate, double *hv) {
    const long long total = (long long)in.vox() * in.C * nout;
    ProfScope ps(ctx, PROF_REDUCE, 0);
    hipLaunchKernelGGL(hvp_fc_wgrad_kernel, dim3(hgrid(total)), dim3(256), 0, ctx->stream, Rdelta, a, delta, Ra, in.D, in.H, in.W, in.C, nout,
                       N, accumulate, hv);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// ------------------------------------------------------------------------------------------ conv / conv_transpose weight products
// G[t][v][u] = sum_{n, q} U1[n, q, u] V1[n, s q + t - lo, v] + U2[n, q, u] V2[n, s q + t - lo, v]   (the index rule of wgrad_kernel,
// train.hip: conv U = cotangent, V = input, s = 1; conv_transpose U = input, V = cotangent, s = stride).  A thread owns one
// entry of G and walks one slab of the (sample, q) rows; the slabs are added in order in fp64 by hvp_wgrad_reduce_kernel.
__global__ __launch_bounds__(256) void hvp_wgrad_kernel(HSrc U1, HSrc V1, HSrc U2, HSrc V2, int UC, int VC, int QD, int QH, int QW, int VD, int VH,
                                                        int VW, int ky, int kx, int sz, int sy, int sx, int lz, int ly, int lx, long long rows,
                                                        long long rows_per_slab, long long M, double *partial) {
    const int slab = blockIdx.y;
    for (long long m = blockIdx.x * (long long)blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        const int u = (int)(m % UC);
        const int v = (int)((m / UC) % VC);
        const int t = (int)(m / ((long long)UC * VC));
        const int tz = t / (ky * kx), ty = (t / kx) % ky, tx = t % kx;
        const long long qvox = (long long)QD * QH * QW, vvox = (long long)VD * VH * VW;
        const long long r0 = slab * rows_per_slab, r1 = min(rows, r0 + rows_per_slab);
        double acc = 0.0;
        long long n = r0 / qvox;
        long long q = r0 - n * qvox;
        int qx = (int)(q % QW), qy = (int)((q / QW) % QH), qz = (int)(q / ((long long)QW * QH));
        for (long long r = r0; r < r1; ++r) {
            const int pz = sz * qz + tz - lz, py = sy * qy + ty - ly, px = sx * qx + tx - lx;
            if ((unsigned)pz < (unsigned)VD && (unsigned)py < (unsigned)VH && (unsigned)px < (unsigned)VW) {
                const long long vr = n * vvox + ((long long)pz * VH + py) * VW + px;
                acc = fma(hs_at(U1, r, u), hs_at(V1, vr, v), acc);
                if (hs_on(U2)) acc = fma(hs_at(U2, r, u), hs_at(V2, vr, v), acc);
            }
            if (++qx == QW) { qx = 0; if (++qy == QH) { qy = 0; if (++qz == QD) { qz = 0; ++n; } } }
        }
        partial[(long long)slab * M + m] = acc;
    }
}

__global__ void hvp_wgrad_reduce_kernel(const double *partial, int nslab, long long M, int accumulate, double *hv) {
    for (long long m = blockIdx.x * (long long)blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int sl = 0; sl < nslab; ++sl) s += partial[(long long)sl * M + m];
        hv[m] = accumulate ? hv[m] + s : s;
    }
}

long long hvp_wgrad_partial_doubles(long long M) { return std::max<long long>(1LL << 22, M); }

int k_hvp_wgrad(alq_ctx *ctx, const HSrc &U1, const HSrc &V1, const HSrc &U2, const HSrc &V2, int UC, int VC, const View &Ug, const View &Vg,
                const int k[3], const int s[3], const int lo[3], int N, double *partial, int accumulate, double *hv) {
    const long long M = (long long)k[0] * k[1] * k[2] * UC * VC;
    const long long rows = (long long)N * Ug.vox();
    long long nslab = std::min<long long>(std::max<long long>(rows / 256, 1), std::max<long long>(hvp_wgrad_partial_doubles(M) / M, 1));
    nslab = std::min<long long>(nslab, 65535);
    const long long rps = (rows + nslab - 1) / nslab;
    nslab = (rows + rps - 1) / rps;
    ProfScope ps(ctx, PROF_REDUCE, 0);
    hipLaunchKernelGGL(hvp_wgrad_kernel, dim3(hgrid(M), (unsigned)nslab), dim3(256), 0, ctx->stream, U1, V1, U2, V2, UC, VC, Ug.D, Ug.H, Ug.W,
                       Vg.D, Vg.H, Vg.W, k[1], k[2], s[0], s[1], s[2], lo[0], lo[1], lo[2], rows, rps, M, partial);
    ALQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(hvp_wgrad_reduce_kernel, dim3(hgrid(M)), dim3(256), 0, ctx->stream, partial, (int)nslab, M, accumulate, hv);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// (Hv)_b[c] (+)= sum over all rows of Rdelta[row, c]: one workgroup per channel, fixed tree
__global__ __launch_bounds__(256) void hvp_bias_kernel(const double *Rd, int C, long long rows, int accumulate, double *hv) {
    __shared__ double sh[256];
    const int c = blockIdx.x;
    double s = 0.0;
    for (long long r = threadIdx.x; r < rows; r += 256) s += Rd[r * C + c];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) hv[c] = accumulate ? hv[c] + sh[0] : sh[0];
}

int k_hvp_bias(alq_ctx *ctx, const double *Rd, int C, long long rows, int accumulate, double *hv) {
    ALQ_REQUIRE(C <= 65535, ALQ_EUNSUPPORTED, "hvp: %d bias entries", C);
    hipLaunchKernelGGL(hvp_bias_kernel, dim3((unsigned)C), dim3(256), 0, ctx->stream, Rd, C, rows, accumulate, hv);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// ------------------------------------------------------------------------------------------ routing: ReLU, max-pool
// Rd[row, c] = 0 where the layer's stored activation is not positive (the ReLU's derivative), in place
__global__ void hvp_mask_kernel(double *Rd, int C, HSrc act, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / C;
        const int c = (int)(i - row * C);
        if (!(hs_at(act, row, c) > 0.0)) Rd[i] = 0.0;
    }
}
int k_hvp_mask(alq_ctx *ctx, double *Rd, int C, const HSrc &act, long long rows) {
    const long long total = rows * C;
    hipLaunchKernelGGL(hvp_mask_kernel, dim3(hgrid(total)), dim3(256), 0, ctx->stream, Rd, C, act, total);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// tangent of a max-pool output = tangent of the input element that won (window == stride, arg-max as pool_fwd_kernel stores it)
__global__ void hvp_pool_fwd_kernel(const double *Rin, const uint8_t *argmax, double *Rout, int C, int ID, int IH, int IW, int OD, int OH, int OW,
                                    int wz, int wy, int wx, int lz, int ly, int lx, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int c = (int)(r % C); r /= C;
        const int ox = (int)(r % OW); r /= OW;
        const int oy = (int)(r % OH); r /= OH;
        const int oz = (int)(r % OD); r /= OD;
        const long long n = r;
        const int b = argmax[i];
        const int dx = b % wx, dy = (b / wx) % wy, dz = b / (wx * wy);
        const int iz = oz * wz - lz + dz, iy = oy * wy - ly + dy, ix = ox * wx - lx + dx;
        double v = 0.0;
        if ((unsigned)iz < (unsigned)ID && (unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW)
            v = Rin[(((n * ID + iz) * IH + iy) * IW + ix) * C + c];
        Rout[i] = v;
    }
}
int k_hvp_pool_fwd(alq_ctx *ctx, const double *Rin, const uint8_t *argmax, double *Rout, const View &in, const View &out, const int w[3],
                   const int lo[3], int N) {
    const long long total = (long long)N * out.vox() * out.C;
    hipLaunchKernelGGL(hvp_pool_fwd_kernel, dim3(hgrid(total)), dim3(256), 0, ctx->stream, Rin, argmax, Rout, out.C, in.D, in.H, in.W, out.D,
                       out.H, out.W, w[0], w[1], w[2], lo[0], lo[1], lo[2], total);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// ... and its transpose as a gather (the index rule of pool_bwd_kernel): every input element reads the one window it lies in
__global__ void hvp_pool_bwd_kernel(const double *Rdout, const uint8_t *argmax, double *Rdin, int accumulate, int C, int ID, int IH, int IW, int OD,
                                    int OH, int OW, int wz, int wy, int wx, int lz, int ly, int lx, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int c = (int)(r % C); r /= C;
        const int ix = (int)(r % IW); r /= IW;
        const int iy = (int)(r % IH); r /= IH;
        const int iz = (int)(r % ID); r /= ID;
        const long long n = r;
        const int oz = (iz + lz) / wz, oy = (iy + ly) / wy, ox = (ix + lx) / wx;
        double g = 0.0;
        if (oz < OD && oy < OH && ox < OW) {
            const int widx = (((iz + lz) - oz * wz) * wy + ((iy + ly) - oy * wy)) * wx + ((ix + lx) - ox * wx);
            const long long o = ((n * OD + oz) * OH + oy) * OW + ox;
            if (argmax[o * C + c] == widx) g = Rdout[o * C + c];
        }
        Rdin[i] = accumulate ? Rdin[i] + g : g;
    }
}
int k_hvp_pool_bwd(alq_ctx *ctx, const double *Rdout, const uint8_t *argmax, double *Rdin, int accumulate, const View &in, const View &out,
                   const int w[3], const int lo[3], int N) {
    const long long total = (long long)N * in.vox() * in.C;
    hipLaunchKernelGGL(hvp_pool_bwd_kernel, dim3(hgrid(total)), dim3(256), 0, ctx->stream, Rdout, argmax, Rdin, accumulate, in.C, in.D, in.H,
                       in.W, out.D, out.H, out.W, w[0], w[1], w[2], lo[0], lo[1], lo[2], total);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// ------------------------------------------------------------------------------------------ the loss's second-order term
// Rdelta[n, j] = scale p_j (Rz_j - sum_k p_k Rz_k) = scale ((diag(p) - p p^T) Rz)_j; a label outside [0, c): a zero row, like
// the first-order cotangent of logit_cotangent_kernel (train.hip).  One thread per sample, fp64, classes in order.
__global__ void hvp_softmax2_kernel(const double *p64, const double *Rz, const int *labels, int c, int N, float scale, double *Rdelta) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int y = labels[n];
    const bool live = y >= 0 && y < c;
    const double *p = p64 + (long long)n * c;
    for (int j = 0; j < c; ++j) {
        const double zj = Rz[(long long)n * c + j];
        double s = 0.0;      // sum_k p_k (Rz_j - Rz_k) on the head's fp64 tangent: a common offset of Rz (large next to the
                             // differences when v has a component along the head's weights) cancels instead of leaking
                             // through the rounding of sum p, and the differences carry no fp32 rounding of |Rz|
        for (int k = 0; k < c; ++k) s = fma(p[k], zj - Rz[(long long)n * c + k], s);
        const double r = p[j] * s * (double)scale;
        Rdelta[(long long)n * c + j] = live ? r : 0.0;
    }
}
int k_hvp_softmax2(alq_ctx *ctx, const double *p64, const double *Rz, const int *labels, int c, int N, float scale, double *Rdelta) {
    hipLaunchKernelGGL(hvp_softmax2_kernel, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, p64, Rz, labels, c, N, scale, Rdelta);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// Posteriors of the call from the fp64 logits: p64 [N, c], their fp32 rounding [c, N] (the loss), and the first-order cotangent
// delta[n, j] = scale (p_j - [j == label]) in fp64 (a label outside [0, c): a zero row, as in logit_cotangent_kernel, train.hip)
__global__ void hvp_softmax64_kernel(const double *z64, const int *labels, int c, int N, float scale, float *post_cN, double *p64,
                                     double *delta) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double *z = z64 + (long long)n * c;
    const int y = labels[n];
    const bool live = y >= 0 && y < c;
    double mx = z[0];
    for (int j = 1; j < c; ++j) mx = fmax(mx, z[j]);
    double s = 0.0;
    for (int j = 0; j < c; ++j) s += exp(z[j] - mx);
    for (int j = 0; j < c; ++j) {
        const double p = exp(z[j] - mx) / s;
        p64[(long long)n * c + j] = p;
        post_cN[(long long)j * N + n] = (float)p;
        delta[(long long)n * c + j] = live ? (p - (j == y ? 1.0 : 0.0)) * (double)scale : 0.0;
    }
}
int k_hvp_softmax64(alq_ctx *ctx, const double *z64, const int *labels, int c, int N, float scale, float *post_cN, double *p64,
                    double *delta) {
    hipLaunchKernelGGL(hvp_softmax64_kernel, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, z64, labels, c, N, scale, post_cN, p64,
                       delta);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// scale * sum_n -log p[y_n, n] over the labelled samples: the loss whose Hessian the call applies (one workgroup, fp64, fixed tree)
__global__ __launch_bounds__(256) void hvp_loss_kernel(const float *post_cN, int c, int N, const int *labels, float scale, double *out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const int y = labels[n];
        if (y >= 0 && y < c) s -= log((double)fmaxf(post_cN[(long long)y * N + n], 1e-38f));
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0] * (double)scale;
}
int k_hvp_loss(alq_ctx *ctx, const float *post_cN, int c, int N, const int *labels, float scale, double *d_out) {
    hipLaunchKernelGGL(hvp_loss_kernel, dim3(1), dim3(256), 0, ctx->stream, post_cN, c, N, labels, scale, d_out);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

// TF-layout copy of a wide fc layer's weights from the resident activation-memory-order copy the device packers keep
// (wpack_permute's inverse): Wtf[o][f_tf] = Wres[o][f_mem]
__global__ void hvp_unpermute_kernel(const float *Wres, float *Wtf, int D, int H, int Wd, int C, long long total) {
    const long long vox = (long long)D * H * Wd, F = vox * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long o = i / F, f = i - o * F;
        const long long v = f / C;
        const int c = (int)(f - v * C);
        Wtf[o * F + hvp_ftf(v, c, D, H, Wd)] = Wres[i];
    }
}
int k_hvp_unpermute(alq_ctx *ctx, const float *Wres, float *Wtf, int Co, const View &in) {
    const long long total = (long long)Co * in.vox() * in.C;
    hipLaunchKernelGGL(hvp_unpermute_kernel, dim3(hgrid(total)), dim3(256), 0, ctx->stream, Wres, Wtf, in.D, in.H, in.W, in.C, total);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

}  // namespace alq
