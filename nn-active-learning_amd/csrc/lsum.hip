// Per-class layer sums of the multi-class Fisher query without parameter-sized rows (alq_class_layer_sums): the sum of all
// entries of d log p_j / d theta_t, per sample, class slot and parameterised layer - what shrink_gradient(..., 'sum')
// (NNAL_tools.py:784-796) takes of the gradient lists of NNAL.py:381-397.
//   With delta the masked cotangent of layer t's output, a its input, dsum / asum their channel sums:
//     conv (stride 1, SAME):  sum_x dsum[x] (box_k(asum)[x] + 1)
//     conv_transpose:         sum_q asum[q] sum_tau dsum[s q + tau - lo] + sum_p dsum[p]
//     fc:                     (sum delta) (sum a + 1)
//   All three are  S_j[n][t] = sum_x dsum_j[n, x] F_t[n, x]  with a field F_t that does not depend on the class:
//     F_t[p] = 1 + sum over the taps tau and input points q with s q + tau - lo = p of asum[q]
//   (a stride-1 conv is the case s = 1 with the taps mirrored: q = p + tap - lo_conv = p + (k - 1 - lo_conv) - tau), and for fc
//   the scalar sum a + 1.
//   * Field kernels: one launch per layer and CALL.  A workgroup owns a tile of the field's grid, puts the channel sums of
//     the input points the tile touches into LDS (zero outside the grid; split-concat inputs are two runs of one voxel row)
//     and adds the taps from there.  fp64 throughout and stored as fp64: 8 bytes per voxel beside the 8 C bytes per voxel
//     that every class sweep moves, and no rounding of F enters the sums.
//   * Sweep kernel: one launch per layer and CLASS SLOT inside the backward sweep, in the place of the ReLU-mask +
//     channel-sum launch.  It reads the cotangent once (16 bytes per lane, G lanes along the channels of a voxel, so a wave
//     instruction covers whole 128-byte lines), applies the ReLU mask in place (the backward-data launch below reads the
//     masked tensor), forms the voxel's channel sum in registers in fp64, multiplies by F and accumulates per lane in fp64.
//     Workgroup = a contiguous run of voxels of ONE sample; xor butterfly in the wave, four wave sums through LDS, one
//     partial per workgroup; the finish kernel adds a sample's partials in slab order and divides by |W_t| + |b_t|.  No
//     atomics: a row depends on its own sample only and has the same bits whatever the batch and from run to run.
#include <algorithm>

#include "alq_internal.h"

namespace alq {

namespace {

typedef float ls_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LS_THREADS = 256;
constexpr int LS_MAX_SLABS = 256;         // partials per sample and layer
constexpr size_t LS_MAX_LDS = 60 * 1024;  // staged channel sums of a field tile

__device__ inline double ls_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// 256-thread sum in a fixed order; valid in thread 0
__device__ inline double ls_block_sum(double v, double *sh /*[4]*/) {
    v = ls_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return threadIdx.x == 0 ? (sh[0] + sh[1]) + (sh[2] + sh[3]) : 0.0;
}

// the channels of one View, split concat included (voxel row r of the N-patch tensor)
struct LsView {
    const float *p;
    int cs, c0, C, split;
    long long delta;
    int vec;        // every run of channels is 16-byte aligned and a multiple of 4 long
};

LsView lsview(const View &v) {
    LsView d;
    d.p = v.p; d.cs = v.cs; d.c0 = v.c0; d.C = v.C; d.split = v.split; d.delta = v.delta;
    const int lens = v.split ? (v.split | (v.C - v.split)) : v.C;
    d.vec = (((v.cs | v.c0 | lens) & 3) == 0 && (v.delta & 3) == 0 && ((uintptr_t)v.p & 15) == 0) ? 1 : 0;
    return d;
}

__device__ inline double ls_run_sum(const float *q, int len, int vec) {
    double s = 0.0;
    if (vec) {
        for (int c = 0; c < len; c += 4) {
            const ls_f32x4 v = *reinterpret_cast<const ls_f32x4 *>(q + c);
            s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        }
    } else {
        for (int c = 0; c < len; ++c) s += (double)q[c];
    }
    return s;
}
__device__ inline double ls_chan_sum(const LsView &A, long long row) {
    if (A.split)
        return ls_run_sum(A.p + row * A.cs + A.c0, A.split, A.vec) + ls_run_sum(A.p + A.delta + row * A.cs, A.C - A.split, A.vec);
    return ls_run_sum(A.p + row * A.cs + A.c0, A.C, A.vec);
}

struct LsGeom {
    int I[3], O[3];          // input grid (points q), field grid (points p)
    int k[3], s[3], lo[3];   // p = s q + tau - lo
    int T[3], h[3], tiles[3];
};

__device__ inline int ls_floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// grid (tiles, N); F[n, p] = 1 + sum_{tau, q : s q + tau - lo = p} asum[n, q]
__global__ __launch_bounds__(LS_THREADS) void lsum_field_kernel(LsView A, LsGeom g, double *F) {
    extern __shared__ double ls_as[];      // [h0][h1][h2] channel sums of the input points of this tile
    const int n = blockIdx.y;
    int t = blockIdx.x;
    const int tx = t % g.tiles[2]; t /= g.tiles[2];
    const int ty = t % g.tiles[1];
    const int tz = t / g.tiles[1];
    const int p0[3] = {tz * g.T[0], ty * g.T[1], tx * g.T[2]};
    int qmin[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) qmin[d] = ls_floordiv(p0[d] + g.lo[d] - (g.k[d] - 1), g.s[d]);
    const long long ivox = (long long)g.I[0] * g.I[1] * g.I[2], ovox = (long long)g.O[0] * g.O[1] * g.O[2];
    const int halo = g.h[0] * g.h[1] * g.h[2];
    for (int i = threadIdx.x; i < halo; i += LS_THREADS) {
        int r = i;
        const int hx = r % g.h[2]; r /= g.h[2];
        const int hy = r % g.h[1];
        const int hz = r / g.h[1];
        const int qz = qmin[0] + hz, qy = qmin[1] + hy, qx = qmin[2] + hx;
        double v = 0.0;
        if ((unsigned)qz < (unsigned)g.I[0] && (unsigned)qy < (unsigned)g.I[1] && (unsigned)qx < (unsigned)g.I[2])
            v = ls_chan_sum(A, (long long)n * ivox + ((long long)qz * g.I[1] + qy) * g.I[2] + qx);
        ls_as[i] = v;
    }
    __syncthreads();
    const int tile = g.T[0] * g.T[1] * g.T[2];
    for (int i = threadIdx.x; i < tile; i += LS_THREADS) {
        int r = i;
        const int ix = r % g.T[2]; r /= g.T[2];
        const int iy = r % g.T[1];
        const int iz = r / g.T[1];
        const int pz = p0[0] + iz, py = p0[1] + iy, px = p0[2] + ix;
        if (pz >= g.O[0] || py >= g.O[1] || px >= g.O[2]) continue;
        double f = 1.0;
        for (int az = 0; az < g.k[0]; ++az) {
            const int mz = pz + g.lo[0] - az;
            if (mz < 0 || mz % g.s[0]) continue;
            const int qz = mz / g.s[0];
            if (qz >= g.I[0]) continue;
            for (int ay = 0; ay < g.k[1]; ++ay) {
                const int my = py + g.lo[1] - ay;
                if (my < 0 || my % g.s[1]) continue;
                const int qy = my / g.s[1];
                if (qy >= g.I[1]) continue;
                const double *row = ls_as + ((qz - qmin[0]) * g.h[1] + (qy - qmin[1])) * g.h[2];
                for (int ax = 0; ax < g.k[2]; ++ax) {
                    const int mx = px + g.lo[2] - ax;
                    if (mx < 0 || mx % g.s[2]) continue;
                    const int qx = mx / g.s[2];
                    if (qx < g.I[2]) f += row[qx - qmin[2]];
                }
            }
        }
        F[(long long)n * ovox + ((long long)pz * g.O[1] + py) * g.O[2] + px] = f;
    }
}

// fc: F[n] = 1 + sum of the layer's input; one workgroup per sample, thread t the elements t, t + 256, ..
__global__ __launch_bounds__(LS_THREADS) void lsum_field_fc_kernel(LsView A, int avox, double *F) {
    __shared__ double sh[4];
    const int n = blockIdx.x;
    double s = 0.0;
    if (A.split == 0 && A.cs == A.C) {          // one dense row per sample
        const long long len = (long long)avox * A.C;
        const float *q = A.p + (long long)n * avox * A.cs + A.c0;
        if (A.vec) {
            for (long long f = threadIdx.x * 4; f < len; f += LS_THREADS * 4) {
                const ls_f32x4 v = *reinterpret_cast<const ls_f32x4 *>(q + f);
                s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
            }
        } else {
            for (long long f = threadIdx.x; f < len; f += LS_THREADS) s += (double)q[f];
        }
    } else {
        for (int r = threadIdx.x; r < avox; r += LS_THREADS) s += ls_chan_sum(A, (long long)n * avox + r);
    }
    const double tot = ls_block_sum(s, sh);
    if (threadIdx.x == 0) F[n] = tot + 1.0;
}

// The class sweep of a spatial layer.  grid (nslab, N): workgroup (b, n) owns voxels [b * slab, (b + 1) * slab) of sample
// n; G lanes per voxel, 256 / G voxels per step.  part[n * nslab_max + b] = sum over its voxels of chansum(d) * F.
template <int G, bool VEC>
__global__ __launch_bounds__(LS_THREADS) void lsum_sweep_kernel(float *d, int cs, int c0, int C, const float *act, int acs, int ac0,
                                                                const double *F, int vox, int slab, double *part, int nslab_max) {
    __shared__ double sh[4];
    constexpr int VPB = LS_THREADS / G;
    const int n = blockIdx.y;
    const int v0 = blockIdx.x * slab, v1 = min(vox, v0 + slab);
    const int sub = threadIdx.x % G, vi = threadIdx.x / G;
    const long long base = (long long)n * vox;
    double acc = 0.0;
    for (int vb = v0; vb < v1; vb += VPB) {      // the same trip count for every lane: the shuffles below need all of them
        const int v = vb + vi;
        const bool on = v < v1;
        double s = 0.0;
        if (on) {
            float *row = d + (base + v) * cs + c0;
            const float *arow = act ? act + (base + v) * acs + ac0 : nullptr;
            if (VEC) {
                for (int c = sub * 4; c < C; c += 4 * G) {
                    ls_f32x4 q = *reinterpret_cast<ls_f32x4 *>(row + c);
                    if (arow) {
                        const ls_f32x4 m = *reinterpret_cast<const ls_f32x4 *>(arow + c);
                        q.x = m.x > 0.f ? q.x : 0.f;
                        q.y = m.y > 0.f ? q.y : 0.f;
                        q.z = m.z > 0.f ? q.z : 0.f;
                        q.w = m.w > 0.f ? q.w : 0.f;
                        *reinterpret_cast<ls_f32x4 *>(row + c) = q;
                    }
                    s += ((double)q.x + (double)q.y) + ((double)q.z + (double)q.w);
                }
            } else {
                for (int c = 0; c < C; ++c) {
                    float q = row[c];
                    if (arow) {
                        q = arow[c] > 0.f ? q : 0.f;
                        row[c] = q;
                    }
                    s += (double)q;
                }
            }
        }
#pragma unroll
        for (int o = 1; o < G; o <<= 1) s += __shfl_xor(s, o, 64);
        if (on && sub == 0) acc += s * F[base + v];
    }
    const double tot = ls_block_sum(acc, sh);
    if (threadIdx.x == 0) part[(long long)n * nslab_max + blockIdx.x] = tot;
}

// fc: two row sums and a product.  One workgroup per sample: mask in place, sum delta in fp64, times F[n].
__global__ __launch_bounds__(LS_THREADS) void lsum_sweep_fc_kernel(float *d, int C, const float *act, int vec, const double *F,
                                                                   double *part, int nslab_max) {
    __shared__ double sh[4];
    const int n = blockIdx.x;
    float *row = d + (long long)n * C;
    const float *arow = act ? act + (long long)n * C : nullptr;
    double s = 0.0;
    if (vec) {
        for (int c = threadIdx.x * 4; c < C; c += LS_THREADS * 4) {
            ls_f32x4 q = *reinterpret_cast<ls_f32x4 *>(row + c);
            if (arow) {
                const ls_f32x4 m = *reinterpret_cast<const ls_f32x4 *>(arow + c);
                q.x = m.x > 0.f ? q.x : 0.f;
                q.y = m.y > 0.f ? q.y : 0.f;
                q.z = m.z > 0.f ? q.z : 0.f;
                q.w = m.w > 0.f ? q.w : 0.f;
                *reinterpret_cast<ls_f32x4 *>(row + c) = q;
            }
            s += ((double)q.x + (double)q.y) + ((double)q.z + (double)q.w);
        }
    } else {
        for (int c = threadIdx.x; c < C; c += LS_THREADS) {
            float q = row[c];
            if (arow) {
                q = arow[c] > 0.f ? q : 0.f;
                row[c] = q;
            }
            s += (double)q;
        }
    }
    const double tot = ls_block_sum(s, sh);
    if (threadIdx.x == 0) part[(long long)n * nslab_max] = tot * F[n];
}

struct LsSlabs { int n[64]; };

// g[n][j][t] = (sum of layer t's partials of sample n, in slab order) / sizes[t]
__global__ void lsum_finish_kernel(const double *part, LsSlabs ns, int nslab_max, int max_batch, const double *sizes, int N, int L,
                                   int J, int j, double *g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * L) return;
    const int n = i / L, t = i - n * L;
    const double *p = part + ((long long)t * max_batch + n) * nslab_max;
    double s = 0.0;
    for (int b = 0; b < ns.n[t]; ++b) s += p[b];
    g[((long long)n * J + j) * L + t] = s / sizes[t];
}

// flag[0] = 1 when an entry of cls [count] lies outside [0, c)
__global__ void lsum_check_classes_kernel(const int *cls, int count, int c, int *flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count && (cls[i] < 0 || cls[i] >= c)) flag[0] = 1;
}

int lanes_of(int C) {
    const int q = C / 4;
    int g = 1;
    while (g < 8 && q % (g * 2) == 0) g *= 2;
    return g;
}

// the field's geometry for one layer: conv as the mirrored stride-1 case
LsGeom field_geom(const View &in, const View &out, const int k[3], const int s[3], const int lo[3], bool convt) {
    LsGeom g{};
    g.I[0] = in.D; g.I[1] = in.H; g.I[2] = in.W;
    g.O[0] = out.D; g.O[1] = out.H; g.O[2] = out.W;
    for (int d = 0; d < 3; ++d) {
        g.k[d] = k[d];
        g.s[d] = convt ? s[d] : 1;
        g.lo[d] = convt ? lo[d] : k[d] - 1 - lo[d];
    }
    if (out.D > 1) { g.T[0] = std::min(out.D, 4); g.T[1] = std::min(out.H, 8); g.T[2] = std::min(out.W, 8); }
    else { g.T[0] = 1; g.T[1] = std::min(out.H, 16); g.T[2] = std::min(out.W, 16); }
    for (int d = 0; d < 3; ++d) {
        g.h[d] = (g.T[d] + g.k[d] - 2) / g.s[d] + 2;
        g.tiles[d] = (g.O[d] + g.T[d] - 1) / g.T[d];
    }
    return g;
}

}  // namespace

int lsum_slabs(const View &dout, bool isfc, int *slab_out) {
    if (isfc) { if (slab_out) *slab_out = 1; return 1; }
    const bool vec = ((dout.cs | dout.c0 | dout.C) & 3) == 0;
    const int vpb = LS_THREADS / (vec ? lanes_of(dout.C) : 1);
    const long long vox = dout.vox();
    long long slab = 2 * vpb;
    if ((vox + slab - 1) / slab > LS_MAX_SLABS) {
        slab = (vox + LS_MAX_SLABS - 1) / LS_MAX_SLABS;
        slab = (slab + vpb - 1) / vpb * vpb;
    }
    if (slab_out) *slab_out = (int)slab;
    return (int)((vox + slab - 1) / slab);
}

int k_lsum_field(alq_ctx *ctx, const View &in, const View &out, const int k[3], const int s[3], const int lo[3], int type, int N,
                 double *F) {
    const LsView A = lsview(in);
    if (type == ALQ_FC) {
        hipLaunchKernelGGL(lsum_field_fc_kernel, dim3((unsigned)N), dim3(LS_THREADS), 0, ctx->stream, A, (int)in.vox(), F);
        ALQ_HIP(hipGetLastError());
        return ALQ_OK;
    }
    const LsGeom g = field_geom(in, out, k, s, lo, type == ALQ_CONVT);
    const size_t lds = (size_t)g.h[0] * g.h[1] * g.h[2] * sizeof(double);
    ALQ_REQUIRE(lds <= LS_MAX_LDS, ALQ_EUNSUPPORTED, "alq_class_layer_sums: a %d x %d x %d window does not fit the staged field tile",
                k[0], k[1], k[2]);
    ProfScope ps(ctx, PROF_REDUCE, 0);
    hipLaunchKernelGGL(lsum_field_kernel, dim3((unsigned)(g.tiles[0] * g.tiles[1] * g.tiles[2]), (unsigned)N), dim3(LS_THREADS), lds,
                       ctx->stream, A, g, F);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

// dout: the layer's output cotangent (flat [N, C] for fc), act: its output when the layer has a ReLU, else null
int k_lsum_sweep(alq_ctx *ctx, const View &dout, const View *act, bool isfc, const double *F, int N, double *part, int nslab_max) {
    ProfScope ps(ctx, PROF_REDUCE, 0);
    const float *ap = act ? act->p : nullptr;
    if (isfc) {
        ALQ_REQUIRE(dout.cs == dout.C && dout.c0 == 0 && (!act || (act->cs == dout.C && act->c0 == 0)), ALQ_EUNSUPPORTED,
                    "alq_class_layer_sums: strided fc cotangent");
        const int vec = ((dout.C & 3) == 0 && ((uintptr_t)dout.p & 15) == 0 && ((uintptr_t)ap & 15) == 0) ? 1 : 0;
        hipLaunchKernelGGL(lsum_sweep_fc_kernel, dim3((unsigned)N), dim3(LS_THREADS), 0, ctx->stream, dout.p, dout.C, ap, vec, F, part,
                           nslab_max);
        ALQ_HIP(hipGetLastError());
        return ALQ_OK;
    }
    int slab = 0;
    const int nslab = lsum_slabs(dout, false, &slab);
    ALQ_REQUIRE(nslab <= nslab_max, ALQ_EINVAL, "alq_class_layer_sums: %d slabs, room for %d", nslab, nslab_max);
    const int acs = act ? act->cs : 0, ac0 = act ? act->c0 : 0;
    const bool vec = ((dout.cs | dout.c0 | dout.C | acs | ac0) & 3) == 0 && ((uintptr_t)dout.p & 15) == 0 && ((uintptr_t)ap & 15) == 0;
    // (lsum_slabs sized the slab for the lanes of the aligned form; the scalar form runs one lane per voxel on any slab)
    const int G = vec ? lanes_of(dout.C) : 1;
    const dim3 grid((unsigned)nslab, (unsigned)N);
    const int vox = (int)dout.vox();
#define ALQ_LS(GV, VV) \
    hipLaunchKernelGGL((lsum_sweep_kernel<GV, VV>), grid, dim3(LS_THREADS), 0, ctx->stream, dout.p, dout.cs, dout.c0, dout.C, ap, acs, \
                       ac0, F, vox, slab, part, nslab_max)
    if (!vec) ALQ_LS(1, false);
    else switch (G) {
        case 1: ALQ_LS(1, true); break;
        case 2: ALQ_LS(2, true); break;
        case 4: ALQ_LS(4, true); break;
        default: ALQ_LS(8, true); break;
    }
#undef ALQ_LS
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int k_lsum_finish(alq_ctx *ctx, const double *part, const int *h_nslab, int nslab_max, int max_batch, const double *sizes, int N, int L,
                  int J, int j, double *g) {
    LsSlabs ns{};
    for (int t = 0; t < L; ++t) ns.n[t] = h_nslab[t];
    hipLaunchKernelGGL(lsum_finish_kernel, dim3((unsigned)((N * L + 255) / 256)), dim3(256), 0, ctx->stream, part, ns, nslab_max,
                       max_batch, sizes, N, L, J, j, g);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int k_lsum_check_classes(alq_ctx *ctx, const int *d_cls, int count, int c, int *d_flag) {
    hipLaunchKernelGGL(lsum_check_classes_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, d_cls, count, c,
                       d_flag);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // namespace alq
