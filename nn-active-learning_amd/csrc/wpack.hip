// Device-side weight packing for wide fully connected layers (alq_model_set_weights_device): everything the host packers of
// weights.hip / fcgemm.hip derive from an fc layer's TF weights W[o][f_tf], computed from a DEVICE copy with the same bits.
//
//   wpack_stats_kernel    bwd_l1 = max_f sum_o |W[o][f]| (fp64, rows in the host's order: one thread per column, which is also
//                         the coalesced order) and max |W| (the fp16 pairs' scale exponent) in one pass over W
//   wpack_permute_kernel  Wp[o][f_mem] = W[o][f_tf]: the flatten permutation f_tf = ((c*W+w)*H+h)*D+d -> f_mem = ((d*H+h)*W+w)*C+c
//                         is, per row, the transpose [C][R] -> [R'][C] (R = W*H*D, r' = r with its three axes reversed): 32 x 32
//                         LDS tiles, 128-byte runs on either global side
//   wpack_fc_kernel       from Wp to fcgemm's packed layout [feature tile][k-step][piece][k-group q][feature row][8 along k], bf16
//                         triples and (optionally) fp16 pairs of w 2^w_exp; a workgroup stages one 64 (features) x 32 (k) block
//                         through LDS with coalesced loads, thread (q, row) then holds the block's 8 values along k and writes
//                         ONE 16-byte store per piece at (piece * 256 + thread) * 16: the packed layout's own order
//
// Splits: bf16 by the host's integer round-to-nearest-even and an fp32 subtraction per piece; fp16 by the hardware conversion
// (RNE, subnormals kept, like the host's _Float16 cast) after an exact scaling by 2^w_exp.  No multiply-add can be contracted in
// here (sums of |w|, subtractions, scalings by powers of two), contraction is switched off all the same.
#include "alq_internal.h"

#include <cmath>

#pragma clang fp contract(off)

namespace alq {

typedef float wp_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned wp_u32x4 __attribute__((ext_vector_type(4)));

constexpr int WP_BN = 64, WP_BK = 32;      // fcgemm.hip's FC_BN / FC_BK (the packed block: 64 feature rows x 32 along k)
constexpr int WP_KS = 4;                   // k-steps a workgroup packs one after the other

// scal: [0] (8 bytes) bits of max_f sum_o |W[o][f]| as fp64, [1] low word: bits of max |W| as fp32.  Non-negative IEEE values order
// like their bit patterns; a NaN never wins (the host's std::max(best, x) keeps `best` when x is a NaN).
__global__ __launch_bounds__(64) void wpack_stats_kernel(const float *__restrict__ W, int Co, long long F, unsigned long long *scal) {
    __shared__ unsigned long long s_l1;
    __shared__ unsigned s_amax;
    if (threadIdx.x == 0) { s_l1 = 0ull; s_amax = 0u; }
    __syncthreads();
    const long long f = (long long)blockIdx.x * 64 + threadIdx.x;
    if (f < F) {
        const float *p = W + f;
        double s = 0.0;
        float am = 0.f;
#pragma unroll 8
        for (int o = 0; o < Co; ++o) {
            const float a = __builtin_fabsf(p[(size_t)o * F]);
            s += (double)a;
            am = (am < a) ? a : am;
        }
        if (s == s) atomicMax(&s_l1, (unsigned long long)__builtin_bit_cast(unsigned long long, s));
        atomicMax(&s_amax, __builtin_bit_cast(unsigned, am));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(scal, s_l1);
        atomicMax(reinterpret_cast<unsigned *>(scal + 1), s_amax);
    }
}

// grid (tiles of R x tiles of C, Co), block (32, 8)
__global__ __launch_bounds__(256) void wpack_permute_kernel(const float *__restrict__ W, float *__restrict__ Wp, int D, int H, int Wd, int C) {
    __shared__ float tile[32][33];
    const int R = Wd * H * D;
    const int rt = (R + 31) / 32;
    const int r0 = (blockIdx.x % rt) * 32, c0 = (blockIdx.x / rt) * 32;
    const size_t row = (size_t)blockIdx.y * (size_t)R * C;
    const int tx = threadIdx.x, ty = threadIdx.y;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (c < C && r < R) tile[ty + 8 * i][tx] = W[row + (size_t)c * R + r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        if (c < C && r < R) {
            const int d = r % D, h = (r / D) % H, w = r / (D * H);       // r = (w*H + h)*D + d
            const int rp = (d * H + h) * Wd + w;
            Wp[row + (size_t)rp * C + c] = tile[tx][ty + 8 * i];
        }
    }
}

// the host's fc_bf16_rne / fc_bf16_to_f (fcgemm.hip) on a register
__device__ inline unsigned wp_bf16_split(float &w) {
    unsigned u = __builtin_bit_cast(unsigned, w);
    u += 0x7fffu + ((u >> 16) & 1u);
    const unsigned hb = u >> 16;
    w -= __builtin_bit_cast(float, hb << 16);
    return hb;
}

// frexp's exponent of the fp32 value with (non-negative) bits b: b in [2^(ex-1), 2^ex); 0 for b = 0
__device__ inline int wp_frexp_exp(unsigned b) {
    if (b == 0u) return 0;
    const int e = (int)(b >> 23);
    if (e > 0) return e - 126;
    return (31 - __builtin_clz(b)) - 148;       // subnormal: mantissa m 2^-149, top bit of m at position p -> [2^(p-149), 2^(p-148))
}

// One workgroup: feature tile nt = blockIdx.y, k-steps [blockIdx.x * WP_KS, + WP_KS).  The B matrix [K][N] of the GEMM is read from
// Wp: KMAJOR = false: B[k][n] = Wp[n * ld + k] (the forward orientation: rows = output features, contiguous along k);
// KMAJOR = true: B[k][n] = Wp[k * ld + n] (the backward orientation: the [o][f_mem] rows as they are).  Wp is this library's own
// allocation (256-byte aligned) and ld, K, N are multiples of 32: the 16-byte loads are aligned.
template <bool KMAJOR>
__global__ __launch_bounds__(256) void wpack_fc_kernel(const float *__restrict__ Wp, long long ld, int K, int N, unsigned short *__restrict__ out3,
                                                       unsigned short *__restrict__ out16, const unsigned long long *scal) {
    __shared__ __attribute__((aligned(16))) float tile[KMAJOR ? WP_BK : WP_BN][KMAJOR ? WP_BN : WP_BK + 1];
    const int tid = threadIdx.x;
    const int q = tid >> 6, r = tid & 63;
    const int nt = blockIdx.y, nks = K / WP_BK;
    int w_exp = 0;
    if (out16) w_exp = 14 - wp_frexp_exp(*reinterpret_cast<const unsigned *>(scal + 1));
    for (int s = 0; s < WP_KS; ++s) {
        const int ks = blockIdx.x * WP_KS + s;
        if (ks >= nks) break;
        if (s) __syncthreads();
        if constexpr (KMAJOR) {
            // 32 rows (k) of 64 floats: 16 threads per row, two passes
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int kr = (tid >> 4) + 16 * i, c4 = (tid & 15) * 4;
                const wp_f32x4 v = *reinterpret_cast<const wp_f32x4 *>(Wp + (size_t)(ks * WP_BK + kr) * ld + (size_t)nt * WP_BN + c4);
                *reinterpret_cast<wp_f32x4 *>(&tile[kr][c4]) = v;
            }
        } else {
            // 64 rows (features) of 32 floats: 8 threads per row, two passes
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int nr = (tid >> 3) + 32 * i, c4 = (tid & 7) * 4;
                const wp_f32x4 v = *reinterpret_cast<const wp_f32x4 *>(Wp + (size_t)(nt * WP_BN + nr) * ld + (size_t)ks * WP_BK + c4);
                tile[nr][c4] = v.x; tile[nr][c4 + 1] = v.y; tile[nr][c4 + 2] = v.z; tile[nr][c4 + 3] = v.w;
            }
        }
        __syncthreads();
        float w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = KMAJOR ? tile[q * 8 + j][r] : tile[r][q * 8 + j];
        const size_t blk = (size_t)nt * nks + ks;
        if (out16) {
            unsigned hb[8], lb[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float ws = __builtin_ldexpf(w[j], w_exp);
                const _Float16 h = (_Float16)ws;
                const _Float16 l = (_Float16)(ws - (float)h);
                hb[j] = (unsigned)__builtin_bit_cast(unsigned short, h);
                lb[j] = (unsigned)__builtin_bit_cast(unsigned short, l);
            }
            wp_u32x4 *o = reinterpret_cast<wp_u32x4 *>(out16) + blk * 2 * 256 + tid;
            o[0] = wp_u32x4{hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16), hb[4] | (hb[5] << 16), hb[6] | (hb[7] << 16)};
            o[256] = wp_u32x4{lb[0] | (lb[1] << 16), lb[2] | (lb[3] << 16), lb[4] | (lb[5] << 16), lb[6] | (lb[7] << 16)};
        }
        wp_u32x4 *o3 = reinterpret_cast<wp_u32x4 *>(out3) + blk * 3 * 256 + tid;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            unsigned b[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = wp_bf16_split(w[j]);
            o3[p * 256] = wp_u32x4{b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16)};
        }
    }
}

int wpack_stats(alq_ctx *ctx, const float *d_W, int Co, long long F, void *d_scal) {
    ALQ_HIP(hipMemsetAsync(d_scal, 0, 16, ctx->stream));
    hipLaunchKernelGGL(wpack_stats_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, ctx->stream, d_W, Co, F,
                       reinterpret_cast<unsigned long long *>(d_scal));
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int wpack_permute(alq_ctx *ctx, const float *d_W, float *d_Wp, int Co, int D, int H, int Wd, int C) {
    const long long F = (long long)D * H * Wd * C;
    const int big = (D > 1) + (H > 1) + (Wd > 1) + (C > 1);
    if (big <= 1) {      // at most one axis longer than 1: both orders are the same
        ALQ_HIP(hipMemcpyAsync(d_Wp, d_W, (size_t)Co * F * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return ALQ_OK;
    }
    const int R = Wd * H * D;
    ALQ_REQUIRE(Co <= 65535, ALQ_EUNSUPPORTED, "wpack_permute: %d output features", Co);
    hipLaunchKernelGGL(wpack_permute_kernel, dim3((unsigned)(((R + 31) / 32) * ((C + 31) / 32)), (unsigned)Co), dim3(32, 8), 0, ctx->stream,
                       d_W, d_Wp, D, H, Wd, C);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

// d_W3: K * N * 3 bf16, d_W16 (or null): K * N * 2 fp16; kmajor: B[k][n] = Wp[k * ld + n], else Wp[n * ld + k]
int wpack_fc(alq_ctx *ctx, const float *d_Wp, long long ld, int K, int N, int kmajor, void *d_W3, void *d_W16, const void *d_scal) {
    ALQ_REQUIRE(K % WP_BK == 0 && N % WP_BN == 0 && ld % 4 == 0, ALQ_EINVAL, "wpack_fc: K = %d, N = %d", K, N);
    const int nks = K / WP_BK;
    const dim3 grid((unsigned)((nks + WP_KS - 1) / WP_KS), (unsigned)(N / WP_BN));
    ALQ_REQUIRE(grid.y <= 65535, ALQ_EUNSUPPORTED, "wpack_fc: N = %d", N);
    if (kmajor)
        hipLaunchKernelGGL((wpack_fc_kernel<true>), grid, dim3(256), 0, ctx->stream, d_Wp, ld, K, N, reinterpret_cast<unsigned short *>(d_W3),
                           reinterpret_cast<unsigned short *>(d_W16), reinterpret_cast<const unsigned long long *>(d_scal));
    else
        hipLaunchKernelGGL((wpack_fc_kernel<false>), grid, dim3(256), 0, ctx->stream, d_Wp, ld, K, N, reinterpret_cast<unsigned short *>(d_W3),
                           reinterpret_cast<unsigned short *>(d_W16), reinterpret_cast<const unsigned long long *>(d_scal));
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // namespace alq
