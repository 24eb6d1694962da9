// Slice queries of a fully-convolutional model: per-voxel uncertainty folded into per-slice sums on the device (no reference
// counterpart: the reference stops at the (c, h, w, z) volumes of eval_utils.full_slice_segment, eval_utils.py:176-198).
// The posteriors are read where the library writes them: class-major, post [c, R] fp32, R = n_slices V rows.
//   * sq_entropy<C>: h(p) = -sum_j p_j log p_j in fp64, a term with p_j <= 0 exactly 0.  The ONE statement of the entropy: both
//     kernels call it (the file is built without contraction into fused multiply-adds), so h of the same doubles is the same
//     double in both - BALD of a single pass is exactly 0.
//   * unc_accumulate_kernel: one dropout pass into the running sums, sum_p [c, R] (+)= (double)p and sum_h [R] (+)= h(p); a sum of
//     fp32 values in fp64 is exact.  A lane owns 4 consecutive rows: one 16-byte load per class plane, 16-byte loads / stores of
//     the fp64 planes.  Grid-stride.
//   * slice_scores_kernel: the rows of the call as one flat sequence, swept SQ_SWEEP = 1024 rows at a time by a workgroup (a lane
//     owns 4 consecutive rows of the sweep, as above), whatever V is: a sweep may hold the end of one slice and the start of
//     the next, or a thousand slices.  The lanes put the values (+0.0 outside the ROI) and the ROI flags of their rows into LDS;
//     the part of a slice that lies in the sweep - a segment - is summed by a team of T lanes of one wave (T a power of two
//     from V alone: member m takes elements m, m + T, ..., then a shuffle tree), and the team's first lane stores (sum, count)
//     as ONE partial at [slice][sweep - first sweep of the slice].  Every partial has exactly one writer: no atomics, no memset.
//   * slice_finish_kernel: a thread per slice adds the partials of its slice in ascending order.
// The order of every addition depends on (V, n_slices) alone: bit-identical from run to run.
// LDS image of a sweep: element e = 4 lane + i lies at word i * SQ_PLANE + lane - the lanes write consecutive words, and
// the planes are padded by 8 doubles (16 banks), so that the 32 consecutive elements a half wave of a team reads lie on 32
// different 8-byte bank pairs.
#include <algorithm>
#include <cstdint>

#include "alq_internal.h"

namespace alq {

namespace {

constexpr int SQ_THREADS = 256;
constexpr int SQ_VEC = 4;                          // rows of a lane: one 16-byte load per fp32 plane
constexpr int SQ_SWEEP = SQ_THREADS * SQ_VEC;      // rows of a workgroup sweep
constexpr int SQ_PLANE = SQ_THREADS + 8;
constexpr int SQ_MIN_C = 2, SQ_MAX_C = 8;          // the range of the dense head (dense.hip)
constexpr int64_t SQ_MAX_ROWS = (int64_t)1 << 31;

struct SqPartial {
    double sum;
    long long cnt;
};

template <int C>
__device__ inline double sq_entropy(const double (&p)[C]) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        if (!(p[j] <= 0.0)) acc += p[j] * log(p[j]);
    }
    return 0.0 - acc;
}

// rows r .. r + 3 of a plane of R rows; vec: R % 4 == 0 and the plane 16-byte aligned (r is a multiple of 4: all four rows exist
// when the first does).  Rows past the end read as 0.
__device__ inline void sq_load4(const float *p, long long r, long long R, bool vec, float (&v)[SQ_VEC]) {
    if (vec) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < R) q = *reinterpret_cast<const float4 *>(p + r);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < SQ_VEC; ++i) v[i] = r + i < R ? p[r + i] : 0.f;
    }
}

__device__ inline void sq_load4(const double *p, long long r, long long R, bool vec, double (&v)[SQ_VEC]) {
    if (vec) {
        double2 a = make_double2(0., 0.), b = a;
        if (r < R) {
            a = *reinterpret_cast<const double2 *>(p + r);
            b = *reinterpret_cast<const double2 *>(p + r + 2);
        }
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
#pragma unroll
        for (int i = 0; i < SQ_VEC; ++i) v[i] = r + i < R ? p[r + i] : 0.;
    }
}

__device__ inline void sq_store4(double *p, long long r, long long R, bool vec, const double (&v)[SQ_VEC]) {
    if (vec) {
        if (r < R) {
            *reinterpret_cast<double2 *>(p + r) = make_double2(v[0], v[1]);
            *reinterpret_cast<double2 *>(p + r + 2) = make_double2(v[2], v[3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < SQ_VEC; ++i)
            if (r + i < R) p[r + i] = v[i];
    }
}

template <int C>
__global__ __launch_bounds__(SQ_THREADS) void unc_accumulate_kernel(const float *__restrict__ post, long long R, int first, int vec,
                                                                    double *__restrict__ sum_p, double *__restrict__ sum_h) {
    const long long groups = (R + SQ_VEC - 1) / SQ_VEC;
    const long long stride = (long long)gridDim.x * SQ_THREADS;
    for (long long g = (long long)blockIdx.x * SQ_THREADS + threadIdx.x; g < groups; g += stride) {
        const long long r = g * SQ_VEC;
        float v[C][SQ_VEC];
#pragma unroll
        for (int j = 0; j < C; ++j) sq_load4(post + (long long)j * R, r, R, vec != 0, v[j]);
        double h[SQ_VEC];
        if (sum_h) {
#pragma unroll
            for (int i = 0; i < SQ_VEC; ++i) {
                double p[C];
#pragma unroll
                for (int j = 0; j < C; ++j) p[j] = (double)v[j][i];
                h[i] = sq_entropy<C>(p);
            }
        }
#pragma unroll
        for (int j = 0; j < C; ++j) {
            double s[SQ_VEC];
            if (first) {
#pragma unroll
                for (int i = 0; i < SQ_VEC; ++i) s[i] = (double)v[j][i];
            } else {
                sq_load4(sum_p + (long long)j * R, r, R, vec != 0, s);
#pragma unroll
                for (int i = 0; i < SQ_VEC; ++i) s[i] += (double)v[j][i];
            }
            sq_store4(sum_p + (long long)j * R, r, R, vec != 0, s);
        }
        if (sum_h) {
            if (!first) {
                double s[SQ_VEC];
                sq_load4(sum_h, r, R, vec != 0, s);
#pragma unroll
                for (int i = 0; i < SQ_VEC; ++i) h[i] = s[i] + h[i];
            }
            sq_store4(sum_h, r, R, vec != 0, h);
        }
    }
}

struct SqArgs {
    const double *sum_p, *sum_h;      // MC kinds; sum_h null: MC-entropy
    const float *f32;                 // entropy: post [c, R]; mean: map [R]
    const unsigned char *roi;         // [R] or null
    SqPartial *part;                  // [n_slices][P]
    unsigned R, V;                    // R < 2^31
    int P;                            // partials per slice
    int tshift;                       // log2 of the team size
    int vec, roi_vec;                 // planes / ROI readable 16 / 4 bytes at a time
    double T;
};

enum { SQ_SRC_F32 = 0, SQ_SRC_SUMS = 1, SQ_SRC_MEAN = 2 };

// the values of rows r .. r + 3 (rows outside the ROI or past the end: +0.0, nothing evaluated)
template <int C, int SRC>
__device__ inline void sq_values(const SqArgs &a, long long r, const bool (&in)[SQ_VEC], double (&val)[SQ_VEC]) {
    const long long R = a.R;
    if (SRC == SQ_SRC_MEAN) {
        float v[SQ_VEC];
        sq_load4(a.f32, r, R, a.vec != 0, v);
#pragma unroll
        for (int i = 0; i < SQ_VEC; ++i) val[i] = in[i] ? (double)v[i] : 0.0;
        return;
    }
    double q[C][SQ_VEC];
    if (SRC == SQ_SRC_F32) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            float v[SQ_VEC];
            sq_load4(a.f32 + (long long)j * R, r, R, a.vec != 0, v);
#pragma unroll
            for (int i = 0; i < SQ_VEC; ++i) q[j][i] = (double)v[i];
        }
    } else {
#pragma unroll
        for (int j = 0; j < C; ++j) sq_load4(a.sum_p + (long long)j * R, r, R, a.vec != 0, q[j]);
    }
    double sh[SQ_VEC] = {0., 0., 0., 0.};
    if (SRC == SQ_SRC_SUMS && a.sum_h) sq_load4(a.sum_h, r, R, a.vec != 0, sh);
#pragma unroll
    for (int i = 0; i < SQ_VEC; ++i) {
        val[i] = 0.0;
        if (in[i]) {
            double p[C];
#pragma unroll
            for (int j = 0; j < C; ++j) p[j] = SRC == SQ_SRC_SUMS ? q[j][i] / a.T : q[j][i];
            const double h = sq_entropy<C>(p);
            val[i] = (SRC == SQ_SRC_SUMS && a.sum_h) ? h - sh[i] / a.T : h;
        }
    }
}

template <int C, int SRC>
__global__ __launch_bounds__(SQ_THREADS) void slice_scores_kernel(SqArgs a) {
    __shared__ double s_val[SQ_VEC * SQ_PLANE];
    __shared__ int s_inc[SQ_VEC * SQ_PLANE];
    const unsigned tid = threadIdx.x;
    const unsigned sweeps = (a.R + SQ_SWEEP - 1) / SQ_SWEEP;
    const unsigned tsize = 1u << a.tshift, member = tid & (tsize - 1), team = tid >> a.tshift, teams = SQ_THREADS >> a.tshift;
    for (unsigned w = blockIdx.x; w < sweeps; w += gridDim.x) {
        const unsigned w0 = w * SQ_SWEEP, w1 = min(w0 + (unsigned)SQ_SWEEP, a.R);      // (w0 + 1024 <= 2^31 + 1023: no wrap)
        const unsigned r = w0 + tid * SQ_VEC;
        bool in[SQ_VEC];
        if (!a.roi) {
#pragma unroll
            for (int i = 0; i < SQ_VEC; ++i) in[i] = r + i < a.R;
        } else if (a.roi_vec) {
            const unsigned m = r < a.R ? *reinterpret_cast<const unsigned *>(a.roi + r) : 0u;
#pragma unroll
            for (int i = 0; i < SQ_VEC; ++i) in[i] = ((m >> (8 * i)) & 255u) != 0;
        } else {
#pragma unroll
            for (int i = 0; i < SQ_VEC; ++i) in[i] = r + i < a.R && a.roi[r + i] != 0;
        }
        double val[SQ_VEC];
        sq_values<C, SRC>(a, (long long)r, in, val);
#pragma unroll
        for (int i = 0; i < SQ_VEC; ++i) {
            s_val[i * SQ_PLANE + tid] = val[i];
            s_inc[i * SQ_PLANE + tid] = in[i] ? 1 : 0;
        }
        __syncthreads();
        // the segments of this sweep: slices s_lo .. s_hi, one team each (a team lies inside one wave and stays together)
        const unsigned s_lo = w0 / a.V, s_hi = (w1 - 1) / a.V;
        for (unsigned s = s_lo + team; s <= s_hi; s += teams) {
            const unsigned long long b0 = (unsigned long long)s * a.V, b1 = b0 + a.V;
            const unsigned lo = b0 > w0 ? (unsigned)(b0 - w0) : 0u;
            const unsigned hi = b1 < w1 ? (unsigned)(b1 - w0) : w1 - w0;
            double acc = 0.0;
            int cnt = 0;
            for (unsigned e = lo + member; e < hi; e += tsize) {
                const unsigned at = (e & 3u) * SQ_PLANE + (e >> 2);
                acc += s_val[at];
                cnt += s_inc[at];
            }
            for (unsigned off = tsize >> 1; off >= 1; off >>= 1) {
                acc += __shfl_xor(acc, (int)off);
                cnt += __shfl_xor(cnt, (int)off);
            }
            if (member == 0) {
                SqPartial pt;
                pt.sum = acc;
                pt.cnt = cnt;
                a.part[(unsigned long long)s * a.P + (w - (unsigned)(b0 / SQ_SWEEP))] = pt;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SQ_THREADS) void slice_finish_kernel(const SqPartial *__restrict__ part, unsigned n_slices, unsigned V, int P,
                                                                  double *__restrict__ scores, long long *__restrict__ counts) {
    const unsigned s = blockIdx.x * SQ_THREADS + threadIdx.x;
    if (s >= n_slices) return;
    const unsigned long long b0 = (unsigned long long)s * V;
    const unsigned n = (unsigned)((b0 + V - 1) / SQ_SWEEP - b0 / SQ_SWEEP) + 1;
    double acc = 0.0;
    long long cnt = 0;
    for (unsigned k = 0; k < n; ++k) {
        const SqPartial pt = part[(unsigned long long)s * P + k];
        acc += pt.sum;
        cnt += pt.cnt;
    }
    scores[s] = acc;
    counts[s] = cnt;
}

// the sweeps a slice of V rows can meet, wherever it starts
int sq_partials(int64_t V) { return (int)((V + SQ_SWEEP - 2) / SQ_SWEEP) + 1; }

int sq_tshift(int64_t V) {
    int t = 0;
    while (t < 6 && ((int64_t)16 << t) < V) ++t;      // a member adds about 16 elements of a long segment
    return t;
}

bool sq_aligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

// the context's partials, grown by doubling; a buffer that was outgrown may still be read by a queued launch, so it lives on
// until the context goes (no free, no synchronisation here)
int sq_reserve(alq_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->sq_part_bytes) return ALQ_OK;
    size_t want = std::max<size_t>(bytes, ctx->sq_part_bytes * 2);
    void *p = nullptr;
    ALQ_HIP(hipMalloc(&p, want));
    if (ctx->sq_part) ctx->sq_retired.push_back(ctx->sq_part);
    ctx->sq_part = p;
    ctx->sq_part_bytes = want;
    return ALQ_OK;
}

template <int SRC>
void sq_launch_c(int c, dim3 grid, hipStream_t st, const SqArgs &a) {
    switch (c) {
    case 2: hipLaunchKernelGGL((slice_scores_kernel<2, SRC>), grid, dim3(SQ_THREADS), 0, st, a); break;
    case 3: hipLaunchKernelGGL((slice_scores_kernel<3, SRC>), grid, dim3(SQ_THREADS), 0, st, a); break;
    case 4: hipLaunchKernelGGL((slice_scores_kernel<4, SRC>), grid, dim3(SQ_THREADS), 0, st, a); break;
    case 5: hipLaunchKernelGGL((slice_scores_kernel<5, SRC>), grid, dim3(SQ_THREADS), 0, st, a); break;
    case 6: hipLaunchKernelGGL((slice_scores_kernel<6, SRC>), grid, dim3(SQ_THREADS), 0, st, a); break;
    case 7: hipLaunchKernelGGL((slice_scores_kernel<7, SRC>), grid, dim3(SQ_THREADS), 0, st, a); break;
    default: hipLaunchKernelGGL((slice_scores_kernel<8, SRC>), grid, dim3(SQ_THREADS), 0, st, a); break;
    }
}

}  // namespace

}  // namespace alq

using namespace alq;

extern "C" {

int alq_slice_scores_geometry(int c, int64_t n_slices, int64_t V, int64_t *out) {
    ALQ_REQUIRE(out && n_slices >= 1 && V >= 1, ALQ_EINVAL, "alq_slice_scores_geometry: null argument, no slices or no voxels");
    ALQ_REQUIRE(c >= SQ_MIN_C && c <= SQ_MAX_C, ALQ_EUNSUPPORTED, "alq_slice_scores_geometry: %d classes (%d .. %d)", c, SQ_MIN_C, SQ_MAX_C);
    ALQ_REQUIRE(n_slices < SQ_MAX_ROWS && V < SQ_MAX_ROWS && n_slices * V < SQ_MAX_ROWS, ALQ_EUNSUPPORTED,
                "alq_slice_scores_geometry: %lld x %lld rows (fewer than 2^31)", (long long)n_slices, (long long)V);
    out[0] = SQ_THREADS;
    out[1] = SQ_SWEEP;
    out[2] = ALQ_SQ_MAX_BLOCKS;
    out[3] = sq_partials(V);
    return ALQ_OK;
}

int alq_unc_accumulate(alq_ctx *ctx, const float *d_post, int c, int64_t R, int first, double *d_sum_p, double *d_sum_h) {
    ALQ_REQUIRE(ctx && d_post && d_sum_p, ALQ_EINVAL, "alq_unc_accumulate: null argument");
    ALQ_REQUIRE(R >= 1, ALQ_EINVAL, "alq_unc_accumulate: R = %lld", (long long)R);
    ALQ_REQUIRE(sq_aligned(d_post, 4) && sq_aligned(d_sum_p, 8) && sq_aligned(d_sum_h, 8), ALQ_EINVAL,
                "alq_unc_accumulate: a pointer is not aligned to its element");
    ALQ_REQUIRE(c >= SQ_MIN_C && c <= SQ_MAX_C, ALQ_EUNSUPPORTED, "alq_unc_accumulate: %d classes (%d .. %d)", c, SQ_MIN_C, SQ_MAX_C);
    ALQ_REQUIRE(R < SQ_MAX_ROWS, ALQ_EUNSUPPORTED, "alq_unc_accumulate: %lld rows (fewer than 2^31)", (long long)R);
    ALQ_HIP(hipSetDevice(ctx->device));
    const int vec = R % SQ_VEC == 0 && sq_aligned(d_post, 16) && sq_aligned(d_sum_p, 16) && sq_aligned(d_sum_h, 16);
    const int64_t groups = (R + SQ_VEC - 1) / SQ_VEC;
    const dim3 grid((unsigned)std::min<int64_t>((groups + SQ_THREADS - 1) / SQ_THREADS, ALQ_SQ_MAX_BLOCKS));
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
#define SQ_ACC(CC) \
    hipLaunchKernelGGL((unc_accumulate_kernel<CC>), grid, dim3(SQ_THREADS), 0, ctx->stream, d_post, (long long)R, first, vec, d_sum_p, d_sum_h)
    switch (c) {
    case 2: SQ_ACC(2); break;
    case 3: SQ_ACC(3); break;
    case 4: SQ_ACC(4); break;
    case 5: SQ_ACC(5); break;
    case 6: SQ_ACC(6); break;
    case 7: SQ_ACC(7); break;
    default: SQ_ACC(8); break;
    }
#undef SQ_ACC
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int alq_slice_scores(alq_ctx *ctx, int kind, int T, int c, int64_t n_slices, int64_t V, const double *d_sum_p, const double *d_sum_h,
                     const float *d_f32, const uint8_t *d_roi, double *d_scores, int64_t *d_counts) {
    ALQ_REQUIRE(ctx && d_scores && d_counts, ALQ_EINVAL, "alq_slice_scores: null argument");
    ALQ_REQUIRE(kind == ALQ_UNC_ENTROPY || kind == ALQ_UNC_MC_ENTROPY || kind == ALQ_UNC_BALD || kind == ALQ_UNC_MEAN, ALQ_EINVAL,
                "alq_slice_scores: kind %d", kind);
    const bool sums = kind == ALQ_UNC_MC_ENTROPY || kind == ALQ_UNC_BALD;
    ALQ_REQUIRE(sums ? d_sum_p != nullptr : d_f32 != nullptr, ALQ_EINVAL, "alq_slice_scores: kind %d without its input", kind);
    ALQ_REQUIRE(kind != ALQ_UNC_BALD || d_sum_h, ALQ_EINVAL, "alq_slice_scores: BALD without the entropy sums");
    ALQ_REQUIRE(T >= 1 && n_slices >= 1 && V >= 1, ALQ_EINVAL, "alq_slice_scores: T = %d, %lld slices of %lld voxels", T, (long long)n_slices,
                (long long)V);
    ALQ_REQUIRE(sq_aligned(d_sum_p, 8) && sq_aligned(d_sum_h, 8) && sq_aligned(d_f32, 4) && sq_aligned(d_scores, 8) && sq_aligned(d_counts, 8),
                ALQ_EINVAL, "alq_slice_scores: a pointer is not aligned to its element");
    ALQ_REQUIRE(c >= SQ_MIN_C && c <= SQ_MAX_C, ALQ_EUNSUPPORTED, "alq_slice_scores: %d classes (%d .. %d)", c, SQ_MIN_C, SQ_MAX_C);
    ALQ_REQUIRE(n_slices < SQ_MAX_ROWS && V < SQ_MAX_ROWS && n_slices * V < SQ_MAX_ROWS, ALQ_EUNSUPPORTED,
                "alq_slice_scores: %lld x %lld rows (fewer than 2^31)", (long long)n_slices, (long long)V);
    ALQ_HIP(hipSetDevice(ctx->device));
    const int64_t R = n_slices * V;
    SqArgs a;
    a.sum_p = sums ? d_sum_p : nullptr;
    a.sum_h = kind == ALQ_UNC_BALD ? d_sum_h : nullptr;
    a.f32 = sums ? nullptr : d_f32;
    a.roi = d_roi;
    a.R = (unsigned)R;
    a.V = (unsigned)V;
    a.P = sq_partials(V);
    a.tshift = sq_tshift(V);
    a.vec = R % SQ_VEC == 0 && sq_aligned(a.sum_p, 16) && sq_aligned(a.sum_h, 16) && sq_aligned(a.f32, 16);
    a.roi_vec = R % SQ_VEC == 0 && sq_aligned(d_roi, 4);
    a.T = (double)T;
    ALQ_TRY(sq_reserve(ctx, (size_t)n_slices * a.P * sizeof(SqPartial)));
    a.part = static_cast<SqPartial *>(ctx->sq_part);
    const int64_t sweeps = (R + SQ_SWEEP - 1) / SQ_SWEEP;
    const dim3 grid((unsigned)std::min<int64_t>(sweeps, ALQ_SQ_MAX_BLOCKS));
    {
        ProfScope ps(ctx, PROF_REDUCE, 0);
        if (kind == ALQ_UNC_MEAN)
            hipLaunchKernelGGL((slice_scores_kernel<2, SQ_SRC_MEAN>), grid, dim3(SQ_THREADS), 0, ctx->stream, a);
        else if (sums)
            sq_launch_c<SQ_SRC_SUMS>(c, grid, ctx->stream, a);
        else
            sq_launch_c<SQ_SRC_F32>(c, grid, ctx->stream, a);
        ALQ_HIP(hipGetLastError());
    }
    {
        ProfScope ps(ctx, PROF_REDUCE, 0);
        hipLaunchKernelGGL(slice_finish_kernel, dim3((unsigned)((n_slices + SQ_THREADS - 1) / SQ_THREADS)), dim3(SQ_THREADS), 0, ctx->stream,
                           a.part, (unsigned)n_slices, (unsigned)V, a.P, d_scores, reinterpret_cast<long long *>(d_counts));
        ALQ_HIP(hipGetLastError());
    }
    return ALQ_OK;
}

}  // extern "C"
