// Region primitives of the pseudo-random and super-pixel strategies (PW_NNAL.py:632-669 get_HV_inds, :944-1021 superpix_scoring;
// patch_utils.py:794-826 get_vars_2d):
//
//   alq_local_var2d   the d x d local-variance map of every slice of a zero-padded volume that is resident for the gather:
//                     t = trunc(v), S1 = sum t, S2 = sum t^2 over the window rows [i - d/2, i + (d-1)/2] x columns
//                     [j - d/2, j + (d-1)/2] clipped to the slice, both 64-bit INTEGER sums, then
//                     var = double(S2) / double(d d) - (double(S1) / double(d d))^2, operation by operation (no contraction:
//                     this file is compiled with -ffp-contract=off, like aopt.hip).  That is scipy's
//                     convolve2d(np.uint64(img), ones((d, d)), 'same') statement of the reference wherever both are exact.
//   alq_segment_min   per (slice, label) minimum of per-voxel scores: atomicMin on an order-preserving 64-bit key of the double.
//                     A minimum does not depend on arrival order, so the table has the same bits every run.
//
// Whole map: z is the contiguous axis of the volume, so the lanes of a wave run along z (a wave-load is a run of consecutive
// addresses, a wave-store a run of consecutive doubles) and every lane filters its own slice column.  A lane owns LV_TW
// columns x `th` rows of one slice: per row that enters or leaves the row window it forms the LV_TW horizontal box sums as one
// running sum along j (d + 2 (LV_TW - 1) loads) and adds them to / takes them from LV_TW vertical running sums in registers.
// Unsigned 64-bit arithmetic is modular, so add-then-subtract is exact.  Loads per output: about
// ((d + 2 LV_TW - 2) / LV_TW) x ((2 th + d - 1) / th) instead of d^2; the re-reads of a row are served by L1 / L2.
// Indexed form (d_inds): one thread per query forms its own window (only those windows are formed).
#include <algorithm>
#include <cstdlib>

#include "alq_internal.h"

#pragma clang fp contract(off)

namespace alq {

namespace {

typedef unsigned long long u64;

constexpr int LV_TW = 8;      // columns per lane: 2 x LV_TW 64-bit running sums in registers

template <typename T>
__device__ inline unsigned lv_trunc(T v) { return (unsigned)v; }      // trunc toward zero; the caller guarantees 0 <= v < 2^32

__device__ inline double lv_var(u64 s1, u64 s2, double dd) {
    const double ex2 = (double)s2 / dd;
    const double ex = (double)s1 / dd;
    const double sq = ex * ex;
    return ex2 - sq;
}

struct LvGeo {
    long long sy, sx;      // element strides of a step in i and in j inside the padded volume (D1 * D2, D2)
    long long org;         // element offset of un-padded voxel (0, 0, 0)
    int H, W, S;           // un-padded box
    int lo, hi;            // window = [x - lo, x + hi]
};

// horizontal box sums of row i for columns j0 .. j0 + LV_TW - 1, added to (SIGN > 0) or taken from the vertical sums
template <typename T, int SIGN>
__device__ inline void lv_row(const T *__restrict__ p, const LvGeo &g, int i, int j0, u64 (&V1)[LV_TW], u64 (&V2)[LV_TW]) {
    if (i < 0 || i >= g.H) return;      // a row outside the slice is zero fill
    const T *rp = p + (long long)i * g.sy;
    u64 h1 = 0, h2 = 0;
    const int c0 = max(j0 - g.lo, 0), c1 = min(j0 + g.hi, g.W - 1);
#pragma unroll 4
    for (int c = c0; c <= c1; ++c) {
        const u64 t = lv_trunc(rp[(long long)c * g.sx]);
        h1 += t;
        h2 += t * t;
    }
    if (SIGN > 0) { V1[0] += h1; V2[0] += h2; } else { V1[0] -= h1; V2[0] -= h2; }
#pragma unroll
    for (int jj = 1; jj < LV_TW; ++jj) {
        const int ca = j0 + jj + g.hi, cb = j0 + jj - 1 - g.lo;
        const u64 a = (ca >= 0 && ca < g.W) ? (u64)lv_trunc(rp[(long long)ca * g.sx]) : 0ull;
        const u64 b = (cb >= 0 && cb < g.W) ? (u64)lv_trunc(rp[(long long)cb * g.sx]) : 0ull;
        h1 += a - b;
        h2 += a * a - b * b;
        if (SIGN > 0) { V1[jj] += h1; V2[jj] += h2; } else { V1[jj] -= h1; V2[jj] -= h2; }
    }
}

__device__ inline void lv_emit(double *__restrict__ out, const LvGeo &g, int i, int j0, int z, const u64 (&V1)[LV_TW],
                               const u64 (&V2)[LV_TW], double dd) {
#pragma unroll
    for (int jj = 0; jj < LV_TW; ++jj) {
        const int j = j0 + jj;
        if (j < g.W) out[((long long)i * g.W + j) * g.S + z] = lv_var(V1[jj], V2[jj], dd);
    }
}

// one thread = (slice z, column tile jt, row tile it), z fastest: neighbouring lanes are neighbouring slices
template <typename T>
__global__ __launch_bounds__(256) void local_var_map_kernel(const T *__restrict__ vol, LvGeo g, int th, int njt, long long total, double dd,
                                                            double *__restrict__ out) {
    const long long gid = blockIdx.x * 256LL + threadIdx.x;
    if (gid >= total) return;
    const int z = (int)(gid % g.S);
    const long long rest = gid / g.S;
    const int j0 = (int)(rest % njt) * LV_TW;
    const int i0 = (int)(rest / njt) * th;
    const T *p = vol + g.org + z;
    u64 V1[LV_TW], V2[LV_TW];
#pragma unroll
    for (int jj = 0; jj < LV_TW; ++jj) { V1[jj] = 0; V2[jj] = 0; }
    for (int i = i0 - g.lo; i <= i0 + g.hi; ++i) lv_row<T, 1>(p, g, i, j0, V1, V2);
    lv_emit(out, g, i0, j0, z, V1, V2, dd);
    const int i1 = min(i0 + th, g.H);
    for (int i = i0 + 1; i < i1; ++i) {
        lv_row<T, 1>(p, g, i + g.hi, j0, V1, V2);
        lv_row<T, -1>(p, g, i - 1 - g.lo, j0, V1, V2);
        lv_emit(out, g, i, j0, z, V1, V2, dd);
    }
}

// one thread per query: its own clipped window
template <typename T>
__global__ __launch_bounds__(256) void local_var_inds_kernel(const T *__restrict__ vol, LvGeo g, const long long *__restrict__ inds, long long n,
                                                             double dd, double *__restrict__ out) {
    const long long nvox = (long long)g.H * g.W * g.S;
    for (long long q = blockIdx.x * 256LL + threadIdx.x; q < n; q += (long long)gridDim.x * 256) {
        const long long ind = inds[q];
        if (ind < 0 || ind >= nvox) { out[q] = __longlong_as_double(0x7ff8000000000000LL); continue; }      // outside the box: NaN, nothing read
        const int z = (int)(ind % g.S);
        const int j = (int)((ind / g.S) % g.W);
        const int i = (int)(ind / ((long long)g.S * g.W));
        const T *p = vol + g.org + z;
        const int r0 = max(i - g.lo, 0), r1 = min(i + g.hi, g.H - 1);
        const int c0 = max(j - g.lo, 0), c1 = min(j + g.hi, g.W - 1);
        u64 s1 = 0, s2 = 0;
        for (int r = r0; r <= r1; ++r) {
            const T *rp = p + (long long)r * g.sy;
#pragma unroll 4
            for (int c = c0; c <= c1; ++c) {
                const u64 t = lv_trunc(rp[(long long)c * g.sx]);
                s1 += t;
                s2 += t * t;
            }
        }
        out[q] = lv_var(s1, s2, dd);
    }
}

// ---- segment minimum -----------------------------------------------------------------------------------------------------
// order-preserving key of a double: unsigned order of the keys = numeric order of the values (-0.0 below +0.0)
__device__ inline u64 sm_key(double x) {
    const u64 b = (u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline u64 sm_unkey_bits(u64 k) { return (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; }      // the double's bit pattern

__global__ __launch_bounds__(256) void segmin_fill_kernel(u64 *__restrict__ table, long long m) {
    const u64 kinf = 0xfff0000000000000ull;      // sm_key(+inf)
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < m; e += (long long)gridDim.x * 256) table[e] = kinf;
}

__global__ __launch_bounds__(256) void segmin_scatter_kernel(const int *__restrict__ labels, long long nvox, int S, int n_labels,
                                                             const long long *__restrict__ inds, const double *__restrict__ scores, long long n,
                                                             u64 *__restrict__ table) {
    for (long long q = blockIdx.x * 256LL + threadIdx.x; q < n; q += (long long)gridDim.x * 256) {
        const long long ind = inds[q];
        if (ind < 0 || ind >= nvox) continue;
        const int l = labels[ind];
        if (l < 1 || l >= n_labels) continue;      // label 0 is background (regionprops ignores it); no out-of-range store
        u64 *cell = table + (long long)(ind % S) * n_labels + l;
        const u64 k = sm_key(scores[q]);
        // a cell only ever decreases, so a (possibly stale) plain read that is already <= k proves the atomic would change
        // nothing: with many voxels per cell almost every atomic is skipped
        if (__atomic_load_n(cell, __ATOMIC_RELAXED) <= k) continue;
        atomicMin(cell, k);
    }
}

__global__ __launch_bounds__(256) void segmin_finish_kernel(u64 *__restrict__ table, long long m) {
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < m; e += (long long)gridDim.x * 256)
        table[e] = sm_unkey_bits(table[e]);      // in place: the caller reads the cells as doubles
}

unsigned stream_grid(const alq_ctx *ctx, long long n) {
    return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)ctx->num_cus * 8));
}

// rows per lane of the whole-map launch: the tallest tile (least re-summed window rows) that still gives every SIMD of the
// device two waves - the launch is bound by its dependent load -> 64-bit add chains, and measured at 256 x 256 x 128, d = 12,
// 8 rows (8 waves per CU) took 0.136 ms against 0.184 at 16 and 0.154 at 4 (tools/gpu_regions.py); ALQ_LVAR_ROWS overrides
// (tuning runs: same bits for every value)
int lv_rows_per_lane(const alq_ctx *ctx, int H, int W, int S) {
    const char *e = getenv("ALQ_LVAR_ROWS");
    if (e && atoi(e) >= 1) return std::min(atoi(e), H);
    const long long njt = (W + LV_TW - 1) / LV_TW;
    int th = 64;
    while (th > 8 && (long long)S * njt * ((H + th - 1) / th) < (long long)ctx->num_cus * 8 * 64) th >>= 1;
    return std::min(th, H);
}

}  // namespace

}  // namespace alq

using namespace alq;

extern "C" {

int alq_local_var2d(alq_ctx *ctx, const void *d_vol, int vol_is_f64, const int64_t pad_dims[3], const int32_t rads[3], int d,
                    const int64_t *d_inds, int64_t n, double *d_out) {
    ALQ_REQUIRE(ctx && d_vol && pad_dims && rads && d_out, ALQ_EINVAL, "alq_local_var2d: null argument");
    ALQ_REQUIRE(d >= 1 && d <= 65, ALQ_EINVAL, "alq_local_var2d: window %d outside [1, 65]", d);
    ALQ_REQUIRE(n >= 0, ALQ_EINVAL, "alq_local_var2d: n = %lld", (long long)n);
    int64_t box[3];
    for (int a = 0; a < 3; ++a) {
        ALQ_REQUIRE(rads[a] >= 0 && pad_dims[a] >= 1 && pad_dims[a] - 2 * (int64_t)rads[a] >= 1, ALQ_EINVAL,
                    "alq_local_var2d: axis %d: padded size %lld, radius %d", a, (long long)pad_dims[a], (int)rads[a]);
        box[a] = pad_dims[a] - 2 * (int64_t)rads[a];
        ALQ_REQUIRE(pad_dims[a] < (1LL << 31), ALQ_EINVAL, "alq_local_var2d: axis %d too long", a);
    }
    LvGeo g;
    g.sy = pad_dims[1] * pad_dims[2];
    g.sx = pad_dims[2];
    g.org = ((int64_t)rads[0] * pad_dims[1] + rads[1]) * pad_dims[2] + rads[2];
    g.H = (int)box[0];
    g.W = (int)box[1];
    g.S = (int)box[2];
    g.lo = d / 2;
    g.hi = (d - 1) / 2;
    const double dd = (double)(d * d);
    ALQ_HIP(hipSetDevice(ctx->device));
    if (d_inds) {
        if (n == 0) return ALQ_OK;
        ProfScope ps(ctx, PROF_ELEMWISE, 0);
        const dim3 grid(stream_grid(ctx, n));
        if (vol_is_f64)
            hipLaunchKernelGGL(local_var_inds_kernel<double>, grid, dim3(256), 0, ctx->stream, (const double *)d_vol, g,
                               (const long long *)d_inds, (long long)n, dd, d_out);
        else
            hipLaunchKernelGGL(local_var_inds_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float *)d_vol, g,
                               (const long long *)d_inds, (long long)n, dd, d_out);
        ALQ_HIP(hipGetLastError());
        return ALQ_OK;
    }
    const int th = lv_rows_per_lane(ctx, g.H, g.W, g.S);
    const int njt = (g.W + LV_TW - 1) / LV_TW;
    const long long total = (long long)g.S * njt * ((g.H + th - 1) / th);
    ALQ_REQUIRE((total + 255) / 256 < (1LL << 31), ALQ_EINVAL, "alq_local_var2d: volume too large for one launch");
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vol_is_f64)
        hipLaunchKernelGGL(local_var_map_kernel<double>, grid, dim3(256), 0, ctx->stream, (const double *)d_vol, g, th, njt, total, dd, d_out);
    else
        hipLaunchKernelGGL(local_var_map_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float *)d_vol, g, th, njt, total, dd, d_out);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int alq_segment_min(alq_ctx *ctx, const int32_t *d_labels, const int64_t dims[3], int32_t n_labels, const int64_t *d_inds,
                    const double *d_scores, int64_t n, double *d_table) {
    ALQ_REQUIRE(ctx && dims && d_table, ALQ_EINVAL, "alq_segment_min: null argument");
    ALQ_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && dims[2] < (1LL << 31) && n_labels >= 1 && n >= 0, ALQ_EINVAL,
                "alq_segment_min: bad shape (dims %lld x %lld x %lld, %d labels, n = %lld)", (long long)dims[0], (long long)dims[1],
                (long long)dims[2], (int)n_labels, (long long)n);
    ALQ_REQUIRE(n == 0 || (d_labels && d_inds && d_scores), ALQ_EINVAL, "alq_segment_min: null argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    const long long m = (long long)dims[2] * n_labels;
    u64 *keys = reinterpret_cast<u64 *>(d_table);
    ProfScope ps(ctx, PROF_REDUCE, 0);
    hipLaunchKernelGGL(segmin_fill_kernel, dim3(stream_grid(ctx, m)), dim3(256), 0, ctx->stream, keys, m);
    ALQ_HIP(hipGetLastError());
    if (n > 0) {
        hipLaunchKernelGGL(segmin_scatter_kernel, dim3(stream_grid(ctx, n)), dim3(256), 0, ctx->stream, (const int *)d_labels,
                           (long long)(dims[0] * dims[1] * dims[2]), (int)dims[2], (int)n_labels, (const long long *)d_inds, d_scores,
                           (long long)n, keys);
        ALQ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(segmin_finish_kernel, dim3(stream_grid(ctx, m)), dim3(256), 0, ctx->stream, keys, m);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // extern "C"
