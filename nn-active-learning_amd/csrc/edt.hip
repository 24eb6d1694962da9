// Surface-distance primitives on resident volumes (Hausdorff, HD95, ASSD, modified Hausdorff; surfdist.py states them in NumPy):
//
//   alq_surface_mask       out[v] = 1 on a foreground voxel with a 6-neighbour that is background or outside the volume
//   alq_edt_sq             the exact squared Euclidean distance transform to the non-zero voxels of a feature map, fp64
//   alq_masked_dist_stats  count, sum of sqrt, max and min of the masked entries of a squared-distance map
//   alq_masked_select      up to 8 order statistics of the masked entries, by radix selection on the bit pattern
//
// Volumes are [H, W, S] in C order, z contiguous (ccl.hip).
//
// The distance transform is the separable minimum itself, no parabola envelope: three line passes (z, then w, then h), each
//     out[x] = min over x' of (g[x'] + s2 * (double)((x - x')^2))            product rounded, then the sum rounded
// (-ffp-contract=off: no fused multiply-add may skip the product's rounding).  Rounding and + are monotone, so the three passes
// give min over the feature voxels of ((s2z dz^2 + s2w dw^2) + s2h dh^2): the kernels are held to equality with that statement.
// A workgroup stages whole lines in LDS; a thread takes one output at a time, walks outward from its own position in both
// directions at once and stops when s2 * dx^2 >= best - exact, because g >= 0 makes every candidate further out at least that
// large.  Near a feature that is a handful of steps; far from every feature it is the distance in voxels.
//   line pass     the lines are contiguous in memory (the z pass; the w pass of a one-slice volume): a tile is a run of `lz`
//                 whole lines = one contiguous stretch of memory, LDS image = memory image, 256 threads.  A flag per line
//                 tells whether it holds a finite value at all: most z lines of a volume miss the surface, and their outputs
//                 are +inf without a walk.
//   strided pass  the line's elements lie `inner` apart (w pass: inner = S, one h per tile; h pass: inner = W S): a tile is all L
//                 elements of `tz` neighbouring lines, LDS image [x][column], global loads and stores in runs of tz doubles;
//                 up to 1024 threads, since a full tile (64 KiB) leaves room for two workgroups on a compute unit.
// In both images the columns (z) are the fastest LDS index and the lanes run along them: at step dx lane t reads word t -
// dx * pitch and t + dx * pitch, so a wave reads consecutive 8-byte words whatever the pitch is - lanes that differ in z never
// share a bank (ds_read_b64: 64 banks of 4 bytes per 32-lane half), and a pad between rows would only break the run apart.
// Both passes may run in place: a tile holds whole lines, is staged completely before the first store, and no other workgroup
// touches its lines.  No grid cap: one workgroup per tile (at most 2^31 / 1024 of them).
//
// The masked reductions are fixed-order (lane-strided partials, wave butterfly, one row of partials per workgroup, one combine
// launch that folds the rows in workgroup order: aopt.hip's scheme) - no float atomics, the same bits on every run.  The
// selection histograms one 8-bit digit of the double's bit pattern per pass (ascending bits = ascending value for non-negative
// doubles and +inf) with integer counts: a lane folds runs of equal bins in registers, the waves count into LDS histograms of
// their own, a workgroup issues at most one integer atomic per non-zero bin; a one-workgroup kernel then finds each rank's bin
// and leaves prefix and residual rank on the device for the next pass.  Eight passes, no host round trip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "alq_internal.h"

namespace alq {

namespace {

#define ALQ_LAUNCH_CHECK() ALQ_HIP(hipGetLastError())

typedef unsigned long long u64;

constexpr int EDT_THREADS = 256;
constexpr int EDT_STRIDED_THREADS = 1024;   // at most; a strided tile of fewer elements takes fewer (a multiple of 256)
constexpr int EDT_MAX_AXIS = 1024;
constexpr int EDT_TILE = 8192;        // doubles of a staged tile: 64 KiB of LDS at most (EDT_MAX_AXIS lines' elements x 8 columns)
constexpr int EDT_LINE_TILE = 2048;   // doubles of a line-pass tile (a single line up to EDT_MAX_AXIS always fits)
constexpr int EDT_TZ = 32;            // columns of a strided tile while L <= EDT_TILE / 32 = 256; halved until L tz fits

constexpr int MS_THREADS = 256;
constexpr int MS_WAVES = MS_THREADS / 64;
constexpr int MS_MAXB = 256;          // workgroups (and partial rows) of the masked reductions: grid-stride beyond
constexpr int MS_MAXR = 8;            // ranks of one selection
constexpr int MS_BINS = 256;          // one 8-bit digit per pass

struct EdtGeo {
    int H, W, S;
    long long nvox;
    int lz;               // lines per tile of the z pass
    int tz;               // columns per tile of the strided passes
    long long wg_z;       // workgroups of the z pass
    long long wg_w, wg_h; // workgroups of the w / h pass (0: the pass is the identity, the axis has extent 1)
    int lw;               // lines per tile of the w pass when it runs as a line pass (S == 1)
};

int edt_lines_per_tile(long long nlines, int len) {
    return (int)std::max<long long>(1, std::min<long long>(nlines, EDT_LINE_TILE / len));
}

// LDS of a line-pass workgroup: the tile and one flag per line
size_t edt_line_lds(int lz, int len) { return (size_t)lz * len * sizeof(double) + (size_t)lz * sizeof(int); }

// threads of a strided workgroup: a tile of L tz elements, 256 .. EDT_STRIDED_THREADS in steps of 256
unsigned edt_strided_threads(int L, int tz) {
    const int ne = L * tz;
    return (unsigned)std::min(EDT_STRIDED_THREADS, std::max(EDT_THREADS, (ne + EDT_THREADS - 1) / EDT_THREADS * EDT_THREADS));
}

bool edt_geometry(const int64_t dims[3], EdtGeo *g) {
    if (!dims) return false;
    for (int k = 0; k < 3; ++k)
        if (dims[k] < 1 || dims[k] > EDT_MAX_AXIS) return false;
    if (dims[0] * dims[1] * dims[2] >= ((int64_t)1 << 31)) return false;
    g->H = (int)dims[0];
    g->W = (int)dims[1];
    g->S = (int)dims[2];
    g->nvox = (long long)(dims[0] * dims[1] * dims[2]);
    const long long nlines = (long long)g->H * g->W;
    g->lz = edt_lines_per_tile(nlines, g->S);
    g->wg_z = (nlines + g->lz - 1) / g->lz;
    int tz = EDT_TZ;
    while ((long long)tz * std::max(g->H, g->W) > EDT_TILE) tz >>= 1;
    g->tz = tz;
    g->lw = edt_lines_per_tile(g->H, g->W);
    if (g->W == 1)
        g->wg_w = 0;
    else if (g->S == 1)
        g->wg_w = (g->H + g->lw - 1) / g->lw;
    else
        g->wg_w = (long long)g->H * ((g->S + tz - 1) / tz);
    const long long inner = (long long)g->W * g->S;
    g->wg_h = g->H == 1 ? 0 : (inner + tz - 1) / tz;
    return true;
}

// The minimum over one line for the output at position x: `t` = its word in the LDS image, `pitch` = words between neighbours
// of the line, `len` = elements of the line.
__device__ inline double edt_walk(const double *tile, int t, int pitch, int x, int len, double s2) {
    double best = tile[t];
    for (int dx = 1;; ++dx) {
        const bool l = dx <= x, r = x + dx < len;
        if (!l && !r) break;
        const double c = s2 * (double)(dx * dx);      // dx < 1024: the square is exact in int and in double
        if (c >= best) break;                         // g >= 0: nothing at dx or beyond can be smaller
        if (l) {
            const double v = tile[t - dx * pitch] + c;
            best = v < best ? v : best;
        }
        if (r) {
            const double v = tile[t + dx * pitch] + c;
            best = v < best ? v : best;
        }
    }
    return best;
}

// lines contiguous in memory: workgroup b owns lines [b lz, b lz + lz).  FEAT: g = 0 on a feature voxel, +inf elsewhere
template <bool FEAT>
__global__ __launch_bounds__(EDT_THREADS) void edt_line_kernel(const unsigned char *__restrict__ feat, double *d, long long nlines, int len,
                                                               int lz, double s2) {
    extern __shared__ double edt_tile[];      // [lz][len] doubles, then [lz] ints: the line holds a finite value
    int *finite = reinterpret_cast<int *>(edt_tile + (size_t)lz * len);
    const double inf = std::numeric_limits<double>::infinity();
    const long long line0 = (long long)blockIdx.x * lz;
    const int nl = (int)min((long long)lz, nlines - line0);
    const int ne = nl * len;
    const long long base = line0 * len;
    for (int t = threadIdx.x; t < nl; t += EDT_THREADS) finite[t] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < ne; t += EDT_THREADS) {
        const double v = FEAT ? (feat[base + t] ? 0.0 : inf) : d[base + t];
        edt_tile[t] = v;
        if (v < inf) finite[t / len] = 1;      // every writer stores the same value
    }
    __syncthreads();
    // a line without a finite value stays +inf: nothing to walk (most z lines of a volume miss the surface altogether)
    for (int t = threadIdx.x; t < ne; t += EDT_THREADS) {
        const int line = t / len;
        d[base + t] = finite[line] ? edt_walk(edt_tile, t, 1, t - line * len, len, s2) : inf;
    }
}

// lines of L elements `inner` apart, `outer` blocks of L inner elements: a workgroup owns columns [c0, c0 + ncol) of one block
// (up to 1024 threads: a full tile is 64 KiB of LDS, two workgroups per compute unit - the walks wait on LDS, and 256 threads
// each would leave a SIMD with two waves to hide that behind)
__global__ __launch_bounds__(EDT_STRIDED_THREADS) void edt_strided_kernel(double *d, int L, long long inner, int tz, int tiles_per_outer,
                                                                          double s2) {
    extern __shared__ double edt_tile[];
    const long long o = blockIdx.x / (unsigned)tiles_per_outer;
    const long long c0 = (long long)(blockIdx.x % (unsigned)tiles_per_outer) * tz;
    const int ncol = (int)min((long long)tz, inner - c0);
    const int ne = L * ncol;
    double *p = d + (o * L * inner + c0);
    for (int t = threadIdx.x; t < ne; t += blockDim.x) {
        const int x = t / ncol, c = t - x * ncol;
        edt_tile[t] = p[x * inner + c];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ne; t += blockDim.x) {
        const int x = t / ncol, c = t - x * ncol;
        p[x * inner + c] = edt_walk(edt_tile, t, ncol, x, L, s2);
    }
}

__global__ __launch_bounds__(EDT_THREADS) void surface_mask_kernel(const unsigned char *__restrict__ seg, int H, int W, int S, long long nvox,
                                                                   int label, unsigned char *__restrict__ out) {
    for (long long v = blockIdx.x * (long long)EDT_THREADS + threadIdx.x; v < nvox; v += (long long)gridDim.x * EDT_THREADS) {
        const auto fg = [&](long long u) { return label < 0 ? seg[u] != 0 : (int)seg[u] == label; };
        bool surf = false;
        if (fg(v)) {
            const int z = (int)(v % S);
            const long long row = v / S;
            const int j = (int)(row % W), i = (int)(row / W);
            const long long sw = S, sh = (long long)W * S;
            // an axis of extent 1 has no neighbours and does not make a voxel a surface voxel
            if (S > 1) surf = surf || z == 0 || z == S - 1 || !fg(v - 1) || !fg(v + 1);
            if (W > 1) surf = surf || j == 0 || j == W - 1 || !fg(v - sw) || !fg(v + sw);
            if (H > 1) surf = surf || i == 0 || i == H - 1 || !fg(v - sh) || !fg(v + sh);
        }
        out[v] = (unsigned char)surf;
    }
}

// ---- masked reductions ------------------------------------------------------------------------------------------------------

__device__ inline double ms_shfl_xor(double v, int off) {
    const u64 b = (u64)__double_as_longlong(v);
    const unsigned lo = __shfl_xor((unsigned)b, off), hi = __shfl_xor((unsigned)(b >> 32), off);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}

// part[b][4] = (count, sum of sqrt, max, min) of workgroup b's elements: lane-strided partials, wave butterfly, waves in order
__global__ __launch_bounds__(MS_THREADS) void masked_stats_kernel(const double *__restrict__ d2, const unsigned char *__restrict__ mask, long long n,
                                                                  double *__restrict__ part) {
    __shared__ double wp[MS_WAVES][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double inf = std::numeric_limits<double>::infinity();
    unsigned cnt = 0;
    double sum = 0.0, mx = -inf, mn = inf;
    for (long long i = blockIdx.x * (long long)MS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * MS_THREADS) {
        if (mask[i]) {
            const double v = d2[i];
            ++cnt;
            sum = sum + sqrt(v);
            mx = v > mx ? v : mx;
            mn = v < mn ? v : mn;
        }
    }
    double c = (double)cnt;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        c = c + ms_shfl_xor(c, off);
        sum = sum + ms_shfl_xor(sum, off);
        const double a = ms_shfl_xor(mx, off), b = ms_shfl_xor(mn, off);
        mx = a > mx ? a : mx;
        mn = b < mn ? b : mn;
    }
    if (lane == 0) {
        wp[wave][0] = c;
        wp[wave][1] = sum;
        wp[wave][2] = mx;
        wp[wave][3] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MS_WAVES; ++w) {
            c = c + wp[w][0];
            sum = sum + wp[w][1];
            mx = wp[w][2] > mx ? wp[w][2] : mx;
            mn = wp[w][3] < mn ? wp[w][3] : mn;
        }
        double *row = part + (long long)blockIdx.x * 4;
        row[0] = c;
        row[1] = sum;
        row[2] = mx;
        row[3] = mn;
    }
}

// out[e] = the rows folded in workgroup order (e = 0, 1: sums; 2: max; 3: min)
__global__ void masked_stats_combine_kernel(const double *__restrict__ part, int nb, double *__restrict__ out) {
    const int e = threadIdx.x;
    if (e >= 4) return;
    double s = part[e];
    for (int b = 1; b < nb; ++b) {
        const double v = part[(long long)b * 4 + e];
        if (e == 2)
            s = v > s ? v : s;
        else if (e == 3)
            s = v < s ? v : s;
        else
            s = s + v;
    }
    out[e] = s;
}

struct MsRanks {
    long long r[MS_MAXR];
};

// state of a selection on the device: the bits found so far and the rank that is left inside them, per asked rank
struct MsState {
    u64 prefix[MS_MAXR];        // the digits above the current one, in place (the bits below are 0)
    long long resid[MS_MAXR];   // rank among the masked values that share the prefix; -1: the rank is at or above the count
};

__device__ inline void ms_flush(unsigned *hist, int bin, unsigned cnt) {
    if (cnt) atomicAdd(hist + bin, cnt);
}

// hist[r][digit] += the masked values whose bits above `shift + 8` equal rank r's prefix (pass 0: all of them)
__global__ __launch_bounds__(MS_THREADS) void masked_hist_kernel(const double *__restrict__ d2, const unsigned char *__restrict__ mask, long long n,
                                                                 int R, int shift, const MsState *__restrict__ st, unsigned *__restrict__ hist) {
    __shared__ unsigned lh[MS_WAVES][MS_MAXR * MS_BINS];      // 32 KiB: a histogram per wave
    const int wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < MS_WAVES * MS_MAXR * MS_BINS; k += MS_THREADS) (&lh[0][0])[k] = 0;
    __syncthreads();
    u64 prefix[MS_MAXR];
    bool live[MS_MAXR];
    int bin[MS_MAXR];
    unsigned cnt[MS_MAXR];
    const bool first = shift == 56;
#pragma unroll
    for (int r = 0; r < MS_MAXR; ++r) {
        live[r] = r < R && (first || st->resid[r] >= 0);
        prefix[r] = (first || r >= R) ? 0 : st->prefix[r];
        bin[r] = 0;
        cnt[r] = 0;
    }
    const u64 himask = first ? 0 : ~(((u64)1 << (shift + 8)) - 1);
    for (long long i = blockIdx.x * (long long)MS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * MS_THREADS) {
        if (!mask[i]) continue;
        const u64 b = (u64)__double_as_longlong(d2[i]);
        const int dg = (int)((b >> shift) & (MS_BINS - 1));
#pragma unroll
        for (int r = 0; r < MS_MAXR; ++r) {
            if (!live[r] || (b & himask) != prefix[r]) continue;
            if (dg == bin[r]) {
                ++cnt[r];
            } else {
                ms_flush(lh[wave] + r * MS_BINS, bin[r], cnt[r]);
                bin[r] = dg;
                cnt[r] = 1;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < MS_MAXR; ++r) ms_flush(lh[wave] + r * MS_BINS, bin[r], cnt[r]);
    __syncthreads();
    for (int k = threadIdx.x; k < R * MS_BINS; k += MS_THREADS) {
        unsigned s = 0;
        for (int w = 0; w < MS_WAVES; ++w) s += lh[w][k];
        if (s) atomicAdd(hist + k, s);
    }
}

// one workgroup: thread r walks rank r's 256 bins to the one that holds it, then every thread clears the histogram for the next
// pass.  After the last digit (shift 0) the prefix is the value: out[r] = it, or NaN for a rank at or above the count.
__global__ __launch_bounds__(MS_THREADS) void masked_find_kernel(int R, int shift, MsRanks ranks, MsState *st, unsigned *hist, double *out) {
    const int r = threadIdx.x;
    if (r < R) {
        const bool first = shift == 56;
        long long resid = first ? ranks.r[r] : st->resid[r];
        u64 prefix = first ? 0 : st->prefix[r];
        if (resid >= 0) {
            const unsigned *h = hist + r * MS_BINS;
            int b = 0;
            for (; b < MS_BINS; ++b) {
                const long long c = h[b];
                if (resid < c) break;
                resid -= c;
            }
            if (b == MS_BINS)
                resid = -1;      // the bins hold fewer values than the rank asks for (only the first pass can find that)
            else
                prefix |= (u64)b << shift;
        }
        st->resid[r] = resid;
        st->prefix[r] = prefix;
        if (shift == 0) out[r] = resid >= 0 ? __longlong_as_double((long long)prefix) : __longlong_as_double(0x7ff8000000000000ll);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < R * MS_BINS; k += MS_THREADS) hist[k] = 0;
}

int ms_grid(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + MS_THREADS - 1) / MS_THREADS, MS_MAXB)); }

struct MsWork {
    double *part;       // [MS_MAXB][4]
    unsigned *hist;     // [MS_MAXR][MS_BINS]
    MsState *st;
};

constexpr size_t MS_PART_BYTES = (size_t)MS_MAXB * 4 * sizeof(double);
constexpr size_t MS_HIST_BYTES = (size_t)MS_MAXR * MS_BINS * sizeof(unsigned);

MsWork ms_work(void *d_work) {
    MsWork w;
    char *p = static_cast<char *>(d_work);
    w.part = reinterpret_cast<double *>(p);
    w.hist = reinterpret_cast<unsigned *>(p + MS_PART_BYTES);
    w.st = reinterpret_cast<MsState *>(p + MS_PART_BYTES + MS_HIST_BYTES);
    return w;
}

bool ms_n_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

}  // namespace

}  // namespace alq

using namespace alq;

extern "C" {

int alq_edt_max_axis(void) { return EDT_MAX_AXIS; }

size_t alq_edt_work_bytes(const int64_t dims[3]) {
    EdtGeo g;
    if (!edt_geometry(dims, &g)) return 0;
    return 64;      // the passes run in place in d_out; the buffer is part of the contract so that this may change
}

int alq_edt_geometry(const int64_t dims[3], int32_t out[4]) {
    ALQ_REQUIRE(out, ALQ_EINVAL, "alq_edt_geometry: null argument");
    EdtGeo g;
    if (!edt_geometry(dims, &g)) {
        for (int k = 0; k < 4; ++k) out[k] = -1;
        set_error("alq_edt_geometry: dims outside 1 .. %d per axis, below 2^31 voxels", EDT_MAX_AXIS);
        return ALQ_EUNSUPPORTED;
    }
    out[0] = g.lz;
    out[1] = g.tz;
    out[2] = (int32_t)g.wg_z;
    out[3] = (int32_t)std::max(g.wg_w, g.wg_h);
    return ALQ_OK;
}

int alq_surface_mask(alq_ctx *ctx, const uint8_t *d_seg, const int64_t dims[3], int label, uint8_t *d_out) {
    ALQ_REQUIRE(ctx && d_seg && dims && d_out, ALQ_EINVAL, "alq_surface_mask: null argument");
    ALQ_REQUIRE(d_seg != d_out, ALQ_EINVAL, "alq_surface_mask: d_out may not be d_seg (a voxel reads its neighbours)");
    ALQ_REQUIRE(label <= 255, ALQ_EINVAL, "alq_surface_mask: label %d (below 0: every non-zero voxel, else 0 .. 255)", label);
    for (int k = 0; k < 3; ++k)
        ALQ_REQUIRE(dims[k] >= 1 && dims[k] < ((int64_t)1 << 31), ALQ_EINVAL, "alq_surface_mask: dims[%d] = %lld", k, (long long)dims[k]);
    ALQ_REQUIRE(dims[0] * dims[1] < ((int64_t)1 << 31) && dims[0] * dims[1] * dims[2] < ((int64_t)1 << 31), ALQ_EUNSUPPORTED,
                "alq_surface_mask: 2^31 voxels or more");
    const long long nvox = (long long)(dims[0] * dims[1] * dims[2]);
    ALQ_HIP(hipSetDevice(ctx->device));
    const long long blocks = std::max<long long>(1, std::min<long long>((nvox + EDT_THREADS - 1) / EDT_THREADS, (long long)ctx->num_cus * 8));
    ProfScope ps(ctx, PROF_EVAL, 0);
    hipLaunchKernelGGL(surface_mask_kernel, dim3((unsigned)blocks), dim3(EDT_THREADS), 0, ctx->stream, d_seg, (int)dims[0], (int)dims[1],
                       (int)dims[2], nvox, label, d_out);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

int alq_edt_sq(alq_ctx *ctx, const uint8_t *d_feat, const int64_t dims[3], const double spacing2[3], double *d_out, void *d_work) {
    ALQ_REQUIRE(ctx && d_feat && dims && spacing2 && d_out && d_work, ALQ_EINVAL, "alq_edt_sq: null argument");
    for (int k = 0; k < 3; ++k)
        ALQ_REQUIRE(std::isfinite(spacing2[k]) && spacing2[k] > 0.0, ALQ_EINVAL, "alq_edt_sq: spacing2[%d] = %g (finite and > 0)", k, spacing2[k]);
    ALQ_REQUIRE(((uintptr_t)d_out & 7) == 0, ALQ_EINVAL, "alq_edt_sq: d_out not 8-byte aligned");
    EdtGeo g;
    ALQ_REQUIRE(edt_geometry(dims, &g), ALQ_EUNSUPPORTED, "alq_edt_sq: dims %lld x %lld x %lld (each 1 .. %d, below 2^31 voxels)", (long long)dims[0],
                (long long)dims[1], (long long)dims[2], EDT_MAX_AXIS);
    ALQ_HIP(hipSetDevice(ctx->device));
    ProfScope ps(ctx, PROF_EVAL, 0);
    const long long nlines = (long long)g.H * g.W;
    hipLaunchKernelGGL(edt_line_kernel<true>, dim3((unsigned)g.wg_z), dim3(EDT_THREADS), edt_line_lds(g.lz, g.S), ctx->stream, d_feat,
                       d_out, nlines, g.S, g.lz, spacing2[2]);
    ALQ_LAUNCH_CHECK();
    if (g.wg_w) {
        if (g.S == 1) {
            hipLaunchKernelGGL(edt_line_kernel<false>, dim3((unsigned)g.wg_w), dim3(EDT_THREADS), edt_line_lds(g.lw, g.W), ctx->stream,
                               (const unsigned char *)nullptr, d_out, (long long)g.H, g.W, g.lw, spacing2[1]);
        } else {
            const int tiles = (g.S + g.tz - 1) / g.tz;
            hipLaunchKernelGGL(edt_strided_kernel, dim3((unsigned)g.wg_w), dim3(edt_strided_threads(g.W, g.tz)),
                               (size_t)g.W * g.tz * sizeof(double), ctx->stream, d_out, g.W, (long long)g.S, g.tz, tiles, spacing2[1]);
        }
        ALQ_LAUNCH_CHECK();
    }
    if (g.wg_h) {
        hipLaunchKernelGGL(edt_strided_kernel, dim3((unsigned)g.wg_h), dim3(edt_strided_threads(g.H, g.tz)),
                           (size_t)g.H * g.tz * sizeof(double), ctx->stream, d_out, g.H, (long long)g.W * g.S, g.tz, (int)g.wg_h, spacing2[0]);
        ALQ_LAUNCH_CHECK();
    }
    return ALQ_OK;
}

size_t alq_masked_work_bytes(int64_t n) { return ms_n_ok(n) ? MS_PART_BYTES + MS_HIST_BYTES + sizeof(MsState) : 0; }

int alq_masked_geometry(int64_t n, int32_t out[2]) {
    ALQ_REQUIRE(out, ALQ_EINVAL, "alq_masked_geometry: null argument");
    if (!ms_n_ok(n)) {
        out[0] = out[1] = -1;
        set_error("alq_masked_geometry: n = %lld (0 .. 2^31 - 1)", (long long)n);
        return ALQ_EUNSUPPORTED;
    }
    out[0] = MS_THREADS;
    out[1] = ms_grid(n);
    return ALQ_OK;
}

int alq_masked_dist_stats(alq_ctx *ctx, const double *d_d2, const uint8_t *d_mask, int64_t n, double *d_out, void *d_work) {
    ALQ_REQUIRE(ctx && d_d2 && d_mask && d_out && d_work, ALQ_EINVAL, "alq_masked_dist_stats: null argument");
    ALQ_REQUIRE(ms_n_ok(n), ALQ_EUNSUPPORTED, "alq_masked_dist_stats: n = %lld (0 .. 2^31 - 1)", (long long)n);
    ALQ_REQUIRE((((uintptr_t)d_d2 | (uintptr_t)d_out | (uintptr_t)d_work) & 7) == 0, ALQ_EINVAL, "alq_masked_dist_stats: a pointer is not 8-byte aligned");
    ALQ_HIP(hipSetDevice(ctx->device));
    const MsWork w = ms_work(d_work);
    const int nb = ms_grid(n);
    ProfScope ps(ctx, PROF_EVAL, 0);
    hipLaunchKernelGGL(masked_stats_kernel, dim3((unsigned)nb), dim3(MS_THREADS), 0, ctx->stream, d_d2, d_mask, (long long)n, w.part);
    ALQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(masked_stats_combine_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double *)w.part, nb, d_out);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

int alq_masked_select(alq_ctx *ctx, const double *d_d2, const uint8_t *d_mask, int64_t n, const int64_t *h_ranks, int R, double *d_out,
                      void *d_work) {
    ALQ_REQUIRE(ctx && d_d2 && d_mask && h_ranks && d_out && d_work, ALQ_EINVAL, "alq_masked_select: null argument");
    ALQ_REQUIRE(R >= 1 && R <= MS_MAXR, ALQ_EINVAL, "alq_masked_select: R = %d (1 .. %d)", R, MS_MAXR);
    ALQ_REQUIRE(ms_n_ok(n), ALQ_EUNSUPPORTED, "alq_masked_select: n = %lld (0 .. 2^31 - 1)", (long long)n);
    MsRanks ranks;
    for (int r = 0; r < MS_MAXR; ++r) {
        ALQ_REQUIRE(r >= R || h_ranks[r] >= 0, ALQ_EINVAL, "alq_masked_select: rank %d = %lld is negative", r, (long long)h_ranks[r]);
        ranks.r[r] = r < R ? (long long)h_ranks[r] : -1;
    }
    ALQ_REQUIRE((((uintptr_t)d_d2 | (uintptr_t)d_out | (uintptr_t)d_work) & 7) == 0, ALQ_EINVAL, "alq_masked_select: a pointer is not 8-byte aligned");
    ALQ_HIP(hipSetDevice(ctx->device));
    const MsWork w = ms_work(d_work);
    const int nb = ms_grid(n);
    ALQ_HIP(hipMemsetAsync(w.hist, 0, MS_HIST_BYTES + sizeof(MsState), ctx->stream));
    ProfScope ps(ctx, PROF_EVAL, 0);
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(masked_hist_kernel, dim3((unsigned)nb), dim3(MS_THREADS), 0, ctx->stream, d_d2, d_mask, (long long)n, R, shift,
                           (const MsState *)w.st, w.hist);
        ALQ_LAUNCH_CHECK();
        hipLaunchKernelGGL(masked_find_kernel, dim3(1), dim3(MS_THREADS), 0, ctx->stream, R, shift, ranks, w.st, w.hist, d_out);
        ALQ_LAUNCH_CHECK();
    }
    return ALQ_OK;
}

}  // extern "C"
