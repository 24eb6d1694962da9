// Multi-class confusion counts over resident label maps (eval_utils.eval_metrics / eval_full_segs_*: np.argmax, concatenate and
// count on the host in the reference).  For every element i of [0, n), with j = first + i and g = (j / inner) % groups:
//     t = lab[i]   (outside [0, C): `fill` when 0 <= fill < C, else the element is skipped)
//     p = pred[i]  (outside [0, C): the element is skipped)
//     counts[g][t][p] += 1
// added to int64 totals [groups, C, C] that stay on the device; the skipped elements are counted into one more word.
// Integers only: a lane folds runs of equal cells in registers, the lanes of a block count into 32-bit LDS histograms that
// meet in LDS, and the block issues at most one 64-bit atomic add per non-zero cell of its histogram - the
// totals are exact and bit-identical, whatever the grid, the chunking or the order the blocks retire in.
//
// The common input is a segmentation that is mostly background: nearly every lane of a block adds to cell (0, 0), and LDS
// atomics on one address serialise - those of one instruction, and (measured: 3 to 6 times the kernel's time when the four
// waves shared 64 copies) those of different waves as well.  So the block's histogram of `cells` words is kept in R copies (R
// a power of two, at most 256 = one per lane of the block, as many as CF_BLOCK_WORDS holds), copy-fastest: cell k of copy r
// lies at word k R + r, and lane l of wave w adds to copy (64 w + l) >> (8 - log2 R).  With groups = 1 and C <= 5, R = 256:
// every lane owns its words, nothing serialises; any R >= 4 still gives every wave copies of its own.  With many groups R
// shrinks to 1 (the four waves share one histogram) and the lanes spread over the groups instead (inner = 1: consecutive
// elements lie in consecutive groups).  The copies meet at the end: a shuffle sum over the lanes that hold the copies of one
// cell, one more LDS step for R > 64, one thread per cell for the global atomic.
// A lane holds (cell, count) of its current run across the whole sweep and touches LDS only where the cell changes: on a
// background-heavy map that is a handful of adds per lane.
//
// Streaming: 16-byte loads per lane (16 uint8, 4 int32 or 2 int64 ids; the wider of two types takes several) where both
// pointers are 16-byte aligned, VEC = 16 / the smaller element size elements per lane and step; the tail, and all of an
// unaligned call, goes through the guarded one-element path.  Grid-stride, 256 threads.
// groups C^2 cells beyond CF_BLOCK_WORDS: the launcher walks windows of alq_confusion_window(C) groups, one launch per
// window; elements of other groups are passed over (and counted as skipped by the first window only).
#include <algorithm>

#include "alq_internal.h"

namespace alq {

namespace {

typedef unsigned long long u64;

constexpr int CF_THREADS = 256;
constexpr int CF_WAVES = CF_THREADS / 64;
constexpr int CF_BLOCK_WORDS = 8192;     // 32-bit words of a block's histogram (all copies): 32 KiB of LDS, four blocks per CU
constexpr int CF_BLOCKS_PER_CU = 4;
constexpr int CF_MAX_C = 16;

struct CfArgs {
    long long n;          // elements of this launch
    long long first;      // j of element 0
    long long inner, groups;
    int C, fill;          // fill < 0: no fill
    long long g0;         // window [g0, g0 + gw)
    int gw;
    int rshift;           // log2 R, 0 .. 8
    int small;            // first + n, inner and groups fit 32 bits
};

template <typename T>
__device__ inline bool cf_in(T v, int C) {
    return v >= (T)0 && (long long)v < (long long)C;
}

template <typename T, int VEC>
__device__ inline void cf_load(const T *p, T (&e)[VEC]) {
    constexpr int NB = (int)(VEC * sizeof(T) / 16);
    static_assert(NB >= 1 && NB * 16 == (int)(VEC * sizeof(T)), "whole 16-byte loads");
    union {
        uint4 q[NB];
        T v[VEC];
    } u;
    const uint4 *s = reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (int b = 0; b < NB; ++b) u.q[b] = s[b];
#pragma unroll
    for (int k = 0; k < VEC; ++k) e[k] = u.v[k];
}

// the lane's run of equal cells: (cell, count), added to the lane's copy of the histogram where the cell changes
struct CfRun {
    int cell;
    unsigned cnt;
};

__device__ inline void cf_flush(const CfRun &r, unsigned *hist, int rshift, int rep) {
    if (r.cell >= 0 && r.cnt) atomicAdd(hist + ((r.cell << rshift) + rep), r.cnt);
}

// position of element j: q = j / inner (only its group matters), r = j % inner
struct CfPos {
    long long g;      // (j / inner) % groups
    long long r;      // j % inner
};

__device__ inline CfPos cf_pos(const CfArgs &a, long long i) {
    CfPos s;
    const long long j = a.first + i;
    if (a.groups == 1) {
        s.g = 0;
        s.r = 0;
    } else if (a.small) {
        const unsigned q = (unsigned)j / (unsigned)a.inner;
        s.r = (unsigned)j % (unsigned)a.inner;
        s.g = q % (unsigned)a.groups;
    } else {
        const long long q = j / a.inner;
        s.r = j % a.inner;
        s.g = q % a.groups;
    }
    return s;
}

__device__ inline void cf_step(const CfArgs &a, CfPos &s) {
    if (a.groups == 1) return;
    if (++s.r == a.inner) {
        s.r = 0;
        if (++s.g == a.groups) s.g = 0;
    }
}

template <typename PT, typename LT>
__device__ inline void cf_count(const CfArgs &a, PT pv, LT lv, long long g, CfRun &run, unsigned &skipped, unsigned *hist, int rep) {
    int t = (int)lv, cell = -1;
    bool ok = cf_in(lv, a.C);
    if (!ok && a.fill >= 0) {
        t = a.fill;
        ok = true;
    }
    ok = ok && cf_in(pv, a.C);
    if (!ok) {
        ++skipped;
    } else {
        const long long gl = g - a.g0;
        if (gl >= 0 && gl < a.gw) cell = ((int)gl * a.C + t) * a.C + (int)pv;
    }
    if (cell == run.cell) {
        ++run.cnt;
    } else {
        cf_flush(run, hist, a.rshift, rep);
        run.cell = cell;
        run.cnt = 1;
    }
}

template <typename PT, typename LT>
__global__ __launch_bounds__(CF_THREADS) void confusion_kernel(const PT *__restrict__ pred, const LT *__restrict__ lab, CfArgs a, long long nvec,
                                                               u64 *__restrict__ counts, u64 *__restrict__ skipped_out) {
    constexpr int VEC = 16 / (int)(sizeof(PT) < sizeof(LT) ? sizeof(PT) : sizeof(LT));
    extern __shared__ unsigned cf_lds[];      // [cells << rshift], then [CF_WAVES] skipped
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cells = a.gw * a.C * a.C;
    const int words = cells << a.rshift;
    for (int k = threadIdx.x; k < words + CF_WAVES; k += CF_THREADS) cf_lds[k] = 0;
    __syncthreads();
    unsigned *hist = cf_lds;
    const int rep = (int)threadIdx.x >> (8 - a.rshift);
    CfRun run;
    run.cell = -1;
    run.cnt = 0;
    unsigned skipped = 0;      // at most n / (threads of the grid) + VEC < 2^32
    const long long tid = blockIdx.x * (long long)CF_THREADS + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * CF_THREADS;
    // whole vectors: elements [0, nvec VEC)
    for (long long v = tid; v < nvec; v += nthreads) {
        const long long i0 = v * VEC;
        PT pe[VEC];
        LT le[VEC];
        cf_load<PT, VEC>(pred + i0, pe);
        cf_load<LT, VEC>(lab + i0, le);
        CfPos s = cf_pos(a, i0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            cf_count(a, pe[k], le[k], s.g, run, skipped, hist, rep);
            cf_step(a, s);
        }
    }
    // the tail (and everything, when a pointer is not 16-byte aligned): one guarded element per lane and step
    for (long long i = nvec * VEC + tid; i < a.n; i += nthreads) {
        const CfPos s = cf_pos(a, i);
        cf_count(a, pred[i], lab[i], s.g, run, skipped, hist, rep);
    }
    cf_flush(run, hist, a.rshift, rep);
    if (skipped_out) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) skipped += __shfl_xor(skipped, off);
        if (lane == 0) cf_lds[words + wave] = skipped;
    }
    __syncthreads();
    // the copies of a cell are neighbours: up to 64 of them meet in a shuffle sum (the groups of rw lanes are whole: rw divides
    // 256 and `words`), the first lane of a group puts the sum back into its own word.  32 bits hold every sum: a launch counts
    // at most 2^31 elements
    const int rw = a.rshift < 6 ? 1 << a.rshift : 64;
    for (int w = threadIdx.x; w < words; w += CF_THREADS) {
        unsigned s = cf_lds[w];
        for (int off = rw >> 1; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if ((w & (rw - 1)) == 0) cf_lds[w] = s;
    }
    __syncthreads();
    const int parts = a.rshift > 6 ? 1 << (a.rshift - 6) : 1;
    for (int k = threadIdx.x; k < cells; k += CF_THREADS) {
        u64 s = 0;
        for (int j = 0; j < parts; ++j) s += cf_lds[(k << a.rshift) + (j << 6)];
        if (s) atomicAdd(counts + (a.g0 * a.C * a.C + k), s);
    }
    if (skipped_out && threadIdx.x == 0) {
        u64 s = 0;
        for (int w = 0; w < CF_WAVES; ++w) s += cf_lds[words + w];
        if (s) atomicAdd(skipped_out, s);
    }
}

int cf_elem_bytes(int type) { return type == ALQ_IDS_U8 ? 1 : type == ALQ_IDS_I32 ? 4 : type == ALQ_IDS_I64 ? 8 : 0; }

template <typename PT, typename LT>
int cf_launch(alq_ctx *ctx, const void *pred, const void *lab, const CfArgs &a, u64 *counts, u64 *skipped) {
    constexpr int VEC = 16 / (int)(sizeof(PT) < sizeof(LT) ? sizeof(PT) : sizeof(LT));
    const bool aligned = (((uintptr_t)pred | (uintptr_t)lab) & 15) == 0;
    const long long nvec = aligned ? a.n / VEC : 0;
    const long long work = nvec + (a.n - nvec * VEC);      // lane steps
    const long long blocks = std::min<long long>((work + CF_THREADS - 1) / CF_THREADS, (long long)ctx->num_cus * CF_BLOCKS_PER_CU);
    const int words = (a.gw * a.C * a.C) << a.rshift;
    const size_t lds = (size_t)(words + CF_WAVES) * sizeof(unsigned);
    ProfScope ps(ctx, PROF_EVAL, 0);
    hipLaunchKernelGGL((confusion_kernel<PT, LT>), dim3((unsigned)std::max<long long>(blocks, 1)), dim3(CF_THREADS), lds, ctx->stream,
                       static_cast<const PT *>(pred), static_cast<const LT *>(lab), a, nvec, counts, skipped);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

template <typename PT>
int cf_launch_lab(alq_ctx *ctx, const void *pred, const void *lab, int lab_type, const CfArgs &a, u64 *counts, u64 *skipped) {
    if (lab_type == ALQ_IDS_U8) return cf_launch<PT, unsigned char>(ctx, pred, lab, a, counts, skipped);
    if (lab_type == ALQ_IDS_I32) return cf_launch<PT, int>(ctx, pred, lab, a, counts, skipped);
    return cf_launch<PT, long long>(ctx, pred, lab, a, counts, skipped);
}

int cf_window(int C) { return std::max(1, CF_BLOCK_WORDS / (C * C)); }

}  // namespace

}  // namespace alq

using namespace alq;

extern "C" {

int alq_confusion_window(int C) { return (C >= 1 && C <= CF_MAX_C) ? cf_window(C) : 0; }

int alq_confusion_counts(alq_ctx *ctx, const void *d_pred, int pred_type, const void *d_lab, int lab_type, int64_t n, int64_t first,
                         int64_t inner, int64_t groups, int C, int fill, int64_t *d_counts, int64_t *d_skipped) {
    ALQ_REQUIRE(ctx && d_pred && d_lab && d_counts, ALQ_EINVAL, "alq_confusion_counts: null argument");
    const int pb = cf_elem_bytes(pred_type), lb = cf_elem_bytes(lab_type);
    ALQ_REQUIRE(pb && lb, ALQ_EINVAL, "alq_confusion_counts: id types %d / %d (ALQ_IDS_U8, _I32 or _I64)", pred_type, lab_type);
    ALQ_REQUIRE(C >= 1 && C <= CF_MAX_C, ALQ_EINVAL, "alq_confusion_counts: C = %d (1 .. %d)", C, CF_MAX_C);
    ALQ_REQUIRE(n >= 0 && first >= 0 && inner >= 1 && groups >= 1, ALQ_EINVAL,
                "alq_confusion_counts: bad argument (n=%lld first=%lld inner=%lld groups=%lld)", (long long)n, (long long)first, (long long)inner,
                (long long)groups);
    ALQ_REQUIRE(first <= INT64_MAX - n, ALQ_EINVAL, "alq_confusion_counts: first + n overflows");
    ALQ_REQUIRE(((uintptr_t)d_pred % pb) == 0 && ((uintptr_t)d_lab % lb) == 0 && ((uintptr_t)d_counts & 7) == 0 && ((uintptr_t)d_skipped & 7) == 0,
                ALQ_EINVAL, "alq_confusion_counts: a pointer is not aligned to its element");
    if (n == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(ctx->device));
    const int win = cf_window(C);
    // launches of at most 2^31 elements: the 32-bit counts of a lane, a wave and a block cannot wrap
    const int64_t step = (int64_t)1 << 31;
    for (int64_t at = 0; at < n; at += step) {
        CfArgs a;
        a.n = (long long)std::min<int64_t>(step, n - at);
        a.first = (long long)(first + at);
        a.inner = (long long)inner;
        a.groups = (long long)groups;
        a.C = C;
        a.fill = (fill >= 0 && fill < C) ? fill : -1;
        const int64_t lim = (int64_t)1 << 32;
        a.small = (a.first + a.n < lim && inner < lim && groups < lim) ? 1 : 0;
        const char *p = static_cast<const char *>(d_pred) + at * pb;
        const char *l = static_cast<const char *>(d_lab) + at * lb;
        for (int64_t g0 = 0; g0 < groups; g0 += win) {
            a.g0 = (long long)g0;
            a.gw = (int)std::min<int64_t>(win, groups - g0);
            const int cells = a.gw * C * C;
            a.rshift = 0;
            while (a.rshift < 8 && (cells << (a.rshift + 1)) <= CF_BLOCK_WORDS) ++a.rshift;
            u64 *cnt = reinterpret_cast<u64 *>(d_counts);
            u64 *skp = g0 == 0 ? reinterpret_cast<u64 *>(d_skipped) : nullptr;
            if (pred_type == ALQ_IDS_U8)
                ALQ_TRY(cf_launch_lab<unsigned char>(ctx, p, l, lab_type, a, cnt, skp));
            else if (pred_type == ALQ_IDS_I32)
                ALQ_TRY(cf_launch_lab<int>(ctx, p, l, lab_type, a, cnt, skp));
            else
                ALQ_TRY(cf_launch_lab<long long>(ctx, p, l, lab_type, a, cnt, skp));
        }
    }
    return ALQ_OK;
}

}  // extern "C"
