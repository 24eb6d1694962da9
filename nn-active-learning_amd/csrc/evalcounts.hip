// Confusion counts of a test-set evaluation (PW_analyze_results.get_preds_stats, PW_analyze_results.py:234-258): for every
// evaluated voxel i with prediction pred[i] and label l = mask[inds[i]] (or mask[i] when there is no index vector)
//     P += l > 0    N += l == 0    TP += pred > 0 && l > 0    FP += pred > 0 && l == 0
//     TN += pred == 0 && l == 0    FN += pred == 0 && l > 0
// added to six running int64 totals that stay on the device, and optionally seg[inds[i]] = pred[i] (the uint8 volume of
// full_model_eval, :613-625 / :663-665; seg[i] when there is no index vector).  A NaN or negative label satisfies none of
// the comparisons and counts nowhere, like NumPy's.  Integers only: per 64-sample step a wave ballots each predicate and adds the popcount to a wave-uniform counter,
// the four waves of a block meet in LDS, and the block issues at most one 64-bit atomic add per counter - the totals are
// exact, whatever the grid, the chunking or the order the blocks retire in.
// An index outside [0, mask_elems) reads nothing, writes nothing, counts nowhere and raises the flag word.
// An HBM-streaming kernel (8 + 8 + 4 or 8 bytes in, 1 out per sample; no reuse): grid-stride, 256 threads.
#include <algorithm>

#include "alq_internal.h"

namespace alq {

namespace {

constexpr int EC_THREADS = 256;
constexpr int EC_WAVES = EC_THREADS / 64;

template <typename MaskT, bool HAS_INDS>
__global__ __launch_bounds__(EC_THREADS) void eval_counts_kernel(const long long *__restrict__ pred, const long long *__restrict__ inds,
                                                                 long long n, const MaskT *__restrict__ mask, long long mask_elems,
                                                                 unsigned long long *__restrict__ counts, unsigned char *__restrict__ seg,
                                                                 int *__restrict__ bad) {
    __shared__ unsigned int part[EC_WAVES][6];
    unsigned int c[6] = {0, 0, 0, 0, 0, 0};       // wave-uniform: at most n / gridDim per block < 2^32 (the launcher bounds n per launch)
    bool any_bad = false;
    // every lane of a block walks the same number of steps, so each ballot sees the whole wave
    for (long long base = blockIdx.x * (long long)EC_THREADS; base < n; base += (long long)gridDim.x * EC_THREADS) {
        const long long r = base + threadIdx.x;
        bool pos = false, zero = false, ppos = false, pzero = false;
        if (r < n) {
            long long at = r;
            bool ok = true;
            if (HAS_INDS) {
                at = inds[r];
                ok = at >= 0 && at < mask_elems;
                any_bad |= !ok;
            }
            if (ok) {
                const long long p = pred[r];
                const MaskT l = mask[at];
                pos = l > (MaskT)0;
                zero = l == (MaskT)0;
                ppos = p > 0;
                pzero = p == 0;
                if (seg) seg[at] = (unsigned char)p;
            }
        }
        c[0] += __popcll(__ballot(pos));
        c[1] += __popcll(__ballot(zero));
        c[2] += __popcll(__ballot(ppos && pos));
        c[3] += __popcll(__ballot(ppos && zero));
        c[4] += __popcll(__ballot(pzero && zero));
        c[5] += __popcll(__ballot(pzero && pos));
    }
    if (HAS_INDS && any_bad) atomicOr(bad, 1);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        for (int k = 0; k < 6; ++k) part[wave][k] = c[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned long long s = 0;
        for (int w = 0; w < EC_WAVES; ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(&counts[threadIdx.x], s);
    }
}

}  // namespace

int eval_counts_impl(alq_ctx *ctx, const int64_t *d_pred, const int64_t *d_inds, int64_t n, const void *d_mask, int mask_is_f64,
                     int64_t mask_elems, int64_t *d_counts, uint8_t *d_seg, int *d_bad) {
    // launches of at most 2^31 samples: a block's 32-bit partial counts cannot wrap
    const int64_t step = (int64_t)1 << 31;
    for (int64_t a = 0; a < n; a += step) {
        const long long cnt = (long long)std::min<int64_t>(step, n - a);
        const long long blocks = std::min<long long>((cnt + EC_THREADS - 1) / EC_THREADS, (long long)ctx->num_cus * 8);
        const dim3 grid((unsigned)std::max<long long>(blocks, 1));
        const long long *p = reinterpret_cast<const long long *>(d_pred) + a;
        unsigned long long *c = reinterpret_cast<unsigned long long *>(d_counts);
        ProfScope ps(ctx, PROF_EVAL, 0);
        if (d_inds) {
            const long long *ix = reinterpret_cast<const long long *>(d_inds) + a;
            if (mask_is_f64)
                hipLaunchKernelGGL((eval_counts_kernel<double, true>), grid, dim3(EC_THREADS), 0, ctx->stream, p, ix, cnt,
                                   static_cast<const double *>(d_mask), (long long)mask_elems, c, d_seg, d_bad);
            else
                hipLaunchKernelGGL((eval_counts_kernel<float, true>), grid, dim3(EC_THREADS), 0, ctx->stream, p, ix, cnt,
                                   static_cast<const float *>(d_mask), (long long)mask_elems, c, d_seg, d_bad);
        } else {
            if (mask_is_f64)
                hipLaunchKernelGGL((eval_counts_kernel<double, false>), grid, dim3(EC_THREADS), 0, ctx->stream, p, (const long long *)nullptr, cnt,
                                   static_cast<const double *>(d_mask) + a, (long long)mask_elems, c, d_seg ? d_seg + a : nullptr, d_bad);
            else
                hipLaunchKernelGGL((eval_counts_kernel<float, false>), grid, dim3(EC_THREADS), 0, ctx->stream, p, (const long long *)nullptr, cnt,
                                   static_cast<const float *>(d_mask) + a, (long long)mask_elems, c, d_seg ? d_seg + a : nullptr, d_bad);
        }
        ALQ_HIP(hipGetLastError());
    }
    return ALQ_OK;
}

}  // namespace alq
