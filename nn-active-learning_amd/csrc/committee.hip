// Committee statistics of the `ensemble` and `QBC-JS` queries (PW_NNAL.py:453-545): for member i of M, the running means
//     av   = (p + i*av) / (i+1)                                        (float64, from the un-lifted p)
//     avH  = (ent(p) + i*avH) / (i+1)                                  (QBC-JS only)
//     ent(x) = -x*log(x) - (1-x)*log(1-x), an exact 0 in x or in 1-x lifted to 1e-6 first
// over the n pool rows of one rank, in ONE launch per member, and at the last member the top-k keys:
//     ensemble: |av - .5|                QBC-JS: 0.0 - (ent(av) - avH)
// Every operation is the reference's NumPy float64 operation in the reference's order.  Contraction is off in this file:
// hipcc compiles with fp-contract=fast, and a fused p + i*av (one rounding instead of two) would change the bits.  The only
// v_fma_f64 left in the device code are those inside the correctly rounded division (v_div_scale / v_rcp / v_fma /
// v_div_fmas / v_div_fixup) and inside log: the update's own products and sums are separate v_mul_f64 / v_add_f64.
// An HBM-streaming kernel (4 + 8 + 8 bytes in, 8 + 8 (+ 8) out per row; no reuse): grid-stride, 256 threads.
#include <algorithm>

#include "alq_internal.h"

#pragma clang fp contract(off)

namespace alq {

namespace {

__device__ inline double cm_lift(double x) { return x == 0.0 ? 1e-6 : x; }      // x[x == 0] += 1e-6: 0 + 1e-6 is 1e-6

// -x*log(x) - (1-x)*log(1-x) as the reference writes it: neg = 1 - x BEFORE x is lifted, then both lifted
__device__ inline double cm_ent(double x) {
    const double a = cm_lift(x);
    const double b = cm_lift(1.0 - x);
    return (-a) * log(a) - b * log(b);
}

template <int MODE>
__global__ __launch_bounds__(256) void committee_update_kernel(const float *__restrict__ p1, long long n, int member,
                                                               double *__restrict__ mean_p, double *__restrict__ mean_h,
                                                               double *__restrict__ keys) {
    const double fi = (double)member, fi1 = (double)(member + 1);
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const double p = (double)p1[r];
        // member 0: (p + 0*0) / 1 with the reference's integer 0 as the mean - the buffers are not read
        const double av = member == 0 ? (p + 0.0) / 1.0 : (p + fi * mean_p[r]) / fi1;
        mean_p[r] = av;
        if (MODE == ALQ_COMMITTEE_QBC_JS) {
            const double h = cm_ent(p);
            const double avh = member == 0 ? (h + 0.0) / 1.0 : (h + fi * mean_h[r]) / fi1;
            mean_h[r] = avh;
            if (keys) {
                const double score = cm_ent(av) - avh;
                keys[r] = 0.0 - score;          // not -score: a +0 score gives +0, never -0 (equal keys, exact row sums)
            }
        } else if (keys) {
            keys[r] = fabs(av - 0.5);
        }
    }
}

}  // namespace

int committee_update_impl(alq_ctx *ctx, const float *d_p1, int64_t n, int member, int mode, double *d_mean_p, double *d_mean_h,
                          double *d_keys) {
    const long long blocks = std::min<long long>((n + 255) / 256, (long long)ctx->num_cus * 8);
    ProfScope ps(ctx, PROF_COMMITTEE, 0);
    const dim3 grid((unsigned)std::max<long long>(blocks, 1));
    if (mode == ALQ_COMMITTEE_QBC_JS)
        hipLaunchKernelGGL(committee_update_kernel<ALQ_COMMITTEE_QBC_JS>, grid, dim3(256), 0, ctx->stream, d_p1, (long long)n, member,
                           d_mean_p, d_mean_h, d_keys);
    else
        hipLaunchKernelGGL(committee_update_kernel<ALQ_COMMITTEE_ENSEMBLE>, grid, dim3(256), 0, ctx->stream, d_p1, (long long)n, member,
                           d_mean_p, d_mean_h, d_keys);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // namespace alq
