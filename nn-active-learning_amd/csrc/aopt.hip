// The O(n) side of the A-optimal design solve behind the `fi` query (NNAL_tools._aopt_newton: min tr((sum q_i A_i)^-1) over
// the simplex, the lambda = 0 form of the reference's query SDP, NNAL_tools.py:612-659).  A Newton step of the log-barrier
// method is four elementwise maps over the candidates, each followed by a reduction with O(m^2) output, m = L(L+1)/2 <= 36;
// everything of size m stays on the host (DeviceSession.aopt_design).  All arithmetic is fp64.
//
// Determinism: a candidate tile is AO_T = 64 candidates; a launch uses min(tiles, AO_MAXB) workgroups, workgroup b walks the
// tiles b, b + grid, ... in order, every reduced entry is owned by one lane (or reduced over a wave by a fixed xor butterfly)
// and added in candidate order; the per-workgroup partials are folded in workgroup order by one combine launch.  No atomics,
// no grid barrier: the same inputs give the same bits on every run.
// The elementwise maps are written without fused multiply-adds (this file is built with -ffp-contract=off), in the operation
// order tests/aopt_ref.py states: every term of every sum is then the same IEEE double on the host and on the device, and
// only the summation order (and, in the combine, nothing else) separates the two.  The reductions use explicit fma().
#include "alq_internal.h"

namespace alq {

#define ALQ_LAUNCH_CHECK() ALQ_HIP(hipGetLastError())

constexpr int AO_T = 64;          // candidates per tile
constexpr int AO_MAXM = 36;       // L = 8
constexpr int AO_MAXB = 256;      // workgroups (and partial rows) per launch (1024 was slower, profiles/aopt_solve_grid1024.json: the combine walks the rows in order)
constexpr int AO_MAXJ = 64;       // line-search candidates per launch
constexpr int AO_VS = AO_MAXM + 1;   // LDS row stride of a V tile: odd, lanes that differ in the candidate hit different banks
constexpr int AO_US = AO_MAXM + 3;   // LDS row stride of the augmented u tile (u, r, 1), odd as well
constexpr int AO_MAXOUT = (AO_MAXM + 2) * (AO_MAXM + 3) / 2 + 1;

struct AoVec { double v[AO_MAXM]; };
struct AoAlpha { double a[AO_MAXJ]; };

__device__ __forceinline__ double ao_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double ao_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double ao_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

// V[i, c] = A_i[a, b] (a == b) or sqrt(2) A_i[a, b] (a < b), c walking the upper triangle row by row (_svec_basis's columns)
__global__ __launch_bounds__(256) void aopt_svec_kernel(const double *A, long long total, int L, int m, double *V) {
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256LL) {
        const long long i = e / m;
        int rem = (int)(e - i * m), a = 0;
        while (rem >= L - a) { rem -= L - a; ++a; }
        const int b = a + rem;
        const double x = A[i * L * L + a * L + b];
        V[e] = (a == b) ? x : x * 1.4142135623730951;
    }
}

// stages the V rows of one tile; rows beyond n are zeros and are never read from memory
__device__ __forceinline__ void ao_load_tile(const double *V, long long base, int cnt, int m, int nthreads, double *Vt) {
    for (int e = threadIdx.x; e < AO_T * m; e += nthreads) {
        const int ii = e / m, j = e - ii * m;
        Vt[ii * AO_VS + j] = (ii < cnt) ? V[base * m + e] : 0.0;
    }
}

// Launch A.  Per candidate u~ = (R^T V_i, r_i, 1) and w_i; the workgroup's partial is the upper triangle of
// sum_i w_i u~ u~^T (row by row, (m+2)(m+3)/2 entries: G, h_r, h_1, s_r, s_1 are its blocks) and then max d_i.
__global__ __launch_bounds__(256) void aopt_stats_kernel(const double *V, const double *q, int n, int m, AoVec kv, const double *R,
                                                         double mu, double obj, int ntiles, double *part) {
    __shared__ double Rs[AO_MAXM * AO_MAXM], Vt[AO_T * AO_VS], Ut[AO_T * AO_US], wt[AO_T], kvs[AO_MAXM];
    const int t = threadIdx.x, i = t & 63, kg = t >> 6;
    const int ma = m + 2, ne = ma * (ma + 1) / 2, nout = ne + 1;
    for (int e = t; e < m * m; e += 256) Rs[e] = R[e];
    if (t < m) kvs[t] = kv.v[t];
    int ea[3], eb[3];
    double acc[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int e = t + 256 * s;
        acc[s] = 0.0;
        ea[s] = eb[s] = -1;
        if (e < ne) {
            int rem = e, a = 0;
            while (rem >= ma - a) { rem -= ma - a; ++a; }
            ea[s] = a;
            eb[s] = a + rem;
        }
    }
    double mx = -INFINITY;
    const double c0 = obj + (double)n * mu;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();
        const long long base = (long long)tile * AO_T;
        const int cnt = (int)min((long long)AO_T, (long long)n - base);
        ao_load_tile(V, base, cnt, m, 256, Vt);
        __syncthreads();
        const bool live = i < cnt;
        if (kg == 0) {
            double w = 0.0, r = 0.0;
            if (live) {
                double d = 0.0;
                for (int j = 0; j < m; ++j) d = d + Vt[i * AO_VS + j] * kvs[j];
                const double qi = q[base + i];
                r = (-d - mu / qi) + c0;
                w = qi * qi / mu;
                mx = fmax(mx, d);
            }
            wt[i] = w;
            Ut[i * AO_US + m] = r;
            Ut[i * AO_US + m + 1] = live ? 1.0 : 0.0;
        }
        for (int k = kg; k < m; k += 4) {
            double u = 0.0;
            for (int j = 0; j < m; ++j) u = u + Vt[i * AO_VS + j] * Rs[j * m + k];
            Ut[i * AO_US + k] = u;
        }
        __syncthreads();
        for (int ii = 0; ii < AO_T; ++ii) {
            const double w = wt[ii];
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (ea[s] >= 0) acc[s] = fma(w * Ut[ii * AO_US + ea[s]], Ut[ii * AO_US + eb[s]], acc[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s)
        if (ea[s] >= 0) part[(long long)blockIdx.x * nout + t + 256 * s] = acc[s];
    if (kg == 0) {
        mx = ao_wave_max(mx);
        if (i == 0) part[(long long)blockIdx.x * nout + ne] = mx;
    }
}

// Launch B: like launch A the four waves share the m x m products u_i = R^T V_i of a tile (wave w: the columns k = w mod 4) through
// LDS; wave 0 then finishes the candidates, one lane each, the dot products over k left to right.
// partial = (-sum r_i dq_i, min over dq_i < 0 of -q_i / dq_i, sum_i dq_i V_i [m])
__global__ __launch_bounds__(256) void aopt_direction_kernel(const double *V, const double *q, int n, int m, AoVec kv, AoVec cr, AoVec c1,
                                                             const double *R, double ratio, double mu, double obj, int ntiles, double *dq,
                                                             double *part) {
    __shared__ double Rs[AO_MAXM * AO_MAXM], Vt[AO_T * AO_VS], Ut[AO_T * AO_US], dqs[AO_T];
    const int t = threadIdx.x, i = t & 63, kg = t >> 6, nout = 2 + m;
    for (int e = t; e < m * m; e += 256) Rs[e] = R[e];
    double accv = 0.0, rdq = 0.0, mn = INFINITY;
    const double c0 = obj + (double)n * mu;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();
        const long long base = (long long)tile * AO_T;
        const int cnt = (int)min((long long)AO_T, (long long)n - base);
        ao_load_tile(V, base, cnt, m, 256, Vt);
        __syncthreads();
        for (int k = kg; k < m; k += 4) {
            double u = 0.0;
            for (int j = 0; j < m; ++j) u = u + Vt[i * AO_VS + j] * Rs[j * m + k];
            Ut[i * AO_US + k] = u;
        }
        __syncthreads();
        if (kg == 0) {
            double dqi = 0.0;
            if (i < cnt) {
                double d = 0.0;
                for (int j = 0; j < m; ++j) d = d + Vt[i * AO_VS + j] * kv.v[j];
                const double qi = q[base + i];
                const double r = (-d - mu / qi) + c0;
                const double w = qi * qi / mu;
                double dr = 0.0, d1 = 0.0;
                for (int k = 0; k < m; ++k) {
                    const double wu = w * Ut[i * AO_US + k];
                    dr = dr + wu * cr.v[k];
                    d1 = d1 + wu * c1.v[k];
                }
                const double a = w * r - dr, b = w - d1;
                dqi = -a + ratio * b;
                dq[base + i] = dqi;
                rdq = fma(r, dqi, rdq);
                if (dqi < 0.0) mn = fmin(mn, -qi / dqi);
            }
            dqs[i] = dqi;
        }
        __syncthreads();
        if (t < m)
            for (int ii = 0; ii < AO_T; ++ii) accv = fma(dqs[ii], Vt[ii * AO_VS + t], accv);
    }
    double *p = part + (long long)blockIdx.x * nout;
    if (kg == 0) {
        rdq = ao_wave_sum(rdq);
        mn = ao_wave_min(mn);
        if (i == 0) { p[0] = -rdq; p[1] = mn; }
    }
    if (t < m) p[2 + t] = accv;
}

// Launch C: slot j < J is sum_i log(q_i + alpha_j dq_i), slot J is sum_i log q_i (alpha = 0).  Wave w owns the slots j = w mod 4;
// a tail lane holds (q, dq) = (1, 0): log 1 = 0 enters the butterfly
__global__ __launch_bounds__(256) void aopt_linesearch_kernel(const double *q, const double *dq, int n, AoAlpha al, int J, int ntiles,
                                                              double *part) {
    __shared__ double qs[AO_T], ds[AO_T], acc[AO_MAXJ + 1];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t <= J) acc[t] = 0.0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();
        const long long base = (long long)tile * AO_T;
        if (t < AO_T) {
            const bool live = base + t < n;
            qs[t] = live ? q[base + t] : 1.0;
            ds[t] = live ? dq[base + t] : 0.0;
        }
        __syncthreads();
        for (int j = wv; j <= J; j += 4) {
            const double a = (j < J) ? al.a[j] : 0.0;
            double v = log(qs[lane] + a * ds[lane]);
            v = ao_wave_sum(v);
            if (lane == 0) acc[j] = acc[j] + v;
        }
    }
    __syncthreads();
    if (t <= J) part[(long long)blockIdx.x * (J + 1) + t] = acc[t];
}

// Launch D, first kernel: q <- q + alpha dq, partial sums of the new q
__global__ __launch_bounds__(64) void aopt_step_kernel(double *q, const double *dq, int n, double alpha, int ntiles, double *part) {
    const int i = threadIdx.x;
    double s = 0.0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long e = (long long)tile * AO_T + i;
        if (e < n) {
            const double qn = q[e] + alpha * dq[e];
            q[e] = qn;
            s = s + qn;
        }
    }
    s = ao_wave_sum(s);
    if (i == 0) part[blockIdx.x] = s;
}
// second kernel: every workgroup folds the first kernel's partials in the same order (the same bits everywhere), divides its
// tiles by that sum and adds up q_i V_i.  partial = (the sum - workgroup 0 only, others 0 -, sum_i q_i V_i [m])
__global__ __launch_bounds__(64) void aopt_normalize_kernel(double *q, const double *V, int n, int m, int ntiles, const double *psum, int nb,
                                                            double *part) {
    __shared__ double qs[AO_T];
    const int i = threadIdx.x;
    double tot = 0.0;
    for (int b = i; b < nb; b += 64) tot = tot + psum[b];
    tot = ao_wave_sum(tot);
    double accv = 0.0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();
        const long long base = (long long)tile * AO_T;
        const int cnt = (int)min((long long)AO_T, (long long)n - base);
        double qi = 0.0;
        if (i < cnt) {
            qi = q[base + i] / tot;
            q[base + i] = qi;
        }
        qs[i] = qi;
        __syncthreads();
        if (i < m)
            for (int ii = 0; ii < cnt; ++ii) accv = fma(qs[ii], V[(base + ii) * m + i], accv);
    }
    double *p = part + (long long)blockIdx.x * (m + 1);
    if (i == 0) p[0] = (blockIdx.x == 0) ? tot : 0.0;
    if (i < m) p[1 + i] = accv;
}

// out[e] = fold over the workgroups' partial rows, in workgroup order; entry imax is a maximum, imin a minimum, the rest sums
__global__ __launch_bounds__(256) void aopt_combine_kernel(const double *part, int nb, int nout, int imax, int imin, double *out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nout) return;
    double s = part[e];
    if (e == imax) {
        for (int b = 1; b < nb; ++b) s = fmax(s, part[(long long)b * nout + e]);
    } else if (e == imin) {
        for (int b = 1; b < nb; ++b) s = fmin(s, part[(long long)b * nout + e]);
    } else {
        for (int b = 1; b < nb; ++b) s = s + part[(long long)b * nout + e];
    }
    out[e] = s;
}

static int ao_L_of_m(int m) {
    for (int L = 1; L <= 8; ++L)
        if (L * (L + 1) / 2 == m) return L;
    return 0;
}
static int ao_tiles(int64_t n) { return (int)((n + AO_T - 1) / AO_T); }
static int ao_grid(int64_t n) { const int t = ao_tiles(n); return t < AO_MAXB ? t : AO_MAXB; }

// the checks every launch shares: 1 <= L <= 8 (m = L(L+1)/2) and 1 <= n < 2^31 / m
static int ao_check(const char *who, const alq_ctx *ctx, int64_t n, int m) {
    ALQ_REQUIRE(ctx, ALQ_EINVAL, "%s: null context", who);
    ALQ_REQUIRE(m >= 1 && ao_L_of_m(m) != 0, ALQ_EUNSUPPORTED, "%s: m = %d is not L(L+1)/2 of an L in 1..8", who, m);
    ALQ_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) / m, ALQ_EUNSUPPORTED, "%s: n = %lld outside 1 <= n < 2^31 / m (m = %d)", who,
                (long long)n, m);
    return ALQ_OK;
}

static int ao_combine(alq_ctx *ctx, const double *part, int nb, int nout, int imax, int imin, double *d_out) {
    hipLaunchKernelGGL(aopt_combine_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, ctx->stream, part, nb, nout, imax, imin,
                       d_out);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

static void ao_vec(AoVec *dst, const double *src, int m) {
    for (int k = 0; k < AO_MAXM; ++k) dst->v[k] = k < m ? src[k] : 0.0;
}

}  // namespace alq

using namespace alq;

extern "C" {

int alq_aopt_tile(void) { return AO_T; }
int alq_aopt_max_workgroups(void) { return AO_MAXB; }

size_t alq_aopt_work_bytes(int64_t n, int L) {
    if (n < 1 || L < 1 || L > 8) return 0;
    // the staged R, then the partial rows of the widest launch (stats: AO_MAXOUT per workgroup; update: 1 + (m + 1) per workgroup)
    return ((size_t)AO_MAXM * AO_MAXM + (size_t)ao_grid(n) * (AO_MAXOUT + 1)) * sizeof(double);
}

int alq_aopt_svec(alq_ctx *ctx, const double *d_A, int64_t n, int L, double *d_V) {
    ALQ_REQUIRE(L >= 1 && L <= 8, ALQ_EUNSUPPORTED, "alq_aopt_svec: L = %d outside 1..8", L);
    const int m = L * (L + 1) / 2;
    ALQ_TRY(ao_check("alq_aopt_svec", ctx, n, m));
    ALQ_REQUIRE(d_A && d_V, ALQ_EINVAL, "alq_aopt_svec: null tensor");
    ALQ_HIP(hipSetDevice(ctx->device));
    const long long total = (long long)n * m;
    const long long g = (total + 255) / 256;
    hipLaunchKernelGGL(aopt_svec_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, ctx->stream, d_A, total, L, m, d_V);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

int alq_aopt_stats(alq_ctx *ctx, const double *d_V, const double *d_q, int64_t n, int m, const double *h_kvec, const double *h_R, double mu,
                   double obj, double *d_out, void *d_work) {
    ALQ_TRY(ao_check("alq_aopt_stats", ctx, n, m));
    ALQ_REQUIRE(d_V && d_q && h_kvec && h_R && d_out && d_work, ALQ_EINVAL, "alq_aopt_stats: null argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    ProfScope ps(ctx, PROF_REDUCE, (double)n * (2.0 * m * m + 3.0 * (m + 2) * (m + 3) / 2));
    double *d_R = reinterpret_cast<double *>(d_work), *part = d_R + AO_MAXM * AO_MAXM;
    ALQ_HIP(hipMemcpyAsync(d_R, h_R, sizeof(double) * m * m, hipMemcpyHostToDevice, ctx->stream));
    AoVec kv;
    ao_vec(&kv, h_kvec, m);
    const int nb = ao_grid(n), ne = (m + 2) * (m + 3) / 2;
    hipLaunchKernelGGL(aopt_stats_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_V, d_q, (int)n, m, kv, d_R, mu, obj, ao_tiles(n), part);
    ALQ_LAUNCH_CHECK();
    return ao_combine(ctx, part, nb, ne + 1, ne, -1, d_out);
}

int alq_aopt_direction(alq_ctx *ctx, const double *d_V, const double *d_q, int64_t n, int m, const double *h_kvec, const double *h_R,
                       const double *h_c_r, const double *h_c_1, double ratio, double mu, double obj, double *d_dq, double *d_out,
                       void *d_work) {
    ALQ_TRY(ao_check("alq_aopt_direction", ctx, n, m));
    ALQ_REQUIRE(d_V && d_q && h_kvec && h_R && h_c_r && h_c_1 && d_dq && d_out && d_work, ALQ_EINVAL, "alq_aopt_direction: null argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    ProfScope ps(ctx, PROF_REDUCE, (double)n * (2.0 * m * m + 8.0 * m));
    double *d_R = reinterpret_cast<double *>(d_work), *part = d_R + AO_MAXM * AO_MAXM;
    ALQ_HIP(hipMemcpyAsync(d_R, h_R, sizeof(double) * m * m, hipMemcpyHostToDevice, ctx->stream));
    AoVec kv, cr, c1;
    ao_vec(&kv, h_kvec, m);
    ao_vec(&cr, h_c_r, m);
    ao_vec(&c1, h_c_1, m);
    const int nb = ao_grid(n);
    hipLaunchKernelGGL(aopt_direction_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_V, d_q, (int)n, m, kv, cr, c1, d_R, ratio, mu, obj,
                       ao_tiles(n), d_dq, part);
    ALQ_LAUNCH_CHECK();
    return ao_combine(ctx, part, nb, 2 + m, -1, 1, d_out);
}

int alq_aopt_linesearch(alq_ctx *ctx, const double *d_q, const double *d_dq, int64_t n, const double *h_alpha, int J, double *d_out,
                        void *d_work) {
    ALQ_TRY(ao_check("alq_aopt_linesearch", ctx, n, 1));
    ALQ_REQUIRE(J >= 0 && J <= AO_MAXJ, ALQ_EUNSUPPORTED, "alq_aopt_linesearch: J = %d outside 0..%d", J, AO_MAXJ);
    ALQ_REQUIRE(d_q && d_dq && (J == 0 || h_alpha) && d_out && d_work, ALQ_EINVAL, "alq_aopt_linesearch: null argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    ProfScope ps(ctx, PROF_REDUCE, (double)n * (J + 1) * 2.0);
    double *part = reinterpret_cast<double *>(d_work) + AO_MAXM * AO_MAXM;
    AoAlpha al;
    for (int j = 0; j < AO_MAXJ; ++j) al.a[j] = j < J ? h_alpha[j] : 0.0;
    const int nb = ao_grid(n);
    hipLaunchKernelGGL(aopt_linesearch_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_q, d_dq, (int)n, al, J, ao_tiles(n), part);
    ALQ_LAUNCH_CHECK();
    return ao_combine(ctx, part, nb, J + 1, -1, -1, d_out);
}

int alq_aopt_update(alq_ctx *ctx, double *d_q, const double *d_dq, const double *d_V, int64_t n, int m, double alpha, double *d_out,
                    void *d_work) {
    ALQ_TRY(ao_check("alq_aopt_update", ctx, n, m));
    ALQ_REQUIRE(d_q && d_dq && d_V && d_out && d_work, ALQ_EINVAL, "alq_aopt_update: null argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    ProfScope ps(ctx, PROF_REDUCE, (double)n * (2.0 * m + 4.0));
    const int nb = ao_grid(n), nt = ao_tiles(n);
    double *psum = reinterpret_cast<double *>(d_work) + AO_MAXM * AO_MAXM, *part = psum + nb;   // nb (m + 2) <= nb (AO_MAXOUT + 1)
    hipLaunchKernelGGL(aopt_step_kernel, dim3(nb), dim3(64), 0, ctx->stream, d_q, d_dq, (int)n, alpha, nt, psum);
    ALQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(aopt_normalize_kernel, dim3(nb), dim3(64), 0, ctx->stream, d_q, d_V, (int)n, m, nt, psum, nb, part);
    ALQ_LAUNCH_CHECK();
    return ao_combine(ctx, part, nb, m + 1, -1, -1, d_out);
}

}  // extern "C"
