// SLIC super-pixel over-segmentation of every axial slice of a resident subject (alq_slic; the NumPy statement the device equals
// byte for byte is nnal_amd/slic.py - there is no reference counterpart, the reference calls skimage.segmentation.slic):
//
//   quantise   q = clamp(rint((double(v) - lo_c) * scale_c), 0, 65535) per channel, out pixels (non-finite, mask byte 255) marked;
//              every later cluster sum is a 64-bit integer sum, so the centres do not depend on the order of the reduction.
//   iterate    T x (assign, update).  assign: a workgroup owns a 16 x 16 pixel tile of a slice, stages the centres of every cell
//              its pixels may name (at most 18 x 18 cells: the home cells of the tile and one ring) in LDS, and each lane
//              compares its pixel, held in registers, with its up to nine candidates in ascending k.  d is formed operation by
//              operation (this file is compiled with -ffp-contract=off).  update: one wave per cluster gathers the members from
//              the pixel window of its 3 x 3 cells (gSLIC: a cluster never leaves that window), lanes add 64-bit integers, a
//              shuffle tree folds them, lane 0 divides.  No atomics: nothing to order.
//   connect    the atomic-min union-find of ccl.hip (unionfind.h) over pixels of equal cluster label (left and upper
//              neighbour), exact sizes by integer atomics, the kept component of a cluster by atomicMax of (size << 32) | ~root,
//              adoption rounds inside ONE launch (a workgroup owns a slice and loops scan / apply on an LDS flag: no host
//              round trip), a second union over the orphans no round adopted, first pixels by atomicMin, ranks by a workgroup
//              scan per slice, and a last pass that writes the labels in either layout.
// All index arithmetic is 32-bit: the call refuses 2^31 pixels and more.  Work volumes are [Z, H, W] like the packed subject.
// Every grid is capped (sl_cap: 8 workgroups per CU; ALQ_SLIC_MAX_GROUPS overrides for tests and tuning, same bytes for every
// value) and strides: the stream kernels over pixels, assign over (slice, tile), update over (slice, cluster) by waves, the two
// per-slice kernels over slices.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "alq_internal.h"
#include "unionfind.h"

#pragma clang fp contract(off)

namespace alq {

namespace {

typedef unsigned long long u64;
typedef unsigned short u16;

constexpr int SL_THREADS = 256;
constexpr int SL_WAVES = SL_THREADS / 64;      // clusters one update workgroup reduces at a time
constexpr int SL_TILE = 16;                    // assign: pixels per tile side
constexpr int SL_RING = SL_TILE + 2;           // cells per side a tile may name
constexpr int SL_MAXM = 8;
constexpr int SL_SLICE_THREADS = 1024;         // the per-slice kernels (adoption, ranks)
constexpr int SL_NONE = 0x7fffffff;

struct SlGeo {
    int H, W, Z, m, gh, gw, K;
    int HW, N;           // pixels of a slice, of the subject
    int nty, ntx;        // assign tiles per slice
};

struct SlQuant {
    double lo[SL_MAXM], scale[SL_MAXM];
};

__device__ inline int sl_cell_start(int i, int D, int g) { return (int)(((long long)i * D + g - 1) / g); }      // first y with y g / D >= i

// ---- quantise --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SL_THREADS) void slic_quant_kernel(const float *__restrict__ vol, const unsigned char *__restrict__ mask, SlGeo g,
                                                                SlQuant qp, u16 *__restrict__ q, int *__restrict__ lab) {
    for (long long vl = blockIdx.x * (long long)SL_THREADS + threadIdx.x; vl < g.N; vl += (long long)gridDim.x * SL_THREADS) {
        const int v = (int)vl;
        bool in = !(mask && mask[v] == 255);
        for (int c = 0; c < g.m; ++c) {
            const float f = vol[(long long)v * g.m + c];
            const bool fin = isfinite(f);
            in = in && fin;
            const double t = ((double)(fin ? f : 0.0f) - qp.lo[c]) * qp.scale[c];
            double r = rint(t);
            r = r < 0.0 ? 0.0 : (r > 65535.0 ? 65535.0 : r);
            q[(long long)v * g.m + c] = (u16)(int)r;
        }
        const int x = v % g.W, y = (v / g.W) % g.H;
        lab[v] = in ? (int)(((long long)y * g.gh) / g.H) * g.gw + (int)(((long long)x * g.gw) / g.W) : -1;
    }
}

// centre record of cluster (z, k): m channel means, cy, cx
__global__ __launch_bounds__(SL_THREADS) void slic_start_kernel(SlGeo g, const u16 *__restrict__ q, const int *__restrict__ lab,
                                                                double *__restrict__ cen) {
    const long long total = (long long)g.Z * g.K;
    for (long long e = blockIdx.x * (long long)SL_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * SL_THREADS) {
        const int k = (int)(e % g.K), z = (int)(e / g.K);
        const int i = k / g.gw, j = k % g.gw;
        const int py = (int)(((2LL * i + 1) * g.H) / (2LL * g.gh)), px = (int)(((2LL * j + 1) * g.W) / (2LL * g.gw));
        const int v = (z * g.H + py) * g.W + px;
        const bool in = lab[v] >= 0;
        double *c = cen + e * (g.m + 2);
        for (int ch = 0; ch < g.m; ++ch) c[ch] = in ? (double)q[(long long)v * g.m + ch] : 0.0;
        c[g.m] = (double)py;
        c[g.m + 1] = (double)px;
    }
}

// ---- assign ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SL_THREADS) void slic_assign_kernel(SlGeo g, const u16 *__restrict__ q, const double *__restrict__ cen, double w,
                                                                 int *__restrict__ lab) {
    __shared__ double sc[SL_RING * SL_RING * (SL_MAXM + 2)];
    __shared__ int home[2][SL_TILE];      // home cell row of the tile's rows, home cell column of its columns
    const int rec = g.m + 2;
    const int tx = threadIdx.x % SL_TILE, ty = threadIdx.x / SL_TILE;
    const long long ntiles = (long long)g.Z * g.nty * g.ntx;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int z = (int)(t / (g.nty * g.ntx));
        const int tt = (int)(t % (g.nty * g.ntx));
        const int y0 = (tt / g.ntx) * SL_TILE, x0 = (tt % g.ntx) * SL_TILE;
        const int y1 = min(y0 + SL_TILE, g.H) - 1, x1 = min(x0 + SL_TILE, g.W) - 1;
        const int ci0 = max((int)(((long long)y0 * g.gh) / g.H) - 1, 0), ci1 = min((int)(((long long)y1 * g.gh) / g.H) + 1, g.gh - 1);
        const int cj0 = max((int)(((long long)x0 * g.gw) / g.W) - 1, 0), cj1 = min((int)(((long long)x1 * g.gw) / g.W) + 1, g.gw - 1);
        const int nci = ci1 - ci0 + 1, ncj = cj1 - cj0 + 1;      // each <= SL_RING: home cells rise by at most one per pixel
        if (threadIdx.x < SL_TILE) home[0][threadIdx.x] = (int)(((long long)min(y0 + (int)threadIdx.x, g.H - 1) * g.gh) / g.H);
        else if (threadIdx.x < 2 * SL_TILE) home[1][threadIdx.x - SL_TILE] = (int)(((long long)min(x0 + (int)threadIdx.x - SL_TILE, g.W - 1) * g.gw) / g.W);
        for (int e = threadIdx.x; e < nci * ncj * rec; e += SL_THREADS) {
            const int f = e % rec, cell = e / rec;
            const int k = (ci0 + cell / ncj) * g.gw + cj0 + cell % ncj;
            sc[e] = cen[((long long)z * g.K + k) * rec + f];
        }
        __syncthreads();
        const int y = y0 + ty, x = x0 + tx;
        if (y <= y1 && x <= x1) {
            const int v = (z * g.H + y) * g.W + x;
            if (lab[v] >= 0) {
                double qd[SL_MAXM];
#pragma unroll
                for (int c = 0; c < SL_MAXM; ++c) qd[c] = c < g.m ? (double)q[(long long)v * g.m + c] : 0.0;
                const int hi = home[0][ty], hj = home[1][tx];
                const double yd = (double)y, xd = (double)x;
                double best = __longlong_as_double(0x7ff0000000000000LL);      // +inf
                int bk = hi * g.gw + hj;
                for (int di = -1; di <= 1; ++di) {
                    const int ci = hi + di;
                    if (ci < 0 || ci >= g.gh) continue;
                    for (int dj = -1; dj <= 1; ++dj) {
                        const int cj = hj + dj;
                        if (cj < 0 || cj >= g.gw) continue;
                        const double *c = sc + ((ci - ci0) * ncj + (cj - cj0)) * rec;
                        double t0 = qd[0] - c[0];
                        double acc = t0 * t0;
#pragma unroll
                        for (int ch = 1; ch < SL_MAXM; ++ch) {
                            if (ch < g.m) {
                                const double tc = qd[ch] - c[ch];
                                acc = acc + tc * tc;
                            }
                        }
                        const double dy = yd - c[g.m], dx = xd - c[g.m + 1];
                        const double s = dy * dy + dx * dx;
                        const double d = acc + w * s;
                        if (d < best) {
                            best = d;
                            bk = ci * g.gw + cj;
                        }
                    }
                }
                lab[v] = bk;
            }
        }
        __syncthreads();      // the next tile's centres overwrite sc
    }
}

// ---- update ----------------------------------------------------------------------------------------------------------------
__device__ inline u64 sl_wave_sum(u64 s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)s, off), hi = __shfl_xor((unsigned)(s >> 32), off);
        s += ((u64)hi << 32) | lo;
    }
    return s;
}

__global__ __launch_bounds__(SL_THREADS) void slic_update_kernel(SlGeo g, const u16 *__restrict__ q, const int *__restrict__ lab,
                                                                 double *__restrict__ cen) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long total = (long long)g.Z * g.K;
    for (long long e = blockIdx.x * (long long)SL_WAVES + wave; e < total; e += (long long)gridDim.x * SL_WAVES) {      // wave-uniform
        const int k = (int)(e % g.K), z = (int)(e / g.K);
        const int i = k / g.gw, j = k % g.gw;
        const int wy0 = sl_cell_start(max(i - 1, 0), g.H, g.gh), wy1 = sl_cell_start(min(i + 2, g.gh), g.H, g.gh);
        const int wx0 = sl_cell_start(max(j - 1, 0), g.W, g.gw), wx1 = sl_cell_start(min(j + 2, g.gw), g.W, g.gw);
        const int ww = wx1 - wx0, npx = (wy1 - wy0) * ww;
        u64 n = 0, sy = 0, sx = 0, sq[SL_MAXM];
#pragma unroll
        for (int c = 0; c < SL_MAXM; ++c) sq[c] = 0;
        // a lane's pixels are 64 apart in the window's raster order: (row, column) advance by (64 / ww, 64 % ww) with a carry, so the
        // two divisions are per cluster, not per pixel; four labels are loaded before the first is looked at (the sweep is a chain
        // of load latencies otherwise)
        const int step_y = 64 / ww, step_x = 64 % ww;
        int py = lane / ww, px = lane % ww;
        for (int p = lane; p < npx; p += 4 * 64) {
            int vv[4], yy[4], xx[4], ll[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                yy[u] = wy0 + py;
                xx[u] = wx0 + px;
                vv[u] = (z * g.H + yy[u]) * g.W + xx[u];
                ll[u] = p + u * 64 < npx ? lab[vv[u]] : -1;
                px += step_x;
                py += step_y;
                if (px >= ww) {
                    px -= ww;
                    ++py;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (ll[u] != k) continue;
                n += 1;
                sy += (u64)yy[u];
                sx += (u64)xx[u];
#pragma unroll
                for (int c = 0; c < SL_MAXM; ++c)
                    if (c < g.m) sq[c] += (u64)q[(long long)vv[u] * g.m + c];
            }
        }
        n = sl_wave_sum(n);
        if (n == 0) continue;      // an empty cluster keeps its centre (wave-uniform)
        sy = sl_wave_sum(sy);
        sx = sl_wave_sum(sx);
        double *c = cen + e * (g.m + 2);
        const double nd = (double)n;
#pragma unroll
        for (int ch = 0; ch < SL_MAXM; ++ch) {
            if (ch < g.m) {
                const u64 s = sl_wave_sum(sq[ch]);
                if (lane == 0) c[ch] = (double)s / nd;
            }
        }
        if (lane == 0) {
            c[g.m] = (double)sy / nd;
            c[g.m + 1] = (double)sx / nd;
        }
    }
}

// ---- connectivity ------------------------------------------------------------------------------------------------------------
// reg[v] = v on in pixels, -1 elsewhere; size = 0; best = none; the cluster keys of the slice = 0
__global__ __launch_bounds__(SL_THREADS) void slic_cc_init_kernel(SlGeo g, const int *__restrict__ lab, int *__restrict__ reg,
                                                                  unsigned *__restrict__ size, int *__restrict__ best, u64 *__restrict__ ckey) {
    const long long nk = (long long)g.Z * g.K;
    for (long long vl = blockIdx.x * (long long)SL_THREADS + threadIdx.x; vl < max((long long)g.N, nk); vl += (long long)gridDim.x * SL_THREADS) {
        if (vl < g.N) {
            reg[vl] = lab[vl] >= 0 ? (int)vl : -1;
            size[vl] = 0;
            best[vl] = SL_NONE;
        }
        if (vl < nk) ckey[vl] = 0;
    }
}

// unite every in pixel with its left and upper neighbour of the same cluster
__global__ __launch_bounds__(SL_THREADS) void slic_cc_merge_kernel(SlGeo g, const int *__restrict__ lab, int *reg) {
    for (long long vl = blockIdx.x * (long long)SL_THREADS + threadIdx.x; vl < g.N; vl += (long long)gridDim.x * SL_THREADS) {
        const int v = (int)vl;
        const int l = lab[v];
        if (l < 0) continue;
        const int x = v % g.W, y = (v / g.W) % g.H;
        int top = v;
        if (x > 0 && lab[v - 1] == l) top = cc_unite(reg, top, v - 1);
        if (y > 0 && lab[v - g.W] == l) cc_unite(reg, top, v - g.W);
    }
}

// reg[v] = root, size[root] += 1 (integer atomics: exact)
__global__ __launch_bounds__(SL_THREADS) void slic_cc_compress_kernel(SlGeo g, int *reg, unsigned *size) {
    for (long long vl = blockIdx.x * (long long)SL_THREADS + threadIdx.x; vl < g.N; vl += (long long)gridDim.x * SL_THREADS) {
        const int v = (int)vl;
        if (reg[v] < 0) continue;
        const int r = cc_find(reg, v);
        reg[v] = r;
        atomicAdd(size + r, 1u);
    }
}

// per cluster the maximum of (size << 32) | ~(root inside the slice) over its components
__global__ __launch_bounds__(SL_THREADS) void slic_cc_key_kernel(SlGeo g, const int *__restrict__ lab, const int *__restrict__ reg,
                                                                 const unsigned *__restrict__ size, u64 *ckey) {
    for (long long vl = blockIdx.x * (long long)SL_THREADS + threadIdx.x; vl < g.N; vl += (long long)gridDim.x * SL_THREADS) {
        const int v = (int)vl;
        if (reg[v] != v) continue;
        const int z = v / g.HW;
        atomicMax(ckey + (long long)z * g.K + lab[v], ((u64)size[v] << 32) | (unsigned)~(unsigned)(v - z * g.HW));
    }
}

// size[root] becomes the kept flag: 1 for the winning component of a cluster if it has min_size pixels, 0 for an orphan
__global__ __launch_bounds__(SL_THREADS) void slic_cc_keep_kernel(SlGeo g, const int *__restrict__ lab, const int *__restrict__ reg,
                                                                  unsigned *__restrict__ size, const u64 *__restrict__ ckey, int min_size) {
    for (long long vl = blockIdx.x * (long long)SL_THREADS + threadIdx.x; vl < g.N; vl += (long long)gridDim.x * SL_THREADS) {
        const int v = (int)vl;
        if (reg[v] != v) continue;
        const int z = v / g.HW;
        const u64 key = ((u64)size[v] << 32) | (unsigned)~(unsigned)(v - z * g.HW);
        size[v] = (ckey[(long long)z * g.K + lab[v]] == key && size[v] >= (unsigned)min_size) ? 1u : 0u;
    }
}

// Adoption rounds of one slice per workgroup, until a round changes nothing.  scan: every pixel of an orphan looks at its four
// neighbours and offers the index of each that lies in a kept region to best[orphan root] (atomicMin); apply: every pixel of
// an orphan with an offer takes the region of the offered pixel - a pixel of a kept region, which no apply step writes, so
// the round decides on the regions as they stood when it began.  reg[] and best[] of this slice are written by this workgroup
// alone; they are read through agent-scope atomic loads so that no lane meets a stale L1 line of a word an atomic changed.
__global__ __launch_bounds__(SL_SLICE_THREADS) void slic_adopt_kernel(SlGeo g, int *reg, const unsigned *__restrict__ kept, int *best) {
    __shared__ int changed;
    for (int z = blockIdx.x; z < g.Z; z += gridDim.x) {
        const int base = z * g.HW;
        for (;;) {
            if (threadIdx.x == 0) changed = 0;
            __syncthreads();
            for (int p = threadIdx.x; p < g.HW; p += SL_SLICE_THREADS) {
                const int r = cc_load(reg + base + p);
                if (r < 0 || kept[r]) continue;
                const int x = p % g.W, y = p / g.W;
                // ascending neighbour index, though the minimum does not need the order
                if (y > 0) { const int rn = cc_load(reg + base + p - g.W); if (rn >= 0 && kept[rn]) atomicMin(best + r, base + p - g.W); }
                if (x > 0) { const int rn = cc_load(reg + base + p - 1); if (rn >= 0 && kept[rn]) atomicMin(best + r, base + p - 1); }
                if (x < g.W - 1) { const int rn = cc_load(reg + base + p + 1); if (rn >= 0 && kept[rn]) atomicMin(best + r, base + p + 1); }
                if (y < g.H - 1) { const int rn = cc_load(reg + base + p + g.W); if (rn >= 0 && kept[rn]) atomicMin(best + r, base + p + g.W); }
            }
            __syncthreads();
            for (int p = threadIdx.x; p < g.HW; p += SL_SLICE_THREADS) {
                const int r = cc_load(reg + base + p);
                if (r < 0 || kept[r]) continue;
                const int b = cc_load(best + r);
                if (b == SL_NONE) continue;
                __hip_atomic_store(reg + base + p, cc_load(reg + b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                changed = 1;
            }
            __syncthreads();
            const int c = changed;
            __syncthreads();      // everyone has read the flag before lane 0 clears it
            if (!c) break;
        }
    }
}

// orphans no round adopted unite with the unadopted orphans left of and above them, whatever their cluster
__global__ __launch_bounds__(SL_THREADS) void slic_orphan_merge_kernel(SlGeo g, int *reg, const unsigned *__restrict__ kept) {
    for (long long vl = blockIdx.x * (long long)SL_THREADS + threadIdx.x; vl < g.N; vl += (long long)gridDim.x * SL_THREADS) {
        const int v = (int)vl;
        const int r = cc_load(reg + v);
        if (r < 0 || kept[r]) continue;      // a hooked orphan root names another orphan root: kept[] is 0 for both
        const int x = v % g.W, y = (v / g.W) % g.H;
        int top = v;
        if (x > 0) { const int rn = cc_load(reg + v - 1); if (rn >= 0 && !kept[rn]) top = cc_unite(reg, top, v - 1); }
        if (y > 0) { const int rn = cc_load(reg + v - g.W); if (rn >= 0 && !kept[rn]) cc_unite(reg, top, v - g.W); }
    }
}

// reg[v] = root of the merged forest; best[root] = the first pixel of the region (only a pixel at or below the root can be it)
__global__ __launch_bounds__(SL_THREADS) void slic_first_kernel(SlGeo g, int *reg, int *best) {
    for (long long vl = blockIdx.x * (long long)SL_THREADS + threadIdx.x; vl < g.N; vl += (long long)gridDim.x * SL_THREADS) {
        const int v = (int)vl;
        if (reg[v] < 0) continue;
        const int r = cc_find(reg, v);
        reg[v] = r;
        if (v <= r) atomicMin(best + r, v);
    }
}

// ranks of one slice per workgroup: a lane owns a run of consecutive pixels, counts the first pixels in it, the workgroup scans
// the counts, the lane numbers its first pixels from its offset.  num[root] = rank, 1-based; nlab[z] = regions of the slice
__global__ __launch_bounds__(SL_SLICE_THREADS) void slic_rank_kernel(SlGeo g, const int *__restrict__ reg, const int *__restrict__ best,
                                                                     unsigned *__restrict__ num, int *__restrict__ nlab) {
    __shared__ int cnt[2][SL_SLICE_THREADS];
    const int chunk = (g.HW + SL_SLICE_THREADS - 1) / SL_SLICE_THREADS;
    for (int z = blockIdx.x; z < g.Z; z += gridDim.x) {
        const int base = z * g.HW;
        const int p0 = min(threadIdx.x * chunk, g.HW), p1 = min(p0 + chunk, g.HW);
        int mine = 0;
        for (int p = p0; p < p1; ++p) {
            const int r = reg[base + p];
            mine += (r >= 0 && best[r] == base + p) ? 1 : 0;
        }
        int cur = 0;
        cnt[0][threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < SL_SLICE_THREADS; off <<= 1) {      // inclusive scan, two buffers
            const int a = cnt[cur][threadIdx.x] + (threadIdx.x >= off ? cnt[cur][threadIdx.x - off] : 0);
            cnt[cur ^ 1][threadIdx.x] = a;
            cur ^= 1;
            __syncthreads();
        }
        int next = cnt[cur][threadIdx.x] - mine + 1;
        for (int p = p0; p < p1; ++p) {
            const int r = reg[base + p];
            if (r >= 0 && best[r] == base + p) num[r] = (unsigned)next++;
        }
        if (threadIdx.x == SL_SLICE_THREADS - 1) nlab[z] = cnt[cur][threadIdx.x];
        __syncthreads();      // cnt is reused by the next slice
    }
}

// out = num[reg] (0 on out pixels); hwz: out is [H, W, Z], else [Z, H, W]
__global__ __launch_bounds__(SL_THREADS) void slic_emit_kernel(SlGeo g, const int *__restrict__ reg, const unsigned *__restrict__ num, int hwz,
                                                               int *__restrict__ out) {
    for (long long el = blockIdx.x * (long long)SL_THREADS + threadIdx.x; el < g.N; el += (long long)gridDim.x * SL_THREADS) {
        const int e = (int)el;
        int v = e;
        if (hwz) {
            const int z = e % g.Z, yx = e / g.Z;
            v = z * g.HW + yx;
        }
        const int r = reg[v];
        out[e] = r >= 0 ? (int)num[r] : 0;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
int sl_cap(const alq_ctx *ctx) {
    const char *e = getenv("ALQ_SLIC_MAX_GROUPS");
    if (e && atoi(e) >= 1) return atoi(e);
    return (ctx ? ctx->num_cus : 256) * 8;
}

unsigned sl_grid(long long want, int cap) { return (unsigned)std::max<long long>(1, std::min<long long>(want, cap)); }

// 0: fine; otherwise the error code, message set
int sl_geometry(const int64_t dims[3], int m, int gh, int gw, const char *who, SlGeo *g) {
    ALQ_REQUIRE(dims, ALQ_EINVAL, "%s: null dims", who);
    ALQ_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && m >= 1, ALQ_EINVAL, "%s: dims %lld x %lld x %lld, m = %d (each >= 1)", who,
                (long long)dims[0], (long long)dims[1], (long long)dims[2], m);
    ALQ_REQUIRE(gh >= 1 && gh <= dims[0] && gw >= 1 && gw <= dims[1], ALQ_EINVAL, "%s: grid %d x %d outside [1, %lld] x [1, %lld]", who, gh, gw,
                (long long)dims[0], (long long)dims[1]);
    ALQ_REQUIRE(m <= SL_MAXM, ALQ_EUNSUPPORTED, "%s: m = %d above %d", who, m, SL_MAXM);
    const int64_t lim = (int64_t)1 << 31;
    ALQ_REQUIRE(dims[0] < lim && dims[1] < lim && dims[2] < lim && dims[0] * dims[1] < lim && dims[0] * dims[1] * dims[2] < lim, ALQ_EUNSUPPORTED,
                "%s: 2^31 pixels or more", who);
    g->H = (int)dims[0];
    g->W = (int)dims[1];
    g->Z = (int)dims[2];
    g->m = m;
    g->gh = gh;
    g->gw = gw;
    g->K = gh * gw;
    g->HW = g->H * g->W;
    g->N = g->HW * g->Z;
    g->nty = (g->H + SL_TILE - 1) / SL_TILE;
    g->ntx = (g->W + SL_TILE - 1) / SL_TILE;
    return ALQ_OK;
}

size_t sl_up8(size_t b) { return (b + 7) & ~(size_t)7; }

struct SlWork {
    double *cen;
    u64 *ckey;
    int *lab, *reg, *best;
    unsigned *size;
    u16 *q;
    size_t bytes;
};

SlWork sl_work(void *d_work, const SlGeo &g) {
    SlWork w;
    char *p = static_cast<char *>(d_work);
    const size_t zk = (size_t)g.Z * g.K, n = (size_t)g.N;
    size_t off = 0;
    w.cen = reinterpret_cast<double *>(p + off);
    off += zk * (g.m + 2) * 8;
    w.ckey = reinterpret_cast<u64 *>(p + off);
    off += zk * 8;
    w.lab = reinterpret_cast<int *>(p + off);
    off += sl_up8(n * 4);
    w.reg = reinterpret_cast<int *>(p + off);
    off += sl_up8(n * 4);
    w.best = reinterpret_cast<int *>(p + off);
    off += sl_up8(n * 4);
    w.size = reinterpret_cast<unsigned *>(p + off);
    off += sl_up8(n * 4);
    w.q = reinterpret_cast<u16 *>(p + off);
    off += sl_up8(n * g.m * 2);
    w.bytes = off;
    return w;
}

}  // namespace

}  // namespace alq

using namespace alq;

extern "C" {

size_t alq_slic_work_bytes(const int64_t dims[3], int m, int gh, int gw) {
    SlGeo g;
    if (sl_geometry(dims, m, gh, gw, "alq_slic_work_bytes", &g) != ALQ_OK) return 0;
    return sl_work(nullptr, g).bytes;
}

int alq_slic_geometry(alq_ctx *ctx, const int64_t dims[3], int m, int gh, int gw, int64_t out[8]) {
    ALQ_REQUIRE(ctx && out, ALQ_EINVAL, "alq_slic_geometry: null argument");
    SlGeo g;
    ALQ_TRY(sl_geometry(dims, m, gh, gw, "alq_slic_geometry", &g));
    const int cap = sl_cap(ctx);
    const long long tiles = (long long)g.Z * g.nty * g.ntx, zk = (long long)g.Z * g.K;
    out[0] = tiles;
    out[1] = sl_grid(tiles, cap);
    out[2] = SL_WAVES;
    out[3] = sl_grid((zk + SL_WAVES - 1) / SL_WAVES, cap);
    out[4] = sl_grid(g.Z, cap);
    out[5] = cap;
    out[6] = sl_grid(((long long)g.N + SL_THREADS - 1) / SL_THREADS, cap);
    out[7] = SL_TILE;
    return ALQ_OK;
}

int alq_slic(alq_ctx *ctx, const float *d_vol, const uint8_t *d_mask, const int64_t dims[3], int m, const double *lo, const double *scale, int gh,
             int gw, double w, int T, int min_size, int hwz, int32_t *d_labels, int32_t *d_nlabels, void *d_work) {
    ALQ_REQUIRE(ctx && d_vol && lo && scale && d_labels && d_nlabels && d_work, ALQ_EINVAL, "alq_slic: null argument");
    SlGeo g;
    ALQ_TRY(sl_geometry(dims, m, gh, gw, "alq_slic", &g));
    ALQ_REQUIRE(std::isfinite(w) && w >= 0.0, ALQ_EINVAL, "alq_slic: spatial weight %g (finite, >= 0)", w);
    ALQ_REQUIRE(T >= 0 && min_size >= 0, ALQ_EINVAL, "alq_slic: T = %d, min_size = %d (each >= 0)", T, min_size);
    ALQ_REQUIRE(hwz == 0 || hwz == 1, ALQ_EINVAL, "alq_slic: hwz = %d (0 or 1)", hwz);
    ALQ_REQUIRE(((uintptr_t)d_work & 7) == 0 && ((uintptr_t)d_labels & 3) == 0 && ((uintptr_t)d_nlabels & 3) == 0 && ((uintptr_t)d_vol & 3) == 0,
                ALQ_EINVAL, "alq_slic: misaligned pointer (d_work 8 bytes, the others 4)");
    SlQuant qp;
    for (int c = 0; c < SL_MAXM; ++c) {
        qp.lo[c] = c < m ? lo[c] : 0.0;
        qp.scale[c] = c < m ? scale[c] : 0.0;
        ALQ_REQUIRE(std::isfinite(qp.lo[c]) && std::isfinite(qp.scale[c]), ALQ_EINVAL, "alq_slic: lo / scale of channel %d not finite", c);
    }
    ALQ_HIP(hipSetDevice(ctx->device));
    const SlWork k = sl_work(d_work, g);
    const int cap = sl_cap(ctx);
    const dim3 blk(SL_THREADS), sgrid(sl_grid(((long long)g.N + SL_THREADS - 1) / SL_THREADS, cap));
    const long long zk = (long long)g.Z * g.K;
    const dim3 kgrid(sl_grid((zk + SL_THREADS - 1) / SL_THREADS, cap));
    {
        ProfScope ps(ctx, PROF_ELEMWISE, 0);
        hipLaunchKernelGGL(slic_quant_kernel, sgrid, blk, 0, ctx->stream, d_vol, (const unsigned char *)d_mask, g, qp, k.q, k.lab);
        ALQ_HIP(hipGetLastError());
        hipLaunchKernelGGL(slic_start_kernel, kgrid, blk, 0, ctx->stream, g, (const u16 *)k.q, (const int *)k.lab, k.cen);
        ALQ_HIP(hipGetLastError());
    }
    const dim3 agrid(sl_grid((long long)g.Z * g.nty * g.ntx, cap)), ugrid(sl_grid((zk + SL_WAVES - 1) / SL_WAVES, cap));
    for (int t = 0; t < T; ++t) {
        {
            ProfScope ps(ctx, PROF_ELEMWISE, 0);
            hipLaunchKernelGGL(slic_assign_kernel, agrid, blk, 0, ctx->stream, g, (const u16 *)k.q, (const double *)k.cen, w, k.lab);
            ALQ_HIP(hipGetLastError());
        }
        ProfScope ps(ctx, PROF_REDUCE, 0);
        hipLaunchKernelGGL(slic_update_kernel, ugrid, blk, 0, ctx->stream, g, (const u16 *)k.q, (const int *)k.lab, k.cen);
        ALQ_HIP(hipGetLastError());
    }
    const dim3 zgrid(sl_grid(g.Z, cap)), zblk(SL_SLICE_THREADS);
    const dim3 igrid(sl_grid((std::max<long long>(g.N, zk) + SL_THREADS - 1) / SL_THREADS, cap));
    ProfScope ps(ctx, PROF_REDUCE, 0);
    hipLaunchKernelGGL(slic_cc_init_kernel, igrid, blk, 0, ctx->stream, g, (const int *)k.lab, k.reg, k.size, k.best, k.ckey);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(slic_cc_merge_kernel, sgrid, blk, 0, ctx->stream, g, (const int *)k.lab, k.reg);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(slic_cc_compress_kernel, sgrid, blk, 0, ctx->stream, g, k.reg, k.size);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(slic_cc_key_kernel, sgrid, blk, 0, ctx->stream, g, (const int *)k.lab, (const int *)k.reg, (const unsigned *)k.size, k.ckey);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(slic_cc_keep_kernel, sgrid, blk, 0, ctx->stream, g, (const int *)k.lab, (const int *)k.reg, k.size, (const u64 *)k.ckey, min_size);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(slic_adopt_kernel, zgrid, zblk, 0, ctx->stream, g, k.reg, (const unsigned *)k.size, k.best);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(slic_orphan_merge_kernel, sgrid, blk, 0, ctx->stream, g, k.reg, (const unsigned *)k.size);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(slic_first_kernel, sgrid, blk, 0, ctx->stream, g, k.reg, k.best);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(slic_rank_kernel, zgrid, zblk, 0, ctx->stream, g, (const int *)k.reg, (const int *)k.best, k.size, d_nlabels);
    ALQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(slic_emit_kernel, sgrid, blk, 0, ctx->stream, g, (const int *)k.reg, (const unsigned *)k.size, hwz, d_labels);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // extern "C"
