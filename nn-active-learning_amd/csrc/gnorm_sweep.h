// The voxel sweep of a sample's conv weight gradient on the exact-fp32 matrix cores, shared by the per-sample squared norms
// (gnorm.hip) and the diagonal Fisher (dfisher.hip): geometry, box staging and the two-level fp32 fold.  See gnorm.hip's
// header comment for the method; this file holds the pieces both kernels are built from.
#pragma once
#include <algorithm>

#include "alq_internal.h"

namespace alq {
namespace gn {

typedef float gn_f32x4 __attribute__((ext_vector_type(4)));

constexpr int GN_WAVES = 4;
constexpr int GN_THREADS = GN_WAVES * 64;
constexpr int GN_KC_MAX = 128;            // points per box
constexpr int GN_HALO_MAX = 13312;        // floats of the staged Y halo (52 KiB; with X rows + table: < 64 KiB LDS)

// element (voxel row r of the N-patch tensor, channel c) of a View, split concat included
struct GnView {
    const float *p;
    int cs, c0, split;
    long long delta;
    __device__ inline float at(long long row, int c) const {
        if (split && c >= split) return p[delta + row * cs + (c - split)];
        return p[row * cs + c0 + c];
    }
};
inline GnView gview(const View &v) {
    GnView d;
    d.p = v.p; d.cs = v.cs; d.c0 = v.c0; d.split = v.split; d.delta = v.delta;
    return d;
}

struct GnGeom {
    int XD, XH, XW, Ca;          // unshifted operand: grid of the swept points r, channels a (tile columns)
    int YD, YH, YW, Cb;          // shifted operand: grid, channels b (tile rows (tap, b))
    int k[3], s[3], sg, base[3];
    int omin[3], span[3];        // tap offsets o = sg * t + base: minimum and extent per dimension
    int RY, RX, hy, hx;          // box of X points (1 x RY x RX); halo extent in y and x (z: span[0])
    int T, MT, NT, groups;       // taps, row tiles, column tiles, row-tile groups per column tile
    int halo_fl;                 // floats of the staged halo (the X rows and the offset table follow it in LDS)
};

inline int span_of(int s, int n_pts, int span) { return s * (n_pts - 1) + span; }

// the kernel's geometry for U / V of a layer (see gnorm.hip's header comment); mirrored form for a narrow stride-1 conv
inline GnGeom make_geom(const View &U, const View &V, const int k[3], const int s[3], const int lo[3], bool *mirror) {
    GnGeom g{};
    const bool stride1 = s[0] == 1 && s[1] == 1 && s[2] == 1;
    *mirror = stride1 && U.C < 16 && V.C > U.C;
    const View &X = *mirror ? V : U, &Y = *mirror ? U : V;
    g.XD = X.D; g.XH = X.H; g.XW = X.W; g.Ca = X.C;
    g.YD = Y.D; g.YH = Y.H; g.YW = Y.W; g.Cb = Y.C;
    g.sg = *mirror ? -1 : 1;
    for (int d = 0; d < 3; ++d) {
        g.k[d] = k[d];
        g.s[d] = s[d];
        g.base[d] = *mirror ? lo[d] : -lo[d];
        g.omin[d] = *mirror ? lo[d] - (k[d] - 1) : -lo[d];
        g.span[d] = k[d];
    }
    g.T = k[0] * k[1] * k[2];
    g.MT = (g.T * g.Cb + 15) / 16;
    g.NT = (g.Ca + 15) / 16;
    // box: whole x rows where they fit, as many rows as the point and halo budgets allow
    g.RX = std::min(g.XW, GN_KC_MAX);
    g.RY = std::max(1, std::min(g.XH, GN_KC_MAX / g.RX));
    for (;;) {
        g.hy = span_of(g.s[1], g.RY, g.span[1]);
        g.hx = span_of(g.s[2], g.RX, g.span[2]);
        if ((long long)g.span[0] * g.hy * g.hx * g.Cb <= GN_HALO_MAX) break;
        if (g.RY > 1) --g.RY;
        else if (g.RX > 1) --g.RX;
        else break;
    }
    g.halo_fl = g.span[0] * g.hy * g.hx * g.Cb;
    return g;
}

inline int gn_tpw(int MT) {
    const int need = (MT + GN_WAVES - 1) / GN_WAVES;
    return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
}

// LDS of one workgroup: only what the layer's box needs (more workgroups share a CU when the halo is small)
inline size_t gnorm_dyn_lds_bytes(const GnGeom &g) {
    const int kc = (g.RY * g.RX + 3) & ~3;
    return (size_t)(g.halo_fl + kc * 16) * 4 + (size_t)kc * 4;
}

#ifdef __HIPCC__
// Row tiles of this wave in row-tile group rg: tile j is row tile rt = rg * (GN_WAVES * TPW) + wave + GN_WAVES * j.
// toff[j] = the halo offset of the tile's row (tap, b) = lane & 15, or -1 for a row past the end; returns the tiles in use.
template <int TPW>
__device__ __forceinline__ int gn_tile_rows(const GnGeom &g, int rg, int (&toff)[TPW]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rows = g.T * g.Cb;
    int ntile = 0;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int rt = rg * (GN_WAVES * TPW) + w + GN_WAVES * j;
        if (rt < g.MT) ntile = j + 1;
        const int m = rt * 16 + (lane & 15);
        if (rt < g.MT && m < rows) {
            const int tap = m / g.Cb, b = m - tap * g.Cb;
            const int tz = tap / (g.k[1] * g.k[2]), ty = (tap / g.k[2]) % g.k[1], tx = tap % g.k[2];
            const int oz = g.sg * tz + g.base[0] - g.omin[0];
            const int oy = g.sg * ty + g.base[1] - g.omin[1];
            const int ox = g.sg * tx + g.base[2] - g.omin[2];
            toff[j] = ((oz * g.hy + oy) * g.hx + ox) * g.Cb + b;
        } else {
            toff[j] = -1;
        }
    }
    return ntile;
}

// The whole voxel sweep of sample n for the column tile at col0: tot[j] = this wave's tile j of H (C/D layout of
// v_mfma_f32_16x16x4_f32: register r of lane l holds row 4 * (l >> 4) + r, column l & 15).  Boxes are staged in the
// workgroup's dynamic LDS (gnorm_dyn_lds_bytes), every box's fp32 sums are folded into tot (two-level sum).  All
// GN_THREADS threads of the workgroup must call it; it starts with a barrier, so calls may follow each other.
template <int TPW>
__device__ __forceinline__ void gn_sweep_sample(const GnView &X, const GnView &Y, const GnGeom &g, int n, int col0,
                                                const int (&toff)[TPW], int ntile, gn_f32x4 (&tot)[TPW]) {
    extern __shared__ float gn_lds[];
    float *Ys = gn_lds;                                   // [span0][hy][hx][Cb]
    float *Xs = gn_lds + g.halo_fl;                       // [ksteps * 4][16]
    int *hb = (int *)(Xs + ((g.RY * g.RX + 3) & ~3) * 16);   // [ksteps * 4] halo offset of box point kk
    const int lane = threadIdx.x & 63;
    const long long xvox = (long long)g.XD * g.XH * g.XW, yvox = (long long)g.YD * g.YH * g.YW;
    gn_f32x4 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) { acc[j] = gn_f32x4{0.f, 0.f, 0.f, 0.f}; tot[j] = acc[j]; }

    const int KC = g.RY * g.RX;
    const int ksteps = (KC + 3) / 4;
    const int halo = g.halo_fl;
    for (int z = 0; z < g.XD; ++z) {
        for (int y0 = 0; y0 < g.XH; y0 += g.RY) {
            for (int x0 = 0; x0 < g.XW; x0 += g.RX) {
                __syncthreads();
                // X rows of the box: Xs[kk][a], zero outside the grid and past the channels
                for (int i = threadIdx.x; i < ksteps * 4 * 16; i += GN_THREADS) {
                    const int kk = i >> 4, a = i & 15;
                    const int ry = kk / g.RX, rx = kk - ry * g.RX;
                    const int y = y0 + ry, x = x0 + rx;
                    float v = 0.f;
                    if (kk < KC && y < g.XH && x < g.XW && col0 + a < g.Ca)
                        v = X.at((long long)n * xvox + ((long long)z * g.XH + y) * g.XW + x, col0 + a);
                    Xs[i] = v;
                }
                for (int kk = threadIdx.x; kk < ksteps * 4; kk += GN_THREADS) {
                    const int ry = kk / g.RX, rx = kk - ry * g.RX;
                    hb[kk] = kk < KC ? (g.s[1] * ry * g.hx + g.s[2] * rx) * g.Cb : 0;
                }
                // Y halo: Ys[hz][hy][hx][b] = Y[origin + (hz, hy, hx), b]
                const int oz = g.s[0] * z + g.omin[0], oy = g.s[1] * y0 + g.omin[1], ox = g.s[2] * x0 + g.omin[2];
                for (int i = threadIdx.x; i < halo; i += GN_THREADS) {
                    int r = i / g.Cb;
                    const int b = i - r * g.Cb;
                    const int hx_ = r % g.hx; r /= g.hx;
                    const int hy_ = r % g.hy;
                    const int hz_ = r / g.hy;
                    const int pz = oz + hz_, py = oy + hy_, px = ox + hx_;
                    float v = 0.f;
                    if ((unsigned)pz < (unsigned)g.YD && (unsigned)py < (unsigned)g.YH && (unsigned)px < (unsigned)g.YW)
                        v = Y.at((long long)n * yvox + ((long long)pz * g.YH + py) * g.YW + px, b);
                    Ys[i] = v;
                }
                __syncthreads();
                for (int ks = 0; ks < ksteps; ++ks) {
                    const int kk = ks * 4 + (lane >> 4);
                    const float bv = Xs[kk * 16 + (lane & 15)];
                    const int h = hb[kk];
#pragma unroll
                    for (int j = 0; j < TPW; ++j) {
                        if (j < ntile) {
                            const float av = toff[j] >= 0 ? Ys[h + toff[j]] : 0.f;
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < TPW; ++j) { tot[j] += acc[j]; acc[j] = gn_f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
        }
    }
}
#endif  // __HIPCC__

}  // namespace gn
}  // namespace alq
