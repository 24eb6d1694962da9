// Whole-volume inference of a fully-convolutional model: the volume is cut into overlapping tiles of the model's input shape,
// the model runs on the tiles, and the tiles' posteriors are blended back with a separable window (nnal_amd/tiled.py is the
// NumPy statement of every operation here; no reference counterpart - the reference builds one model per image size).
//   * the lattice (host arithmetic, no device call): along an axis of length D with tile t and stride s, one tile at 0 when D <= t
//     (it overhangs the volume by t - D), else ceil((D - t) / s) + 1 tiles at min(i s, D - t) - the last one is clamped so that it ends
//     with the volume.  Tile (iz, ih, iw) has the index (iz nH + ih) nW + iw.
//   * tile_gather_kernel: X [n, tz, th, tw, m] out of a packed volume [Z, H, W, m].  A row of tw m floats is contiguous on both sides;
//     an item is 16 bytes of an output row (<VEC>: rows of whole 16-byte pieces that start on 16-byte boundaries of X; the piece is
//     loaded as 16 bytes where its source address allows, else as four floats) or one float.  Consecutive lanes take consecutive
//     items.  What lies outside the volume - only on an axis with D < t - is `fill`.
//   * tile_blend_kernel: a GATHER - a lane owns a voxel of the bounding box of the call's tiles, walks the tiles that cover it in
//     ascending tile index (the covering indices of an axis are one contiguous range: tiles_covering) and, for those of the call,
//     adds w p_k to the voxel's c sums and w to its weight sum, w = (wz[lz] wh[lh]) ww[lw]; every product and sum is rounded on its
//     own (the file is built without contraction into fused multiply-adds).  One writer per voxel, no atomics: the order of a
//     voxel's additions is the tile order whatever the batch cuts, so consecutive calls leave the bytes of one call over all tiles.
//     Lanes that follow each other along w read consecutive floats of a tile's row of posteriors.  The voxel's sums are loaded ahead
//     of the walk and the tiles of a lattice row two at a time ahead of their additions (the launch is a chain of latencies).
//   * tile_finalize_kernel: q_k = acc[k] / acc[c] (correctly rounded: the compiler's default for HIP) and the first maximum of q as
//     a byte.  <HWZ = false>: outputs in the accumulator's own [Z, H, W] order, four voxels a lane where the alignment allows.
//     <HWZ = true>: [H, W, Z], z fastest - the transpose of the [Z, H W] matrix through an LDS tile of 32 planes x 64 voxels (pitch
//     65: the transposed read of a half wave walks 32 banks), read along h w - all c + 1 planes of the tile before the first
//     quotient - and written along z, one class plane after the other; the labels leave as runs of bytes along z, four a lane
//     where Z and the pointer allow.
#include <algorithm>
#include <cstdint>
#include <initializer_list>

#include "alq_internal.h"

namespace alq {

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_MAX_BLOCKS = 2048;              // workgroups of a gather / blend launch (8 per compute unit): grid-stride beyond
constexpr int TL_MAX_M = 8;                      // as alq_vol_pack
constexpr int TL_MIN_C = 2, TL_MAX_C = 8;        // the range of the dense head (dense.hip)
constexpr int64_t TL_MAX_ELEMS = (int64_t)1 << 31;
constexpr int TF_Z = 32, TF_R = 64, TF_PITCH = TF_R + 1;      // the transpose tile of finalize

struct TileLat {
    int D[3], t[3], s[3], n[3];      // order Z, H, W; n: tiles per axis
};

// x / d for 0 <= x < 2^31 as a multiplication and a shift (Granlund and Montgomery: l = ceil(log2 d), m = ceil(2^(31 + l) / d) < 2^32,
// x / d = floor(m x / 2^(31 + l))): the divisors of a launch are its arguments, and an integer division in the kernel costs some
// thirty vector instructions - five of them per 16 bytes in the gather, eight per voxel in the blend.
struct FastDiv {
    unsigned m;
    int sh;
};

FastDiv fd_make(unsigned d) {
    int l = 0;
    while (((unsigned long long)1 << l) < d) ++l;
    FastDiv f;
    f.m = (unsigned)((((unsigned long long)1 << (31 + l)) + d - 1) / d);
    f.sh = 31 + l;
    return f;
}

__device__ inline unsigned fd_div(unsigned x, FastDiv f) { return (unsigned)(((unsigned long long)x * f.m) >> f.sh); }

__host__ __device__ inline int tl_count(int D, int t, int s) { return D <= t ? 1 : (int)(((long long)D - t + s - 1) / s) + 1; }

// (i s <= D - t + s - 1 for i < n: no overflow)
__host__ __device__ inline int tl_origin(int i, int D, int t, int s) { return D <= t ? 0 : (i * s < D - t ? i * s : D - t); }

// the tiles of an axis that cover coordinate x, lo .. hi (never empty).  Tiles before the last start at i s: i s <= x < i s + t; the
// last one starts at D - t, and every tile before it starts below that: x >= D - t is covered by lo .. n - 1.
__device__ inline void tiles_covering(int x, int D, int t, int s, int n, FastDiv by_s, int &lo, int &hi) {
    if (n == 1) { lo = hi = 0; return; }
    lo = x - t + 1 <= 0 ? 0 : (int)fd_div((unsigned)(x - t + s), by_s);
    hi = x >= D - t ? n - 1 : (int)fd_div((unsigned)x, by_s);
}

bool tl_aligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

// ---------------------------------------------------------------------------------------------------- gather
struct GatherDiv {
    FastDiv q, th, tz, nw, nh;
};

template <bool VEC>
__global__ __launch_bounds__(TL_THREADS) void tile_gather_kernel(const float *__restrict__ vol, float *__restrict__ X, TileLat L, GatherDiv dv,
                                                                 unsigned first, unsigned items, unsigned q, int m, float fill) {
    const unsigned stride = gridDim.x * TL_THREADS;
    const int tz = L.t[0], th = L.t[1], tw = L.t[2], Z = L.D[0], H = L.D[1], W = L.D[2];
    const unsigned rowlen = (unsigned)tw * (unsigned)m;
    for (unsigned item = blockIdx.x * TL_THREADS + threadIdx.x; item < items; item += stride) {
        const unsigned row = fd_div(item, dv.q), k = item - row * q;          // q: items of a row
        const unsigned t2 = fd_div(row, dv.th), j = fd_div(t2, dv.tz);
        const int lh = (int)(row - t2 * (unsigned)th), lz = (int)(t2 - j * (unsigned)tz);
        const unsigned idx = first + j, u = fd_div(idx, dv.nw);          // (fewer tiles than voxels: below 2^31)
        const int iw = (int)(idx - u * (unsigned)L.n[2]), iz = (int)fd_div(u, dv.nh), ih = (int)(u - (unsigned)iz * (unsigned)L.n[1]);
        const int z = tl_origin(iz, Z, tz, L.s[0]) + lz, h = tl_origin(ih, H, th, L.s[1]) + lh, ow = tl_origin(iw, W, tw, L.s[2]);
        const unsigned valid = (z < Z && h < H) ? (unsigned)std::min(tw, W - ow) * (unsigned)m : 0u;      // floats of the row inside the volume
        const float *__restrict__ src = vol + (((long long)z * H + h) * W + ow) * m;                 // (read only below `valid`)
        float *__restrict__ dst = X + (long long)row * rowlen;
        if (VEC) {
            const unsigned e = 4 * k;
            float4 v = make_float4(fill, fill, fill, fill);
            if (e + 4 <= valid) {
                if ((reinterpret_cast<uintptr_t>(src + e) & 15) == 0) {
                    v = *reinterpret_cast<const float4 *>(src + e);
                } else {
                    v.x = src[e]; v.y = src[e + 1]; v.z = src[e + 2]; v.w = src[e + 3];
                }
            } else if (e < valid) {          // the row leaves the volume inside this piece
                v.x = src[e];
                if (e + 1 < valid) v.y = src[e + 1];
                if (e + 2 < valid) v.z = src[e + 2];
            }
            *reinterpret_cast<float4 *>(dst + e) = v;
        } else {
            dst[k] = k < valid ? src[k] : fill;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- blend
struct BlendArgs {
    const float *post, *wz, *wh, *ww;
    float *acc;
    TileLat L;
    long long first, n;          // the call's tiles
    int b0[3], bn[3];            // bounding box of the call's tiles: first voxel, extent (inside the volume)
    unsigned total;              // voxels of the box
    FastDiv by_bw, by_bh, by_s[3];
};

template <int C>
__global__ __launch_bounds__(TL_THREADS) void tile_blend_kernel(BlendArgs a) {
    const unsigned stride = gridDim.x * TL_THREADS;
    const TileLat &L = a.L;
    const int tz = L.t[0], th = L.t[1], tw = L.t[2];
    const long long V = (long long)tz * th * tw, nV = a.n * V, N = (long long)L.D[0] * L.D[1] * L.D[2];
    for (unsigned e = blockIdx.x * TL_THREADS + threadIdx.x; e < a.total; e += stride) {
        const unsigned r = fd_div(e, a.by_bw), rz = fd_div(r, a.by_bh);
        const int w = a.b0[2] + (int)(e - r * (unsigned)a.bn[2]), h = a.b0[1] + (int)(r - rz * (unsigned)a.bn[1]), z = a.b0[0] + (int)rz;
        int z_lo, z_hi, h_lo, h_hi, w_lo, w_hi;
        tiles_covering(z, L.D[0], tz, L.s[0], L.n[0], a.by_s[0], z_lo, z_hi);
        tiles_covering(h, L.D[1], th, L.s[1], L.n[1], a.by_s[1], h_lo, h_hi);
        tiles_covering(w, L.D[2], tw, L.s[2], L.n[2], a.by_s[2], w_lo, w_hi);
        float *__restrict__ acc = a.acc + ((long long)z * L.D[1] + h) * L.D[2] + w;
        // The voxel's sums are loaded before it is known whether a tile of the call covers it (it lies in the volume), and two tiles
        // of a row of the lattice are loaded before either is added: a lane's time is a chain of memory latencies, not bytes.
        float s[C + 1];
#pragma unroll
        for (int k = 0; k <= C; ++k) s[k] = acc[k * N];
        bool any = false;
        for (int iz = z_lo; iz <= z_hi; ++iz) {
            const int lz = z - tl_origin(iz, L.D[0], tz, L.s[0]);
            const float vz = a.wz[lz];
            for (int ih = h_lo; ih <= h_hi; ++ih) {
                // tile (iz, ih, iw) is tile base + iw of the call: those with 0 <= base + iw < n take part
                const long long base = ((long long)iz * L.n[1] + ih) * L.n[2] - a.first;
                const long long j0 = std::max<long long>(w_lo, -base), j1 = std::min<long long>(w_hi, a.n - 1 - base);
                if (j0 > j1) continue;
                const int i0 = (int)j0, i1 = (int)j1;          // (inside w_lo .. w_hi)
                any = true;
                const int lh = h - tl_origin(ih, L.D[1], th, L.s[1]);
                const float wzh = vz * a.wh[lh];
                const float *__restrict__ row = a.post + ((long long)lz * th + lh) * tw;
                for (int iw = i0; iw <= i1; iw += 2) {
                    const bool two = iw < i1;
                    const int iw1 = two ? iw + 1 : iw;          // (a single tile is loaded twice: no branch between the loads)
                    const int lw0 = w - tl_origin(iw, L.D[2], tw, L.s[2]), lw1 = w - tl_origin(iw1, L.D[2], tw, L.s[2]);
                    const float *__restrict__ p0 = row + (base + iw) * V + lw0;
                    const float *__restrict__ p1 = row + (base + iw1) * V + lw1;
                    const float ww0 = a.ww[lw0], ww1 = a.ww[lw1];
                    float v0[C], v1[C];
#pragma unroll
                    for (int k = 0; k < C; ++k) { v0[k] = p0[k * nV]; v1[k] = p1[k * nV]; }
                    const float wt0 = wzh * ww0;
#pragma unroll
                    for (int k = 0; k < C; ++k) s[k] = s[k] + wt0 * v0[k];
                    s[C] = s[C] + wt0;
                    if (two) {
                        const float wt1 = wzh * ww1;
#pragma unroll
                        for (int k = 0; k < C; ++k) s[k] = s[k] + wt1 * v1[k];
                        s[C] = s[C] + wt1;
                    }
                }
            }
        }
        if (any) {
#pragma unroll
            for (int k = 0; k <= C; ++k) acc[k * N] = s[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- finalize
template <int C>
__device__ inline void tf_voxel(const float (&s)[C + 1], float (&q)[C], unsigned char &lab) {
    float best = 0.f;
    int at = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        q[k] = s[k] / s[C];
        if (k == 0 || q[k] > best) { best = q[k]; at = k; }          // strict: the first maximum stays
    }
    lab = (unsigned char)at;
}

template <int C, bool VEC>
__global__ __launch_bounds__(TL_THREADS) void tile_finalize_kernel(const float *__restrict__ acc, long long N, float *__restrict__ post,
                                                                   unsigned char *__restrict__ label) {
    constexpr int U = VEC ? 4 : 1;
    const long long groups = (N + U - 1) / U, stride = (long long)gridDim.x * TL_THREADS;
    for (long long g = (long long)blockIdx.x * TL_THREADS + threadIdx.x; g < groups; g += stride) {
        const long long v = g * U;
        float s[U][C + 1], q[U][C];
        unsigned char lab[U];
        if (VEC) {          // N % 4 == 0 and every plane starts on a 16-byte boundary
#pragma unroll
            for (int k = 0; k <= C; ++k) {
                const float4 x = *reinterpret_cast<const float4 *>(acc + k * N + v);
                s[0][k] = x.x; s[1 % U][k] = x.y; s[2 % U][k] = x.z; s[3 % U][k] = x.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k <= C; ++k) s[0][k] = acc[k * N + v];
        }
#pragma unroll
        for (int i = 0; i < U; ++i) tf_voxel<C>(s[i], q[i], lab[i]);
        if (post) {
#pragma unroll
            for (int k = 0; k < C; ++k) {
                if (VEC) *reinterpret_cast<float4 *>(post + k * N + v) = make_float4(q[0][k], q[1 % U][k], q[2 % U][k], q[3 % U][k]);
                else post[k * N + v] = q[0][k];
            }
        }
        if (label) {
            if (VEC) *reinterpret_cast<uchar4 *>(label + v) = make_uchar4(lab[0], lab[1 % U], lab[2 % U], lab[3 % U]);
            else label[v] = lab[0];
        }
    }
}

// [Z, H W] -> [H W, Z]: workgroup (bx, by) owns voxels hw0 .. hw0 + 63 of planes z0 .. z0 + 31
template <int C>
__global__ __launch_bounds__(TL_THREADS) void tile_finalize_hwz_kernel(const float *__restrict__ acc, long long HW, int Z, unsigned by,
                                                                       float *__restrict__ post, unsigned char *__restrict__ label, int lab_vec) {
    __shared__ float s_q[TF_Z * TF_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char s_lab[TF_R * TF_Z];          // [r][zl]: the bytes of a voxel's run lie together
    constexpr int PER = TF_Z * TF_R / TL_THREADS;          // voxels of a lane
    const long long N = HW * Z;
    const unsigned bx = blockIdx.x / by;
    const long long hw0 = (long long)bx * TF_R;
    const int z0 = (int)(blockIdx.x - bx * by) * TF_Z;
    const int nr = (int)std::min<long long>(TF_R, HW - hw0), nz = std::min(TF_Z, Z - z0);
    float v[C + 1][PER], best[PER];
    unsigned char lab[PER];
    // read layout: element i of a lane is plane zl = (tid + 256 i) / 64, voxel r = tid % 64 - a wave reads 64 consecutive floats.
    // Every load of the tile is issued before the first quotient: one memory latency a tile, not one a class plane.
    const int r_in = threadIdx.x & (TF_R - 1), zl_in0 = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k <= C; ++k) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int zl = zl_in0 + 4 * i;
            const bool live = r_in < nr && zl < nz;
            v[k][i] = live ? acc[k * N + (long long)(z0 + zl) * HW + hw0 + r_in] : (k == C ? 1.f : 0.f);
        }
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const float q = v[k][i] / v[C][i];
            if (k == 0 || q > best[i]) { best[i] = q; lab[i] = (unsigned char)k; }
            v[k][i] = q;
        }
        if (post) {          // (uniform)
#pragma unroll
            for (int i = 0; i < PER; ++i) s_q[(zl_in0 + 4 * i) * TF_PITCH + r_in] = v[k][i];
            __syncthreads();
            // write layout: r = e / 32, zl = e % 32 - a half wave writes 32 consecutive floats along z
            for (int e = threadIdx.x; e < TF_R * TF_Z; e += TL_THREADS) {
                const int r = e >> 5, zl = e & 31;
                if (r < nr && zl < nz) post[k * N + (hw0 + r) * Z + z0 + zl] = s_q[zl * TF_PITCH + r];
            }
            __syncthreads();
        }
    }
    if (label) {
#pragma unroll
        for (int i = 0; i < PER; ++i) s_lab[r_in * TF_Z + zl_in0 + 4 * i] = lab[i];
        __syncthreads();
        if (lab_vec && nz == TF_Z) {          // Z % 4 == 0 and the pointer on a 4-byte boundary: four planes a lane
            for (int e = threadIdx.x; e < TF_R * TF_Z / 4; e += TL_THREADS) {
                const int r = e >> 3, zl = (e & 7) << 2;
                if (r < nr) *reinterpret_cast<uchar4 *>(label + (hw0 + r) * Z + z0 + zl) = *reinterpret_cast<const uchar4 *>(s_lab + r * TF_Z + zl);
            }
        } else {
            for (int e = threadIdx.x; e < TF_R * TF_Z; e += TL_THREADS) {
                const int r = e >> 5, zl = e & 31;
                if (r < nr && zl < nz) label[(hw0 + r) * Z + z0 + zl] = s_lab[r * TF_Z + zl];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host side
int lat_check(const char *who, const alq_tile_lattice_t *lat) {
    ALQ_REQUIRE(lat, ALQ_EINVAL, "%s: null lattice", who);
    for (int a = 0; a < 3; ++a) {
        ALQ_REQUIRE(lat->dims[a] >= 1 && lat->tile[a] >= 1, ALQ_EINVAL, "%s: axis %d has %d voxels and a tile of %d (both at least 1)", who, a,
                    lat->dims[a], lat->tile[a]);
        ALQ_REQUIRE(lat->stride[a] >= 1 && lat->stride[a] <= lat->tile[a], ALQ_EINVAL, "%s: axis %d has stride %d (1 .. the tile, %d)", who, a,
                    lat->stride[a], lat->tile[a]);
    }
    return ALQ_OK;
}

TileLat lat_resolve(const alq_tile_lattice_t *lat) {
    TileLat L;
    for (int a = 0; a < 3; ++a) {
        L.D[a] = lat->dims[a]; L.t[a] = lat->tile[a]; L.s[a] = lat->stride[a];
        L.n[a] = tl_count(L.D[a], L.t[a], L.s[a]);
    }
    return L;
}

// a product of extents, or 2^62 once it passes that (no overflow)
int64_t capped_product(std::initializer_list<int64_t> f) {
    int64_t p = 1;
    for (int64_t v : f) p = (v == 0) ? 0 : (p > ((int64_t)1 << 62) / v ? (int64_t)1 << 62 : p * v);
    return p;
}

// the checks the gather and the blend share; V: voxels of a tile
int range_check(const char *who, const alq_tile_lattice_t *lat, int64_t first, int64_t n, TileLat &L, int64_t &V) {
    ALQ_TRY(lat_check(who, lat));
    L = lat_resolve(lat);
    const int64_t tiles = (int64_t)L.n[0] * L.n[1] * L.n[2];
    V = capped_product({L.t[0], L.t[1], L.t[2]});
    ALQ_REQUIRE(first >= 0 && n >= 1 && first <= tiles - n, ALQ_EINVAL, "%s: tiles %lld .. %lld of %lld", who, (long long)first,
                (long long)(first + n - 1), (long long)tiles);
    return ALQ_OK;
}

template <template <int> class F, typename... A>
void per_class(int c, A &&...a) {
    switch (c) {
    case 2: F<2>::run(a...); break;
    case 3: F<3>::run(a...); break;
    case 4: F<4>::run(a...); break;
    case 5: F<5>::run(a...); break;
    case 6: F<6>::run(a...); break;
    case 7: F<7>::run(a...); break;
    default: F<8>::run(a...); break;
    }
}

template <int C> struct BlendLaunch {
    static void run(dim3 grid, hipStream_t st, const BlendArgs &a) { hipLaunchKernelGGL((tile_blend_kernel<C>), grid, dim3(TL_THREADS), 0, st, a); }
};

template <int C> struct FinalizeLaunch {
    static void run(dim3 grid, hipStream_t st, bool vec, const float *acc, long long N, float *post, unsigned char *label) {
        if (vec) hipLaunchKernelGGL((tile_finalize_kernel<C, true>), grid, dim3(TL_THREADS), 0, st, acc, N, post, label);
        else hipLaunchKernelGGL((tile_finalize_kernel<C, false>), grid, dim3(TL_THREADS), 0, st, acc, N, post, label);
    }
};

template <int C> struct FinalizeHwzLaunch {
    static void run(dim3 grid, hipStream_t st, const float *acc, long long HW, int Z, unsigned by, float *post, unsigned char *label, int lab_vec) {
        hipLaunchKernelGGL((tile_finalize_hwz_kernel<C>), grid, dim3(TL_THREADS), 0, st, acc, HW, Z, by, post, label, lab_vec);
    }
};

}  // namespace

}  // namespace alq

using namespace alq;

extern "C" {

int alq_tile_lattice_check(const alq_tile_lattice_t *lat) { return lat_check("alq_tile_lattice_check", lat); }

int64_t alq_tile_count(const alq_tile_lattice_t *lat, int32_t counts[3]) {
    ALQ_TRY(lat_check("alq_tile_count", lat));
    const TileLat L = lat_resolve(lat);
    if (counts)
        for (int a = 0; a < 3; ++a) counts[a] = L.n[a];
    return (int64_t)L.n[0] * L.n[1] * L.n[2];
}

int alq_tile_origin(const alq_tile_lattice_t *lat, int64_t idx, int32_t origin[3]) {
    ALQ_TRY(lat_check("alq_tile_origin", lat));
    ALQ_REQUIRE(origin, ALQ_EINVAL, "alq_tile_origin: null origin");
    const TileLat L = lat_resolve(lat);
    ALQ_REQUIRE(idx >= 0 && idx < (int64_t)L.n[0] * L.n[1] * L.n[2], ALQ_EINVAL, "alq_tile_origin: tile %lld of %lld", (long long)idx,
                (long long)((int64_t)L.n[0] * L.n[1] * L.n[2]));
    const int64_t u = idx / L.n[2];
    const int i[3] = {(int)(u / L.n[1]), (int)(u % L.n[1]), (int)(idx % L.n[2])};
    for (int a = 0; a < 3; ++a) origin[a] = tl_origin(i[a], L.D[a], L.t[a], L.s[a]);
    return ALQ_OK;
}

int64_t alq_tile_blend_trip_voxels(void) { return (int64_t)TL_MAX_BLOCKS * TL_THREADS; }

int alq_tile_gather(alq_ctx *ctx, const float *d_vol, int m, const alq_tile_lattice_t *lat, int64_t first, int64_t n, float fill, float *d_X) {
    ALQ_REQUIRE(ctx && d_vol && d_X, ALQ_EINVAL, "alq_tile_gather: null argument");
    TileLat L;
    int64_t V;
    ALQ_TRY(range_check("alq_tile_gather", lat, first, n, L, V));
    ALQ_REQUIRE(m >= 1, ALQ_EINVAL, "alq_tile_gather: %d modalities", m);
    ALQ_REQUIRE(tl_aligned(d_vol, 4) && tl_aligned(d_X, 4), ALQ_EINVAL, "alq_tile_gather: a pointer is not aligned to its element");
    ALQ_REQUIRE(m <= TL_MAX_M, ALQ_EUNSUPPORTED, "alq_tile_gather: %d modalities (1 .. %d)", m, TL_MAX_M);
    ALQ_REQUIRE(capped_product({L.D[0], L.D[1], L.D[2]}) < TL_MAX_ELEMS, ALQ_EUNSUPPORTED, "alq_tile_gather: the volume has 2^31 voxels or more");
    ALQ_REQUIRE(capped_product({n, L.t[0], L.t[1], L.t[2], m}) < TL_MAX_ELEMS, ALQ_EUNSUPPORTED,
                "alq_tile_gather: %lld tiles of %d x %d x %d x %d are 2^31 elements or more", (long long)n, L.t[0], L.t[1], L.t[2], m);
    ALQ_HIP(hipSetDevice(ctx->device));
    const int64_t rows = n * L.t[0] * L.t[1], rowlen = (int64_t)L.t[2] * m;
    const bool vec = rowlen % 4 == 0 && tl_aligned(d_X, 16);
    const int64_t q = vec ? rowlen / 4 : rowlen, items = rows * q;
    const dim3 grid((unsigned)std::min<int64_t>((items + TL_THREADS - 1) / TL_THREADS, TL_MAX_BLOCKS));
    const GatherDiv dv = {fd_make((unsigned)q), fd_make((unsigned)L.t[1]), fd_make((unsigned)L.t[0]), fd_make((unsigned)L.n[2]),
                          fd_make((unsigned)L.n[1])};
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    if (vec)
        hipLaunchKernelGGL((tile_gather_kernel<true>), grid, dim3(TL_THREADS), 0, ctx->stream, d_vol, d_X, L, dv, (unsigned)first, (unsigned)items,
                           (unsigned)q, m, fill);
    else
        hipLaunchKernelGGL((tile_gather_kernel<false>), grid, dim3(TL_THREADS), 0, ctx->stream, d_vol, d_X, L, dv, (unsigned)first, (unsigned)items,
                           (unsigned)q, m, fill);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int alq_tile_blend(alq_ctx *ctx, const float *d_post, int c, const alq_tile_lattice_t *lat, int64_t first, int64_t n, const float *d_wz,
                   const float *d_wh, const float *d_ww, float *d_acc) {
    ALQ_REQUIRE(ctx && d_post && d_wz && d_wh && d_ww && d_acc, ALQ_EINVAL, "alq_tile_blend: null argument");
    TileLat L;
    int64_t V;
    ALQ_TRY(range_check("alq_tile_blend", lat, first, n, L, V));
    ALQ_REQUIRE(tl_aligned(d_post, 4) && tl_aligned(d_wz, 4) && tl_aligned(d_wh, 4) && tl_aligned(d_ww, 4) && tl_aligned(d_acc, 4), ALQ_EINVAL,
                "alq_tile_blend: a pointer is not aligned to its element");
    ALQ_REQUIRE(c >= TL_MIN_C && c <= TL_MAX_C, ALQ_EUNSUPPORTED, "alq_tile_blend: %d classes (%d .. %d)", c, TL_MIN_C, TL_MAX_C);
    ALQ_REQUIRE(capped_product({L.D[0], L.D[1], L.D[2]}) < TL_MAX_ELEMS, ALQ_EUNSUPPORTED, "alq_tile_blend: the volume has 2^31 voxels or more");
    ALQ_REQUIRE(capped_product({n, L.t[0], L.t[1], L.t[2]}) < TL_MAX_ELEMS, ALQ_EUNSUPPORTED,
                "alq_tile_blend: %lld tiles of %d x %d x %d are 2^31 voxels or more", (long long)n, L.t[0], L.t[1], L.t[2]);
    ALQ_HIP(hipSetDevice(ctx->device));
    BlendArgs a;
    a.post = d_post; a.wz = d_wz; a.wh = d_wh; a.ww = d_ww; a.acc = d_acc;
    a.L = L; a.first = first; a.n = n;
    // the box: tile indices first .. last differ in their slowest digit or agree in it; behind the first digit that differs every
    // value of the faster digits may occur
    const int64_t last = first + n - 1;
    const int64_t lo[3] = {first / ((int64_t)L.n[1] * L.n[2]), (first / L.n[2]) % L.n[1], first % L.n[2]};
    const int64_t hi[3] = {last / ((int64_t)L.n[1] * L.n[2]), (last / L.n[2]) % L.n[1], last % L.n[2]};
    bool whole = false;
    int64_t total = 1;
    for (int ax = 0; ax < 3; ++ax) {
        const int i0 = whole ? 0 : (int)lo[ax], i1 = whole ? L.n[ax] - 1 : (int)hi[ax];
        a.b0[ax] = tl_origin(i0, L.D[ax], L.t[ax], L.s[ax]);
        a.bn[ax] = std::min(tl_origin(i1, L.D[ax], L.t[ax], L.s[ax]) + L.t[ax], L.D[ax]) - a.b0[ax];
        total *= a.bn[ax];
        whole = whole || lo[ax] != hi[ax];
    }
    a.total = (unsigned)total;
    a.by_bw = fd_make((unsigned)a.bn[2]);
    a.by_bh = fd_make((unsigned)a.bn[1]);
    for (int ax = 0; ax < 3; ++ax) a.by_s[ax] = fd_make((unsigned)L.s[ax]);
    const dim3 grid((unsigned)std::min<int64_t>((total + TL_THREADS - 1) / TL_THREADS, TL_MAX_BLOCKS));
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    per_class<BlendLaunch>(c, grid, ctx->stream, a);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int alq_tile_finalize(alq_ctx *ctx, const float *d_acc, int c, const int32_t dims[3], int hwz, float *d_post_out, uint8_t *d_label) {
    ALQ_REQUIRE(ctx && d_acc && dims, ALQ_EINVAL, "alq_tile_finalize: null argument");
    ALQ_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, ALQ_EINVAL, "alq_tile_finalize: volume %d x %d x %d", dims[0], dims[1], dims[2]);
    ALQ_REQUIRE(hwz == 0 || hwz == 1, ALQ_EINVAL, "alq_tile_finalize: hwz = %d (0 or 1)", hwz);
    ALQ_REQUIRE(tl_aligned(d_acc, 4) && tl_aligned(d_post_out, 4), ALQ_EINVAL, "alq_tile_finalize: a pointer is not aligned to its element");
    ALQ_REQUIRE(c >= TL_MIN_C && c <= TL_MAX_C, ALQ_EUNSUPPORTED, "alq_tile_finalize: %d classes (%d .. %d)", c, TL_MIN_C, TL_MAX_C);
    const int64_t N = capped_product({dims[0], dims[1], dims[2]});
    ALQ_REQUIRE(N < TL_MAX_ELEMS, ALQ_EUNSUPPORTED, "alq_tile_finalize: the volume has 2^31 voxels or more");
    if (!d_post_out && !d_label) return ALQ_OK;
    ALQ_HIP(hipSetDevice(ctx->device));
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    if (hwz) {
        const int64_t HW = (int64_t)dims[1] * dims[2], bx = (HW + TF_R - 1) / TF_R, by = (dims[0] + TF_Z - 1) / TF_Z;
        const int lab_vec = dims[0] % 4 == 0 && tl_aligned(d_label, 4);
        per_class<FinalizeHwzLaunch>(c, dim3((unsigned)(bx * by)), ctx->stream, d_acc, (long long)HW, (int)dims[0], (unsigned)by, d_post_out, d_label,
                                     lab_vec);
    } else {
        const bool vec = N % 4 == 0 && tl_aligned(d_acc, 16) && tl_aligned(d_post_out, 16) && tl_aligned(d_label, 4);
        const int64_t groups = vec ? N / 4 : N;
        const dim3 grid((unsigned)std::min<int64_t>((groups + TL_THREADS - 1) / TL_THREADS, TL_MAX_BLOCKS));
        per_class<FinalizeLaunch>(c, grid, ctx->stream, vec, d_acc, (long long)N, d_post_out, d_label);
    }
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // extern "C"
