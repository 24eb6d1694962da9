// Resident volumes and the batches cut from them (datasets/data_holders.py, datasets/utils.prepare_batch_BrVol).
//   * vol_pack_kernel: a subject as the reference holds it - m arrays [H, W, Z] in C order, z fastest, of float / double / int16 /
//     uint8 - into ONE array [Z, H, W, m] of floats (alq_vol_pack) or, for a class-id mask, [Z, H, W] of bytes (alq_mask_pack):
//     the transpose of the [H W, Z] matrix through an LDS tile of 64 (32 for m > 4) rows x 32 planes, the m sources interleaved
//     on the way out.  A tile is read along z (runs of min(32, Z) elements; a tile that spans all of Z is one contiguous run) and
//     written as one run of 64 m outputs per plane, four outputs a lane where the alignment allows (16-byte stores of floats).
//     Row pitch 33: the transposed read of 64 rows walks 64 banks; the planes of the m sources are shifted against each other by
//     32 / 16 / 8 words (m = 2 / 3..4 / 5..8), so that a wave reading one plane position of neighbouring (row, source) pairs
//     meets every bank once.
//   * slice_batch_kernel: a batch X [b, z, h, w, m] with its labels [b, z, h, w] (int32: the class id, -1 for an unlabelled sample
//     or a mask byte >= C) and the voxel count of every class and of the -1 voxels.  Output row (i, jz, r) is w m consecutive floats
//     of a packed subject: a wave copies a row - single floats up to the first 16-byte boundary of the OUTPUT, then 16-byte stores
//     (the source run sits at any float offset: its loads are declared 4-byte aligned), then single floats - and turns its w mask
//     bytes into labels; a lane issues the loads of four pieces and four mask bytes together, ahead of their stores.  Counts: ballots per class and wave for C <= 8, LDS counters beyond; one atomic per workgroup and
//     non-empty class.  Integer counts: the result does not depend on the order of the atomics.
// The windows are resolved and checked on the host (alq_slice_batch); the kernel receives pointers to their first elements by
// value, 64 samples a launch: no table is uploaded, nothing a descriptor holds is trusted on the device.
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "alq_internal.h"

namespace alq {

#define ALQ_LAUNCH_CHECK() ALQ_HIP(hipGetLastError())

constexpr int VP_BLOCK = 256;
constexpr int VP_TZ = 32, VP_PITCH = VP_TZ + 1;
constexpr int VP_MAX_M = 8;

static int vp_rows(int m) { return m <= 4 ? 64 : 32; }
static int vp_plane_pad(int m) { return m <= 1 ? 0 : m == 2 ? 32 : m <= 4 ? 16 : 8; }

struct VolPackArgs {
    const void *src[VP_MAX_M];
    void *out;
    long long HW;
    int Z, m, rows, plane;      // rows of a tile; words between the LDS planes of two sources
    int vec;                    // four outputs a lane
};

template <typename T> __device__ inline float vp_value(T v) { return (float)v; }      // (double: round to nearest even, once)

template <typename OUT>
__device__ inline void vp_store4(OUT *p, const float (&v)[4]) {
    if constexpr (std::is_same<OUT, float>::value) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *reinterpret_cast<uchar4 *>(p) = make_uchar4((unsigned char)v[0], (unsigned char)v[1], (unsigned char)v[2], (unsigned char)v[3]);
    }
}

template <typename T, typename OUT>
__global__ __launch_bounds__(VP_BLOCK) void vol_pack_kernel(VolPackArgs a) {
    extern __shared__ float vp_tile[];
    const int m = a.m, Z = a.Z;
    const long long hw0 = (long long)blockIdx.x * a.rows;
    const int z0 = blockIdx.y * VP_TZ;
    const int thw = (int)std::min<long long>(a.rows, a.HW - hw0), tz = std::min(VP_TZ, Z - z0);
    const int n_in = thw * tz;
    for (int j = 0; j < m; ++j) {
        const T *__restrict__ s = static_cast<const T *>(a.src[j]) + hw0 * Z + z0;
        float *pl = vp_tile + j * a.plane;
        for (int e = threadIdx.x; e < n_in; e += VP_BLOCK) {
            int r, zl;
            if (tz == VP_TZ) { r = e >> 5; zl = e & 31; } else { r = e / tz; zl = e - r * tz; }
            pl[r * VP_PITCH + zl] = vp_value(s[(long long)r * Z + zl]);
        }
    }
    __syncthreads();
    const int run = thw * m;                       // outputs of one plane of the tile, consecutive in memory
    OUT *__restrict__ out = static_cast<OUT *>(a.out);
    if (a.vec) {                                   // run % 4 == 0 and every run starts on a 4-output boundary
        const int q = run >> 2, n_out = q * tz;
        for (int e = threadIdx.x; e < n_out; e += VP_BLOCK) {
            const int zl = e / q, k = (e - zl * q) << 2;
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = (k + u) / m, j = (k + u) - r * m;
                v[u] = vp_tile[j * a.plane + r * VP_PITCH + zl];
            }
            vp_store4<OUT>(out + ((long long)(z0 + zl) * a.HW + hw0) * m + k, v);
        }
    } else {
        const int n_out = run * tz;
        for (int e = threadIdx.x; e < n_out; e += VP_BLOCK) {
            const int zl = e / run, k = e - zl * run;
            const int r = k / m, j = k - r * m;
            out[((long long)(z0 + zl) * a.HW + hw0) * m + k] = (OUT)vp_tile[j * a.plane + r * VP_PITCH + zl];
        }
    }
}

static bool aligned_to(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

template <typename T, typename OUT>
static int vol_pack_launch(alq_ctx *ctx, const void *const *d_src, int m, const int *dims, OUT *d_out) {
    VolPackArgs a;
    for (int j = 0; j < VP_MAX_M; ++j) a.src[j] = j < m ? d_src[j] : nullptr;
    a.out = d_out;
    a.HW = (long long)dims[0] * dims[1];
    a.Z = dims[2];
    a.m = m;
    a.rows = vp_rows(m);
    a.plane = a.rows * VP_PITCH + vp_plane_pad(m);
    // a tile's run of plane z starts at output (z HW + hw0) m with hw0 a multiple of 32: on a 4-output boundary when HW m % 4 == 0
    a.vec = (a.HW * m) % 4 == 0 && aligned_to(d_out, 4 * sizeof(OUT));
    const long long bx = (a.HW + a.rows - 1) / a.rows;
    const int by = (a.Z + VP_TZ - 1) / VP_TZ;
    ALQ_REQUIRE(bx < (1LL << 31) && by <= 65535, ALQ_EUNSUPPORTED, "vol_pack: %lld x %d tiles pass the grid", bx, by);
    const size_t lds = (size_t)m * a.plane * sizeof(float);
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    hipLaunchKernelGGL((vol_pack_kernel<T, OUT>), dim3((unsigned)bx, (unsigned)by), dim3(VP_BLOCK), lds, ctx->stream, a);
    ALQ_LAUNCH_CHECK();
    return ALQ_OK;
}

static int vol_dims_check(const char *who, const int *dims, int m) {
    ALQ_REQUIRE(dims && dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, ALQ_EINVAL, "%s: null or non-positive dims", who);
    ALQ_REQUIRE((long long)dims[0] * dims[1] * dims[2] * m < (1LL << 40), ALQ_EUNSUPPORTED, "%s: the volume is too large", who);
    return ALQ_OK;
}

// ------------------------------------------------------------------------------------------ batches
constexpr int SB_BLOCK = 256, SB_WAVES = SB_BLOCK / 64;
constexpr int SB_MAX_BLOCKS = 2048;          // workgroups of a launch (8 per compute unit): grid-stride beyond
constexpr int SB_SAMPLES = 64;               // samples of a launch: their windows travel as kernel arguments (24 bytes each)
constexpr int SB_BALLOT_C = 8;

struct SliceWindow {
    const float *x;              // first element of the window in the packed volume [Z, H, W, m]
    const unsigned char *mask;   // ... in the packed mask [Z, H, W]; null: an unlabelled sample
    int H, W;                    // of the subject: the strides of the window
};

struct SliceBatchArgs {
    SliceWindow win[SB_SAMPLES];
    float *X;                    // [n, z, h, w, m] of this launch's samples
    int *lab;                    // [n, z, h, w]
    unsigned long long *counts;  // [C + 1]
    long long rows;              // n z h
    int z, h, w, m, C;
};

typedef float sb_f4u __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at any float address

__global__ __launch_bounds__(SB_BLOCK) void slice_batch_kernel(SliceBatchArgs a) {
    __shared__ unsigned hist[256];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int C = a.C, w = a.w, n = a.w * a.m;
    const bool ballots = C <= SB_BALLOT_C;
    hist[threadIdx.x] = 0;
    __syncthreads();
    unsigned cnt[SB_BALLOT_C + 1];          // wave-uniform: voxels of class j seen by this wave; [SB_BALLOT_C]: the -1 voxels
#pragma unroll
    for (int j = 0; j <= SB_BALLOT_C; ++j) cnt[j] = 0;
    // (a launch holds fewer than 2^31 rows - the entry checks it -: 32-bit index arithmetic)
    const unsigned rows = (unsigned)a.rows, stride = gridDim.x * SB_WAVES;
    constexpr int U = 4;          // pieces of a row a lane has in flight: their loads are issued together, ahead of the stores
    for (unsigned row = blockIdx.x * SB_WAVES + wave; row < rows; row += stride) {
        const unsigned t = row / (unsigned)a.h;
        const int r = (int)(row - t * (unsigned)a.h);
        const unsigned i = t / (unsigned)a.z;
        const int jz = (int)(t - i * (unsigned)a.z);
        const SliceWindow &sw = a.win[i];
        const long long srow = ((long long)jz * sw.H + r) * sw.W;
        const float *__restrict__ src = sw.x + srow * a.m;
        float *__restrict__ dst = a.X + (long long)row * n;
        const unsigned char *__restrict__ mk = sw.mask ? sw.mask + srow : nullptr;
        int *__restrict__ lrow = a.lab + (long long)row * w;
        // floats up to the first 16-byte boundary of the output row, whole pieces of four, the rest
        const int head = std::min(n, (int)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3));
        const int q = (n - head) >> 2, tail0 = head + 4 * q;
        float edge = 0.f;
        const int ek = lane < head ? lane : tail0 + lane - head;          // lanes [0, head): the head; the next n - tail0: the tail
        const bool has_edge = lane < head + (n - tail0);
        if (has_edge) edge = src[ek];
        for (int k0 = 0; k0 < q || k0 < w; k0 += U * 64) {
            sb_f4u v[U];
            int mv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * 64 + lane;
                if (k < q) v[u] = *reinterpret_cast<const sb_f4u *>(src + head + 4 * k);
                mv[u] = (k < w && mk) ? (int)mk[k] : 255;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * 64 + lane;
                if (k < q) *reinterpret_cast<float4 *>(dst + head + 4 * k) = make_float4(v[u].x, v[u].y, v[u].z, v[u].w);
                const bool live = k < w;
                const int lab = mv[u] < C ? mv[u] : -1;
                if (live) lrow[k] = lab;
                if (k0 + u * 64 < w) {          // (wave-uniform: this piece holds labels)
                    if (ballots) {
#pragma unroll
                        for (int j = 0; j < SB_BALLOT_C; ++j)
                            if (j < C) cnt[j] += (unsigned)__popcll(__ballot(live && lab == j));
                        cnt[SB_BALLOT_C] += (unsigned)__popcll(__ballot(live && lab < 0));
                    } else if (live) {
                        atomicAdd(&hist[lab < 0 ? C : lab], 1u);
                    }
                }
            }
        }
        if (has_edge) dst[ek] = edge;
    }
    if (ballots && lane == 0) {
#pragma unroll
        for (int j = 0; j < SB_BALLOT_C; ++j)
            if (j < C && cnt[j]) atomicAdd(&hist[j], cnt[j]);
        if (cnt[SB_BALLOT_C]) atomicAdd(&hist[C], cnt[SB_BALLOT_C]);
    }
    __syncthreads();
    if ((int)threadIdx.x <= C && hist[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

}  // namespace alq

extern "C" {

int alq_vol_pack(alq_ctx *ctx, const void *const *d_src, int m, int src_type, const int32_t *dims, float *d_out) {
    ALQ_REQUIRE(ctx && d_src && d_out, ALQ_EINVAL, "alq_vol_pack: null argument");
    ALQ_REQUIRE(m >= 1, ALQ_EINVAL, "alq_vol_pack: %d modalities", m);
    ALQ_REQUIRE(m <= alq::VP_MAX_M, ALQ_EUNSUPPORTED, "alq_vol_pack: %d modalities (1 .. %d)", m, alq::VP_MAX_M);
    ALQ_TRY(alq::vol_dims_check("alq_vol_pack", dims, m));
    for (int j = 0; j < m; ++j) ALQ_REQUIRE(d_src[j], ALQ_EINVAL, "alq_vol_pack: source %d is null", j);
    ALQ_HIP(hipSetDevice(ctx->device));
    switch (src_type) {
        case ALQ_SRC_F32: return alq::vol_pack_launch<float, float>(ctx, d_src, m, dims, d_out);
        case ALQ_SRC_F64: return alq::vol_pack_launch<double, float>(ctx, d_src, m, dims, d_out);
        case ALQ_SRC_I16: return alq::vol_pack_launch<int16_t, float>(ctx, d_src, m, dims, d_out);
        case ALQ_SRC_U8: return alq::vol_pack_launch<uint8_t, float>(ctx, d_src, m, dims, d_out);
        default: break;
    }
    alq::set_error("alq_vol_pack: source type %d", src_type);
    return ALQ_EINVAL;
}

int alq_mask_pack(alq_ctx *ctx, const uint8_t *d_src, const int32_t *dims, uint8_t *d_out) {
    ALQ_REQUIRE(ctx && d_src && d_out, ALQ_EINVAL, "alq_mask_pack: null argument");
    ALQ_TRY(alq::vol_dims_check("alq_mask_pack", dims, 1));
    ALQ_HIP(hipSetDevice(ctx->device));
    const void *src[1] = {d_src};
    return alq::vol_pack_launch<uint8_t, uint8_t>(ctx, src, 1, dims, d_out);
}

int64_t alq_slice_batch_trip_rows(void) { return (int64_t)alq::SB_MAX_BLOCKS * alq::SB_WAVES; }

int alq_slice_batch_launch_samples(void) { return alq::SB_SAMPLES; }

int alq_slice_batch_check(const int32_t *h_dims, int nvol, const int32_t *h_desc, int b, const int32_t *crop, int C) {
    ALQ_REQUIRE(h_dims && h_desc && crop, ALQ_EINVAL, "alq_slice_batch: null argument");
    ALQ_REQUIRE(nvol >= 1 && b >= 1, ALQ_EINVAL, "alq_slice_batch: %d subjects, %d samples", nvol, b);
    ALQ_REQUIRE(C >= 1 && C <= 254, ALQ_EINVAL, "alq_slice_batch: %d classes (1 .. 254)", C);
    const int z = crop[0], h = crop[1], w = crop[2];
    ALQ_REQUIRE(z >= 1 && h >= 1 && w >= 1, ALQ_EINVAL, "alq_slice_batch: crop %d x %d x %d", z, h, w);
    for (int v = 0; v < nvol; ++v)
        ALQ_REQUIRE(h_dims[3 * v] >= 1 && h_dims[3 * v + 1] >= 1 && h_dims[3 * v + 2] >= 1, ALQ_EINVAL, "alq_slice_batch: subject %d has an empty axis", v);
    for (int i = 0; i < b; ++i) {
        const int32_t *d = h_desc + 5 * i;
        const long long vol = d[0], zc = d[1], h0 = d[2], w0 = d[3];
        ALQ_REQUIRE(vol >= 0 && vol < nvol, ALQ_EINVAL, "alq_slice_batch: sample %d names subject %lld of %d", i, vol, nvol);
        ALQ_REQUIRE(d[4] == 0 || d[4] == 1, ALQ_EINVAL, "alq_slice_batch: sample %d has the labelled flag %d", i, d[4]);
        const int H = h_dims[3 * vol], W = h_dims[3 * vol + 1], Z = h_dims[3 * vol + 2];
        const long long zlo = zc - z / 2;
        ALQ_REQUIRE(zc >= 0 && zlo >= 0 && zlo + z <= Z, ALQ_EINVAL,
                    "alq_slice_batch: sample %d: planes %lld .. %lld leave subject %lld (%d planes)", i, zlo, zlo + z - 1, vol, Z);
        ALQ_REQUIRE(h0 >= 0 && h0 + h <= H && w0 >= 0 && w0 + w <= W, ALQ_EINVAL,
                    "alq_slice_batch: sample %d: the %d x %d window at (%lld, %lld) leaves the %d x %d slices of subject %lld", i, h, w, h0, w0, H, W, vol);
    }
    return ALQ_OK;
}

int alq_slice_batch(alq_ctx *ctx, const float *const *h_vols, const uint8_t *const *h_masks, const int32_t *h_dims, int nvol, int m,
                    const int32_t *h_desc, int b, const int32_t *crop, int C, float *d_X, int32_t *d_lab, int64_t *d_counts) {
    ALQ_REQUIRE(ctx && h_vols && h_masks && d_X && d_lab && d_counts, ALQ_EINVAL, "alq_slice_batch: null argument");
    ALQ_REQUIRE(m >= 1, ALQ_EINVAL, "alq_slice_batch: %d modalities", m);
    ALQ_TRY(alq_slice_batch_check(h_dims, nvol, h_desc, b, crop, C));
    const int z = crop[0], h = crop[1], w = crop[2];
    ALQ_REQUIRE((long long)w * m < (1LL << 24) && (long long)z * h * alq::SB_SAMPLES < (1LL << 31), ALQ_EUNSUPPORTED,
                "alq_slice_batch: crop too large");
    for (int i = 0; i < b; ++i) {
        const int vol = h_desc[5 * i];
        ALQ_REQUIRE(h_vols[vol] && (!h_desc[5 * i + 4] || h_masks[vol]), ALQ_EINVAL, "alq_slice_batch: subject %d has no packed %s", vol,
                    h_vols[vol] ? "mask" : "volume");
    }
    ALQ_HIP(hipSetDevice(ctx->device));
    ALQ_HIP(hipMemsetAsync(d_counts, 0, (size_t)(C + 1) * sizeof(int64_t), ctx->stream));
    const long long per = (long long)z * h;          // rows of a sample
    for (int i0 = 0; i0 < b; i0 += alq::SB_SAMPLES) {
        const int n = std::min(alq::SB_SAMPLES, b - i0);
        alq::SliceBatchArgs a;
        for (int i = 0; i < alq::SB_SAMPLES; ++i) {
            if (i >= n) { a.win[i] = alq::SliceWindow{nullptr, nullptr, 0, 0}; continue; }
            const int32_t *d = h_desc + 5 * (i0 + i);
            const int vol = d[0], H = h_dims[3 * vol], W = h_dims[3 * vol + 1];
            const long long first = ((long long)(d[1] - z / 2) * H + d[2]) * W + d[3];
            a.win[i] = alq::SliceWindow{h_vols[vol] + first * m, d[4] ? h_masks[vol] + first : nullptr, H, W};
        }
        a.X = d_X + (long long)i0 * per * w * m;
        a.lab = d_lab + (long long)i0 * per * w;
        a.counts = reinterpret_cast<unsigned long long *>(d_counts);
        a.rows = (long long)n * per;
        a.z = z; a.h = h; a.w = w; a.m = m; a.C = C;
        const unsigned nblk = (unsigned)std::min<long long>((a.rows + alq::SB_WAVES - 1) / alq::SB_WAVES, alq::SB_MAX_BLOCKS);
        alq::ProfScope ps(ctx, alq::PROF_ELEMWISE, 0);
        hipLaunchKernelGGL(alq::slice_batch_kernel, dim3(nblk), dim3(alq::SB_BLOCK), 0, ctx->stream, a);
        ALQ_HIP(hipGetLastError());
    }
    return ALQ_OK;
}

}  // extern "C"
