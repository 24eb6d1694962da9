// Connected components of a binary volume and the two post-processing steps built on them (the reference's post_processing.py:
// connected_component_analysis_3d = skimage.measure.label + largest component, fill_holes = scipy's binary_fill_holes):
//
//   alq_cc_label          labels[v] = the smallest raveled index of the component that holds v (selected voxels), -1 elsewhere
//   alq_cc_keep_largest   out[v] = [v lies in the largest component], ties -> the component whose first voxel comes first
//   alq_fill_holes        out[v] = seg[v] != 0 or v lies in a 6-connected background component that touches no face
//   alq_cc_sizes          sizes[root] = voxels of the component, 0 at every other voxel (labels of alq_cc_label in)
//   alq_cc_relabel        out[v] = table[labels[v]] (0 outside), or out[v] = sizes[labels[v]] >= min_size
//
// Volumes are [H, W, S] in C order, z contiguous.  The labelling is the atomic-min union-find of Komura / Playne & Hawick in
// three launches:
//   init      lanes run along z: a wave ballots "selected" over its 64 consecutive voxels and every selected voxel takes the
//             first voxel of its z-run (inside the wave, never across a row end) as its parent - the runs are flat trees
//             before any atomic is issued.
//   merge     every selected voxel unites with its selected neighbours among the 13 / 9 / 3 that precede it in C order.  A
//             pair (v, n) is skipped when (v - 1, n - 1) is a selected pair of the same two rows (that pair has the same
//             offset and both runs are already one set), or when the neighbour one step back in n's row was united a moment
//             ago; what is left is about one union per pair of touching runs.  unite() hooks the larger root under the
//             smaller with atomicMin and carries on from the value the atomic returned, so a hook that another workgroup
//             overtook is never lost; indices strictly decrease, so it terminates.  No wave waits for another one.
//   compress  labels[v] = find(v), after the kernel boundary has published every hook.
// Visibility inside the merge launch: a word of parent[] that another workgroup may write is read only through the return
// value of an atomic or through a relaxed agent-scope atomic load (never a plain load, which another XCD's L2 or this CU's
// L1 may serve from a stale line).  parent[x] <= x always holds, so the root of a finished tree is the minimum of its set:
// the labels are a pure function of the input, whatever order the workgroups ran in.
// Sizes are integer adds of whole z-runs (the run's first lane contributes the run length to size[root]; a wave sums what its
// runs give to one root before it issues the atomic), the winner is the maximum of the 64-bit key (size << 32) | ~root: exact
// and order-independent as well.
// Memory: 4 bytes of parent per voxel (alq_cc_label: the caller's label volume itself) + 4 bytes of size / face flag per
// voxel + a 64-byte header in the work buffer.  Every kernel streams HBM or issues integer atomics: grid-stride, 256 threads.
#include <algorithm>

#include "alq_internal.h"
#include "unionfind.h"

namespace alq {

namespace {

typedef unsigned long long u64;

constexpr int CC_THREADS = 256;
constexpr int CC_WAVES = CC_THREADS / 64;
constexpr size_t CC_HEADER = 64;      // bytes in front of parent[]: word 0 = the winner's key

struct CcGeo {
    int H, W, S;
    int nvox;
    int maxnz;        // non-zero offset components a neighbour may have: 1 (6), 2 (18), 3 (26)
    int sel_zero;     // select voxels == 0 instead of != 0
};

__device__ inline bool cc_sel(const unsigned char *seg, int v, int sel_zero) { return (seg[v] != 0) != (sel_zero != 0); }

// ballots of one wave step: which lanes are selected, which start a row (z == 0)
struct CcRuns {
    u64 mask, brk;
};

// first lane of the z-run that holds `lane` (the caller's lane is selected)
__device__ inline int cc_run_start(const CcRuns &r, int lane) {
    const u64 starts = r.mask & (~(r.mask << 1) | r.brk);
    const u64 le = (lane == 63) ? ~0ull : ((2ull << lane) - 1);
    return 63 - __clzll((long long)(starts & le));
}

// voxels of the run from `lane` to its end inside the wave
__device__ inline int cc_run_len(const CcRuns &r, int lane) {
    const u64 above = (lane == 63) ? 0ull : ~((2ull << lane) - 1);
    const u64 stop = (~r.mask | r.brk) & above;
    return (stop ? __ffsll((long long)stop) - 1 : 64) - lane;
}

// parent[v] = first voxel of v's z-run inside its wave (-1: not selected); aux[v] = 0; adds the number of selected voxels to
// *count (when given); clears the header
__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(const unsigned char *seg, CcGeo g, int *__restrict__ parent,
                                                             unsigned *__restrict__ aux, u64 *__restrict__ header,
                                                             u64 *__restrict__ count) {
    __shared__ unsigned part[CC_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (header && blockIdx.x == 0 && threadIdx.x < (int)(CC_HEADER / 8)) header[threadIdx.x] = 0;
    unsigned nsel = 0;      // wave-uniform
    // every lane of a block walks the same number of steps, so each ballot sees the whole wave
    for (long long base = blockIdx.x * (long long)CC_THREADS; base < g.nvox; base += (long long)gridDim.x * CC_THREADS) {
        const long long vl = base + threadIdx.x;
        const bool in = vl < g.nvox;
        const int v = (int)vl;
        const bool sel = in && cc_sel(seg, v, g.sel_zero);
        CcRuns r;
        r.mask = __ballot(sel);
        r.brk = __ballot(in && v % g.S == 0);
        nsel += __popcll(r.mask);
        if (in) {
            parent[v] = sel ? v - lane + cc_run_start(r, lane) : -1;
            if (aux) aux[v] = 0;
        }
    }
    if (!count) return;
    if (lane == 0) part[wave] = nsel;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int w = 0; w < CC_WAVES; ++w) s += part[w];
        if (s) atomicAdd(count, s);
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const unsigned char *__restrict__ seg, CcGeo g, int *parent) {
    for (long long vl = blockIdx.x * (long long)CC_THREADS + threadIdx.x; vl < g.nvox; vl += (long long)gridDim.x * CC_THREADS) {
        const int v = (int)vl;
        if (!cc_sel(seg, v, g.sel_zero)) continue;
        const int z = v % g.S;
        const int row = v / g.S;
        const int j = row % g.W, i = row / g.W;
        const bool own_prev = z > 0 && cc_sel(seg, v - 1, g.sel_zero);
        // a run that crosses from one wave into the next: init saw its two halves apart
        int top = v;      // a member of v's set at or above v in its tree: where the next find starts
        if (own_prev && (v & 63) == 0) top = cc_unite(parent, top, v - 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int di = q < 3 ? -1 : 0;
            const int dj = q < 3 ? q - 1 : -1;
            const int nzr = (di != 0) + (dj != 0);
            if (nzr > g.maxnz) continue;
            if (i + di < 0 || j + dj < 0 || j + dj >= g.W) continue;
            const int nb = v + (di * g.W + dj) * g.S;      // (i + di, j + dj, z)
            // m[k + 2] = selected at (i + di, j + dj, z + k), k = -2 .. 1
            bool m[4];
#pragma unroll
            for (int k = -2; k <= 1; ++k) m[k + 2] = (z + k >= 0 && z + k < g.S) && cc_sel(seg, nb + k, g.sel_zero);
            bool prev_in = false;      // the neighbour one step back along z is selected and already in v's set
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) {
                const bool ok = m[dz + 2] && nzr + (dz != 0) <= g.maxnz;
                if (ok && !prev_in && !(own_prev && m[dz + 1])) top = cc_unite(parent, top, nb + dz);
                prev_in = ok;
            }
        }
    }
}

// The size pass of one wave step.  r.mask: the selected lanes, r.brk: lanes at which a run starts whatever came before; a
// selected lane's `root` is its component.  The first lane of every run adds the run length to size[root]; a wave sums what
// the runs of a step give to one root before it issues the atomic, and the root that holds most of the step's selected
// voxels goes into a wave-uniform (root, sum) pair kept across the steps: it reaches memory when another root takes its
// place and at the end (cc_flush_held).  Integer sums: the same totals whatever is held back.  Every lane of the wave calls.
struct CcHeld {
    int root = -1;
    unsigned sum = 0;
};

__device__ inline void cc_add_runs(const CcRuns &r, bool sel, int root, int lane, unsigned *size, CcHeld &h) {
    const bool lead = sel && cc_run_start(r, lane) == lane;
    const unsigned len = lead ? (unsigned)cc_run_len(r, lane) : 0u;
    const unsigned nsel = __popcll(r.mask);
    u64 todo = __ballot(lead);      // wave-uniform: the loop below is too
    while (todo) {
        const int l0 = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(root, l0);
        const bool same = lead && root == r0;
        const u64 sm = __ballot(same);
        unsigned s = same ? len : 0u;
        if (sm & (sm - 1)) {      // more than one run of that root in this step
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        } else {
            s = __shfl(s, l0);
        }
        if (r0 == h.root) {
            h.sum += s;
        } else if (2 * s > nsel) {
            if (h.sum && lane == 0) atomicAdd(size + h.root, h.sum);
            h.root = r0;
            h.sum = s;
        } else if (lane == l0) {
            atomicAdd(size + r0, s);
        }
        todo &= ~sm;
    }
}

__device__ inline void cc_flush_held(unsigned *size, const CcHeld &h, int lane) {
    if (h.sum && lane == 0) atomicAdd(size + h.root, h.sum);
}

// labels[v] = find(v) (in place over parent[]: a concurrent reader meets either the old parent or the root, both ancestors).
// MODE 1: the first lane of every z-run adds the run length to size[root]; MODE 2: a selected voxel on a face of the volume
// raises flag[root]
template <int MODE>
__global__ __launch_bounds__(CC_THREADS) void cc_compress_kernel(CcGeo g, int *labels, unsigned *aux) {
    const int lane = threadIdx.x & 63;
    // MODE 1: a giant component would draw one atomic per run of the whole volume to ONE word (measured: 12 ns each, 23 ms at
    // 256 x 256 x 128).  So a wave first sums the runs of a step per root, and the root that holds most of the step's
    // selected voxels goes into a wave-uniform (root, sum) pair kept across the steps; it reaches memory when another root
    // takes its place and at the end.  Integer sums: the same totals whatever is held back
    CcHeld held;
    for (long long base = blockIdx.x * (long long)CC_THREADS; base < g.nvox; base += (long long)gridDim.x * CC_THREADS) {
        const long long vl = base + threadIdx.x;
        const bool in = vl < g.nvox;
        const int v = (int)vl;
        const bool sel = in && labels[v] >= 0;
        int root = -1;
        if (sel) {
            root = cc_find(labels, v);
            labels[v] = root;
        }
        if (MODE == 1) {
            CcRuns r;
            r.mask = __ballot(sel);
            r.brk = __ballot(in && v % g.S == 0);
            cc_add_runs(r, sel, root, lane, aux, held);
        }
        if (MODE == 2 && sel) {
            const int z = v % g.S;
            const int row = v / g.S;
            const int j = row % g.W, i = row / g.W;
            if (z == 0 || z == g.S - 1 || j == 0 || j == g.W - 1 || i == 0 || i == g.H - 1) aux[root] = 1;
        }
    }
    if (MODE == 1) cc_flush_held(aux, held, lane);
}

// the maximum of (size << 32) | ~root over the candidate roots -> header[0]; their number -> info[0]
__global__ __launch_bounds__(CC_THREADS) void cc_winner_kernel(CcGeo g, const int *__restrict__ labels, const unsigned *__restrict__ size,
                                                               int skip_origin, u64 *header, u64 *info) {
    __shared__ u64 pkey[CC_WAVES];
    __shared__ unsigned pcnt[CC_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 key = 0;
    unsigned ncand = 0;      // wave-uniform
    for (long long base = blockIdx.x * (long long)CC_THREADS; base < g.nvox; base += (long long)gridDim.x * CC_THREADS) {
        const long long vl = base + threadIdx.x;
        const int v = (int)vl;
        const bool cand = vl < g.nvox && labels[v] == v && !(skip_origin && v == 0);
        if (cand) key = max(key, ((u64)size[v] << 32) | (unsigned)~v);
        ncand += __popcll(__ballot(cand));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)key, off), hi = __shfl_xor((unsigned)(key >> 32), off);
        key = max(key, ((u64)hi << 32) | lo);
    }
    if (lane == 0) {
        pkey[wave] = key;
        pcnt[wave] = ncand;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 k = 0, c = 0;
        for (int w = 0; w < CC_WAVES; ++w) {
            k = max(k, pkey[w]);
            c += pcnt[w];
        }
        if (k) atomicMax(header, k);
        if (c) atomicAdd(info, c);
    }
}

// out[v] = labels[v] == winner; info[1] = winner (-1: none), info[2] = its size
__global__ __launch_bounds__(CC_THREADS) void cc_select_kernel(CcGeo g, const int *__restrict__ labels, const u64 *__restrict__ header,
                                                               unsigned char *out, long long *info) {
    const u64 key = header[0];
    const int winner = key ? (int)~(unsigned)key : -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        info[1] = winner;
        info[2] = (long long)(key >> 32);
    }
    for (long long vl = blockIdx.x * (long long)CC_THREADS + threadIdx.x; vl < g.nvox; vl += (long long)gridDim.x * CC_THREADS)
        out[vl] = (unsigned char)(winner >= 0 && labels[vl] == winner);
}

// out[v] = seg[v] != 0 || v's background component touches no face; info[0] += enclosed components, info[1] += voxels filled
// (seg and out may be the same buffer: a thread reads its own voxel before it writes it)
__global__ __launch_bounds__(CC_THREADS) void cc_fill_kernel(const unsigned char *seg, CcGeo g, const int *__restrict__ labels,
                                                             const unsigned *__restrict__ outside, unsigned char *out, u64 *info) {
    __shared__ unsigned part[CC_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned ncomp = 0, nfill = 0;      // wave-uniform
    for (long long base = blockIdx.x * (long long)CC_THREADS; base < g.nvox; base += (long long)gridDim.x * CC_THREADS) {
        const long long vl = base + threadIdx.x;
        bool fill = false, comp = false;
        if (vl < g.nvox) {
            const int lab = labels[vl];
            fill = lab >= 0 && !outside[lab];
            comp = fill && lab == (int)vl;
            out[vl] = (unsigned char)(seg[vl] != 0 || fill);
        }
        nfill += __popcll(__ballot(fill));
        ncomp += __popcll(__ballot(comp));
    }
    if (lane == 0) {
        part[wave][0] = ncomp;
        part[wave][1] = nfill;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        u64 s = 0;
        for (int w = 0; w < CC_WAVES; ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(info + threadIdx.x, s);
    }
}

// size[root] += the voxels of every run of equal labels (alq_cc_sizes: labels as alq_cc_label left them, size zeroed before)
__global__ __launch_bounds__(CC_THREADS) void cc_sizes_kernel(const int *__restrict__ labels, long long n, unsigned *size) {
    const int lane = threadIdx.x & 63;
    CcHeld held;
    // every lane of a block walks the same number of steps, so each ballot sees the whole wave
    for (long long base = blockIdx.x * (long long)CC_THREADS; base < n; base += (long long)gridDim.x * CC_THREADS) {
        const long long vl = base + threadIdx.x;
        const int lab = vl < n ? labels[vl] : -1;
        const bool sel = lab >= 0 && lab < n;
        const int before = __shfl_up(lab, 1);
        CcRuns r;
        r.mask = __ballot(sel);
        r.brk = __ballot(sel && (lane == 0 || before != lab));      // a run ends where the label changes
        cc_add_runs(r, sel, lab, lane, size, held);
    }
    cc_flush_held(size, held, lane);
}

// out_i32[v] = label < 0 ? 0 : table[label], or out_u8[v] = label >= 0 && sizes[label] >= min_size
__global__ __launch_bounds__(CC_THREADS) void cc_relabel_kernel(const int *__restrict__ labels, long long n, const int *__restrict__ table,
                                                                const int *__restrict__ sizes, int min_size, int *__restrict__ out_i32,
                                                                unsigned char *__restrict__ out_u8) {
    for (long long vl = blockIdx.x * (long long)CC_THREADS + threadIdx.x; vl < n; vl += (long long)gridDim.x * CC_THREADS) {
        const int lab = labels[vl];
        const bool sel = lab >= 0 && lab < n;
        if (out_i32)
            out_i32[vl] = sel ? table[lab] : 0;
        else
            out_u8[vl] = (unsigned char)(sel && sizes[lab] >= min_size);
    }
}

unsigned cc_grid(const alq_ctx *ctx, long long n) {
    return (unsigned)std::max<long long>(1, std::min<long long>((n + CC_THREADS - 1) / CC_THREADS, (long long)ctx->num_cus * 8));
}

// dims -> geometry; false: an axis below 1 or 2^31 voxels and more
bool cc_geometry(const int64_t dims[3], int connectivity, int sel_zero, CcGeo *g) {
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
    const int64_t lim = (int64_t)1 << 31;
    if (dims[0] >= lim || dims[1] >= lim || dims[2] >= lim) return false;
    if (dims[0] * dims[1] >= lim || dims[0] * dims[1] * dims[2] >= lim) return false;
    g->H = (int)dims[0];
    g->W = (int)dims[1];
    g->S = (int)dims[2];
    g->nvox = (int)(dims[0] * dims[1] * dims[2]);
    g->maxnz = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
    g->sel_zero = sel_zero ? 1 : 0;
    return true;
}

struct CcWork {
    u64 *header;
    int *parent;
    unsigned *aux;
};

CcWork cc_work(void *d_work, const CcGeo &g) {
    CcWork w;
    char *p = static_cast<char *>(d_work);
    w.header = reinterpret_cast<u64 *>(p);
    w.parent = reinterpret_cast<int *>(p + CC_HEADER);
    w.aux = reinterpret_cast<unsigned *>(p + CC_HEADER + (size_t)g.nvox * 4);
    return w;
}

// init + merge: the forest of the selected voxels in parent[] (aux / header / count: see cc_init_kernel)
int cc_forest(alq_ctx *ctx, const uint8_t *d_seg, const CcGeo &g, int *parent, unsigned *aux, u64 *header, u64 *count) {
    const dim3 grid(cc_grid(ctx, g.nvox));
    {
        ProfScope ps(ctx, PROF_ELEMWISE, 0);
        hipLaunchKernelGGL(cc_init_kernel, grid, dim3(CC_THREADS), 0, ctx->stream, d_seg, g, parent, aux, header, count);
        ALQ_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, PROF_REDUCE, 0);
    hipLaunchKernelGGL(cc_merge_kernel, grid, dim3(CC_THREADS), 0, ctx->stream, d_seg, g, parent);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // namespace

}  // namespace alq

using namespace alq;

extern "C" {

size_t alq_cc_work_bytes(const int64_t dims[3]) {
    CcGeo g;
    if (!dims || !cc_geometry(dims, 26, 0, &g)) return 0;
    return CC_HEADER + (size_t)g.nvox * 8;
}

int alq_cc_label(alq_ctx *ctx, const uint8_t *d_seg, const int64_t dims[3], int connectivity, int select_zero, int32_t *d_labels) {
    ALQ_REQUIRE(ctx && d_seg && dims && d_labels, ALQ_EINVAL, "alq_cc_label: null argument");
    ALQ_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, ALQ_EINVAL, "alq_cc_label: connectivity %d (6, 18 or 26)",
                connectivity);
    CcGeo g;
    ALQ_REQUIRE(cc_geometry(dims, connectivity, select_zero, &g), ALQ_EINVAL, "alq_cc_label: dims %lld x %lld x %lld (each >= 1, below 2^31 voxels)",
                (long long)dims[0], (long long)dims[1], (long long)dims[2]);
    ALQ_HIP(hipSetDevice(ctx->device));
    ALQ_TRY(cc_forest(ctx, d_seg, g, d_labels, nullptr, nullptr, nullptr));
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    hipLaunchKernelGGL(cc_compress_kernel<0>, dim3(cc_grid(ctx, g.nvox)), dim3(CC_THREADS), 0, ctx->stream, g, d_labels, (unsigned *)nullptr);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int alq_cc_keep_largest(alq_ctx *ctx, const uint8_t *d_seg, const int64_t dims[3], int connectivity, int skip_origin, uint8_t *d_out,
                        int64_t *d_info, void *d_work) {
    ALQ_REQUIRE(ctx && d_seg && dims && d_out && d_info && d_work, ALQ_EINVAL, "alq_cc_keep_largest: null argument");
    ALQ_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, ALQ_EINVAL,
                "alq_cc_keep_largest: connectivity %d (6, 18 or 26)", connectivity);
    CcGeo g;
    ALQ_REQUIRE(cc_geometry(dims, connectivity, 0, &g), ALQ_EINVAL, "alq_cc_keep_largest: dims %lld x %lld x %lld (each >= 1, below 2^31 voxels)",
                (long long)dims[0], (long long)dims[1], (long long)dims[2]);
    ALQ_REQUIRE(((uintptr_t)d_work & 7) == 0 && ((uintptr_t)d_info & 7) == 0, ALQ_EINVAL, "alq_cc_keep_largest: d_work / d_info not 8-byte aligned");
    ALQ_HIP(hipSetDevice(ctx->device));
    const CcWork w = cc_work(d_work, g);
    u64 *info = reinterpret_cast<u64 *>(d_info);
    ALQ_HIP(hipMemsetAsync(d_info, 0, 4 * sizeof(int64_t), ctx->stream));
    ALQ_TRY(cc_forest(ctx, d_seg, g, w.parent, w.aux, w.header, info + 3));
    const dim3 grid(cc_grid(ctx, g.nvox));
    {
        ProfScope ps(ctx, PROF_REDUCE, 0);
        hipLaunchKernelGGL(cc_compress_kernel<1>, grid, dim3(CC_THREADS), 0, ctx->stream, g, w.parent, w.aux);
        ALQ_HIP(hipGetLastError());
        hipLaunchKernelGGL(cc_winner_kernel, grid, dim3(CC_THREADS), 0, ctx->stream, g, (const int *)w.parent, (const unsigned *)w.aux,
                           skip_origin ? 1 : 0, w.header, info);
        ALQ_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    hipLaunchKernelGGL(cc_select_kernel, grid, dim3(CC_THREADS), 0, ctx->stream, g, (const int *)w.parent, (const u64 *)w.header, d_out,
                       reinterpret_cast<long long *>(d_info));
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int alq_cc_sizes(alq_ctx *ctx, const int32_t *d_labels, int64_t n, int32_t *d_sizes) {
    ALQ_REQUIRE(ctx && d_labels && d_sizes, ALQ_EINVAL, "alq_cc_sizes: null argument");
    ALQ_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), ALQ_EINVAL, "alq_cc_sizes: n = %lld (0 .. 2^31 - 1)", (long long)n);
    if (n == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(ctx->device));
    ALQ_HIP(hipMemsetAsync(d_sizes, 0, (size_t)n * sizeof(int32_t), ctx->stream));
    ProfScope ps(ctx, PROF_REDUCE, 0);
    hipLaunchKernelGGL(cc_sizes_kernel, dim3(cc_grid(ctx, n)), dim3(CC_THREADS), 0, ctx->stream, (const int *)d_labels, (long long)n,
                       reinterpret_cast<unsigned *>(d_sizes));
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int alq_cc_relabel(alq_ctx *ctx, const int32_t *d_labels, int64_t n, const int32_t *d_table, const int32_t *d_sizes, int32_t min_size,
                   int32_t *d_out_i32, uint8_t *d_out_u8) {
    ALQ_REQUIRE(ctx && d_labels, ALQ_EINVAL, "alq_cc_relabel: null argument");
    ALQ_REQUIRE((d_out_i32 != nullptr) != (d_out_u8 != nullptr), ALQ_EINVAL, "alq_cc_relabel: exactly one of d_out_i32 / d_out_u8");
    ALQ_REQUIRE(d_out_i32 ? d_table != nullptr : d_sizes != nullptr, ALQ_EINVAL, "alq_cc_relabel: null %s", d_out_i32 ? "d_table" : "d_sizes");
    ALQ_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), ALQ_EINVAL, "alq_cc_relabel: n = %lld (0 .. 2^31 - 1)", (long long)n);
    if (n == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(ctx->device));
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    hipLaunchKernelGGL(cc_relabel_kernel, dim3(cc_grid(ctx, n)), dim3(CC_THREADS), 0, ctx->stream, (const int *)d_labels, (long long)n,
                       (const int *)d_table, (const int *)d_sizes, (int)min_size, (int *)d_out_i32, (unsigned char *)d_out_u8);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

int alq_fill_holes(alq_ctx *ctx, const uint8_t *d_seg, const int64_t dims[3], uint8_t *d_out, int64_t *d_info, void *d_work) {
    ALQ_REQUIRE(ctx && d_seg && dims && d_out && d_info && d_work, ALQ_EINVAL, "alq_fill_holes: null argument");
    CcGeo g;
    ALQ_REQUIRE(cc_geometry(dims, 6, 1, &g), ALQ_EINVAL, "alq_fill_holes: dims %lld x %lld x %lld (each >= 1, below 2^31 voxels)",
                (long long)dims[0], (long long)dims[1], (long long)dims[2]);
    ALQ_REQUIRE(((uintptr_t)d_work & 7) == 0 && ((uintptr_t)d_info & 7) == 0, ALQ_EINVAL, "alq_fill_holes: d_work / d_info not 8-byte aligned");
    ALQ_HIP(hipSetDevice(ctx->device));
    const CcWork w = cc_work(d_work, g);
    ALQ_HIP(hipMemsetAsync(d_info, 0, 4 * sizeof(int64_t), ctx->stream));
    ALQ_TRY(cc_forest(ctx, d_seg, g, w.parent, w.aux, w.header, nullptr));
    const dim3 grid(cc_grid(ctx, g.nvox));
    {
        ProfScope ps(ctx, PROF_REDUCE, 0);
        hipLaunchKernelGGL(cc_compress_kernel<2>, grid, dim3(CC_THREADS), 0, ctx->stream, g, w.parent, w.aux);
        ALQ_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, PROF_ELEMWISE, 0);
    hipLaunchKernelGGL(cc_fill_kernel, grid, dim3(CC_THREADS), 0, ctx->stream, d_seg, g, (const int *)w.parent, (const unsigned *)w.aux, d_out,
                       reinterpret_cast<u64 *>(d_info));
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // extern "C"
