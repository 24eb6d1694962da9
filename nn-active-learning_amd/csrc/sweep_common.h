// What the layer kernels of a Fisher pass (c3d, d3d, f3d, e3d, t3d, t3d8b .hip) have in common: vector types, buffer
// addressing, the per-patch scale exponent, the XCD-aware patch order, and on the host the grid rule, the geometry test,
// the patch-count guard and the launch sequence.  Included by those six files only; the tile engines (igemm*.hip,
// fcgemm.hip, wpack.hip) keep their own typedefs.
#ifndef ALQ_SWEEP_COMMON_H
#define ALQ_SWEEP_COMMON_H
#include "alq_internal.h"

#include <algorithm>

namespace alq {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------------------- device
// ONE buffer resource per array for the whole launch: the patch goes into the scalar offset (not range-checked by the
// hardware), a lane with nothing to load or store aims past the array through its VECTOR offset, SW_OOB (loads then return
// 0, stores are dropped).  Fewer than 4096 patches per pass keep every byte offset below 2^32 (SWEEP_REQUIRE_PATCHES).
__device__ inline __amdgpu_buffer_rsrc_t sw_rsrc(const void *base, unsigned long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)(unsigned)bytes, 0x00020000);
}
constexpr unsigned SW_OOB = 0xffffff00u;

// a scalar the compiler must keep scalar: with ~100 live SGPRs it moved some row offsets to vector registers and wrapped every
// buffer access that used them in a waterfall loop
__device__ inline int sw_s(unsigned v) { return __builtin_amdgcn_readfirstlane((int)v); }

// a compile-time index passed to a generic lambda: decltype(arg)::value
template <int V> struct IC { static constexpr int value = V; };

// __builtin_amdgcn_sched_group_barrier mask of what may fill the gap behind an MFMA in a sweep's 1 : PIPE pattern: VALU (0x002) +
// SALU (0x004) + vector memory (0x010) + LDS (0x080).  With VALU alone the address arithmetic, loads and fragment reads piled up
// in a few gaps (a gap with up to two fillers is free, each further one costs its issue cycles -
// tools/probe/mfma_chain_probe.hip): -4 % cycles per step, of which the power-limited clock gives back about a third
constexpr int SW_FILL_MASK = 0x096;

// Scale exponent of a patch from the bit pattern fm of a bound on its max |x|: max |x| < 2^ex -> scale 2^(14 - ex), the hi
// pieces of the fp16 pairs then stay below 2^14; an all-zero patch: 0.  A patch whose maximum is below 2^-82 - fp32
// subnormals included - keeps the scale 2^96: 2^(14 - ex) would overflow the scale or underflow its inverse; such inputs
// are then simply small fp16 values.
__device__ inline int sw_patch_exp(unsigned fm) {
    const int ex = (int)((fm >> 23) & 255u) - 126;
    const int ce = 14 - ex;
    return fm ? (ce < 96 ? ce : 96) : 0;
}

// XCD-aware work order: workgroups b and b + 8 share an XCD (speed only), so grids are multiples of 8 (sweep_grid) and work is
// dealt per XCD: workgroup b belongs to XCD xcd = b % 8, which owns the npx patches 8 k + xcd, and is number jb = b / 8 of the
// G8 workgroups there.  A patch then stays on one XCD and its L2.
// (Macros, not functions: these kernels' instruction streams are scheduled by hand, and every function form tried - a struct
// with a member, a closure returned by value - came out of the compiler with an operand pair of one scalar add swapped.)
#define SW_XCD_DEAL(N)                                                                                         \
    const int G8 = (int)gridDim.x >> 3, xcd = (int)blockIdx.x & 7, jb = (int)blockIdx.x >> 3;                  \
    const int npx = (N) > xcd ? ((N) - xcd + 7) >> 3 : 0
// whole patches: workgroup jb takes k = jb, jb + G8, ... - npw patches; patch_of(i) = its i-th one, clamped to the last for i >= npw
#define SW_PATCH_ORDER(N)                                                                                      \
    SW_XCD_DEAL(N);                                                                                            \
    const int npw = npx > jb ? (npx - jb + G8 - 1) / G8 : 0;                                                   \
    auto patch_of = [&](int i) __attribute__((always_inline)) { return 8 * (jb + (i < npw ? i : npw - 1) * G8) + xcd; }

// ------------------------------------------------------------------------------------------------------------------ host
// Persistent grid: per_cu workgroups per CU, no more than there are work items, and a multiple of 8 (at least 8): work
// items are dealt per XCD (SW_XCD_DEAL).
inline unsigned sweep_grid(const alq_ctx *ctx, long long items, int per_cu) {
    const long long g = std::min<long long>((long long)per_cu * ctx->num_cus, items);
    return (unsigned)std::max<long long>(8, (g + 7) / 8 * 8);
}

// 3x3x3, stride 1, pad 1: the geometry every conv layer kernel is written for
inline bool is_conv3_same(const int k[3], const int lo[3], const int s[3]) {
    return k[0] == 3 && k[1] == 3 && k[2] == 3 && s[0] == 1 && s[1] == 1 && s[2] == 1 && lo[0] == 1 && lo[1] == 1 && lo[2] == 1;
}

// the kernels put (patch index) x (bytes of a patch, up to 1 MiB) into 32-bit scalar offsets
#define SWEEP_REQUIRE_PATCHES(N, name) ALQ_REQUIRE((N) < 4096, ALQ_EUNSUPPORTED, name ": 32-bit byte offsets hold fewer than 4096 patches per pass")

// raises the kernel's dynamic-LDS limit to what the launch asks for, launches on the context's stream, checks the launch
template <typename K, typename A>
inline int sweep_launch(alq_ctx *ctx, K kernel, unsigned grid, unsigned block, size_t lds, const A &args) {
    ALQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, ctx->stream, args);
    ALQ_HIP(hipGetLastError());
    return ALQ_OK;
}

}  // namespace alq

#endif
