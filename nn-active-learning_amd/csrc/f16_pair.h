// The arithmetic of the host weight packers of the layer kernels (c3d, d3d, f3d, e3d, t3d, t3d8b .hip): a weight w becomes the
// fp16 pair w 2^e = h + l 2^-lo_shift.  No HIP dependency: tests/host/f16_pair_main.cpp compiles this header as plain C++ (with
// a compiler that knows _Float16: the clang++ of ROCm).
#ifndef ALQ_F16_PAIR_H
#define ALQ_F16_PAIR_H
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

namespace alq {

// Scale exponent of an array: max |w| < 2^ex -> e = 14 - ex: the largest w 2^e lands in [2^13, 2^14).  An all-zero array: 14.
inline int f16_pair_exp(const float *w, size_t n) {
    float amax = 0.f;
    for (size_t i = 0; i < n; ++i) amax = std::max(amax, std::fabs(w[i]));
    int ex = 0;
    if (amax > 0.f) (void)std::frexp(amax, &ex);
    return 14 - ex;
}

// hi = fp16(w 2^e) (round to nearest even), lo = fp16((w 2^e - hi) 2^lo_shift): the remainder is exact in fp32.  lo_shift = 0: the
// lo piece at its true scale (one accumulator takes all three products; small remainders are fp16 subnormals, which the
// matrix cores must keep: c3d_subnormals_ok); lo_shift = 11: scaled up into the normal range, its two products go to a second
// accumulator that the epilogue scales back.
inline void f16_pair_split(float w, int e, int lo_shift, unsigned short *hi, unsigned short *lo) {
    const float ws = std::ldexp(w, e);
    const _Float16 h = (_Float16)ws;
    const _Float16 l = (_Float16)std::ldexp(ws - (float)h, lo_shift);
    std::memcpy(hi, &h, 2);
    std::memcpy(lo, &l, 2);
}

}  // namespace alq

#endif
