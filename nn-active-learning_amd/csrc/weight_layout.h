// The host arithmetic of weight setting (weights.hip): the L1 norms the static fp16x2 bounds are chained from, the maps from the
// TF filter layouts to the engines' B matrices, and the two-class head's difference vector with its fp16-pair pre-split.  No
// HIP dependency: tests/host/weight_layout_main.cpp compiles this header as plain C++ (f16_pair.h needs the clang++ of ROCm).
#ifndef ALQ_WEIGHT_LAYOUT_H
#define ALQ_WEIGHT_LAYOUT_H
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "f16_pair.h"

namespace alq {

// bwd_l1 = max over ci of sum_{tap, co} |W|; out_l1 = max over co of sum_{tap, ci} |W| and out_bmax = max |b|, both times 1 + 1e-6:
// |cotangent of the input| <= bwd_l1 * max |cotangent of the output|, |out| <= out_l1 * max |in| + out_bmax (a conv_transpose
// counts all taps: an output point sees a subset of them, the bound is only looser).
// conv W[tap][ci][co], conv_transpose (transposed) W[tap][co][ci].  One walk in (tap, ci, co) order: the sum of a ci adds its
// terms taps outer, co inner, the sum of a co taps outer, ci inner.
inline void conv_norms(const float *W, const float *b, int ntaps, int Ci, int Co, bool transposed, double *bwd_l1, float *out_l1, float *out_bmax) {
    std::vector<double> in((size_t)Ci, 0.0), out((size_t)Co, 0.0);
    for (int tp = 0; tp < ntaps; ++tp)
        for (int ci = 0; ci < Ci; ++ci)
            for (int co = 0; co < Co; ++co) {
                const double a = std::fabs((double)(transposed ? W[((size_t)tp * Co + co) * Ci + ci] : W[((size_t)tp * Ci + ci) * Co + co]));
                in[(size_t)ci] += a;
                out[(size_t)co] += a;
            }
    double best = 0, ob = 0, bm = 0;
    for (int ci = 0; ci < Ci; ++ci) best = std::max(best, in[(size_t)ci]);
    for (int co = 0; co < Co; ++co) {
        ob = std::max(ob, out[(size_t)co]);
        bm = std::max(bm, std::fabs((double)b[co]));
    }
    *bwd_l1 = best;
    *out_l1 = (float)(ob * (1.0 + 1e-6));
    *out_bmax = (float)(bm * (1.0 + 1e-6));
}

// bwd_l1 of conv_norms per slice of a concatenated input: part[0] over the input channels ci < split (the skip source's, which a concat
// puts first), part[1] over the others.  The cotangent of either producer is bounded by its own slice's norm: one norm over all
// channels is loose for the producer of the smaller slice by the ratio of the two, and the fp16 pairs of the launches below it
// lose that many bits.
// amax[s] = max |w| of slice s.  The fp16 pairs of a filter share ONE exponent (f16_pair_exp) and the launch ONE input scale per
// patch: slices_within_f16_range says whether both slices keep their bits under that (the pairs sit at 2^14, fp16 ends 2^-24
// below 1: a slice 2^20 below the other still has 18 bits of its hi piece; beyond, the model leaves the fp16-pair launches).
inline void conv_bwd_l1_slices(const float *W, int ntaps, int Ci, int Co, bool transposed, int split, double part[2], float amax[2]) {
    std::vector<double> in((size_t)Ci, 0.0);
    amax[0] = amax[1] = 0.f;
    for (int tp = 0; tp < ntaps; ++tp)
        for (int ci = 0; ci < Ci; ++ci)
            for (int co = 0; co < Co; ++co) {
                const float w = std::fabs(transposed ? W[((size_t)tp * Co + co) * Ci + ci] : W[((size_t)tp * Ci + ci) * Co + co]);
                in[(size_t)ci] += (double)w;
                amax[ci < split ? 0 : 1] = std::max(amax[ci < split ? 0 : 1], w);
            }
    part[0] = part[1] = 0;
    for (int ci = 0; ci < Ci; ++ci) part[ci < split ? 0 : 1] = std::max(part[ci < split ? 0 : 1], in[(size_t)ci]);
}

constexpr int F16_SLICE_BINADES = 20;
inline bool slices_within_f16_range(const float amax[2]) {
    if (!(amax[0] > 0.f) || !(amax[1] > 0.f)) return true;      // an all-zero slice has nothing to lose
    int e0 = 0, e1 = 0;
    (void)std::frexp(amax[0], &e0);
    (void)std::frexp(amax[1], &e1);
    return std::abs(e0 - e1) <= F16_SLICE_BINADES;
}

// fc W[o][f]: max over f of sum_o |W| - |cotangent of input f| <= sum_o |W[o][f]| * max |cotangent of the output|
inline double fc_col_l1(const float *W, int Co, int64_t F) {
    std::vector<double> col((size_t)F, 0.0);
    for (int o = 0; o < Co; ++o)
        for (int64_t f = 0; f < F; ++f) col[(size_t)f] += std::fabs((double)W[(size_t)o * F + f]);
    double best = 0;
    for (int64_t f = 0; f < F; ++f) best = std::max(best, col[(size_t)f]);
    return best;
}

// out[(j, c)][r] = W[(taps[j], r)][c] for j < ntaps (taps == null: tap j itself).  With (R, C) = (Ci, Co) the conv's backward B
// [(tap, co)][ci] from its filter [(tap, ci)][co]; with (R, C) = (Co, Ci) the conv_transpose's forward B [(tap, ci)][co] from
// its filter [(tap, co)][ci], over all taps or the tap list of one output parity class; with one tap the plain transpose, an fc
// layer's B [f_mem][o] from Wp [o][f_mem] with (R, C) = (Co, F).
inline std::vector<float> transpose_taps(const float *W, int R, int C, int ntaps, const int *taps = nullptr) {
    std::vector<float> out((size_t)ntaps * R * C);
    for (int j = 0; j < ntaps; ++j)
        for (int r = 0; r < R; ++r)
            for (int c = 0; c < C; ++c) out[((size_t)j * C + c) * R + r] = W[((size_t)(taps ? taps[j] : j) * R + r) * C + c];
    return out;
}

// columns [j w, (j + 1) w) of B [K][Co]: one output-channel slice of a wide conv
inline std::vector<float> column_slice(const std::vector<float> &B, int K, int Co, int j, int w) {
    std::vector<float> out((size_t)K * w);
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < w; ++c) out[(size_t)k * w + c] = B[(size_t)k * Co + (size_t)j * w + c];
    return out;
}

// fc: TF W[o][f_tf] -> Wp[o][f_mem]; activation memory order f_mem = ((d*H+h)*W+w)*C+c, reference flatten order
// f_tf = ((c*W+w)*H+h)*D+d (tf.transpose = full axis reversal, NN.py:296-301)
inline std::vector<float> fc_to_mem_order(const float *W, int Co, int D, int H, int Wd, int C) {
    const int64_t F = (int64_t)D * H * Wd * C;
    std::vector<float> Wp((size_t)Co * F);
    for (int d = 0; d < D; ++d)
        for (int h = 0; h < H; ++h)
            for (int w = 0; w < Wd; ++w)
                for (int c = 0; c < C; ++c) {
                    const int64_t fm = (((int64_t)d * H + h) * Wd + w) * C + c;
                    const int64_t ft = (((int64_t)c * Wd + w) * H + h) * D + d;
                    for (int o = 0; o < Co; ++o) Wp[(size_t)o * F + fm] = W[(size_t)o * F + ft];
                }
    return Wp;
}

// two-class head Wp[2][F]: its input cotangent under the unit cotangent (+1, -1), wv = W0 - W1, and max |wv|
inline std::vector<float> head_wv(const float *Wp, int64_t F, float *amax) {
    std::vector<float> wv((size_t)F);
    *amax = 0.f;
    for (int64_t f = 0; f < F; ++f) {
        wv[(size_t)f] = (0.f + Wp[(size_t)f]) - Wp[(size_t)F + f];
        *amax = std::max(*amax, std::fabs(wv[(size_t)f]));
    }
    return wv;
}

// wv (F % 4 == 0, amax = max |wv| > 0) as fp16 pairs of x 2^e, e = 14 - exponent(amax) (the scale igemm4_launch derives from
// the same maximum): per 4 consecutive values the words [h0 h1 | h2 h3 | l0 l1 | l2 l3], h = fp16(x 2^e), l = fp16((x 2^e - h) 2^11)
inline std::vector<unsigned> head_wv16(const std::vector<float> &wv, float amax, int *e_out) {
    int ex = 0;
    (void)std::frexp(amax, &ex);
    const int e = *e_out = 14 - ex;
    std::vector<unsigned> sp(wv.size());
    for (size_t f = 0; f + 4 <= wv.size(); f += 4) {
        unsigned short h[4], l[4];
        for (int k = 0; k < 4; ++k) f16_pair_split(wv[f + k], e, 11, &h[k], &l[k]);
        sp[f] = h[0] | ((unsigned)h[1] << 16); sp[f + 1] = h[2] | ((unsigned)h[3] << 16);
        sp[f + 2] = l[0] | ((unsigned)l[1] << 16); sp[f + 3] = l[2] | ((unsigned)l[3] << 16);
    }
    return sp;
}

}  // namespace alq

#endif
