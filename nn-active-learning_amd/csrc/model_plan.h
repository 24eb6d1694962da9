// Model planning as host arithmetic: the shape pass of a layer list (SAME pads, skip topology, the head rules, the batch caps)
// and the geometry descriptors of every contraction (ConvDesc for the igemm engines, G4Geom for the two-slot engine), each
// written once.  No dependency beyond alq.h and the standard library: tests/host/model_plan_main.cpp compiles this header with
// the host compiler alone and supplies its own set_error.  build_model allocates and plans from what is computed here.
#ifndef ALQ_MODEL_PLAN_H
#define ALQ_MODEL_PLAN_H
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "alq.h"

namespace alq {

void set_error(const char *fmt, ...);

#define ALQ_REQUIRE(cond, code, ...)                                                      \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            ::alq::set_error(__VA_ARGS__);                                                \
            return (code);                                                                \
        }                                                                                 \
    } while (0)

#define ALQ_TRY(expr)                                                                     \
    do {                                                                                  \
        int rc_ = (expr);                                                                 \
        if (rc_ != ALQ_OK) return rc_;                                                    \
    } while (0)

struct ConvDesc {
    // geometry of one GEMM: taps are INPUT offsets relative to m*sm
    int ID, IH, IW, Ci;
    int OD, OH, OW, Co;
    int MD, MH, MW;
    int sm = 1, so = 1, ooff[3] = {0, 0, 0};
    std::vector<int> tz, ty, tx;  // tap offsets
};

struct G4Geom {
    int kind = 0;             // 0 stride-1 conv (fwd, or bwd-data when flipped), 1 conv_transpose bwd-data, 2 conv_transpose fwd (all classes),
                              // 3 conv_transpose fwd, the one output parity class `cls`,
                              // 4 conv_transpose fwd, every class as its own tiles of one launch (input restaged per class)
    int cls[3] = {0, 0, 0};
    int ID = 1, IH = 1, IW = 1, Ci = 0;     // GEMM input tensor
    int OD = 1, OH = 1, OW = 1, Co = 0;     // GEMM output tensor
    int k[3] = {1, 1, 1}, s[3] = {1, 1, 1}, lo[3] = {0, 0, 0};
    bool flipped = false;
    double flops_per_patch = 0;
};

inline void same_pads(int in, int k, int s, int *out, int *lo) {
    *out = (in + s - 1) / s;
    int total = (*out - 1) * s + k - in;
    if (total < 0) total = 0;
    *lo = total / 2;
}

inline void enum_taps(const int k[3], std::vector<int> *tz, std::vector<int> *ty, std::vector<int> *tx) {
    for (int z = 0; z < k[0]; ++z)
        for (int y = 0; y < k[1]; ++y)
            for (int x = 0; x < k[2]; ++x) {
                tz->push_back(z); ty->push_back(y); tx->push_back(x);
            }
}

// ---- shape pass ------------------------------------------------------------------------------------------------------------
struct Shp { int D, H, W, C; };

struct LayerShape {
    Shp in = {1, 1, 1, 0};     // incl. concatenated skip channels
    Shp out = {1, 1, 1, 0};
    int lo[3] = {0, 0, 0};     // SAME pad-before (conv: of the fwd conv; convT: of the conv it transposes)
    int pidx = -1;             // parameterised-layer index t, or -1
    int64_t w_elems = 0, b_elems = 0;
    int64_t F = 0;             // fc: input features
};

struct ModelShape {
    std::vector<LayerShape> layers;
    std::vector<int> src_of;   // dest layer -> src layer
    std::vector<int> dest_of;  // src layer -> dest layer
    int L = 0;                 // parameterised layers
    bool dense = false;        // the head is a 1x1 conv: every voxel of its output is a sample
    int64_t V = 1;             // samples per patch
    int nclass = 0;
    int max_batch = 0;         // the requested batch under the caps below
};

// Shapes, pads, parameter counts and skip topology of a layer list on patches of in_dims (D, H, W, C; epp = their product), every
// rejection of a model the library does not run, and the workspace batch: requested_max_batch under the caps of the allocations.
inline int plan_shapes(const alq_layer_t *specs, int n_layers, const int32_t in_dims[4], long long epp, int requested_max_batch,
                       ModelShape *out) {
    ModelShape &ms = *out;
    ms = ModelShape();
    ms.layers.resize(n_layers);
    ms.src_of.assign(n_layers, -1);
    ms.dest_of.assign(n_layers, -1);
    ms.max_batch = requested_max_batch;
    std::vector<int> &src_of = ms.src_of, &dest_of = ms.dest_of;
    Shp cur = {in_dims[0], in_dims[1], in_dims[2], in_dims[3]};
    bool flat = false;
    int pidx = 0;
    for (int i = 0; i < n_layers; ++i) {
        LayerShape &ly = ms.layers[i];
        const alq_layer_t &sp = specs[i];
        Shp in = cur;
        if (sp.skip_src >= 0) {
            ALQ_REQUIRE(sp.skip_src < i - 1, ALQ_EUNSUPPORTED, "layer %d: skip source %d must be an earlier, non-adjacent layer", i, sp.skip_src);
            ALQ_REQUIRE(dest_of[sp.skip_src] < 0, ALQ_EUNSUPPORTED, "layer %d feeds more than one concat", sp.skip_src);
            const Shp &s = ms.layers[sp.skip_src].out;
            ALQ_REQUIRE(!flat && s.D == cur.D && s.H == cur.H && s.W == cur.W, ALQ_EUNSUPPORTED,
                        "layer %d: concat of maps of different size (resize_image_with_crop_or_pad) is outside the scored path", i);
            in.C = cur.C + s.C;
            src_of[i] = sp.skip_src;
            dest_of[sp.skip_src] = i;
        }
        Shp o = in;
        const int ind[3] = {in.D, in.H, in.W};
        switch (sp.type) {
            case ALQ_CONV: {
                ALQ_REQUIRE(!flat, ALQ_EINVAL, "layer %d: conv after fc", i);
                ALQ_REQUIRE(sp.s[0] == 1 && sp.s[1] == 1 && sp.s[2] == 1, ALQ_EUNSUPPORTED, "layer %d: strided conv", i);
                for (int d = 0; d < 3; ++d) {
                    int od;
                    same_pads(ind[d], sp.k[d], 1, &od, &ly.lo[d]);
                }
                o.C = sp.cout;
                ly.pidx = pidx++;
                ly.w_elems = (int64_t)sp.k[0] * sp.k[1] * sp.k[2] * in.C * sp.cout;
                ly.b_elems = sp.cout;
                break;
            }
            case ALQ_CONVT: {
                ALQ_REQUIRE(!flat, ALQ_EINVAL, "layer %d: conv_transpose after fc", i);
                for (int d = 0; d < 3; ++d) {
                    ALQ_REQUIRE(sp.k[d] >= sp.s[d], ALQ_EUNSUPPORTED, "layer %d: conv_transpose kernel < stride", i);
                    int od;
                    same_pads(ind[d] * sp.s[d], sp.k[d], sp.s[d], &od, &ly.lo[d]);
                }
                ALQ_REQUIRE(sp.s[0] == sp.s[1] || in.D == 1, ALQ_EUNSUPPORTED, "layer %d: anisotropic stride", i);
                ALQ_REQUIRE(sp.s[1] == sp.s[2], ALQ_EUNSUPPORTED, "layer %d: anisotropic stride", i);
                o.D = in.D * sp.s[0]; o.H = in.H * sp.s[1]; o.W = in.W * sp.s[2];
                o.C = sp.cout;
                ly.pidx = pidx++;
                ly.w_elems = (int64_t)sp.k[0] * sp.k[1] * sp.k[2] * in.C * sp.cout;
                ly.b_elems = sp.cout;
                break;
            }
            case ALQ_POOL: {
                ALQ_REQUIRE(!flat, ALQ_EINVAL, "layer %d: pool after fc", i);
                int od[3] = {in.D, in.H, in.W};
                for (int d = 0; d < 3; ++d) {
                    ALQ_REQUIRE(sp.k[d] == sp.s[d], ALQ_EUNSUPPORTED, "layer %d: pool window != stride", i);
                    ALQ_REQUIRE(sp.k[0] * sp.k[1] * sp.k[2] <= 255, ALQ_EUNSUPPORTED, "layer %d: pool window too large", i);
                    same_pads(ind[d], sp.k[d], sp.s[d], &od[d], &ly.lo[d]);
                }
                o.D = od[0]; o.H = od[1]; o.W = od[2];
                break;
            }
            case ALQ_FC: {
                ly.F = (int64_t)in.D * in.H * in.W * in.C;
                o = {1, 1, 1, sp.cout};
                ly.pidx = pidx++;
                ly.w_elems = ly.F * sp.cout;
                ly.b_elems = sp.cout;
                flat = true;
                break;
            }
            default:
                ALQ_REQUIRE(false, ALQ_EINVAL, "layer %d: unknown type %d", i, sp.type);
        }
        ly.in = in;
        ly.out = o;
        cur = o;
    }
    ms.L = pidx;
    if (n_layers > 0 && specs[n_layers - 1].type == ALQ_CONV) {
        // a fully-convolutional model: the head is a 1x1 conv without ReLU on a dense tensor; anything else that is not an
        // fc layer stays outside the library
        const int hl = n_layers - 1;
        const alq_layer_t &hs = specs[hl];
        const int Cin = hl > 0 ? ms.layers[hl - 1].out.C : in_dims[3];
        ALQ_REQUIRE(hs.k[0] == 1 && hs.k[1] == 1 && hs.k[2] == 1, ALQ_EUNSUPPORTED,
                    "a conv head must be 1x1 (found %dx%dx%d): the scored path needs an fc head or a 1x1 conv head", hs.k[0], hs.k[1], hs.k[2]);
        ALQ_REQUIRE(!hs.relu, ALQ_EUNSUPPORTED, "a conv head takes no ReLU: its outputs are the logits");
        ALQ_REQUIRE(hs.skip_src < 0, ALQ_EUNSUPPORTED, "a conv head on a concat (skip source %d) is unsupported", hs.skip_src);
        ALQ_REQUIRE(hs.cout >= 2 && hs.cout <= 8, ALQ_EUNSUPPORTED, "a conv head of %d classes is unsupported (2 .. 8)", hs.cout);
        ALQ_REQUIRE(dest_of[hl] < 0, ALQ_EUNSUPPORTED, "a conv head cannot be a skip source");
        ALQ_REQUIRE(Cin % 4 == 0 && Cin <= 64, ALQ_EUNSUPPORTED, "a conv head on %d channels is unsupported (a multiple of 4, at most 64)", Cin);
        ALQ_REQUIRE(hl == 0 || dest_of[hl - 1] < 0, ALQ_EUNSUPPORTED, "a conv head whose input is also a skip source is unsupported");
        ms.dense = true;
        ms.V = (int64_t)ms.layers[hl].out.D * ms.layers[hl].out.H * ms.layers[hl].out.W;
    } else {
        ALQ_REQUIRE(n_layers > 0 && specs[n_layers - 1].type == ALQ_FC, ALQ_EUNSUPPORTED,
                    "the scored path needs an fc head (get_gradients, NN_extended.py:1025) or a 1x1 conv head");
    }
    ms.nclass = ms.layers[n_layers - 1].out.C;
    ALQ_REQUIRE(ms.nclass >= 2 && ms.nclass <= 64, ALQ_EUNSUPPORTED, "%d classes unsupported", ms.nclass);
    {   // The GEMM engines address a tensor with unsigned 32-bit BYTE offsets from its base, and the two halves of a split
        // concat are one allocation: the workspace batch is the largest one every allocation stays below 2^30 floats with
        // (NET-C at 32^3: 2047 patches).  A caller that asks for more gets this many per device pass - alq_model_max_batch
        // reports it and the host walks a larger batch in passes (per-patch results do not depend on the split) - instead
        // of an error at the first launch.
        long long worst = epp;                                              // floats per patch of the largest allocation
        for (int i = 0; i < n_layers; ++i) {
            const Shp &o = ms.layers[i].out;
            long long e = (long long)o.D * o.H * o.W * o.C;
            if (src_of[i] >= 0) {                                           // consumer of a concat: source + direct producer share one
                const Shp &sh = ms.layers[src_of[i]].out;
                e = std::max(e, (long long)sh.D * sh.H * sh.W * (sh.C + ms.layers[i - 1].out.C));
            }
            worst = std::max(worst, e);
        }
        const long long limit = std::max(1LL, ((1LL << 30) - 64) / std::max(worst, 1LL));
        if (ms.max_batch > limit) ms.max_batch = (int)limit;
        if (ms.dense) {      // the posterior planes [c, NB V] and the cotangent rows [NB V, c] are allocations of the head's output size
                             // (in `worst` already); the voxels of one pass are indexed in 32 bits
            const long long lim2 = std::max(1LL, ((1LL << 31) - 1) / (long long)ms.V);
            if (ms.max_batch > lim2) ms.max_batch = (int)lim2;
        }
    }
    ALQ_REQUIRE(ms.L <= 16, ALQ_EUNSUPPORTED, "%d parameterised layers > 16", ms.L);
    // concat = two producers writing channel slices of one buffer: the direct producer of a concat's input feeds nothing else
    for (int d = 0; d < n_layers; ++d)
        if (src_of[d] >= 0)
            ALQ_REQUIRE(dest_of[d - 1] < 0 && src_of[d] != d - 1, ALQ_EUNSUPPORTED, "layer %d: unsupported skip topology", d);
    return ALQ_OK;
}

// ---- descriptor builders -----------------------------------------------------------------------------------------------------
// `in` / `out`: the LAYER's input (incl. concatenated channels) and output shape; `lo`: its pad-before; a backward-data descriptor
// is the GEMM from the cotangent of `out` to the cotangent of `in`.
namespace plan_detail {

// the GEMM from tensor a to tensor b, one row per point of grid m
inline ConvDesc desc_of(const Shp &a, const Shp &b, const Shp &m) {
    ConvDesc d;
    d.ID = a.D; d.IH = a.H; d.IW = a.W; d.Ci = a.C;
    d.OD = b.D; d.OH = b.H; d.OW = b.W; d.Co = b.C;
    d.MD = m.D; d.MH = m.H; d.MW = m.W;
    return d;
}

inline G4Geom geom_of(int kind, const Shp &a, const Shp &b, const alq_layer_t &sp, const int lo[3]) {
    G4Geom g;
    g.kind = kind;
    g.ID = a.D; g.IH = a.H; g.IW = a.W; g.Ci = a.C;
    g.OD = b.D; g.OH = b.H; g.OW = b.W; g.Co = b.C;
    for (int q = 0; q < 3; ++q) { g.k[q] = sp.k[q]; g.s[q] = sp.s[q]; g.lo[q] = lo[q]; }
    return g;
}

}  // namespace plan_detail

// stride-1 conv, y[p] = sum_t x[p + t - lo] W[t]: tap t reads at offset t - lo
inline ConvDesc conv_fwd_desc(const Shp &in, const Shp &out, const alq_layer_t &sp, const int lo[3]) {
    ConvDesc d = plan_detail::desc_of(in, out, out);
    enum_taps(sp.k, &d.tz, &d.ty, &d.tx);
    for (size_t t = 0; t < d.tz.size(); ++t) { d.tz[t] -= lo[0]; d.ty[t] -= lo[1]; d.tx[t] -= lo[2]; }
    return d;
}
inline G4Geom conv_fwd_geom(const Shp &in, const Shp &out, const alq_layer_t &sp, const int lo[3]) {
    return plan_detail::geom_of(0, in, out, sp, lo);
}

// ... its backward-data: dx[q] = sum_t dy[q + lo - t] W[t], the flipped taps
inline ConvDesc conv_bwd_desc(const Shp &in, const Shp &out, const alq_layer_t &sp, const int lo[3]) {
    ConvDesc b = plan_detail::desc_of(out, in, in);
    enum_taps(sp.k, &b.tz, &b.ty, &b.tx);
    for (size_t t = 0; t < b.tz.size(); ++t) { b.tz[t] = lo[0] - b.tz[t]; b.ty[t] = lo[1] - b.ty[t]; b.tx[t] = lo[2] - b.tx[t]; }
    return b;
}
inline G4Geom conv_bwd_geom(const Shp &in, const Shp &out, const alq_layer_t &sp, const int lo[3]) {
    G4Geom g = plan_detail::geom_of(0, out, in, sp, lo);
    g.flipped = true;
    return g;
}

// conv_transpose: output parity classes along z (a 2-D layer with s[0] = 1 has one)
inline int convt_classes_z(const Shp &in, const alq_layer_t &sp) { return in.D == 1 && sp.s[0] == 1 ? 1 : sp.s[0]; }

// y[p] = sum_{q,t: s*q + t - lo = p} x[q] W[t]; output parity class c = p mod s uses the
// taps t == (c + lo) mod s at input offset (c + lo - t)/s   (<= 0)
// *taps: the class's taps as indices into the k^3 tap enumeration, in the order of the descriptor's tap offsets
inline ConvDesc convt_class_desc(const Shp &in, const Shp &out, const alq_layer_t &sp, const int lo[3], int cz, int cy, int cx,
                                 std::vector<int> *taps) {
    ConvDesc d = plan_detail::desc_of(in, out, in);
    d.so = sp.s[2];
    d.ooff[0] = cz; d.ooff[1] = cy; d.ooff[2] = cx;
    std::vector<int> az, ay, ax;
    enum_taps(sp.k, &az, &ay, &ax);
    taps->clear();
    for (size_t t = 0; t < az.size(); ++t) {
        const int nz = cz + lo[0] - az[t], ny = cy + lo[1] - ay[t], nx = cx + lo[2] - ax[t];
        if (nz % sp.s[0] || ny % sp.s[1] || nx % sp.s[2]) continue;
        d.tz.push_back(nz / sp.s[0]); d.ty.push_back(ny / sp.s[1]); d.tx.push_back(nx / sp.s[2]);
        taps->push_back((int)t);
    }
    return d;
}
// this class alone on the two-slot engine (used when the fused form does not fit)
inline G4Geom convt_class_geom(const Shp &in, const Shp &out, const alq_layer_t &sp, const int lo[3], int cz, int cy, int cx) {
    G4Geom g = plan_detail::geom_of(3, in, out, sp, lo);
    g.cls[0] = cz; g.cls[1] = cy; g.cls[2] = cx;
    return g;
}
// the whole layer in one launch: kind 2 (every class from one staged block) or 4 (the classes as tiles)
inline G4Geom convt_all_geom(const Shp &in, const Shp &out, const alq_layer_t &sp, const int lo[3], int kind) {
    return plan_detail::geom_of(kind, in, out, sp, lo);
}

// ... its backward-data: dx[q] = sum_t dy[s*q + t - lo] W[t], a GEMM row per input point with row stride sm = s
inline ConvDesc convt_bwd_desc(const Shp &in, const Shp &out, const alq_layer_t &sp, const int lo[3]) {
    ConvDesc b = plan_detail::desc_of(out, in, in);
    b.sm = sp.s[2];
    enum_taps(sp.k, &b.tz, &b.ty, &b.tx);
    for (size_t t = 0; t < b.tz.size(); ++t) { b.tz[t] -= lo[0]; b.ty[t] -= lo[1]; b.tx[t] -= lo[2]; }
    return b;
}
inline G4Geom convt_bwd_geom(const Shp &in, const Shp &out, const alq_layer_t &sp, const int lo[3]) {
    return plan_detail::geom_of(1, out, in, sp, lo);
}

// fc on F features: one point, one tap; its backward-data is the same GEMM with the channels swapped
inline ConvDesc fc_fwd_desc(int64_t F, int cout) {
    const Shp one = {1, 1, 1, 0};
    ConvDesc d = plan_detail::desc_of(one, one, one);
    d.Ci = (int)F; d.Co = cout;
    d.tz = {0}; d.ty = {0}; d.tx = {0};
    return d;
}
inline ConvDesc fc_bwd_desc(int64_t F, int cout) {
    ConvDesc b = fc_fwd_desc(F, cout);
    std::swap(b.Ci, b.Co);
    return b;
}

}  // namespace alq
#endif
