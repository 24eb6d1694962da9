// The model plan of libalq.so: what model.hip (plans, entry points), passes.hip (forward pass, Fisher backward sweep), grads.hip (general gradient
// path) and weights.hip (weight setting) share.  A Layer describes the model and its weights: during a pass only device memory changes.
// The shapes and geometry descriptors a plan is built from (plan_shapes, ConvDesc, G4Geom and their builders) are host arithmetic in model_plan.h.
#pragma once
#include <algorithm>

#include "alq_internal.h"

namespace alq {

struct Layer {
    alq_layer_t spec;
    int pidx = -1;             // parameterised-layer index t, or -1
    View in, out;              // activation views (in = incl. concatenated skip channels)
    View din, dout;            // cotangent views, same geometry
    int lo[3] = {0, 0, 0};     // SAME pad-before (conv: of the fwd conv; convT: of the conv it transposes)
    bool dense_fc_small = false;
    bool dense_head = false;   // the 1x1 conv head of a fully-convolutional model (dense.hip): no engine plans, weights in d_W32 as [Ci][c]
    int64_t F = 0;             // fc: input features
    // weights
    int64_t w_elems = 0, b_elems = 0;
    float *d_bias = nullptr;
    float *d_Wp = nullptr;     // skinny fc: [nout][F] in activation-memory order
    std::vector<Gemm> fwd;        // 1 contraction (conv / fc) or one per output parity class (convT)
    // conv whose output is too wide for the matrix-core engines (NET-B's 96-channel conv: igemm2 / igemm3 hold <= 48, the two-slot
    // engine <= 32 output channels) and would run on the fp32 engine: the same contraction as launches of fwd_co_w output channels
    // each, writing channel slices of the output (round 6)
    std::vector<Gemm> fwd_co;
    int fwd_co_w = 0;
    Igemm4Plan fwd_all;           // convT: every output class from one staged block (igemm4.hip), when eligible
    Gemm bwd;
    bool has_bwd = false;
    bool weights_set = false;
    // wide fc layer packed on the device (alq_model_set_weights_device): the raw fp32 weights stay resident in activation-memory
    // order [o][f_mem]; the forms only the debug knobs select (igemm / igemm2 / igemm3 behind the streaming GEMM) are packed from
    // them on the host when a call first needs them (refresh_fallback_forms)
    float *d_Wres = nullptr;
    bool fallback_stale = false;
    // workspaces
    uint8_t *argmax = nullptr;
    float *asum = nullptr, *dsum = nullptr;
    double *ls_field = nullptr; // [max_batch, out voxels] (fc: [max_batch]): field of alq_class_layer_sums, filled once per call
    float *osum = nullptr;     // channel sums of this layer's OUTPUT (spatial layers): next layers' asum
    float *fc_partials = nullptr;
    // fc head of a Fisher pass on top of a ReLU conv: its input cotangent is [input > 0] * fc_wv for every patch; the
    // forward pass leaves the signs (one byte per 4 elements), the backward pass of the conv below contracts them
    // directly (igemm4 BITSRC)
    unsigned *fc_maskbits = nullptr;
    float *fc_wv = nullptr;
    unsigned *fc_wv16 = nullptr;       // fc_wv pre-split into fp16 pairs for the fp16x2 contraction of the conv below (BITSRC)
    float fc_wv_amax = 0.f;            // max |W0 - W1| of a two-output head (host side, set with the weights)
    unsigned *amax_fwd = nullptr;          // [max_batch] per-patch max |output| of a forward pass that asked for it
    // Static bounds for the fp16x2 contraction of backward launches (no data pass needed): bwd_l1 = max over the input
    // channels of sum_{taps, output channels} |W| (set with the weights), i.e. |cotangent of the input| <= bwd_l1 * max
    // |cotangent of the output|; a Fisher pass chains them down from the unit cotangent at the logits (bwd_bounds, passes.hip).
    double bwd_l1 = 0;
    bool f16_slices_apart = false;     // ... and its two weight slices lie further apart than one fp16-pair exponent holds (slices_within_f16_range):
                                       // every pass of the model then runs on bf16 triples (apply_knobs)
    double bwd_l1_part[2] = {0, 0};    // a conv / conv_transpose over a concat: bwd_l1 of the skip source's channels and of the others (0: no concat)
    // flip-safe fused head (the conv under a two-class head): plain fp32 copy of the weights in TF layout [tap][ci][co] for the
    // exact re-evaluation, and max over co of sum_{tap, ci} |W|
    float *d_W32 = nullptr;
    float fwd_l1 = 0.f;
    float out_l1 = 0.f, out_bmax = 0.f;    // |out| <= out_l1 * max |in| + out_bmax (conv: = fwd_l1; conv_transpose: all taps), set with the weights
    unsigned *bound_fwd = nullptr;         // per-patch bound on |out| derived from the first layer's measured maximum (k_fwd_bounds)
    float *fc_part2 = nullptr;         // partial logits per (tile, wave) when the conv below computes them in its epilogue
    int fc_slices2 = 0;
    // plane-sweep engine (c3d.hip) for the conv under the fused two-class head (and its backward): plans on the conv layer,
    // per-(patch, wave) partials of the logit difference / of the head's input sum on the head layer
    C3dPlan c3f, c3b;
    D3dPlan d3f;                           // forward on the row-sweep engine of d3d.hip (NET-C's dec1)
    F3dPlan f3f;                           // forward fused with the max-pool behind it (f3d.hip; NET-C's enc2)
    E3dPlan e3b;                           // backward fused with the pool backward steps on either side (e3d.hip; NET-C's enc2)
    T3dPlan t3f, t3b;                      // row-sweep engine for the stride-2 conv_transpose (t3d.hip), forward / backward-data
    float *c3_part = nullptr, *c3_asum = nullptr;
    unsigned short *fc_wv16c = nullptr;    // fc_wv as fp16 pairs at their true scale, [voxel][h8 | l8] (c3d_presplit_vec), for c3b
    int fc_slices = 0;
    bool out_is_skip_src = false;
    // convT class tap lists (indices into the k^3 tap enumeration)
    std::vector<std::vector<int>> class_taps;
    // alq_hess_vecp (hvp.hip): the plain fp32 weights in the TF layout.  The host keeps the copy alq_model_set_weights was given
    // (hv_src = 1) or notes that the layer holds them resident in fp32 (hv_src = 2: a device-packed wide fc layer's d_Wres;
    // hv_src = 3: a skinny fc layer's d_Wp); the device copy
    // hv_W and the call's fp64 tensors of this layer's output - activation hv_A, its cotangent hv_D, their tangents hv_Ra / hv_Rd,
    // dense [max_batch, vox, C] - are allocated and filled by the first product.  hv_stale: hv_W is older than the weights.
    std::vector<float> hv_hW;
    int hv_src = 0;
    bool hv_stale = false;
    float *hv_W = nullptr;
    double *hv_A = nullptr, *hv_D = nullptr, *hv_Ra = nullptr, *hv_Rd = nullptr;
};

}  // namespace alq

// What the last pass of a model ran (alq_model_engine_info).  run_forward starts from fwd = {}; run_backward_main, run_backward_general
// and the fp64 sweep of alq_hess_vecp start from bwd = {}: the backward part speaks of the LAST backward pass, whichever kind it was.
struct PassInfo {
    struct Fwd {
        bool head_fused = false;   // the pass did not store the last conv's output (fc head fused into it)
        bool c3 = false;           // it ran the head conv on the plane-sweep engine (c3d.hip)
        int t3f = 0;               // conv_transpose launches on the row-sweep engine (t3d.hip)
        int d3f = 0;               // dec1 ran on the row-sweep engine (d3d.hip)
        int f3f = 0;               // enc2 and the pool behind it ran fused (f3d.hip)
        int dcp = 0;               // form of the first conv + pool kernel, 0 = it did not run (direct.hip: g_dcp_last_form)
        bool f16_derived = false;  // a launch ran on the fp16x2 split with derived input bounds
        bool v3f16 = false;        // igemm3's forward launches ran on fp16 pairs under bounds derived from the input maxima (in_amax)
        bool amax_asked[64] = {};  // per layer: the pass asked its launch for the per-patch output maxima (amax_fwd; plan_input_scales)
        bool signs_ready[64] = {}; // per layer (alq_model_create: at most 64): a launch wrote the sign field of its output (View::sg); the
                                   // backward sweep of the same Fisher pass and alq_model_debug_copy read it
    } fwd;
    struct Bwd {                   // launches of a Fisher pass's backward sweep only
        bool c3_bwd = false;       // the head conv's backward ran on the plane-sweep engine
        int c3b_grid = 0;          // workgroups of that launch
        int t3b = 0;               // conv_transpose launches on the row-sweep engine
        int e3b = 0;               // pool2 backward, enc2 backward and pool1 backward ran as one launch (e3d.hip)
        int e3b_form = 0;          // form of that launch: 0 none, 1 row sweep, 2 z plane sweep
        int d3b = 0;               // dec1's backward-data launch ran on d3d.hip
        int nbounds = 0;           // layers of dout_bound (0: no Fisher backward since)
        float dout_bound[64] = {}; // per layer: the static cotangent bound of bwd_bounds (passes.hip); <= 0 = unknown
    } bwd;
    int lsum = 0;                  // the last GENERAL backward sweep ran the fused layer-sum kernels (set by run_backward_general only)
    bool call_fisher = false;      // the last entry point ran a Fisher pass (prepare_call)
};

struct alq_model {
    alq_ctx *ctx = nullptr;
    int max_batch = 0;
    alq::EngineSwitches sw;          // engine-selection switches, read from the environment ONCE, when this model is created
                                     // (engine_switches.h); every call applies the model's own snapshot
    PassInfo last;                   // what the last pass ran (alq_model_engine_info, alq_model_debug_copy)
    // per-patch max |x| (float bits) of the two producers of the fused-head conv's input, for its fp16x2 contraction
    unsigned *amax_a = nullptr, *amax_b = nullptr, *amax_tiles = nullptr;
    unsigned *flip_cnt = nullptr, *flip_list = nullptr;     // candidates of the flip-safe fused head (igemm4 FCF + F16)
    int flip_cap = 0;
    unsigned *bound_all = nullptr;          // [layer][max_batch] derived per-patch output bounds (float bits), k_fwd_bounds
    unsigned *in_amax = nullptr;            // [max_batch] measured max |x| of every patch of the network input (igemm3's forward fp16 pairs)
    bool v3_fwd_f16 = false;                // some forward conv launch stays on igemm3 and has the fp16-pair twin packed (set at build)
    unsigned *flip_overflow = nullptr;      // marked groups beyond the scan's lists since the model was created: drained by the sweep path of flip_fix_kernel (kernels.hip), none dropped
    size_t amax_tiles_len = 0;
    int in_dims[4] = {1, 1, 1, 1};
    int nclass = 0;
    bool dense = false;            // fully-convolutional: the last layer is a 1x1 conv head, every voxel of its output is a sample
    int64_t V = 1;                 // samples (voxels of the head's output) per patch; 1 for an fc head
    bool aleatoric = false;        // alq_model_set_aleatoric: the head's last channel is a log-variance (AU_4U), nclass - 1 classes
    float *au = nullptr;           // ... [max_batch V]: its ReLU of the running pass
    double *dh_part = nullptr;     // dense head backward: per-workgroup partials of dW and db (dense.hip)
    int L = 0;
    std::vector<alq::Layer> layers;
    std::vector<void *> allocs;
    float *logits = nullptr, *dlogits = nullptr, *post = nullptr;
    double *S = nullptr, *sizes = nullptr, *Apart = nullptr;
    double *Spart = nullptr;       // [L][max_batch][nslab_max] box-dot slab partials
    int *nslab = nullptr;          // [L] slabs actually written per layer
    int nslab_max = 1;
    float *wg_partial = nullptr;   // slab partials of the weight-gradient kernels (grown on demand)
    size_t wg_partial_len = 0;
    double *gn_partial = nullptr;  // per-(sample, workgroup) partials of the gradient-norm kernels (grown on demand)
    size_t gn_partial_len = 0;
    double *df_scratch = nullptr;  // alq_diag_fisher (dfisher.hip), allocated by its first call: sample-group partials of a conv layer's
                                   // weights, per-sample channel sums, squared fc cotangents - whichever is largest
    // alq_class_layer_sums (lsum.hip), allocated by its first call: the layers' class-independent fields (Layer::ls_field), the
    // slab partials [L][max_batch][ls_nslab_max] of one class slot and the slabs each layer writes
    double *ls_part = nullptr;
    std::vector<int> ls_nslab;
    int ls_nslab_max = 0;
    float *x_stage = nullptr;      // [max_batch, elems per patch]: rows gathered by the *_rows entry points
    int64_t epp = 0;               // elements per patch
    int f16_fwd_derived = 0;       // layers (bits) whose forward launch takes the fp16x2 split with DERIVED input bounds (see run_forward)
    int64_t host_pack_elems = 0;   // weight elements that went through the host packers since the model was created (engine info 14)
    void *d_wscal = nullptr;       // 16 bytes: the scalars of the device packers (wpack.hip)
    bool hv_ready = false;         // alq_hess_vecp has allocated its workspaces (first call)
    double *hv_part = nullptr;     // slab partials of the weight products (hvp_wgrad_partial_doubles)
    double *hv_p64 = nullptr;      // [max_batch, c]: the posteriors of the call in fp64

    template <typename T>
    int dalloc(T **p, size_t count) {
        void *q = nullptr;
        const size_t bytes = std::max<size_t>(count * sizeof(T), 256);
        if (hipMalloc(&q, bytes) != hipSuccess) {
            alq::set_error("hipMalloc of %zu bytes failed", bytes);
            return ALQ_ENOMEM;
        }
        allocs.push_back(q);
        *p = reinterpret_cast<T *>(q);
        return ALQ_OK;
    }
};

// *d (a T * or the void * of a plan): count elements of T on the device, allocated on the first call and kept
template <typename T, typename D>
int ensure(alq_model *m, D **d, size_t count) {
    T *p = static_cast<T *>(*d);
    if (!p) ALQ_TRY(m->dalloc(&p, count));
    *d = p;
    return ALQ_OK;
}

// Host array to such a buffer: the copy is queued on the context's stream, and the caller synchronises before h may change
template <typename T, typename D>
int upload(alq_model *m, D **d, const std::vector<T> &h) {
    ALQ_TRY(ensure<T>(m, d, h.size()));
    ALQ_HIP(hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, m->ctx->stream));
    return ALQ_OK;
}

// ... for the plans that do not keep their host copy: upload, synchronise, release h
template <typename T, typename D>
int upload_release(alq_model *m, D **d, std::vector<T> *h) {
    ALQ_TRY(upload(m, d, *h));
    ALQ_HIP(hipStreamSynchronize(m->ctx->stream));
    std::vector<T>().swap(*h);
    return ALQ_OK;
}

namespace alq { int refresh_fallback_forms(alq_model *m); }      // weights.hip

// ---- model.hip and passes.hip, for each other and for the general gradient path (grads.hip)
// dropout of a training / MC forward pass: layers whose OUTPUT is dropped (NN.py:169-171), one keep probability
struct DropSpec {
    unsigned long long layers = 0;     // bit i = layer i
    float keep_prob = 1.f;
    unsigned long long seed = 0;
    long long first_sample = 0;        // id of patch 0 of this call: masks are keyed by sample id, not by batch position
    bool on(int i) const { return keep_prob < 1.f && i < 64 && ((layers >> i) & 1ull); }
};
int make_drop(const alq_model *m, float keep_prob, uint64_t seed, int64_t first_sample, const int32_t *h_layers, int n_layers, DropSpec *d);
int prepare_call(alq_model *m, bool fisher);
int run_forward(alq_model *m, const float *d_x, int N, bool with_sums, bool keep_all = false, const DropSpec *drop = nullptr);
int run_backward(alq_model *m, const float *d_x, int N);      // the backward sweep of a Fisher pass, behind run_forward(..., with_sums = true)
// Which engine a gemm_launch call takes.
enum GemmRoute { ROUTE_DIRECT, ROUTE_FCGEMM, ROUTE_IGEMM4, ROUTE_IGEMM3, ROUTE_IGEMM2, ROUTE_IGEMM };
GemmRoute gemm_route(const alq::Gemm &g, const alq::View &in, const alq::View &out, int accumulate, const alq::Igemm2Fuse *fuse);
int gemm_launch(alq_ctx *ctx, const alq::Gemm &g, const alq::View &in, const alq::View &out, const float *bias, int relu, int accumulate, int N,
                int cls, const alq::Igemm2Fuse *fuse = nullptr, bool *fused = nullptr, float fc_in_bound = 0.f);
alq::View flat_view(const alq::View &v);

// ---- grads.hip, for the entry points of model.hip: the head of a fully-convolutional model, and the refusal of the fc-only calls
// (an aleatoric model: posteriors [nclass - 1, N V] and predictions over the classes; d_au [N V] and d_logits [N V, nclass] optional)
int dense_forward_head(alq_model *m, const float *d_x, int N, float *d_post, int64_t *d_pred, bool want_logits, float *d_au = nullptr,
                       float *d_logits = nullptr);
#define ALQ_REFUSE_ALEATORIC(m, who)                                                                                           \
    ALQ_REQUIRE(!(m) || !(m)->aleatoric, ALQ_EUNSUPPORTED,                                                                      \
                "%s: the model's head has a log-variance channel (alq_model_set_aleatoric): alq_param_grads_loss_mt_au", who)
#define ALQ_REFUSE_DENSE(m, who)                                                                                                \
    ALQ_REQUIRE(!(m) || !(m)->dense, ALQ_EUNSUPPORTED, "%s: not defined for a fully-convolutional model (1x1 conv head)", who)
