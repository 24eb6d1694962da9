// The general gradient path behind the C ABI, what every query but the Fisher pass runs: the general backward sweep, its consumers over
// one parameter walk (gradients, their norms, diagonal Fisher, class layer sums), Hessian-vector products and the dense head.
#include "model_types.h"

using namespace alq;

// General backward-data pass for a cotangent already in m->dlogits ([N, c], w.r.t. the logits as the forward pass left
// them): every layer's masked pre-activation cotangent ends up in its `dout` view (what the weight gradients need), no
// shortcut of the Fisher pass is taken (no unit cotangent, no sign-byte input, every tensor stored).  The forward pass
// must have kept every activation (run_forward(..., keep_all = true)).
// None of the Fisher pass's fused backward launches (c3d / t3d / e3d / d3d) runs in a general sweep or in the fp64 sweep of
// alq_hess_vecp: engine info 2, 8, 9, 11, 13 and 17 speak of the LAST backward pass, not of the last Fisher pass before it.
static int run_backward_general(alq_model *m, int N, const DropSpec *drop, bool layer_sums = false) {
    alq_ctx *ctx = m->ctx;
    const int nl = (int)m->layers.size();
    m->last.lsum = layer_sums ? 1 : 0;
    m->last.bwd = {};
    for (int i = m->dense ? nl - 2 : nl - 1; i >= 0; --i) {      // (a dense model: the head's own kernel has written the cotangent of its input)
        Layer &ly = m->layers[i];
        const bool isfc = ly.spec.type == ALQ_FC;
        const bool prev_is_src = (i > 0 && m->layers[i - 1].out_is_skip_src && ly.spec.skip_src < 0);
        if (drop && drop->on(i))       // out = act * keep / keep_prob: the cotangent takes the same factor
            ALQ_TRY(k_dropout(ctx, isfc ? flat_view(ly.dout) : ly.dout, N, drop->first_sample, drop->seed, i, drop->keep_prob));
        if (ly.spec.type == ALQ_POOL) {
            if (i == 0) break;
            bool fused = false;
            ALQ_TRY(k_pool_bwd(ctx, ly.dout, ly.din, ly.argmax, ly.spec.k, ly.lo, N, prev_is_src ? 1 : 0, nullptr, nullptr, &fused, 1));
            continue;
        }
        View dv = isfc ? flat_view(ly.dout) : ly.dout;
        View av = isfc ? flat_view(ly.out) : ly.out;
        if (layer_sums)     // ReLU-grad mask in place + this slot's layer sum against the layer's field (lsum.hip)
            ALQ_TRY(k_lsum_sweep(ctx, dv, ly.spec.relu ? &av : nullptr, isfc, ly.ls_field, N,
                                 m->ls_part + (size_t)ly.pidx * m->max_batch * m->ls_nslab_max, m->ls_nslab_max));
        else
            ALQ_TRY(k_mask_chansum(ctx, dv, ly.spec.relu ? &av : nullptr, ly.dsum, N));      // ReLU-grad mask in place (+ sums, unused)
        if (ly.pidx == 0) break;      // the first parameterised layer: nothing below needs a cotangent
        const int acc = prev_is_src ? 1 : 0;
        if (isfc) {
            ALQ_REQUIRE(!acc, ALQ_EUNSUPPORTED, "layer %d: fc consumer of a skip source", i);
            if (ly.dense_fc_small) {
                bool fused = false;
                ALQ_TRY(k_fc_small_bwd(ctx, ly.dout.p, ly.spec.cout, ly.d_Wp, ly.F, N, ly.din.p, nullptr, nullptr, 0, &fused));
            } else {
                // no bound (0): this cotangent is arbitrary (loss scale, dropout factors) - the bf16-triple path
                ALQ_TRY(gemm_launch(ctx, ly.bwd, ly.dout, flat_view(ly.din), nullptr, 0, 0, N, PROF_IGEMM_BWD, nullptr, nullptr, 0.f));
            }
        } else {
            ALQ_TRY(gemm_launch(ctx, ly.bwd, ly.dout, ly.din, nullptr, 0, acc, N, PROF_IGEMM_BWD));
        }
    }
    return ALQ_OK;
}

// ---- the parameter walk: one parameterised layer as the consumers of a general backward pass take it.  The flat parameter vector is [W_0, b_0, W_1, b_1, ...]
// in the reference's variable order and TF layouts (conv [k.., ci, co], conv_transpose [k.., co, ci], fc [out, in] with `in` in
// flatten order, NN.py:272-318).
struct ParamLayer {
    const Layer &ly;
    int index;           // of the layer in alq_model::layers
    View in;             // its input (split-concat inputs included); the caller's d_x for layer 0
    View U, V;           // the operands in the order the weight kernels take them: conv (dout, in), conv_transpose (in, dout)
    const int *s;        // ... and their stride: conv {1, 1, 1}, conv_transpose spec.s
    long long off;       // of [W, b] in the flat vector
    bool fc() const { return ly.spec.type == ALQ_FC; }      // an fc layer has kernels of its own: (dout.p, in)
    long long end() const { return off + ly.w_elems + ly.b_elems; }
};

static std::vector<ParamLayer> param_layers(const alq_model *m, const float *d_x = nullptr) {
    static const int one[3] = {1, 1, 1};
    std::vector<ParamLayer> pls;
    for (size_t i = 0; i < m->layers.size(); ++i) {
        const Layer &ly = m->layers[i];
        if (ly.pidx < 0) continue;
        View in = ly.in;
        if (i == 0 && d_x) in.p = const_cast<float *>(d_x);
        const bool convt = ly.spec.type == ALQ_CONVT;
        pls.push_back({ly, (int)i, in, convt ? in : ly.dout, convt ? ly.dout : in, convt ? ly.spec.s : one, pls.empty() ? 0 : pls.back().end()});
    }
    return pls;
}

static long long param_count(const std::vector<ParamLayer> &pls) { return pls.empty() ? 0 : pls.back().end(); }

template <typename T>      // a scratch buffer that is sized by the call's N: allocated anew when a call needs more than it holds
static int grow(alq_model *m, T **d, size_t *len, long long need) {
    if ((size_t)need <= *len) return ALQ_OK;
    ALQ_TRY(m->dalloc(d, (size_t)need));
    *len = (size_t)need;
    return ALQ_OK;
}

// Weight + bias gradients of every parameterised layer from the tensors a general backward pass left behind, written as
// one flat vector per sample (or one for the batch).
static int run_param_grads(alq_model *m, const float *d_x, int N, int sum_n, float *d_out, long long P) {
    alq_ctx *ctx = m->ctx;
    const std::vector<ParamLayer> pls = param_layers(m, d_x);
    long long need = 0;
    for (const ParamLayer &p : pls)
        if (!p.fc() && !p.ly.dense_head) need = std::max(need, wgrad_partial_floats(p.U, p.V, p.ly.spec.k) * N);
    ALQ_TRY(grow(m, &m->wg_partial, &m->wg_partial_len, need));
    const long long stride = sum_n ? 0 : P;
    for (const ParamLayer &p : pls) {
        const Layer &ly = p.ly;
        if (ly.dense_head) continue;      // written by the head's backward launch (dense_backward_head)
        float *gw = d_out + p.off, *gb = gw + ly.w_elems;
        if (p.fc()) {
            ALQ_TRY(k_fc_wgrad(ctx, ly.dout.p, p.in, ly.spec.cout, N, sum_n, gw, stride));
            ALQ_TRY(k_bgrad(ctx, flat_view(ly.dout), N, sum_n, gb, stride));
        } else {
            ALQ_TRY(k_wgrad(ctx, p.U, p.V, ly.spec.k, p.s, ly.lo, N, sum_n, m->wg_partial, gw, stride));
            ALQ_TRY(k_bgrad(ctx, ly.dout, N, sum_n, gb, stride));
        }
    }
    ALQ_REQUIRE(param_count(pls) == P, ALQ_EINVAL, "parameter count mismatch");
    return ALQ_OK;
}

// Per-sample squared norms of every parameterised layer's weight and bias gradient from the same tensors: d_sq [N, 2L],
// [n][2t] = ||dW_t||^2, [n][2t + 1] = ||db_t||^2.  Nothing of the size of the parameters is written (gnorm.hip).
static int run_grad_sqnorms(alq_model *m, const float *d_x, int N, double *d_sq) {
    alq_ctx *ctx = m->ctx;
    const std::vector<ParamLayer> pls = param_layers(m, d_x);
    long long need = 0;
    for (const ParamLayer &p : pls)
        if (!p.fc()) need = std::max(need, gnorm_partials(p.U, p.V, p.ly.spec.k, p.s, p.ly.lo) * N);
    ALQ_TRY(grow(m, &m->gn_partial, &m->gn_partial_len, need));
    const int ld = 2 * m->L;
    for (const ParamLayer &p : pls) {
        const Layer &ly = p.ly;
        const int col = 2 * ly.pidx;
        if (p.fc()) {
            ALQ_TRY(k_gnorm_fc(ctx, ly.dout.p, ly.spec.cout, p.in, N, d_sq, ld, col));
        } else {
            ALQ_TRY(k_gnorm_weight(ctx, p.U, p.V, ly.spec.k, p.s, ly.lo, N, m->gn_partial, d_sq, ld, col));
            ALQ_TRY(k_gnorm_bias(ctx, ly.dout, N, d_sq, ld, col + 1));
        }
    }
    return ALQ_OK;
}

// Squared per-sample gradients summed over the samples, from the same tensors: d_acc [P] += in the flat order.  Nothing of the
// size N x P is written (dfisher.hip).  The scratch is sized once, for max_batch: sample-group partials of a conv layer's weights,
// per-sample channel sums, squared fc cotangents - whichever is largest.
static int run_diag_fisher(alq_model *m, const float *d_x, int N, double *d_acc) {
    alq_ctx *ctx = m->ctx;
    const std::vector<ParamLayer> pls = param_layers(m, d_x);
    if (!m->df_scratch) {
        long long need = 1;
        for (const ParamLayer &p : pls) {
            need = std::max(need, (long long)m->max_batch * p.ly.spec.cout);
            if (!p.fc()) need = std::max(need, dfisher_weight_scratch(p.U, p.V, p.ly.spec.k, p.s, p.ly.lo, m->max_batch));
        }
        ALQ_TRY(m->dalloc(&m->df_scratch, (size_t)need));
    }
    for (const ParamLayer &p : pls) {
        const Layer &ly = p.ly;
        double *aw = d_acc + p.off, *ab = aw + ly.w_elems;
        if (p.fc()) {
            ALQ_TRY(k_dfisher_fc(ctx, ly.dout.p, ly.spec.cout, p.in, N, m->df_scratch, aw, ab));
        } else {
            ALQ_TRY(k_dfisher_weight(ctx, p.U, p.V, ly.spec.k, p.s, ly.lo, N, m->df_scratch, aw));
            ALQ_TRY(k_dfisher_bias(ctx, ly.dout, N, m->df_scratch, ab));
        }
    }
    ALQ_REQUIRE(param_count(pls) == alq_model_num_params(m), ALQ_EINVAL, "parameter count mismatch");
    return ALQ_OK;
}

// ------------------------------------------------------------------------------------------ Hessian-vector product (hvp.hip)
// First call: the tangent tensors of every layer, the slab partials of the weight products and the TF-layout fp32 weights;
// later calls: only the weights of layers that were set since.
static int hvp_prepare(alq_model *m) {
    alq_ctx *ctx = m->ctx;
    const size_t NB = (size_t)m->max_batch;
    if (!m->hv_ready) {
        long long Mmax = 1;
        for (Layer &ly : m->layers) {
            ALQ_REQUIRE(ly.spec.type != ALQ_POOL || (ly.spec.skip_src < 0 && &ly != &m->layers[0]), ALQ_EUNSUPPORTED,
                        "alq_hess_vecp: pool layer first or behind a concat");
            const size_t el = NB * (size_t)ly.out.vox() * ly.out.C;
            ALQ_TRY(m->dalloc(&ly.hv_A, el));
            ALQ_TRY(m->dalloc(&ly.hv_D, el));
            ALQ_TRY(m->dalloc(&ly.hv_Ra, el));
            ALQ_TRY(m->dalloc(&ly.hv_Rd, el));
            if (ly.pidx >= 0) {
                ALQ_TRY(m->dalloc(&ly.hv_W, (size_t)ly.w_elems));
                if (ly.spec.type != ALQ_FC) Mmax = std::max<long long>(Mmax, ly.w_elems);
            }
        }
        ALQ_TRY(m->dalloc(&m->hv_part, (size_t)hvp_wgrad_partial_doubles(Mmax)));
        ALQ_TRY(m->dalloc(&m->hv_p64, NB * (size_t)m->nclass));
        m->hv_ready = true;
    }
    for (Layer &ly : m->layers) {
        if (ly.pidx < 0) continue;
        ALQ_REQUIRE(ly.weights_set && ly.hv_src != 0, ALQ_EINVAL, "alq_hess_vecp: weights of parameterised layer %d not set", ly.pidx);
        if (!ly.hv_stale) continue;
        if (ly.hv_src == 1) {
            ALQ_TRY(upload_release(m, &ly.hv_W, &ly.hv_hW));      // hv_W holds them until the next set_weights
        } else {
            const float *res = ly.hv_src == 2 ? ly.d_Wres : ly.d_Wp;      // both [o][f_mem]
            ALQ_REQUIRE(res != nullptr, ALQ_EINVAL, "alq_hess_vecp: layer %d has no resident weights", ly.pidx);
            ALQ_TRY(k_hvp_unpermute(ctx, res, ly.hv_W, ly.spec.cout, ly.in));
        }
        ly.hv_stale = false;
    }
    return ALQ_OK;
}

// Everything behind the forward pass (which fixed the ReLU and pool decisions: Layer::out's signs, the arg-max fields), in fp64 on
// the call's own tensors: activations, posteriors and first-order cotangents, the tangent pass, the second-order term at the
// logits, the sweep of the tangent cotangent and the products (hvp.hip).
static int run_hess_vecp(alq_model *m, const float *d_x, int N, const int32_t *d_labels, float loss_scale, const float *d_v,
                         const uint8_t *h_layer_on, int accumulate, double *d_hv, double *d_loss) {
    alq_ctx *ctx = m->ctx;
    const int nl = (int)m->layers.size();
    const int one[3] = {1, 1, 1};
    std::vector<long long> off(nl, 0);      // of a parameterised layer's [W, b] in d_v and d_hv
    for (const ParamLayer &p : param_layers(m)) off[p.index] = p.off;
    auto on = [&](const Layer &ly) { return !h_layer_on || h_layer_on[ly.pidx] != 0; };
    // the input of layer i out of the per-layer tensors `which`: the network input itself (fp32) for the first layer's
    // activations and none for its tangent, two producers behind a 'con' skip
    auto src_in = [&](int i, double *Layer::*which, bool tangent) {
        const Layer &ly = m->layers[i];
        if (i == 0) {
            if (tangent) return HSrc();
            View in = ly.in;
            in.p = const_cast<float *>(d_x);
            return hsrc_view(in);
        }
        if (ly.spec.skip_src >= 0) {
            const Layer &sl = m->layers[ly.spec.skip_src], &pl = m->layers[i - 1];
            return hsrc_dense(sl.*which, sl.out.C, pl.*which, pl.out.C);
        }
        return hsrc_dense(m->layers[i - 1].*which, ly.in.C);
    };
    // one forward walk: tangent = false: activations (bias, no v); true: tangents (the v term of switched-on layers)
    auto forward = [&](bool tangent) -> int {
        double *Layer::*out = tangent ? &Layer::hv_Ra : &Layer::hv_A;
        for (int i = 0; i < nl; ++i) {
            Layer &ly = m->layers[i];
            if (ly.spec.type == ALQ_POOL) {
                ALQ_TRY(k_hvp_pool_fwd(ctx, m->layers[i - 1].*out, ly.argmax, ly.*out, ly.in, ly.out, ly.spec.k, ly.lo, N));
                continue;
            }
            const bool lon = tangent && on(ly);
            const float *V = lon ? d_v + off[i] : nullptr;
            const float *cb = tangent ? (lon ? d_v + off[i] + ly.w_elems : nullptr) : ly.d_bias;
            const HSrc a = lon ? src_in(i, &Layer::hv_A, false) : HSrc(), x = src_in(i, out, tangent);
            if (ly.spec.type == ALQ_FC) {
                ALQ_TRY(k_hvp_fc_fwd(ctx, a, V, x, ly.hv_W, cb, ly.spec.relu ? hsrc_view(ly.out) : HSrc(), ly.*out, ly.in, ly.spec.cout, N));
            } else {
                HGeo g;
                ALQ_TRY(hvp_geometry(ly.spec.type, 0, ly.in, ly.out, ly.spec.k, ly.spec.s, ly.lo, &g));
                HDst dst;
                dst.pa = ly.*out; dst.Ca = ly.out.C;
                ALQ_TRY(k_hvp_contract(ctx, a, V, x, ly.hv_W, cb, ly.spec.relu ? hsrc_view(ly.out) : HSrc(), dst, g, N));
            }
        }
        return ALQ_OK;
    };
    // one backward walk over the tensors `X` (the layers' output cotangents; the head's is filled): second = false: the
    // first-order cotangents hv_D; true: their tangents hv_Rd (+ the delta . V term of switched-on layers) and the products
    auto backward = [&](bool second) -> int {
        double *Layer::*X = second ? &Layer::hv_Rd : &Layer::hv_D;
        std::vector<char> written(nl, 0);
        written[nl - 1] = 1;
        for (int i = nl - 1; i >= 0; --i) {
            Layer &ly = m->layers[i];
            ALQ_REQUIRE(written[i], ALQ_EUNSUPPORTED, "alq_hess_vecp: layer %d has no consumer", i);
            if (ly.spec.type == ALQ_POOL) {
                ALQ_TRY(k_hvp_pool_bwd(ctx, ly.*X, ly.argmax, m->layers[i - 1].*X, written[i - 1], ly.in, ly.out, ly.spec.k, ly.lo, N));
                written[i - 1] = 1;
                continue;
            }
            const bool isfc = ly.spec.type == ALQ_FC;
            const long long orows = (long long)N * ly.out.vox();
            if (ly.spec.relu) ALQ_TRY(k_hvp_mask(ctx, ly.*X, ly.out.C, hsrc_view(ly.out), orows));
            const bool lon = second && on(ly);
            if (second) {
                double *hv = d_hv + off[i];
                if (lon) {
                    const HSrc a = src_in(i, &Layer::hv_A, false), Ra = src_in(i, &Layer::hv_Ra, true);
                    const HSrc Rd = hsrc_dense(ly.hv_Rd, ly.out.C), dl = i > 0 ? hsrc_dense(ly.hv_D, ly.out.C) : HSrc();
                    if (isfc) {
                        ALQ_TRY(k_hvp_fc_wgrad(ctx, ly.hv_Rd, a, ly.hv_D, Ra, ly.in, ly.spec.cout, N, accumulate, hv));
                    } else if (ly.spec.type == ALQ_CONV) {
                        ALQ_TRY(k_hvp_wgrad(ctx, Rd, a, dl, Ra, ly.out.C, ly.in.C, ly.out, ly.in, ly.spec.k, one, ly.lo, N, m->hv_part, accumulate,
                                            hv));
                    } else {
                        ALQ_TRY(k_hvp_wgrad(ctx, a, Rd, Ra, dl, ly.in.C, ly.out.C, ly.in, ly.out, ly.spec.k, ly.spec.s, ly.lo, N, m->hv_part,
                                            accumulate, hv));
                    }
                    ALQ_TRY(k_hvp_bias(ctx, ly.hv_Rd, ly.out.C, orows, accumulate, hv + ly.w_elems));
                } else if (!accumulate) {
                    ALQ_HIP(hipMemsetAsync(hv, 0, (size_t)(ly.w_elems + ly.b_elems) * sizeof(double), ctx->stream));
                }
            }
            if (i == 0) break;
            HDst dst;      // the input's cotangent, routed to the producer(s) of the input
            if (ly.spec.skip_src >= 0) {
                const int s = ly.spec.skip_src;
                dst.pa = m->layers[s].*X; dst.Ca = m->layers[s].out.C; dst.acca = written[s];
                dst.pb = m->layers[i - 1].*X; dst.Cb = m->layers[i - 1].out.C; dst.accb = written[i - 1];
                written[s] = 1;
            } else {
                dst.pa = m->layers[i - 1].*X; dst.Ca = ly.in.C; dst.acca = written[i - 1];
            }
            written[i - 1] = 1;
            const float *V = lon ? d_v + off[i] : nullptr;
            if (isfc) {
                ALQ_TRY(k_hvp_fc_bwd(ctx, ly.hv_D, V, ly.*X, ly.hv_W, dst, ly.in, ly.spec.cout, N));
            } else {
                HGeo g;
                ALQ_TRY(hvp_geometry(ly.spec.type, 1, ly.in, ly.out, ly.spec.k, ly.spec.s, ly.lo, &g));
                ALQ_TRY(k_hvp_contract(ctx, lon ? hsrc_dense(ly.hv_D, ly.out.C) : HSrc(), V, hsrc_dense(ly.*X, ly.out.C), ly.hv_W, nullptr, HSrc(),
                                       dst, g, N));
            }
        }
        return ALQ_OK;
    };
    Layer &head = m->layers[nl - 1];
    ALQ_REQUIRE(!head.spec.relu, ALQ_EUNSUPPORTED, "alq_hess_vecp: ReLU on the head");
    ALQ_TRY(forward(false));
    ALQ_TRY(k_hvp_softmax64(ctx, head.hv_A, d_labels, m->nclass, N, loss_scale, m->post, m->hv_p64, head.hv_D));
    if (d_loss) ALQ_TRY(k_hvp_loss(ctx, m->post, m->nclass, N, d_labels, loss_scale, d_loss));
    ALQ_TRY(backward(false));
    ALQ_TRY(forward(true));
    ALQ_TRY(k_hvp_softmax2(ctx, m->hv_p64, head.hv_Ra, d_labels, m->nclass, N, loss_scale, head.hv_Rd));
    return backward(true);
}

// posteriors [c, N V] (and predictions, and the logits into the head's output buffer) from the head's input, after run_forward
int dense_forward_head(alq_model *m, const float *d_x, int N, float *d_post, int64_t *d_pred, bool want_logits, float *d_au,
                       float *d_logits) {
    Layer &h = m->layers.back();
    const float *x = m->layers.size() == 1 ? d_x : h.in.p;
    float *z = d_logits ? d_logits : (want_logits ? h.out.p : nullptr);
    if (m->aleatoric)
        return k_dense_head_fwd_au(m->ctx, x, (long long)N * m->V, h.in.C, m->nclass - 1, h.d_W32, h.d_bias, d_post ? d_post : m->post, d_pred,
                                   d_au, z);
    return k_dense_head_fwd(m->ctx, x, (long long)N * m->V, h.in.C, m->nclass, h.d_W32, h.d_bias, d_post ? d_post : m->post, d_pred, z);
}

// the head's cotangent rows (m->dlogits) -> the cotangent of its input and its own slice [dW, db] of the flat gradient
static int dense_backward_head(alq_model *m, const float *d_x, int N, float *d_grads, long long P) {
    Layer &h = m->layers.back();
    const float *x = m->layers.size() == 1 ? d_x : h.in.p;
    return k_dense_head_bwd(m->ctx, m->dlogits, x, (long long)N * m->V, h.in.C, m->nclass, h.d_W32, h.pidx == 0 ? nullptr : h.din.p, 0,
                            m->dh_part, d_grads + (P - h.w_elems - h.b_elems));
}

// ------------------------------------------------------------------------------------------ what the entry points share
#define REQUIRE_BATCH(m, N, who) \
    ALQ_REQUIRE((N) >= 1 && (N) <= (m)->max_batch, ALQ_EINVAL, "%s: N=%d outside [1, max_batch=%d]", who, N, (m)->max_batch)

// Classes that live on the device: one flag read (a stream synchronisation) before anything is written
static int check_classes(alq_model *m, const int32_t *d_cls, int count, const char *who) {
    alq_ctx *ctx = m->ctx;
    int bad = 0;
    ALQ_TRY(flag_clear(ctx));
    ALQ_TRY(k_lsum_check_classes(ctx, d_cls, count, m->nclass, flag_of(ctx)));
    ALQ_TRY(flag_read(ctx, &bad));
    ALQ_REQUIRE(!bad, ALQ_EINVAL, "%s: a class outside [0, %d)", who, m->nclass);
    return ALQ_OK;
}

// The forward half of every general pass, behind the entry point's argument checks and its hipSetDevice: the call's dropout masks
// into *ds (run_backward_general takes them too; the default: none), the forward pass with every activation kept, and the
// posteriors into `post` (null: none - the caller has a softmax of its own).
static int general_forward(alq_model *m, const float *d_x, int N, float *post, DropSpec *ds, float keep_prob = 1.f, uint64_t seed = 0,
                           int64_t first_sample = 0, const int32_t *h_drop_layers = nullptr, int n_drop_layers = 0) {
    ALQ_TRY(make_drop(m, keep_prob, seed, first_sample, h_drop_layers, n_drop_layers, ds));
    ALQ_TRY(prepare_call(m, /*fisher=*/false));
    ALQ_TRY(run_forward(m, d_x, N, false, /*keep_all=*/true, ds));
    if (post) ALQ_TRY(k_softmax(m->ctx, m->logits, m->nclass, N, post, nullptr));
    return ALQ_OK;
}

// =========================================================================================== C ABI
extern "C" {

int64_t alq_model_num_params(const alq_model *m) { return m ? param_count(param_layers(m)) : ALQ_EINVAL; }

int alq_param_grads(alq_model *m, const float *d_x, int N, int mode, int cls, const int32_t *d_labels, float loss_scale,
                    float keep_prob, uint64_t seed, int64_t first_sample, const int32_t *h_drop_layers, int n_drop_layers,
                    int per_sample, float *d_grads, float *d_post, double *d_loss) {
    ALQ_REFUSE_DENSE(m, "alq_param_grads");
    ALQ_REQUIRE(m && d_x && d_grads, ALQ_EINVAL, "alq_param_grads: null argument");
    REQUIRE_BATCH(m, N, "alq_param_grads");
    ALQ_REQUIRE(mode == 0 || (mode == 1 && d_labels), ALQ_EINVAL, "alq_param_grads: mode %d / labels", mode);
    ALQ_REQUIRE(mode != 0 || (cls >= 0 && cls < m->nclass), ALQ_EINVAL, "alq_param_grads: class %d", cls);
    ALQ_HIP(hipSetDevice(m->ctx->device));
    DropSpec ds;
    float *post = d_post ? d_post : m->post;
    ALQ_TRY(general_forward(m, d_x, N, post, &ds, keep_prob, seed, first_sample, h_drop_layers, n_drop_layers));
    if (d_loss && mode == 1) ALQ_TRY(k_ce_loss(m->ctx, post, m->nclass, N, d_labels, d_loss));
    ALQ_TRY(k_logit_cotangent(m->ctx, post, m->nclass, N, mode, cls, d_labels, loss_scale, m->dlogits));
    ALQ_TRY(run_backward_general(m, N, &ds));
    return run_param_grads(m, d_x, N, per_sample ? 0 : 1, d_grads, alq_model_num_params(m));
}

int alq_grad_sqnorms(alq_model *m, const float *d_x, int N, int cls, const int32_t *d_cls, float *d_post, double *d_sq) {
    ALQ_REFUSE_DENSE(m, "alq_grad_sqnorms");
    ALQ_REQUIRE(m && d_x && d_sq, ALQ_EINVAL, "alq_grad_sqnorms: null argument");
    REQUIRE_BATCH(m, N, "alq_grad_sqnorms");
    ALQ_REQUIRE(d_cls || (cls == -1 && m->nclass == 2) || (cls >= 0 && cls < m->nclass), ALQ_EINVAL,
                "alq_grad_sqnorms: class %d (-1 needs a two-class net, found %d classes)", cls, m->nclass);
    ALQ_HIP(hipSetDevice(m->ctx->device));
    DropSpec ds;
    float *post = d_post ? d_post : m->post;
    ALQ_TRY(general_forward(m, d_x, N, post, &ds));
    const int mode = d_cls ? 3 : (cls < 0 ? 2 : 0);
    ALQ_TRY(k_logit_cotangent(m->ctx, post, m->nclass, N, mode, cls, d_cls, 1.f, m->dlogits));
    ALQ_TRY(run_backward_general(m, N, &ds));
    return run_grad_sqnorms(m, d_x, N, d_sq);
}

int alq_class_layer_sums(alq_model *m, const float *d_x, int N, int J, const int32_t *d_cls, float *d_post, double *d_g) {
    ALQ_REFUSE_DENSE(m, "alq_class_layer_sums");
    ALQ_REQUIRE(m && d_x && d_cls && d_g, ALQ_EINVAL, "alq_class_layer_sums: null argument");
    REQUIRE_BATCH(m, N, "alq_class_layer_sums");
    ALQ_REQUIRE(J >= 1 && J <= 64, ALQ_EINVAL, "alq_class_layer_sums: %d class slots outside [1, 64]", J);
    ALQ_REQUIRE(m->nclass >= 2 && m->nclass <= 64 && m->L <= 64, ALQ_EUNSUPPORTED, "alq_class_layer_sums: %d classes, %d layers",
                m->nclass, m->L);
    alq_ctx *ctx = m->ctx;
    ALQ_HIP(hipSetDevice(ctx->device));
    ALQ_TRY(check_classes(m, d_cls, J * N, "alq_class_layer_sums"));
    if (!m->ls_part) {
        m->ls_nslab.assign(m->L, 1);
        m->ls_nslab_max = 1;
        for (Layer &ly : m->layers) {
            if (ly.pidx < 0) continue;
            const bool isfc = ly.spec.type == ALQ_FC;
            m->ls_nslab[ly.pidx] = lsum_slabs(ly.dout, isfc, nullptr);
            m->ls_nslab_max = std::max(m->ls_nslab_max, m->ls_nslab[ly.pidx]);
            ALQ_TRY(m->dalloc(&ly.ls_field, (size_t)m->max_batch * (isfc ? 1 : (size_t)ly.out.vox())));
        }
        ALQ_TRY(m->dalloc(&m->ls_part, (size_t)m->L * m->max_batch * m->ls_nslab_max));
    }
    DropSpec ds;
    float *post = d_post ? d_post : m->post;
    ALQ_TRY(general_forward(m, d_x, N, post, &ds));
    for (const ParamLayer &p : param_layers(m, d_x))      // the fields: once per call, whatever J
        ALQ_TRY(k_lsum_field(ctx, p.in, p.ly.out, p.ly.spec.k, p.ly.spec.s, p.ly.lo, p.ly.spec.type, N, p.ly.ls_field));
    for (int j = 0; j < J; ++j) {
        ALQ_TRY(k_logit_cotangent(ctx, post, m->nclass, N, 3, 0, d_cls + (size_t)j * N, 1.f, m->dlogits));
        ALQ_TRY(run_backward_general(m, N, &ds, /*layer_sums=*/true));
        ALQ_TRY(k_lsum_finish(ctx, m->ls_part, m->ls_nslab.data(), m->ls_nslab_max, m->max_batch, m->sizes, N, m->L, J, j, d_g));
    }
    return ALQ_OK;
}

int alq_diag_fisher(alq_model *m, const float *d_x, int N, const int32_t *d_cls, double *d_acc) {
    ALQ_REFUSE_DENSE(m, "alq_diag_fisher");
    ALQ_REQUIRE(m && d_x && d_cls && d_acc, ALQ_EINVAL, "alq_diag_fisher: null argument");
    REQUIRE_BATCH(m, N, "alq_diag_fisher");
    ALQ_HIP(hipSetDevice(m->ctx->device));
    ALQ_TRY(check_classes(m, d_cls, N, "alq_diag_fisher"));
    DropSpec ds;
    ALQ_TRY(general_forward(m, d_x, N, m->post, &ds));
    ALQ_TRY(k_logit_cotangent(m->ctx, m->post, m->nclass, N, 3, 0, d_cls, 1.f, m->dlogits));
    ALQ_TRY(run_backward_general(m, N, &ds));
    return run_diag_fisher(m, d_x, N, d_acc);
}

int alq_hess_vecp(alq_model *m, const float *d_x, int N, const int32_t *d_labels, float loss_scale, const float *d_v,
                  const uint8_t *h_layer_on, int accumulate, double *d_hv, double *d_loss) {
    ALQ_REFUSE_DENSE(m, "alq_hess_vecp");
    ALQ_REQUIRE(m && d_x && d_labels && d_v && d_hv, ALQ_EINVAL, "alq_hess_vecp: null argument");
    REQUIRE_BATCH(m, N, "alq_hess_vecp");
    ALQ_HIP(hipSetDevice(m->ctx->device));
    ALQ_TRY(hvp_prepare(m));
    DropSpec ds;
    ALQ_TRY(general_forward(m, d_x, N, nullptr, &ds));      // (the fp64 sweep computes its own posteriors)
    m->last.bwd = {};      // the fp64 sweep runs none of the Fisher pass's fused backward launches
    return run_hess_vecp(m, d_x, N, d_labels, loss_scale, d_v, h_layer_on, accumulate, d_hv, d_loss);
}

int alq_param_grads_loss(alq_model *m, const float *d_x, int N, const int32_t *d_labels, const alq_loss_t *loss, float loss_scale,
                         float lwf_scale, float keep_prob, uint64_t seed, int64_t first_sample, const int32_t *h_drop_layers,
                         int n_drop_layers, float *d_grads, float *d_post, double *d_stats3) {
    ALQ_REQUIRE(m && d_grads, ALQ_EINVAL, "alq_param_grads_loss: null argument");
    ALQ_REFUSE_ALEATORIC(m, "alq_param_grads_loss");
    REQUIRE_BATCH(m, N, "alq_param_grads_loss");
    ALQ_TRY(loss_check("alq_param_grads_loss", d_x, m->nclass, d_labels, loss));
    ALQ_HIP(hipSetDevice(m->ctx->device));
    DropSpec ds;
    float *post = d_post ? d_post : m->post;
    // (a dense model: the head's own launch writes the posteriors)
    ALQ_TRY(general_forward(m, d_x, N, m->dense ? nullptr : post, &ds, keep_prob, seed, first_sample, h_drop_layers, n_drop_layers));
    const long long P = alq_model_num_params(m);
    if (m->dense) {      // every voxel is a sample: the same cotangent kernel over N V columns, then the head's own backward launch
        ALQ_TRY(dense_forward_head(m, d_x, N, post, nullptr, false));
        ALQ_TRY(k_loss_cotangent(m->ctx, post, m->nclass, (int)(N * m->V), d_labels, loss, loss_scale, lwf_scale, m->dlogits, d_stats3));
        ALQ_TRY(dense_backward_head(m, d_x, N, d_grads, P));
    } else {
        ALQ_TRY(k_loss_cotangent(m->ctx, post, m->nclass, N, d_labels, loss, loss_scale, lwf_scale, m->dlogits, d_stats3));
    }
    // (a dense head that is the only parameterised layer: nothing below it)
    if (!m->dense || m->layers.back().pidx > 0) ALQ_TRY(run_backward_general(m, N, &ds));
    return run_param_grads(m, d_x, N, 1, d_grads, P);
}

// alq_param_grads_loss of a dense model with the mean-teacher cotangent (mteach.hip) in place of k_loss_cotangent
int alq_param_grads_loss_mt(alq_model *m, const float *d_x, int N, const int32_t *d_labels, const alq_loss_t *loss, float loss_scale,
                            const float *d_teacher_post, int measure, float cons_scale, float keep_prob, uint64_t seed,
                            int64_t first_sample, const int32_t *h_drop_layers, int n_drop_layers, float *d_grads, float *d_post,
                            double *d_stats3) {
    ALQ_REQUIRE(m && d_grads, ALQ_EINVAL, "alq_param_grads_loss_mt: null argument");
    ALQ_REFUSE_ALEATORIC(m, "alq_param_grads_loss_mt");
    ALQ_REQUIRE(m->dense, ALQ_EUNSUPPORTED, "alq_param_grads_loss_mt: mean-teacher training is defined for a fully-convolutional model");
    REQUIRE_BATCH(m, N, "alq_param_grads_loss_mt");
    ALQ_TRY(mt_check("alq_param_grads_loss_mt", d_x, d_teacher_post, m->nclass, (long long)N * m->V, d_labels, loss, measure));
    ALQ_HIP(hipSetDevice(m->ctx->device));
    DropSpec ds;
    float *post = d_post ? d_post : m->post;
    ALQ_TRY(general_forward(m, d_x, N, nullptr, &ds, keep_prob, seed, first_sample, h_drop_layers, n_drop_layers));
    const long long P = alq_model_num_params(m);
    ALQ_TRY(dense_forward_head(m, d_x, N, post, nullptr, false));
    ALQ_TRY(k_mt_cotangent(m->ctx, post, d_teacher_post, m->nclass, (long long)N * m->V, d_labels, loss, loss_scale, cons_scale, measure,
                           m->dlogits, d_stats3));
    ALQ_TRY(dense_backward_head(m, d_x, N, d_grads, P));
    if (m->layers.back().pidx > 0) ALQ_TRY(run_backward_general(m, N, &ds));
    return run_param_grads(m, d_x, N, 1, d_grads, P);
}

// alq_param_grads_loss_mt of an aleatoric model: the head writes the log-variances beside the posteriors, the cotangent rows have
// nclass = c + 1 columns, and the head's backward launch takes them as they are
int alq_param_grads_loss_mt_au(alq_model *m, const float *d_x, int N, const int32_t *d_labels, const alq_loss_t *loss, float loss_scale,
                               const float *d_teacher_post, int measure, float cons_scale, float au_scale, float au_log_rel_coeff,
                               float keep_prob, uint64_t seed, int64_t first_sample, const int32_t *h_drop_layers, int n_drop_layers,
                               float *d_grads, float *d_post, double *d_stats3) {
    ALQ_REQUIRE(m && d_grads, ALQ_EINVAL, "alq_param_grads_loss_mt_au: null argument");
    ALQ_REQUIRE(m->aleatoric, ALQ_EUNSUPPORTED, "alq_param_grads_loss_mt_au: the model has no log-variance channel (alq_model_set_aleatoric)");
    REQUIRE_BATCH(m, N, "alq_param_grads_loss_mt_au");
    const int c = m->nclass - 1;
    ALQ_TRY(mt_check_au("alq_param_grads_loss_mt_au", d_x, d_teacher_post, m->au, c, (long long)N * m->V, d_labels, loss, measure));
    ALQ_HIP(hipSetDevice(m->ctx->device));
    DropSpec ds;
    float *post = d_post ? d_post : m->post;
    ALQ_TRY(general_forward(m, d_x, N, nullptr, &ds, keep_prob, seed, first_sample, h_drop_layers, n_drop_layers));
    const long long P = alq_model_num_params(m);
    ALQ_TRY(dense_forward_head(m, d_x, N, post, nullptr, false, m->au));
    ALQ_TRY(k_mt_cotangent_au(m->ctx, post, d_teacher_post, m->au, c, (long long)N * m->V, d_labels, loss, loss_scale, cons_scale, au_scale,
                              au_log_rel_coeff, measure, m->dlogits, d_stats3));
    ALQ_TRY(dense_backward_head(m, d_x, N, d_grads, P));
    if (m->layers.back().pidx > 0) ALQ_TRY(run_backward_general(m, N, &ds));
    return run_param_grads(m, d_x, N, 1, d_grads, P);
}

}  // extern "C"
