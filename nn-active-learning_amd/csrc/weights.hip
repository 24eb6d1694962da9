// Weight setting behind the C ABI: a layer's TF-layout weights into every packed form its engines read, the host scalars the launches
// take their scales and bounds from, and the device-packed path of the wide fc layers (wpack.hip).  Host arithmetic: weight_layout.h.
#include <cmath>
#include <cstring>

#include "model_types.h"
#include "weight_layout.h"

using namespace alq;

static int set4(alq_model *m, Igemm4Plan *p4, const std::vector<float> &Bmat) {
    igemm4_pack_weights(p4, Bmat);
    if (!p4->d_tdesc) {
        ALQ_TRY(upload(m, &p4->d_vdesc, p4->h_vdesc));
        ALQ_TRY(upload(m, &p4->d_tdesc, p4->h_tdesc));
        ALQ_TRY(upload(m, &p4->d_sdesc, p4->h_sdesc));
        ALQ_TRY(upload(m, &p4->d_pdesc, p4->h_pdesc));
        ALQ_TRY(upload(m, &p4->d_ttab, p4->h_ttab));
    }
    ALQ_TRY(upload(m, &p4->d_W, p4->h_W));
    if (!p4->h_W16.empty()) ALQ_TRY(upload(m, &p4->d_W16, p4->h_W16));
    ALQ_HIP(hipStreamSynchronize(m->ctx->stream));
    std::vector<unsigned short>().swap(p4->h_W);
    std::vector<unsigned short>().swap(p4->h_W16);
    if (p4->alt16) ALQ_TRY(set4(m, p4->alt16.get(), Bmat));       // the fp16x2-only twin: own tables, two-piece weights
    return ALQ_OK;
}

// parts: 1 = the streaming GEMM's forms of a wide fc layer (pfc), 2 = every other engine's
static int gemm_set(alq_model *m, Gemm *g, const std::vector<float> &Bmat, int parts = 3) {
    if ((parts & 2) && g->p4.ok) ALQ_TRY(set4(m, &g->p4, Bmat));
    if ((parts & 1) && g->pfc.ok) {
        fcgemm_pack_weights(&g->pfc, Bmat);
        ALQ_TRY(upload_release(m, &g->pfc.d_W, &g->pfc.h_W));
        if (g->pfc_f16 && c3d_subnormals_ok(m->ctx)) {      // the fp16-pair twin for launches with a static input bound (backward, Fisher pass)
            fcgemm_pack_weights_f16(&g->pfc, Bmat);
            ALQ_TRY(upload_release(m, &g->pfc.d_W16, &g->pfc.h_W16));
        }
    }
    if (!(parts & 2)) return ALQ_OK;
    if (g->pd.ok) {      // direct kernel reads the B matrix [K][Co] as it is
        ALQ_TRY(upload(m, &g->pd.d_W, Bmat));
        ALQ_HIP(hipStreamSynchronize(m->ctx->stream));
    }
    if (g->p2.ok) {
        igemm2_pack_weights(&g->p2, Bmat);
        if (!g->p2.d_tdesc) {
            ALQ_TRY(upload(m, &g->p2.d_tdesc, g->p2.h_tdesc));
            ALQ_TRY(upload(m, &g->p2.d_sdesc, g->p2.h_sdesc));
            g->p2.a.tdesc = g->p2.d_tdesc;
            g->p2.a.sdesc = g->p2.d_sdesc;
        }
        if (g->p3.ok) {
            igemm3_pack_weights(g->p2, &g->p3, Bmat);
            ALQ_TRY(upload_release(m, &g->p3.d_W, &g->p3.h_W));
            if (g->p3_f16 && !g->p4.ok) {      // (round 6) the fp16-pair twin for launches with a static input bound
                igemm3_pack_weights_f16(g->p2, &g->p3, Bmat);
                ALQ_TRY(upload_release(m, &g->p3.d_W16, &g->p3.h_W16));
            }
        }
        return upload_release(m, &g->p2.d_W, &g->p2.h_W);
    }
    igemm_pack_weights(&g->p1, Bmat);
    if (g->p1.smallc) ALQ_TRY(upload(m, &g->p1.d_koff, g->p1.h_koff));
    return upload_release(m, &g->p1.d_W, &g->p1.h_W);
}

// A wide fc layer whose weights were last set from the device holds stale forms for the engines behind the streaming GEMM;
// gemm_launch selects those only under the debug knobs 4 / 5: pack them now, from the resident fp32 copy, with the host's code.
int alq::refresh_fallback_forms(alq_model *m) {
    for (Layer &ly : m->layers) {
        if (!ly.fallback_stale) continue;
        const int64_t F = ly.F;
        const int Co = ly.spec.cout;
        std::vector<float> Wp((size_t)Co * F);
        ALQ_HIP(hipMemcpyAsync(Wp.data(), ly.d_Wres, Wp.size() * sizeof(float), hipMemcpyDeviceToHost, m->ctx->stream));
        ALQ_HIP(hipStreamSynchronize(m->ctx->stream));
        ALQ_TRY(gemm_set(m, &ly.fwd[0], transpose_taps(Wp.data(), Co, (int)F, 1), 2));      // B[f_mem][o]
        if (ly.has_bwd) ALQ_TRY(gemm_set(m, &ly.bwd, Wp, 2));      // (every path of gemm_set ends with a synchronisation)
        m->host_pack_elems += ly.w_elems;
        ly.fallback_stale = false;
    }
    return ALQ_OK;
}

// the layer with pidx == t, or null with the error text set (ALQ_EINVAL); the read-only entry points, whose model is const, only read it
static Layer *find_param_layer(const alq_model *m, int t) {
    const Layer *found = nullptr;
    for (const Layer &l : m->layers)
        if (l.pidx == t) found = &l;
    if (!found) set_error("no parameterised layer %d", t);
    return const_cast<Layer *>(found);
}

// Which kernels get their weights packed depends on whether the matrix cores keep fp16 subnormals: the answer is a property of
// the device, probed once per context.  A probe that could not RUN must not select engines (it used to read as "flushes
// subnormals" for this call only: the plans of one layer then differed from the others' for good): retry, then fail.
static int require_subnormal_probe(alq_ctx *ctx, const char *who) {
    for (int tries = 0; tries < 3 && ctx->f16_subnormal_mfma < 0; ++tries) (void)c3d_subnormals_ok(ctx);
    ALQ_REQUIRE(ctx->f16_subnormal_mfma >= 0, ALQ_EHIP, "%s: the fp16-subnormal probe of the matrix cores could not run (device error)", who);
    return ALQ_OK;
}

static int set_conv(alq_model *m, Layer &ly, const float *W, const float *b) {
    alq_ctx *ctx = m->ctx;
    const int Ci = ly.in.C, Co = ly.spec.cout;
    const int ntaps = ly.spec.k[0] * ly.spec.k[1] * ly.spec.k[2];
    conv_norms(W, b, ntaps, Ci, Co, false, &ly.bwd_l1, &ly.out_l1, &ly.out_bmax);
    ly.bwd_l1_part[0] = ly.bwd_l1_part[1] = 0;
    ly.f16_slices_apart = false;
    if (ly.spec.skip_src >= 0 && m->layers[ly.spec.skip_src].out.C < Ci) {
        float slice_amax[2];
        conv_bwd_l1_slices(W, ntaps, Ci, Co, false, m->layers[ly.spec.skip_src].out.C, ly.bwd_l1_part, slice_amax);
        ly.f16_slices_apart = !slices_within_f16_range(slice_amax);
    }
    ly.fwd_l1 = ly.out_l1;
    const int li = (int)(&ly - &m->layers[0]);
    if (li + 2 == (int)m->layers.size() && m->layers[li + 1].fc_part2) {      // the conv under a fused two-class head
        ALQ_TRY(ensure<float>(m, &ly.d_W32, (size_t)ly.w_elems));
        ALQ_HIP(hipMemcpyAsync(ly.d_W32, W, ly.w_elems * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    std::vector<float> B(W, W + ly.w_elems);      // TF [tap][ci][co] is already the fwd B matrix [(tap, ci)][co]
    ALQ_TRY(gemm_set(m, &ly.fwd[0], B));
    for (size_t j = 0; j < ly.fwd_co.size(); ++j)      // the output-channel slices of a wide conv: columns [j w, (j + 1) w) of B
        ALQ_TRY(gemm_set(m, &ly.fwd_co[j], column_slice(B, ntaps * Ci, Co, (int)j, ly.fwd_co_w)));
    if (ly.c3f.ok) {
        // one accumulator (pieces at their true scale) only where the matrix cores honour fp16 subnormals
        if (ly.c3f.oneacc && !c3d_subnormals_ok(ctx)) ly.c3f.oneacc = 0;
        c3d_fwd_pack(&ly.c3f, B);
        ALQ_TRY(upload(m, &ly.c3f.d_W, ly.c3f.h_W));
        ALQ_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (ly.c3b.ok && ly.has_bwd && c3d_subnormals_ok(ctx)) {      // (the backward kernel exists in the one-accumulator form only)
        c3d_bwd_pack(&ly.c3b, B);
        ALQ_TRY(upload(m, &ly.c3b.d_W, ly.c3b.h_W));
        c3d_bwd7_pack(&ly.c3b, B);          // the 7-k-step form of the same weights (c3d_bwd7_kernel)
        ALQ_TRY(upload(m, &ly.c3b.d_W7, ly.c3b.h_W7));
        ALQ_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (ly.e3b.ok && ly.has_bwd && c3d_subnormals_ok(ctx)) {      // (fp16 pairs at their true scale: the one-accumulator form)
        e3d_pack(&ly.e3b, W);
        ALQ_TRY(upload(m, &ly.e3b.d_Whi, ly.e3b.h_Whi));
        ALQ_TRY(upload(m, &ly.e3b.d_Wlo, ly.e3b.h_Wlo));
        ALQ_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (ly.f3f.ok && !c3d_subnormals_ok(ctx)) ly.f3f.ok = false;      // (one-accumulator fp16 pairs)
    if (ly.f3f.ok) {
        f3d_pack(&ly.f3f, W);
        ALQ_TRY(upload(m, &ly.f3f.d_Whi, ly.f3f.h_Whi));
        ALQ_TRY(upload(m, &ly.f3f.d_Wlo, ly.f3f.h_Wlo));
        ALQ_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (ly.d3f.ok) {
        d3d_pack(&ly.d3f, W);
        ALQ_TRY(upload(m, &ly.d3f.d_Whi, ly.d3f.h_Whi));
        ALQ_TRY(upload(m, &ly.d3f.d_Wlo, ly.d3f.h_Wlo));
        if (ly.has_bwd) {
            d3d_bwd_pack(&ly.d3f, W);
            ALQ_TRY(upload(m, &ly.d3f.d_Bhi, ly.d3f.h_Bhi));
            ALQ_TRY(upload(m, &ly.d3f.d_Blo, ly.d3f.h_Blo));
        }
        ALQ_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (ly.has_bwd) ALQ_TRY(gemm_set(m, &ly.bwd, transpose_taps(W, Ci, Co, ntaps)));      // [(tap, co)][ci]
    return ALQ_OK;
}

static int set_convt(alq_model *m, Layer &ly, const float *W, const float *b) {
    const int Ci = ly.in.C, Co = ly.spec.cout;
    const int ntaps = ly.spec.k[0] * ly.spec.k[1] * ly.spec.k[2];
    conv_norms(W, b, ntaps, Ci, Co, true, &ly.bwd_l1, &ly.out_l1, &ly.out_bmax);
    ly.bwd_l1_part[0] = ly.bwd_l1_part[1] = 0;
    ly.f16_slices_apart = false;
    if (ly.spec.skip_src >= 0 && m->layers[ly.spec.skip_src].out.C < Ci) {
        float slice_amax[2];
        conv_bwd_l1_slices(W, ntaps, Ci, Co, true, m->layers[ly.spec.skip_src].out.C, ly.bwd_l1_part, slice_amax);
        ly.f16_slices_apart = !slices_within_f16_range(slice_amax);
    }
    // TF [tap][co][ci]; the two-slot plans index taps in the full k^3 enumeration, the older engines by class
    const std::vector<float> Bfull = transpose_taps(W, Co, Ci, ntaps);
    for (size_t c = 0; c < ly.fwd.size(); ++c) {
        const std::vector<int> &tl = ly.class_taps[c];
        const bool p4ok = ly.fwd[c].p4.ok && !ly.fwd_all.ok;     // per-class two-slot plan: only without the fused form
        ly.fwd[c].p4.ok = false;
        ALQ_TRY(gemm_set(m, &ly.fwd[c], transpose_taps(W, Co, Ci, (int)tl.size(), tl.data())));
        if (p4ok) {
            ly.fwd[c].p4.ok = true;
            ALQ_TRY(set4(m, &ly.fwd[c].p4, Bfull));
        }
    }
    if (ly.fwd_all.ok) ALQ_TRY(set4(m, &ly.fwd_all, Bfull));
    // (the t3d plans do not keep their host copy)
    if (ly.t3f.ok) {
        if (ly.t3f.kind == 8) t3d8_fwd_pack(&ly.t3f, W); else t3d_fwd_pack(&ly.t3f, W);
        ALQ_TRY(upload_release(m, &ly.t3f.d_W, &ly.t3f.h_W));
    }
    const bool two_acc = ly.t3b.kind == 8;      // (t3d8b: two accumulators; t3d: one-accumulator fp16 pairs, which need the subnormals)
    if (ly.t3b.ok && ly.has_bwd && (two_acc || c3d_subnormals_ok(m->ctx))) {
        if (two_acc) t3d8_bwd_pack(&ly.t3b, W); else t3d_bwd_pack(&ly.t3b, W);
        ALQ_TRY(upload_release(m, &ly.t3b.d_W, &ly.t3b.h_W));
    }
    if (ly.has_bwd) ALQ_TRY(gemm_set(m, &ly.bwd, std::vector<float>(W, W + ly.w_elems)));   // [(tap, co)][ci] as stored
    return ALQ_OK;
}

static int set_fc(alq_model *m, Layer &ly, const float *W) {
    const int Co = ly.spec.cout;
    const int64_t F = ly.F;
    std::vector<float> Wp = fc_to_mem_order(W, Co, ly.in.D, ly.in.H, ly.in.W, ly.in.C);
    ly.bwd_l1 = fc_col_l1(W, Co, F);      // the layer's L1 bound for the chain of static fp16x2 bounds of the backward pass (like a conv's)
    if (!ly.dense_fc_small) {
        ALQ_TRY(gemm_set(m, &ly.fwd[0], transpose_taps(Wp.data(), Co, (int)F, 1)));      // B[f_mem][o]
        if (ly.has_bwd) ALQ_TRY(gemm_set(m, &ly.bwd, Wp));   // [(o)][f_mem]
        return ALQ_OK;
    }
    ly.fc_wv_amax = 0.f;
    if (Co == 2) {
        // the head's input cotangent under the unit cotangent (+1, -1): W0 - W1.  A head that is not fused into a conv keeps only
        // the bound that cotangent obeys
        std::vector<float> wv = head_wv(Wp.data(), F, &ly.fc_wv_amax);
        if (ly.fc_wv) {
            ALQ_TRY(upload(m, &ly.fc_wv, wv));
            ALQ_HIP(hipStreamSynchronize(m->ctx->stream));
            if (ly.fc_wv16 && ly.fc_wv_amax > 0.f && F % 4 == 0) {
                int e = 0;
                std::vector<unsigned> sp = head_wv16(wv, ly.fc_wv_amax, &e);
                ALQ_TRY(upload_release(m, &ly.fc_wv16, &sp));
                if (ly.fc_wv16c && F % 8 == 0) {      // the same scale, pieces at their true scale, per voxel [h8 | l8] (plane-sweep backward)
                    std::vector<unsigned short> sc;
                    c3d_presplit_vec(wv.data(), F, e, &sc);
                    ALQ_TRY(upload_release(m, &ly.fc_wv16c, &sc));
                }
            }
        }
    }
    return upload_release(m, &ly.d_Wp, &Wp);
}

// the layers alq_model_set_weights_device packs on the device: fc layers whose forward and backward Gemm both run on the
// streaming GEMM of fcgemm.hip (and on nothing else by default)
static bool packs_on_device(const Layer &ly) {
    return ly.spec.type == ALQ_FC && !ly.dense_fc_small && ly.fwd.size() == 1 && ly.fwd[0].pfc.ok && !ly.fwd[0].pd.ok &&
           (!ly.has_bwd || (ly.bwd.pfc.ok && !ly.bwd.pd.ok)) && ly.spec.cout <= 65535;
}

extern "C" {

int alq_model_param_sizes(const alq_model *m, int t, int64_t *w_elems, int64_t *b_elems) {
    ALQ_REQUIRE(m != nullptr, ALQ_EINVAL, "null model");
    const Layer *ly = find_param_layer(m, t);
    if (!ly) return ALQ_EINVAL;
    if (w_elems) *w_elems = ly->w_elems;
    if (b_elems) *b_elems = ly->b_elems;
    return ALQ_OK;
}

int alq_model_set_weights(alq_model *m, int t, const float *W, const float *b) {
    ALQ_REQUIRE(m && W && b, ALQ_EINVAL, "alq_model_set_weights: null argument");
    ALQ_HIP(hipSetDevice(m->ctx->device));
    Layer *lyp = find_param_layer(m, t);
    if (!lyp) return ALQ_EINVAL;
    Layer &ly = *lyp;
    ALQ_TRY(require_subnormal_probe(m->ctx, "alq_model_set_weights"));
    ALQ_HIP(hipMemcpyAsync(ly.d_bias, b, ly.b_elems * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
    if (ly.dense_head) {      // the 1x1 conv head of a fully-convolutional model: TF [1, (1,) 1, Ci, c] is the [Ci][c] the kernels read
        conv_norms(W, b, 1, ly.in.C, ly.spec.cout, false, &ly.bwd_l1, &ly.out_l1, &ly.out_bmax);
        ALQ_HIP(hipMemcpyAsync(ly.d_W32, W, ly.w_elems * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
    } else if (ly.spec.type == ALQ_CONV) ALQ_TRY(set_conv(m, ly, W, b));
    else if (ly.spec.type == ALQ_CONVT) ALQ_TRY(set_convt(m, ly, W, b));
    else ALQ_TRY(set_fc(m, ly, W));
    ALQ_HIP(hipStreamSynchronize(m->ctx->stream));
    ly.weights_set = true;
    ly.fallback_stale = false;
    m->host_pack_elems += ly.w_elems;
    // what alq_hess_vecp contracts with (its next call fills hv_W): a skinny fc layer's exact fp32 weights are already
    // resident (d_Wp, activation-memory order); any other layer's engines hold split forms only, so the host keeps the array
    if (ly.spec.type == ALQ_FC && ly.dense_fc_small && ly.d_Wp) {
        std::vector<float>().swap(ly.hv_hW);
        ly.hv_src = 3;
    } else {
        ly.hv_hW.assign(W, W + ly.w_elems);
        ly.hv_src = 1;
    }
    ly.hv_stale = true;
    return ALQ_OK;
}

int alq_model_layer_packs_on_device(const alq_model *m, int t) {
    ALQ_REQUIRE(m != nullptr, ALQ_EINVAL, "null model");
    const Layer *ly = find_param_layer(m, t);
    if (!ly) return ALQ_EINVAL;
    return packs_on_device(*ly) ? 1 : 0;
}

int alq_model_set_weights_device(alq_model *m, int t, const float *d_W, const float *d_b) {
    ALQ_REQUIRE(m && d_W && d_b, ALQ_EINVAL, "alq_model_set_weights_device: null argument");
    ALQ_HIP(hipSetDevice(m->ctx->device));
    Layer *lyp = find_param_layer(m, t);
    if (!lyp) return ALQ_EINVAL;
    Layer &ly = *lyp;
    alq_ctx *ctx = m->ctx;
    if (ly.dense_head) {      // plain fp32 [Ci][c] + [c]: device to device, nothing to pack
        ALQ_HIP(hipMemcpyAsync(ly.d_W32, d_W, ly.w_elems * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        ALQ_HIP(hipMemcpyAsync(ly.d_bias, d_b, ly.b_elems * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        ly.weights_set = true;
        std::vector<float>().swap(ly.hv_hW);
        ly.hv_src = 0;
        return ALQ_OK;
    }
    if (!packs_on_device(ly)) {      // no device packers for this layer's engines: its slice goes through the host's
        std::vector<float> W((size_t)ly.w_elems), b((size_t)ly.b_elems);
        ALQ_HIP(hipMemcpyAsync(W.data(), d_W, W.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        ALQ_HIP(hipMemcpyAsync(b.data(), d_b, b.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        ALQ_HIP(hipStreamSynchronize(ctx->stream));
        return alq_model_set_weights(m, t, W.data(), b.data());
    }
    ALQ_TRY(require_subnormal_probe(ctx, "alq_model_set_weights_device"));
    const int Co = ly.spec.cout;
    const int64_t F = ly.F;
    ALQ_TRY(ensure<unsigned char>(m, &m->d_wscal, 64));
    ALQ_TRY(ensure<float>(m, &ly.d_Wres, (size_t)ly.w_elems));
    ALQ_HIP(hipMemcpyAsync(ly.d_bias, d_b, ly.b_elems * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    ALQ_TRY(wpack_stats(ctx, d_W, Co, F, m->d_wscal));
    ALQ_TRY(wpack_permute(ctx, d_W, ly.d_Wres, Co, ly.in.D, ly.in.H, ly.in.W, ly.in.C));
    const bool sub = c3d_subnormals_ok(ctx) != 0;
    auto pack = [&](Gemm *g, int K, int N, int kmajor) -> int {
        ALQ_REQUIRE(g->pfc.K == K && g->pfc.N == N, ALQ_EINVAL, "alq_model_set_weights_device: plan %d x %d, layer %d x %d", g->pfc.K, g->pfc.N, K, N);
        ALQ_TRY(ensure<unsigned short>(m, &g->pfc.d_W, (size_t)K * N * 3));
        if (g->pfc_f16 && sub) ALQ_TRY(ensure<unsigned short>(m, &g->pfc.d_W16, (size_t)K * N * 2));
        return wpack_fc(ctx, ly.d_Wres, F, K, N, kmajor, g->pfc.d_W, g->pfc_f16 && sub ? g->pfc.d_W16 : nullptr, m->d_wscal);
    };
    ALQ_TRY(pack(&ly.fwd[0], (int)F, Co, 0));              // B[f_mem][o]
    if (ly.has_bwd) ALQ_TRY(pack(&ly.bwd, Co, (int)F, 1)); // B[o][f_mem]
    // the host scalars the launches take their power-of-two scales from: 12 bytes device-to-host
    unsigned long long sc[2] = {0, 0};
    ALQ_HIP(hipMemcpyAsync(sc, m->d_wscal, 16, hipMemcpyDeviceToHost, ctx->stream));
    ALQ_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(&ly.bwd_l1, &sc[0], 8);
    float amax;
    std::memcpy(&amax, &sc[1], 4);
    int ex = 0;
    if (amax > 0.f) (void)std::frexp(amax, &ex);
    if (ly.fwd[0].pfc_f16 && sub) ly.fwd[0].pfc.w_exp = 14 - ex;
    if (ly.has_bwd && ly.bwd.pfc_f16 && sub) ly.bwd.pfc.w_exp = 14 - ex;
    ly.weights_set = true;
    ly.fallback_stale = true;
    std::vector<float>().swap(ly.hv_hW);
    ly.hv_src = 2;
    ly.hv_stale = true;
    return ALQ_OK;
}

}  // extern "C"
