// Model plan behind the C ABI: shapes, activation / cotangent workspaces (concat skips = channel slices of one buffer), the engine
// plans, gemm_route / gemm_launch, and the entry points with their debug hooks.  The structures are in model_types.h; the forward pass and
// the fused Fisher backward sweep are passes.hip; weights reach the engines' packed forms in weights.hip; the general gradient path is
// grads.hip, everything that takes no model (contexts, profiling, the pass-through entry points) ctx.hip.
#include <algorithm>
#include <cstring>
#include <string>

#include "model_types.h"

using namespace alq;

// ------------------------------------------------------------------------------------------
static int g_knob_override[ALQ_NKNOBS] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // alq_debug_set: >= 0 overrides every model's snapshot

// The kernels' launch helpers read the process-wide g_dbg_knobs / g_no_f16x2; each entry point loads them from the
// model it was called on, so creating another model (or its environment) never changes a live one.
static void apply_knobs(const alq_model *m) {
    for (int k = 0; k < ALQ_NKNOBS; ++k) g_dbg_knobs[k] = g_knob_override[k] >= 0 ? g_knob_override[k] : m->sw.knobs[k];
    g_no_f16x2 = m->sw.no_f16x2;
    // a conv over a concat whose two weight slices no single fp16-pair exponent holds (set with the weights): the launches of this
    // model stay on bf16 triples, which keep fp32's exponent range
    for (const Layer &ly : m->layers) g_no_f16x2 |= ly.f16_slices_apart ? 1 : 0;
    g_no_xcd_order = m->sw.no_xcd_order;
    g_no_fixed = m->sw.no_fixed;
}

static int gemm_build(const EngineSwitches &sw, const ConvDesc &d, int max_batch, Gemm *g, const G4Geom *g4 = nullptr) {
    ALQ_TRY(igemm_build_plan(d, max_batch, &g->p1));
    if (g4 && !sw.disable_v4) {
        G4Geom gg = *g4;
        gg.flops_per_patch = g->p1.flops_per_patch;
        ALQ_TRY(igemm4_build_plan(gg, max_batch, &g->p4));
    }
    ALQ_TRY(igemm2_build_plan(g->p1, &g->p2));
    ALQ_TRY(direct_build_plan(g->p1, &g->pd));
    if (sw.disable_v2) { g->p2.ok = false; g->pd.ok = false; }
    ALQ_TRY(igemm3_build_plan(g->p2, &g->p3));
    if (d.ID == 1 && d.IH == 1 && d.IW == 1 && d.tz.size() == 1 && d.sm == 1 && d.so == 1 && !sw.no_fcgemm)
        ALQ_TRY(fcgemm_build_plan(d.Ci, d.Co, &g->pfc));       // a wide fully connected layer
    if (sw.disable_v3) g->p3.ok = false;
    return ALQ_OK;
}

// first step of every entry point that runs a pass; `fisher`: the pass is a Fisher pass (what alq_model_debug_copy may read)
int prepare_call(alq_model *m, bool fisher) {
    m->last.call_fisher = fisher;
    apply_knobs(m);
    if (!two_slot_allowed()) ALQ_TRY(refresh_fallback_forms(m));
    return ALQ_OK;
}

// Which engine a gemm_launch call takes.  The debug knobs take the two-slot engine away - except for a split concat view,
// which only that engine reads.
GemmRoute gemm_route(const Gemm &g, const View &in, const View &out, int accumulate, const Igemm2Fuse *fuse) {
    if (g.pd.ok && !accumulate && !(fuse && (fuse->mask || fuse->osumB || fuse->split))) return ROUTE_DIRECT;
    if (g.pfc.ok && !accumulate && !fuse && two_slot_allowed()) return ROUTE_FCGEMM;      // wide fc layer: streaming bf16x3 GEMM
    const bool split_view = in.split != 0 || out.split != 0;
    if (g.p4.ok && (two_slot_allowed() || split_view)) return ROUTE_IGEMM4;      // two-slot bf16x3 engine
    if (g.p3.ok && !g_dbg_knobs[KNOB_NO_V3]) return ROUTE_IGEMM3;      // bf16x3 split on the matrix cores (fp32-equivalent accuracy)
    return g.p2.ok ? ROUTE_IGEMM2 : ROUTE_IGEMM;
}

// returns in *fused whether the epilogue fusion request was honoured (only the pipelined kernel can)
int gemm_launch(alq_ctx *ctx, const Gemm &g, const View &in, const View &out, const float *bias, int relu,
                int accumulate, int N, int cls, const Igemm2Fuse *fuse, bool *fused, float fc_in_bound) {
    const GemmRoute route = gemm_route(g, in, out, accumulate, fuse);
    ALQ_REQUIRE(route <= ROUTE_FCGEMM || g.p4.ok || (in.split == 0 && out.split == 0), ALQ_EUNSUPPORTED, "split concat view without a two-slot plan");
    if (fused) *fused = fuse != nullptr && route != ROUTE_FCGEMM && route != ROUTE_IGEMM;
    const int cls3 = cls == PROF_IGEMM_BWD ? PROF_IGEMM3_BWD : PROF_IGEMM3_FWD;
    switch (route) {
        case ROUTE_DIRECT: return direct_launch(ctx, g.pd, in, out, bias, relu, N, fuse ? fuse->osumA : nullptr, PROF_DIRECT);
        case ROUTE_FCGEMM:
            // forward launches of wide fc layers: fp16 pairs under the per-patch maxima the launch measures (fcgemm.hip, round 6)
            return fcgemm_launch(ctx, g.pfc, in, out, bias, relu, N, cls3, (g_no_f16x2 || bias || relu) ? 0.f : fc_in_bound,
                                 (cls == PROF_IGEMM_FWD && !g_no_f16x2) ? g.fc_row_amax : nullptr);
        case ROUTE_IGEMM4: return igemm4_launch(ctx, g.p4, in, out, bias, relu, accumulate, N, cls3, fuse);
        case ROUTE_IGEMM3: return igemm3_launch(ctx, g.p2, g.p3, in, out, bias, relu, accumulate, N, cls3, fuse);
        case ROUTE_IGEMM2: return igemm2_launch(ctx, g.p2, in, out, bias, relu, accumulate, N, cls, fuse);
        case ROUTE_IGEMM: break;
    }
    return igemm_launch(ctx, g.p1, in, out, bias, relu, accumulate, N, cls);
}

// ---- model creation: the shapes and every geometry descriptor come from model_plan.h; what follows allocates and plans --------
static View mkview(float *p, const Shp &s, int cs, int c0, int C) {
    View v; v.p = p; v.D = s.D; v.H = s.H; v.W = s.W; v.cs = cs; v.c0 = c0; v.C = C; return v;
}

struct ActViews { std::vector<View> act, dact, catv, dcatv; };      // per layer: output and its cotangent; a concat consumer's input likewise

// buffers (concat = two producers writing channel slices of one buffer), then the model's own result buffers
static int alloc_activations(alq_model *m, const ModelShape &ms, ActViews *av) {
    const EngineSwitches &sw = m->sw;
    const int n_layers = (int)ms.layers.size(), NB = m->max_batch;
    std::vector<View> &act = av->act, &dact = av->dact, &catv = av->catv, &dcatv = av->dcatv;
    act.resize(n_layers); dact.resize(n_layers); catv.resize(n_layers); dcatv.resize(n_layers);
    for (int d = 0; d < n_layers; ++d) {
        if (ms.src_of[d] < 0) continue;
        const int s = ms.src_of[d];
        const LayerShape &dl = ms.layers[d];
        const alq_layer_t &dsp = m->layers[d].spec;
        const Shp &sh = ms.layers[s].out;
        const int Cs = sh.C, Cp = ms.layers[d - 1].out.C;
        float *buf, *dbuf;
        const size_t el = (size_t)NB * sh.D * sh.H * sh.W * (Cs + Cp);
        ALQ_TRY(m->dalloc(&buf, el));
        ALQ_TRY(m->dalloc(&dbuf, el));
        unsigned char *sbuf = nullptr;      // sign field of the whole allocation (View::sg): float offset / 4
        if (Cs % 4 == 0 && Cp % 4 == 0) ALQ_TRY(m->dalloc(&sbuf, el / 4));
        // Split concat: when the consumer's forward and backward contractions both run on the two-slot engine, the
        // two producers keep DENSE tensors (the halves of one allocation) and the consumer reads / writes them as
        // two channel groups.  Interleaved slices cost twice the cache lines per staged or stored row (32 of 64
        // bytes used), and the engine's staging and store parts are bound by lines touched.
        bool split_ok = false;
        if (Cs == Cp && Cs % 8 == 0 && dsp.type == ALQ_CONV && !sw.disable_v4 && !sw.no_split) {
            Igemm4Plan tf, tb;
            ALQ_TRY(igemm4_build_plan(conv_fwd_geom(dl.in, dl.out, dsp, dl.lo), NB, &tf));
            ALQ_TRY(igemm4_build_plan(conv_bwd_geom(dl.in, dl.out, dsp, dl.lo), NB, &tb));
            split_ok = tf.ok && tb.ok && !tb.a.pair;
        }
        m->layers[s].out_is_skip_src = true;
        if (split_ok) {
            const long long half = (long long)NB * sh.D * sh.H * sh.W * Cs;
            act[s] = mkview(buf, sh, Cs, 0, Cs);
            act[d - 1] = mkview(buf + half, sh, Cp, 0, Cp);
            dact[s] = mkview(dbuf, sh, Cs, 0, Cs);
            dact[d - 1] = mkview(dbuf + half, sh, Cp, 0, Cp);
            catv[d] = mkview(buf, sh, Cs, 0, Cs + Cp);
            catv[d].split = Cs; catv[d].delta = half;
            if (sbuf) { act[s].sg = sbuf; act[d - 1].sg = sbuf + half / 4; catv[d].sg = sbuf; }
            dcatv[d] = mkview(dbuf, sh, Cs, 0, Cs + Cp);
            dcatv[d].split = Cs; dcatv[d].delta = half;
            continue;
        }
        act[s] = mkview(buf, sh, Cs + Cp, 0, Cs);
        act[d - 1] = mkview(buf, sh, Cs + Cp, Cs, Cp);
        dact[s] = mkview(dbuf, sh, Cs + Cp, 0, Cs);
        dact[d - 1] = mkview(dbuf, sh, Cs + Cp, Cs, Cp);
        catv[d] = mkview(buf, sh, Cs + Cp, 0, Cs + Cp);
        dcatv[d] = mkview(dbuf, sh, Cs + Cp, 0, Cs + Cp);
        if (sbuf) { act[s].sg = sbuf; act[d - 1].sg = sbuf; catv[d].sg = sbuf; }
    }
    for (int i = 0; i < n_layers; ++i) {
        if (act[i].p) continue;
        const Shp &sh = ms.layers[i].out;
        const alq_layer_t &sp = m->layers[i].spec;
        float *buf, *dbuf;
        const size_t el = (size_t)NB * sh.D * sh.H * sh.W * sh.C;
        ALQ_TRY(m->dalloc(&buf, el));
        ALQ_TRY(m->dalloc(&dbuf, el));
        act[i] = mkview(buf, sh, sh.C, 0, sh.C);
        dact[i] = mkview(dbuf, sh, sh.C, 0, sh.C);
        if (sh.C % 4 == 0 && sp.type != ALQ_FC && (sp.type == ALQ_POOL || sp.relu)) ALQ_TRY(m->dalloc(&act[i].sg, el / 4));
    }
    m->logits = act[n_layers - 1].p;
    m->dlogits = dact[n_layers - 1].p;
    ALQ_TRY(m->dalloc(&m->post, (size_t)NB * m->nclass * m->V));
    ALQ_TRY(m->dalloc(&m->S, (size_t)NB * m->L));
    ALQ_TRY(m->dalloc(&m->sizes, (size_t)m->L));
    ALQ_TRY(m->dalloc(&m->Apart, (size_t)((NB + 63) / 64) * m->L * m->L));
    return ALQ_OK;
}

static int plan_conv(alq_model *m, const LayerShape &ls, Layer &ly) {
    const EngineSwitches &sw = m->sw;
    const int NB = m->max_batch;
    const alq_layer_t &sp = ly.spec;
    const bool first_param = (ly.pidx == 0);
    const ConvDesc d = conv_fwd_desc(ls.in, ls.out, sp, ly.lo);
    const G4Geom g4 = conv_fwd_geom(ls.in, ls.out, sp, ly.lo);
    ly.fwd.resize(1);
    ALQ_TRY(gemm_build(sw, d, NB, &ly.fwd[0], &g4));
    // a 2-D window of 25 taps or more: the two-slot engine's tiles re-stage too much halo - NET-B's conv2 (24 -> 32 channels,
    // 5 x 5 at 32^2) takes 673 us per 2048 patches there and ~390 on igemm3 (round 6; ALQ_NO_WIDE2D_RULE=1 = the other arm)
    if (ly.fwd[0].p4.ok && ly.fwd[0].p3.ok && d.ID == 1 && d.tz.size() >= 25 && !sw.no_wide2d_rule) ly.fwd[0].p4.ok = false;
    // a forward launch that stays on igemm3, tiles of one patch: the fp16-pair twin of its weights for Fisher / forward-only passes
    // (run_forward, round 6; ALQ_NO_V3_F16_FWD=1: bf16 triples as before)
    if (!ly.fwd[0].p4.ok && !ly.fwd[0].pd.ok && !ly.fwd[0].pfc.ok && ly.fwd[0].p3.ok && ly.fwd[0].p2.a.PT == 1 && sp.skip_src < 0 &&
        !sw.no_v3_f16_fwd && !sw.no_v3_f16) {
        ly.fwd[0].p3_f16 = true;
        m->v3_fwd_f16 = true;
    }
    if (!ly.fwd[0].p4.ok && !ly.fwd[0].p3.ok && !ly.fwd[0].pd.ok && sp.cout > 32 && !sw.no_co_split) {
        for (int w : {32, 48, 16}) {
            if (sp.cout % w || sp.cout <= w) continue;
            std::vector<Gemm> parts(sp.cout / w);
            bool ok = true;
            for (size_t j = 0; j < parts.size() && ok; ++j) {
                ConvDesc dj = d;
                dj.Co = w;
                G4Geom gj = g4;
                gj.Co = w;
                ALQ_TRY(gemm_build(sw, dj, NB, &parts[j], &gj));
                ok = parts[j].p4.ok || parts[j].p3.ok;
            }
            if (ok) { ly.fwd_co = std::move(parts); ly.fwd_co_w = w; break; }
        }
    }
    if (!first_param && sp.relu) {
        ALQ_TRY(c3d_fwd_build(ly.in, ly.out, sp.k, ly.lo, sp.s, &ly.c3f));
        ALQ_TRY(c3d_bwd_build(ly.in, ly.out, sp.k, ly.lo, sp.s, &ly.c3b));
        ALQ_TRY(e3d_build(ly.in, ly.out, sp.k, ly.lo, sp.s, &ly.e3b));
        ALQ_TRY(d3d_build(ly.in, ly.out, sp.k, ly.lo, sp.s, &ly.d3f));
        ALQ_TRY(f3d_build(ly.in, ly.out, sp.k, ly.lo, sp.s, &ly.f3f));
    }
    if (!first_param) {
        const G4Geom gb = conv_bwd_geom(ls.in, ls.out, sp, ly.lo);
        ALQ_TRY(gemm_build(sw, conv_bwd_desc(ls.in, ls.out, sp, ly.lo), NB, &ly.bwd, &gb));
        ly.has_bwd = true;
        // a backward launch that stays on igemm3 (no two-slot plan: NET-B's 5 x 5 and 96-channel convs) takes fp16 pairs under the
        // cotangent bound of a Fisher pass like the two-slot launches do (round 6; ALQ_NO_V3_F16=1: bf16 triples as before)
        ly.bwd.p3_f16 = !ly.bwd.p4.ok && ly.bwd.p3.ok && !sw.no_v3_f16;
    }
    return ALQ_OK;
}

static int plan_convt(alq_model *m, const LayerShape &ls, Layer &ly, int i) {
    const EngineSwitches &sw = m->sw;
    const int NB = m->max_batch;
    const alq_layer_t &sp = ly.spec;
    const bool first_param = (ly.pidx == 0);
    const int nclsz = convt_classes_z(ls.in, sp);
    for (int cz = 0; cz < nclsz; ++cz)
        for (int cy = 0; cy < sp.s[1]; ++cy)
            for (int cx = 0; cx < sp.s[2]; ++cx) {
                std::vector<int> tl;
                const ConvDesc d = convt_class_desc(ls.in, ls.out, sp, ly.lo, cz, cy, cx, &tl);
                ALQ_REQUIRE(!tl.empty(), ALQ_EUNSUPPORTED, "layer %d: empty conv_transpose class", i);
                ly.class_taps.push_back(tl);
                ly.fwd.emplace_back();
                const G4Geom gc = convt_class_geom(ls.in, ls.out, sp, ly.lo, cz, cy, cx);
                ALQ_TRY(gemm_build(sw, d, NB, &ly.fwd.back(), &gc));
            }
    ALQ_REQUIRE(sp.s[0] == sp.s[2] || (ly.in.D == 1 && sp.s[0] == 1), ALQ_EUNSUPPORTED,
                "layer %d: conv_transpose stride must be isotropic", i);
    if (!sw.disable_v4) {
        double flops = 0;
        for (const Gemm &c : ly.fwd) flops += c.p1.flops_per_patch;
        G4Geom gf = convt_all_geom(ls.in, ls.out, sp, ly.lo, 2);
        gf.flops_per_patch = flops;
        ALQ_TRY(igemm4_build_plan(gf, NB, &ly.fwd_all));
        if (!ly.fwd_all.ok && !sw.no_class_tiles) {      // too large to stage once: the classes as tiles of one launch
            gf = convt_all_geom(ls.in, ls.out, sp, ly.lo, 4);
            gf.flops_per_patch = flops;
            ALQ_TRY(igemm4_build_plan(gf, NB, &ly.fwd_all));
        }
    }
    if (!sp.relu) ALQ_TRY(t3d_build(ly.in, ly.out, sp.k, ly.lo, sp.s, &ly.t3f, &ly.t3b));
    if (first_param) ly.t3b.ok = false;
    if (!first_param) {
        const G4Geom gb = convt_bwd_geom(ls.in, ls.out, sp, ly.lo);
        ALQ_TRY(gemm_build(sw, convt_bwd_desc(ls.in, ls.out, sp, ly.lo), NB, &ly.bwd, &gb));
        ly.has_bwd = true;
    }
    return ALQ_OK;
}

static int plan_pool(alq_model *m, Layer &ly) {
    uint8_t *am;
    ALQ_TRY(m->dalloc(&am, (size_t)m->max_batch * ly.out.vox() * ly.out.C));
    ly.argmax = am;
    return ALQ_OK;
}

// `i`: the layer's index (the last layer under a ReLU conv of 8 channels may take the two-class head's workspaces)
static int plan_fc(alq_model *m, Layer &ly, int i) {
    const EngineSwitches &sw = m->sw;
    const int NB = m->max_batch, n_layers = (int)m->layers.size();
    const alq_layer_t &sp = ly.spec;
    ALQ_REQUIRE(ly.in.cs == ly.in.C && ly.in.c0 == 0, ALQ_EUNSUPPORTED, "layer %d: fc on a concat slice", i);
    if (sp.cout > 8) {
        const ConvDesc d = fc_fwd_desc(ly.F, sp.cout);
        ly.fwd.resize(1);
        ALQ_TRY(gemm_build(sw, d, NB, &ly.fwd[0]));
        if (ly.fwd[0].pfc.ok && !sw.no_fc_f16_fwd) {      // forward launch of a wide fc layer on fp16 pairs (measured per-patch maxima)
            ly.fwd[0].pfc_f16 = true;
            ALQ_TRY(m->dalloc(&ly.fwd[0].fc_row_amax, (size_t)m->max_batch));
        }
        if (ly.pidx != 0) {
            ALQ_TRY(gemm_build(sw, fc_bwd_desc(ly.F, sp.cout), NB, &ly.bwd));
            ly.bwd.pfc_f16 = ly.bwd.pfc.ok && !sw.no_fc_f16;      // backward launch: fp16 pairs under the static cotangent bound
            ly.has_bwd = true;
        }
        return ALQ_OK;
    }
    ly.dense_fc_small = true;
    ly.fc_slices = fc_small_slices(ly.F);
    ALQ_TRY(m->dalloc(&ly.d_Wp, (size_t)sp.cout * ly.F));
    ALQ_TRY(m->dalloc(&ly.fc_partials, (size_t)NB * ly.fc_slices * sp.cout));
    if (sp.cout == 2 && ly.F % 1024 == 0 && i == n_layers - 1 && i > 0 && m->layers[i - 1].spec.relu && m->layers[i - 1].pidx > 0 &&
        m->layers[i - 1].spec.type == ALQ_CONV && m->layers[i - 1].out.C == 8 && !sw.no_fc_bits) {
        ALQ_TRY(m->dalloc(&ly.fc_maskbits, (size_t)NB * (ly.F / 16)));      // one sign byte per 4 elements
        ALQ_TRY(m->dalloc(&ly.fc_wv, (size_t)ly.F));
        ALQ_TRY(m->dalloc(&ly.fc_wv16, (size_t)ly.F));
        const Layer &cv = m->layers[i - 1];
        const Igemm4Plan &fp = cv.fwd[0].p4;
        if (!sp.relu && fp.ok && fp.NTW == 1 && !fp.multi && fp.a.pair && fp.a.PT == 1 && cv.out.cs == 8 &&
            cv.out.c0 == 0 && !cv.out.split && cv.osum && !cv.out_is_skip_src && !sw.no_fc_fuse &&
            // the backward pass must be able to work from the bits alone (bits_ok in run_backward)
            cv.bwd.p4.ok && cv.bwd.p4.NTW == 1 && !cv.bwd.p4.multi && cv.bwd.p4.a.PT == 1 && !cv.dout.split) {
            ly.fc_slices2 = fp.a.tpg * 4;
            ALQ_TRY(m->dalloc(&ly.fc_part2, (size_t)NB * ly.fc_slices2));
            if (cv.c3f.ok && ly.F == (int64_t)cv.out.vox() * 8) {
                ALQ_TRY(m->dalloc(&ly.c3_part, (size_t)NB * 4));
                ALQ_TRY(m->dalloc(&ly.c3_asum, (size_t)NB * 4));
                if (cv.c3b.ok) ALQ_TRY(m->dalloc(&ly.fc_wv16c, (size_t)ly.F * 2));
            }
        }
    }
    return ALQ_OK;
}

// layer i's views and the buffers every engine shares: the conv head's own (ly.dense_head: nothing else to plan), or the statistics buffers
static int bind_layer(alq_model *m, const ModelShape &ms, const ActViews &av, int i) {
    const int NB = m->max_batch, n_layers = (int)m->layers.size();
    Layer &ly = m->layers[i];
    if (ms.src_of[i] >= 0) {
        ly.in = av.catv[i];
        ly.din = av.dcatv[i];
    } else if (i == 0) {
        ly.in = mkview(nullptr, ms.layers[0].in, ms.layers[0].in.C, 0, ms.layers[0].in.C);   // pointer bound per call
        ly.din = View();
    } else {
        ly.in = av.act[i - 1];
        ly.din = av.dact[i - 1];
    }
    ly.out = av.act[i];
    ly.dout = av.dact[i];
    if (m->dense && i == n_layers - 1) {      // the 1x1 conv head: plain fp32 weights [Ci][c], no engine plans, no statistics buffers
        ALQ_REQUIRE(ly.in.cs == ly.in.C && ly.in.c0 == 0 && !ly.in.split, ALQ_EUNSUPPORTED, "layer %d: conv head on a concat slice", i);
        ly.dense_head = true;
        ALQ_TRY(m->dalloc(&ly.d_bias, (size_t)ly.b_elems));
        ALQ_TRY(m->dalloc(&ly.d_W32, (size_t)ly.w_elems));
        ALQ_TRY(m->dalloc(&m->dh_part, (size_t)ALQ_DENSE_MAX_BLOCKS * (ly.w_elems + ly.b_elems)));
        return ALQ_OK;
    }
    if (ly.spec.type != ALQ_FC) ALQ_TRY(m->dalloc(&ly.osum, (size_t)NB * ly.out.vox()));
    if (ly.pidx >= 0) {
        ALQ_TRY(m->dalloc(&ly.d_bias, (size_t)ly.b_elems));
        ALQ_TRY(m->dalloc(&ly.asum, (size_t)NB * ly.in.vox()));
        ALQ_TRY(m->dalloc(&ly.dsum, (size_t)NB * ly.out.vox()));
    }
    return ALQ_OK;
}

// box-dot slab partials: conv / fc reduce over the OUTPUT grid, conv_transpose over the input grid
static int alloc_slabs(alq_model *m) {
    std::vector<int> h_nslab(m->L, 1);
    for (const Layer &ly : m->layers) {
        if (ly.pidx < 0) continue;
        if (ly.spec.type == ALQ_CONV) h_nslab[ly.pidx] = boxdot_conv_slabs(ly.out.D, ly.out.H, ly.out.W, ly.spec.k);
        else if (ly.spec.type == ALQ_CONVT) h_nslab[ly.pidx] = boxdot_convT_slabs(ly.in.D, ly.in.H, ly.in.W, ly.spec.k, ly.spec.s);
        else h_nslab[ly.pidx] = boxdot_slabs(1);
        m->nslab_max = std::max(m->nslab_max, h_nslab[ly.pidx]);
    }
    ALQ_TRY(m->dalloc(&m->nslab, (size_t)m->L));
    ALQ_TRY(m->dalloc(&m->Spart, (size_t)m->L * m->max_batch * m->nslab_max));
    ALQ_HIP(hipMemcpy(m->nslab, h_nslab.data(), m->L * sizeof(int), hipMemcpyHostToDevice));
    return ALQ_OK;
}

static int build_model(alq_model *m, const alq_layer_t *specs, int n_layers) {
    ModelShape ms;
    ALQ_TRY(plan_shapes(specs, n_layers, m->in_dims, m->epp, m->max_batch, &ms));
    m->L = ms.L; m->dense = ms.dense; m->V = ms.V; m->nclass = ms.nclass; m->max_batch = ms.max_batch;
    m->layers.resize(n_layers);
    for (int i = 0; i < n_layers; ++i) {
        Layer &ly = m->layers[i];
        const LayerShape &ls = ms.layers[i];
        ly.spec = specs[i];
        for (int q = 0; q < 3; ++q) ly.lo[q] = ls.lo[q];
        ly.pidx = ls.pidx; ly.w_elems = ls.w_elems; ly.b_elems = ls.b_elems; ly.F = ls.F;
    }
    ActViews av;
    ALQ_TRY(alloc_activations(m, ms, &av));
    std::vector<double> h_sizes(m->L);
    for (int i = 0; i < n_layers; ++i) {
        Layer &ly = m->layers[i];
        ALQ_TRY(bind_layer(m, ms, av, i));
        if (ly.pidx >= 0) h_sizes[ly.pidx] = (double)(ly.w_elems + ly.b_elems);
        if (ly.dense_head) continue;
        switch (ly.spec.type) {
            case ALQ_CONV: ALQ_TRY(plan_conv(m, ms.layers[i], ly)); break;
            case ALQ_CONVT: ALQ_TRY(plan_convt(m, ms.layers[i], ly, i)); break;
            case ALQ_POOL: ALQ_TRY(plan_pool(m, ly)); break;
            default: ALQ_TRY(plan_fc(m, ly, i)); break;
        }
    }
    ALQ_HIP(hipMemcpy(m->sizes, h_sizes.data(), m->L * sizeof(double), hipMemcpyHostToDevice));
    return alloc_slabs(m);
}

View flat_view(const View &v) {
    View f;
    f.p = v.p; f.D = f.H = f.W = 1;
    f.C = (int)(v.vox() * v.C); f.cs = f.C; f.c0 = 0;
    return f;
}

int make_drop(const alq_model *m, float keep_prob, uint64_t seed, int64_t first_sample, const int32_t *h_layers, int n_layers,
              DropSpec *d) {
    ALQ_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f, ALQ_EINVAL, "keep_prob %g outside (0, 1]", (double)keep_prob);
    ALQ_REQUIRE(n_layers == 0 || h_layers, ALQ_EINVAL, "dropout layer list missing");
    d->keep_prob = keep_prob; d->seed = seed; d->first_sample = first_sample; d->layers = 0;
    for (int i = 0; i < n_layers; ++i) {
        ALQ_REQUIRE(h_layers[i] >= 0 && h_layers[i] < (int)m->layers.size() && h_layers[i] < 64, ALQ_EINVAL, "dropout layer %d", h_layers[i]);
        d->layers |= 1ull << h_layers[i];
    }
    return ALQ_OK;
}

// =========================================================================================== C ABI
extern "C" {

int alq_model_out_voxels(const alq_model *m) { return m ? (int)m->V : ALQ_EINVAL; }

int alq_model_set_aleatoric(alq_model *m, int on) {
    ALQ_REQUIRE(m, ALQ_EINVAL, "alq_model_set_aleatoric: null model");
    ALQ_REQUIRE(m->dense && m->nclass >= 3, ALQ_EUNSUPPORTED,
                "alq_model_set_aleatoric: a log-variance channel needs a 1x1 conv head of 3 .. 8 channels (2 .. 7 classes beside it)");
    if (on && !m->au) {
        ALQ_HIP(hipSetDevice(m->ctx->device));
        ALQ_TRY(m->dalloc(&m->au, (size_t)m->max_batch * m->V));
    }
    m->aleatoric = on != 0;
    return ALQ_OK;
}

int alq_forward_au(alq_model *m, const float *d_x, int N, float keep_prob, uint64_t seed, int64_t first_sample,
                   const int32_t *h_drop_layers, int n_drop_layers, float *d_post, int64_t *d_pred, float *d_au, float *d_logits) {
    ALQ_REQUIRE(m && d_x && d_au, ALQ_EINVAL, "alq_forward_au: null argument");
    ALQ_REQUIRE(m->aleatoric, ALQ_EUNSUPPORTED, "alq_forward_au: the model has no log-variance channel (alq_model_set_aleatoric)");
    ALQ_REQUIRE(N >= 0 && N <= m->max_batch, ALQ_EINVAL, "alq_forward_au: N=%d exceeds max_batch=%d", N, m->max_batch);
    if (N == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(m->ctx->device));
    DropSpec ds;
    ALQ_TRY(make_drop(m, keep_prob, seed, first_sample, h_drop_layers, n_drop_layers, &ds));
    ALQ_TRY(prepare_call(m, /*fisher=*/false));
    ALQ_TRY(run_forward(m, d_x, N, false, /*keep_all=*/true, &ds));
    return dense_forward_head(m, d_x, N, d_post, d_pred, false, d_au, d_logits);
}

int alq_forward_dropout(alq_model *m, const float *d_x, int N, float keep_prob, uint64_t seed, int64_t first_sample,
                        const int32_t *h_drop_layers, int n_drop_layers, float *d_post, int64_t *d_pred) {
    ALQ_REQUIRE(m && d_x, ALQ_EINVAL, "alq_forward_dropout: null argument");
    ALQ_REQUIRE(N >= 0 && N <= m->max_batch, ALQ_EINVAL, "alq_forward_dropout: N=%d exceeds max_batch=%d", N, m->max_batch);
    if (N == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(m->ctx->device));
    DropSpec ds;
    ALQ_TRY(make_drop(m, keep_prob, seed, first_sample, h_drop_layers, n_drop_layers, &ds));
    ALQ_TRY(prepare_call(m, /*fisher=*/false));
    ALQ_TRY(run_forward(m, d_x, N, false, /*keep_all=*/true, &ds));
    if (m->dense) return dense_forward_head(m, d_x, N, d_post, d_pred, false);
    ALQ_TRY(k_softmax(m->ctx, m->logits, m->nclass, N, d_post ? d_post : m->post, d_pred));
    return ALQ_OK;
}

int alq_model_create(alq_ctx *ctx, const alq_layer_t *layers, int n_layers, const int32_t in_dims[4],
                     int max_batch, alq_model **out) {
    ALQ_REQUIRE(ctx && layers && in_dims && out, ALQ_EINVAL, "alq_model_create: null argument");
    ALQ_REQUIRE(n_layers >= 1 && n_layers <= 64 && max_batch >= 1, ALQ_EINVAL, "alq_model_create: bad sizes");
    ALQ_HIP(hipSetDevice(ctx->device));
    alq_model *m = new alq_model();
    m->ctx = ctx;
    m->max_batch = max_batch;
    m->sw = read_engine_switches();
    for (int i = 0; i < 4; ++i) m->in_dims[i] = in_dims[i];
    m->epp = (int64_t)in_dims[0] * in_dims[1] * in_dims[2] * in_dims[3];
    const int rc = build_model(m, layers, n_layers);
    if (rc != ALQ_OK) {
        alq_model_destroy(m);
        return rc;
    }
    if (const char *t = getenv("ALQ_G4_TUNE")) {
        // diagnostic: per-launch balance of the two-slot engine, "f<layer>:fic=<0|1>,epi=<0..2>;b<layer>:..." (f = forward
        // launch of the layer, b = its backward-data launch); every setting computes the same bits
        std::string all(t);
        size_t pos = 0;
        while (pos < all.size()) {
            size_t end = all.find(';', pos);
            if (end == std::string::npos) end = all.size();
            const std::string item = all.substr(pos, end - pos);
            pos = end + 1;
            if (item.size() < 3 || (item[0] != 'f' && item[0] != 'b')) continue;
            const size_t colon = item.find(':');
            if (colon == std::string::npos) continue;
            const int li = atoi(item.substr(1, colon - 1).c_str());
            if (li < 0 || li >= (int)m->layers.size()) continue;
            Layer &ly = m->layers[li];
            Igemm4Plan *pl = item[0] == 'b' ? &ly.bwd.p4 : (ly.spec.type == ALQ_CONVT ? &ly.fwd_all : (ly.fwd.empty() ? nullptr : &ly.fwd[0].p4));
            if (!pl) continue;
            const size_t fi = item.find("fic="), ei = item.find("epi=");
            if (fi != std::string::npos) pl->tune_fic = atoi(item.c_str() + fi + 4);
            if (ei != std::string::npos) pl->tune_epi = atoi(item.c_str() + ei + 4);
        }
    }
    {   // the conv in front of [conv_transpose without ReLU -> conv under a fused two-class head]: forward launch on the fp16x2 split
        // with derived input bounds (run_forward)
        const int nl = (int)m->layers.size();
        if (nl >= 4 && nl <= 16 && m->layers[nl - 1].fc_part2 && m->layers[nl - 2].spec.type == ALQ_CONV &&
            m->layers[nl - 3].spec.type == ALQ_CONVT && !m->layers[nl - 3].spec.relu && m->layers[nl - 4].spec.type == ALQ_CONV &&
            m->layers[nl - 4].spec.relu)
            m->f16_fwd_derived = 1 << (nl - 4);
        for (int i = 1; i + 1 < nl; ++i)      // enc2 of NET-C: its fused kernel (f3d.hip) contracts fp16 pairs under the first layer's measured maximum
            if (m->layers[i].f3f.ok && m->f16_fwd_derived) m->f16_fwd_derived |= 1 << i;
        if (m->sw.has_f16_derived_mask) m->f16_fwd_derived = m->sw.f16_derived_mask;      // (study: other forward launches on fp16 pairs, by layer bit)
    }
    *out = m;
    return ALQ_OK;
}

int alq_model_destroy(alq_model *m) {
    if (!m) return ALQ_OK;
    (void)hipStreamSynchronize(m->ctx->stream);
    for (void *p : m->allocs) (void)hipFree(p);
    delete m;
    return ALQ_OK;
}

int alq_model_num_param_layers(const alq_model *m) { return m ? m->L : ALQ_EINVAL; }
int alq_model_max_batch(const alq_model *m) { return m ? m->max_batch : ALQ_EINVAL; }

int alq_model_layer_out_elems(const alq_model *m, int layer_idx, int64_t *elems) {
    ALQ_REQUIRE(m && elems && layer_idx >= 0 && layer_idx < (int)m->layers.size(), ALQ_EINVAL, "bad layer index");
    *elems = m->layers[layer_idx].out.elems();
    return ALQ_OK;
}

int alq_forward(alq_model *m, const float *d_x, int N, float *d_post, int64_t *d_pred, float *d_feat,
                int feature_layer_idx) {
    ALQ_REQUIRE(m && d_x, ALQ_EINVAL, "alq_forward: null argument");
    ALQ_REQUIRE(N >= 0 && N <= m->max_batch, ALQ_EINVAL, "alq_forward: N=%d exceeds max_batch=%d", N, m->max_batch);
    if (N == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(m->ctx->device));
    ALQ_TRY(prepare_call(m, /*fisher=*/false));
    ALQ_TRY(run_forward(m, d_x, N, false, /*keep_all=*/d_feat != nullptr));
    if (m->dense) ALQ_TRY(dense_forward_head(m, d_x, N, d_post, d_pred, d_feat && feature_layer_idx == (int)m->layers.size() - 1));
    else ALQ_TRY(k_softmax(m->ctx, m->logits, m->nclass, N, d_post ? d_post : m->post, d_pred));
    if (d_feat) {
        ALQ_REQUIRE(feature_layer_idx >= 0 && feature_layer_idx < (int)m->layers.size(), ALQ_EINVAL, "bad feature layer");
        const View &v = m->layers[feature_layer_idx].out;
        ALQ_REQUIRE(v.cs == v.C, ALQ_EUNSUPPORTED, "feature layer is a concat slice");
        ALQ_HIP(hipMemcpyAsync(d_feat, v.p, (size_t)N * v.elems() * sizeof(float), hipMemcpyDeviceToDevice, m->ctx->stream));
    }
    return ALQ_OK;
}

int alq_fisher(alq_model *m, const float *d_x, int N, const float *d_p1_in, double diag_load, float *d_p1_out,
               double *d_g0, double *d_g1, double *d_A, double *d_trace, double *d_Asum) {
    ALQ_REFUSE_DENSE(m, "alq_fisher");
    ALQ_REQUIRE(m && d_x, ALQ_EINVAL, "alq_fisher: null argument");
    ALQ_REQUIRE(N >= 0 && N <= m->max_batch, ALQ_EINVAL, "alq_fisher: N=%d exceeds max_batch=%d", N, m->max_batch);
    ALQ_HIP(hipSetDevice(m->ctx->device));
    if (N == 0) {
        if (d_Asum) ALQ_HIP(hipMemsetAsync(d_Asum, 0, sizeof(double) * m->L * m->L, m->ctx->stream));
        return ALQ_OK;
    }
    struct SkipGuard {       // sampled profiling: only every prof_every-th pass records events
        alq_ctx *c;
        explicit SkipGuard(alq_ctx *ctx) : c(ctx) { c->prof_skip = c->prof_on && (c->prof_pass++ % c->prof_every) != 0; }
        ~SkipGuard() { c->prof_skip = false; }
    } guard(m->ctx);
    ALQ_TRY(prepare_call(m, /*fisher=*/true));
    ALQ_TRY(run_forward(m, d_x, N, true));
    ALQ_TRY(k_softmax(m->ctx, m->logits, m->nclass, N, m->post, nullptr));
    ALQ_TRY(run_backward(m, d_x, N));
    int nblocks = 0;
    ALQ_TRY(k_fisher_finalize(m->ctx, m->Spart, m->nslab, m->nslab_max, m->max_batch, m->S, m->L, m->sizes, m->post,
                              d_p1_in, N, diag_load, d_p1_out, d_g0, d_g1, d_A, d_trace, m->Apart, &nblocks));
    if (d_Asum) ALQ_TRY(k_reduce_Asum(m->ctx, m->Apart, nblocks, m->L * m->L, d_Asum));
    return ALQ_OK;
}

// rows of a resident pool -> the model's staging buffer (one 16-byte-wide copy kernel, no caller-side temporary)
static int stage_rows(alq_model *m, const float *d_pool, const int64_t *d_rows, int N) {
    ALQ_REQUIRE(d_pool && d_rows, ALQ_EINVAL, "null pool / row list");
    if (!m->x_stage) ALQ_TRY(m->dalloc(&m->x_stage, (size_t)m->max_batch * m->epp));
    return gather_rows_impl(m->ctx, d_pool, d_rows, N, m->epp, m->x_stage);
}

int alq_forward_rows(alq_model *m, const float *d_pool, const int64_t *d_rows, int N, float *d_post, int64_t *d_pred,
                     float *d_feat, int feature_layer_idx) {
    ALQ_REFUSE_DENSE(m, "alq_forward_rows");
    ALQ_REQUIRE(m != nullptr, ALQ_EINVAL, "alq_forward_rows: null model");
    ALQ_REQUIRE(N >= 0 && N <= m->max_batch, ALQ_EINVAL, "alq_forward_rows: N=%d exceeds max_batch=%d", N, m->max_batch);
    if (N == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(m->ctx->device));
    ALQ_TRY(stage_rows(m, d_pool, d_rows, N));
    return alq_forward(m, m->x_stage, N, d_post, d_pred, d_feat, feature_layer_idx);
}

int alq_fisher_rows(alq_model *m, const float *d_pool, const int64_t *d_rows, int N, const float *d_p1_in, double diag_load,
                    float *d_p1_out, double *d_g0, double *d_g1, double *d_A, double *d_trace, double *d_Asum) {
    ALQ_REFUSE_DENSE(m, "alq_fisher_rows");
    ALQ_REQUIRE(m != nullptr, ALQ_EINVAL, "alq_fisher_rows: null model");
    ALQ_REQUIRE(N >= 0 && N <= m->max_batch, ALQ_EINVAL, "alq_fisher_rows: N=%d exceeds max_batch=%d", N, m->max_batch);
    ALQ_HIP(hipSetDevice(m->ctx->device));
    if (N > 0) ALQ_TRY(stage_rows(m, d_pool, d_rows, N));
    return alq_fisher(m, N > 0 ? m->x_stage : d_pool, N, d_p1_in, diag_load, d_p1_out, d_g0, d_g1, d_A, d_trace, d_Asum);
}

int alq_model_debug_copy(alq_model *m, int layer_idx, int what, int N, float *d_out, int64_t *elems_out) {
    ALQ_REQUIRE(m && d_out && N >= 1 && N <= m->max_batch, ALQ_EINVAL, "alq_model_debug_copy: bad argument");
    ALQ_HIP(hipSetDevice(m->ctx->device));
    if (what == 4) {
        if (elems_out) *elems_out = (int64_t)N * m->L;
        return debug_f64_copy(m->ctx, m->S, (long long)N * m->L, d_out);
    }
    if (what == 5) {       // per (tile, wave) partials of the logit difference from the fused fc head (last pass)
        const Layer &head = m->layers.back();
        ALQ_REQUIRE(head.fc_part2 && m->last.fwd.head_fused, ALQ_EUNSUPPORTED, "the last pass did not run the fused fc head");
        const int ns = m->last.fwd.c3 ? 4 : head.fc_slices2;      // plane-sweep engine: one partial per (patch, wave)
        if (elems_out) *elems_out = (int64_t)N * ns;
        ALQ_HIP(hipMemcpyAsync(d_out, m->last.fwd.c3 ? head.c3_part : head.fc_part2, (size_t)N * ns * sizeof(float), hipMemcpyDeviceToDevice,
                               m->ctx->stream));
        return ALQ_OK;
    }
    if (what == 15 || what == 17 || what == 18) {
        // test hooks for the fp16-pair scales of the last pass (layer_idx ignored): 15 = the derived forward bounds [layers, N] (k_fwd_bounds),
        // 17 = the measured maxima of the network input [N], both as the floats whose bits the launches read; 18 = the static cotangent
        // bounds of the Fisher backward [layers] (bwd_bounds; -1 = unknown; N ignored)
        const int nl = (int)m->layers.size();
        if (what == 18) {
            ALQ_REQUIRE(m->last.call_fisher && m->last.bwd.nbounds == nl, ALQ_EUNSUPPORTED, "the last pass ran no Fisher backward sweep");
            float h[64];
            for (int i = 0; i < nl; ++i) h[i] = m->last.bwd.dout_bound[i] > 0.f ? m->last.bwd.dout_bound[i] : -1.f;
            if (elems_out) *elems_out = nl;
            ALQ_HIP(hipMemcpyAsync(d_out, h, (size_t)nl * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
            ALQ_HIP(hipStreamSynchronize(m->ctx->stream));
            return ALQ_OK;
        }
        if (what == 17) {
            ALQ_REQUIRE(m->last.fwd.v3f16 && m->in_amax, ALQ_EUNSUPPORTED, "the last pass measured no input maxima");
            if (elems_out) *elems_out = N;
            ALQ_HIP(hipMemcpyAsync(d_out, m->in_amax, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, m->ctx->stream));
            return ALQ_OK;
        }
        ALQ_REQUIRE((m->last.fwd.f16_derived || m->last.fwd.v3f16) && m->bound_all, ALQ_EUNSUPPORTED, "the last pass derived no forward bounds");
        if (elems_out) *elems_out = (int64_t)nl * N;
        ALQ_HIP(hipMemcpy2DAsync(d_out, (size_t)N * sizeof(float), m->bound_all, (size_t)m->max_batch * sizeof(float), (size_t)N * sizeof(float), nl,
                                 hipMemcpyDeviceToDevice, m->ctx->stream));
        return ALQ_OK;
    }
    ALQ_REQUIRE(layer_idx >= 0 && layer_idx < (int)m->layers.size(), ALQ_EINVAL, "bad layer index");
    const Layer &ly = m->layers[layer_idx];
    if (what == 16) {      // test hook: the per-patch maxima of the layer's output that the last forward pass asked its launch for [N]
        ALQ_REQUIRE(layer_idx < 64 && m->last.fwd.amax_asked[layer_idx] && ly.amax_fwd, ALQ_EUNSUPPORTED, "layer %d: the last pass measured no output maxima", layer_idx);
        if (elems_out) *elems_out = N;
        ALQ_HIP(hipMemcpyAsync(d_out, ly.amax_fwd, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, m->ctx->stream));
        return ALQ_OK;
    }
    if (what >= 6 && what <= 10) {
        // packed weights of a wide fc layer as raw bytes (test hook): 6 / 7 = bf16 triples / fp16 pairs of the forward Gemm, 8 / 9 = of the
        // backward Gemm; 10 = 4 words: w_exp of the forward and the backward plan, then the bits of bwd_l1 (fp64)
        ALQ_REQUIRE(ly.spec.type == ALQ_FC && ly.fwd.size() == 1 && ly.fwd[0].pfc.ok && ly.weights_set, ALQ_EUNSUPPORTED, "layer %d has no streaming-GEMM weights", layer_idx);
        if (what == 10) {
            int32_t wd[4] = {ly.fwd[0].pfc.w_exp, ly.bwd.pfc.w_exp, 0, 0};
            std::memcpy(&wd[2], &ly.bwd_l1, 8);
            if (elems_out) *elems_out = 4;
            ALQ_HIP(hipMemcpyAsync(d_out, wd, 16, hipMemcpyHostToDevice, m->ctx->stream));
            ALQ_HIP(hipStreamSynchronize(m->ctx->stream));
            return ALQ_OK;
        }
        const FcGemmPlan &pl = what <= 7 ? ly.fwd[0].pfc : ly.bwd.pfc;
        const void *src = (what & 1) ? pl.d_W16 : pl.d_W;
        ALQ_REQUIRE(pl.ok && src, ALQ_EUNSUPPORTED, "layer %d: this form is not packed", layer_idx);
        const int64_t e = (int64_t)pl.K * pl.N * ((what & 1) ? 2 : 3) / 2;      // 16-bit pieces in 4-byte words
        if (elems_out) *elems_out = e;
        ALQ_HIP(hipMemcpyAsync(d_out, src, (size_t)e * 4, hipMemcpyDeviceToDevice, m->ctx->stream));
        return ALQ_OK;
    }
    if (what >= 11 && what <= 13) {
        // test hooks for the kernels that write these next to the activation: 11 = channel sums of the layer's output (floats),
        // 12 = the sign field (View::sg) of the rows its output lies in, 13 = a pool layer's arg-max bytes; 12 / 13 as raw bytes
        if (what == 11) {
            ALQ_REQUIRE(ly.osum && m->last.call_fisher, ALQ_EUNSUPPORTED, "layer %d: no channel sums of its output in the last pass", layer_idx);
            if (elems_out) *elems_out = (int64_t)N * ly.out.vox();
            ALQ_HIP(hipMemcpyAsync(d_out, ly.osum, (size_t)N * ly.out.vox() * sizeof(float), hipMemcpyDeviceToDevice, m->ctx->stream));
            return ALQ_OK;
        }
        if (what == 12) {      // cs / 4 bytes per voxel as they lie in memory: the layer's own are the C / 4 from byte c0 / 4 of each
            const View &v = ly.out;
            ALQ_REQUIRE(v.sg && m->last.fwd.signs_ready[layer_idx] && ((v.C | v.cs | v.c0) & 3) == 0 && ((int64_t)N * v.vox() * v.cs) % 16 == 0, ALQ_EUNSUPPORTED,
                        "layer %d: no sign field of its output in the last pass", layer_idx);
            if (elems_out) *elems_out = (int64_t)N * v.vox() * v.cs / 16;
            ALQ_HIP(hipMemcpyAsync(d_out, v.sg, (size_t)N * v.vox() * v.cs / 4, hipMemcpyDeviceToDevice, m->ctx->stream));
            return ALQ_OK;
        }
        ALQ_REQUIRE(ly.spec.type == ALQ_POOL && ly.argmax && ((int64_t)N * ly.out.vox() * ly.out.C) % 4 == 0, ALQ_EUNSUPPORTED, "layer %d has no arg-max field", layer_idx);
        if (elems_out) *elems_out = (int64_t)N * ly.out.vox() * ly.out.C / 4;
        ALQ_HIP(hipMemcpyAsync(d_out, ly.argmax, (size_t)N * ly.out.vox() * ly.out.C, hipMemcpyDeviceToDevice, m->ctx->stream));
        return ALQ_OK;
    }
    if (what == 14) {      // test hook: the sign bytes a two-class head keeps of its input in a Fisher pass, as raw bytes
        ALQ_REQUIRE(ly.spec.type == ALQ_FC && ly.fc_maskbits && m->last.call_fisher && ((int64_t)N * ly.F) % 16 == 0, ALQ_EUNSUPPORTED,
                    "layer %d: no sign bytes of its input in the last pass", layer_idx);
        if (elems_out) *elems_out = (int64_t)N * ly.F / 16;
        ALQ_HIP(hipMemcpyAsync(d_out, ly.fc_maskbits, (size_t)N * ly.F / 4, hipMemcpyDeviceToDevice, m->ctx->stream));
        return ALQ_OK;
    }
    if (what == 0 || what == 1) {
        // the last conv under a fused fc head: a Fisher pass stores neither its output nor the cotangent of it
        const Layer &head = m->layers.back();
        ALQ_REQUIRE(!(layer_idx + 2 == (int)m->layers.size() && head.spec.type == ALQ_FC &&
                      (what == 0 ? m->last.fwd.head_fused
                                 : (m->last.call_fisher && head.fc_maskbits != nullptr && two_slot_allowed()))),
                    ALQ_EUNSUPPORTED, "layer %d: this tensor is not materialised in a Fisher pass (fc head fused into the layer: "
                    "create the model under ALQ_NO_FC_BITS=1 to keep it)", layer_idx);
        const View &v = what == 0 ? ly.out : ly.dout;
        if (elems_out) *elems_out = (int64_t)N * v.elems();
        return debug_view_copy(m->ctx, v, N, d_out);
    }
    ALQ_REQUIRE(ly.pidx >= 0 && !ly.dense_head && (what == 2 || what == 3), ALQ_EINVAL, "layer has no channel-sum fields");
    const bool isfc = ly.spec.type == ALQ_FC;
    const int64_t e = (int64_t)N * (isfc ? 1 : (what == 2 ? ly.in.vox() : ly.out.vox()));
    if (elems_out) *elems_out = e;
    ALQ_HIP(hipMemcpyAsync(d_out, what == 2 ? ly.asum : ly.dsum, e * sizeof(float), hipMemcpyDeviceToDevice,
                           m->ctx->stream));
    return ALQ_OK;
}

int alq_debug_rowmax_abs(alq_ctx *ctx, const float *d_x, int N, int64_t K, uint32_t *d_out) {
    ALQ_REQUIRE(ctx && d_x && d_out && N >= 1 && K >= 1, ALQ_EINVAL, "alq_debug_rowmax_abs: bad argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    return k_rowmax_abs(ctx, d_x, N, (long long)K, d_out);
}

int alq_debug_fwd_bounds(alq_ctx *ctx, const uint32_t *d_amax0, int N, int stride, const float *L, const float *B, const int32_t *src2,
                         int nl, int from_input, uint32_t *d_bound_all) {
    ALQ_REQUIRE(ctx && d_amax0 && d_bound_all && L && B && src2 && N >= 1 && stride >= N && nl >= 1 && nl <= 16, ALQ_EINVAL,
                "alq_debug_fwd_bounds: bad argument");
    FwdBoundsArgs a;
    a.nl = nl;
    a.from_input = from_input ? 1 : 0;
    for (int k = 0; k < nl; ++k) {
        ALQ_REQUIRE(src2[k] >= -1 && src2[k] < k, ALQ_EINVAL, "alq_debug_fwd_bounds: src2[%d] = %d names no earlier layer", k, src2[k]);
        a.L[k] = L[k]; a.B[k] = B[k]; a.src2[k] = src2[k];
    }
    ALQ_HIP(hipSetDevice(ctx->device));
    return k_fwd_bounds(ctx, d_amax0, N, stride, a, d_bound_all);
}

int alq_model_engine_info(alq_model *m, int what) {
    ALQ_REQUIRE(m, ALQ_EINVAL, "alq_model_engine_info: bad argument");
    switch (what) {      // include/alq.h documents every index
        case ALQ_INFO_SUBNORMALS_OK:
            ALQ_HIP(hipSetDevice(m->ctx->device));
            return c3d_subnormals_ok(m->ctx);
        case ALQ_INFO_C3D_FWD: return m->last.fwd.c3 ? 1 : 0;
        case ALQ_INFO_C3D_BWD: return m->last.bwd.c3_bwd ? 1 : 0;
        case ALQ_INFO_C3D_ONE_ACC:
            for (const Layer &ly : m->layers)
                if (ly.c3f.ok) return ly.c3f.oneacc;
            return 0;
        case ALQ_INFO_FLIP_OVERFLOW: {      // marked groups beyond their list segment since the model was created
            ALQ_HIP(hipSetDevice(m->ctx->device));
            if (!m->flip_overflow) return 0;
            unsigned h = 0;
            ALQ_HIP(hipMemcpyAsync(&h, m->flip_overflow, sizeof(unsigned), hipMemcpyDeviceToHost, m->ctx->stream));
            ALQ_HIP(hipStreamSynchronize(m->ctx->stream));
            return h > 0x7fffffffu ? 0x7fffffff : (int)h;
        }
        case ALQ_INFO_F16_DERIVED: return m->last.fwd.f16_derived ? 1 : 0;
        case ALQ_INFO_T3D_FWD: return m->last.fwd.t3f;
        case ALQ_INFO_T3D_BWD: return m->last.bwd.t3b;
        case ALQ_INFO_E3D_BWD: return m->last.bwd.e3b;
        case ALQ_INFO_D3D_FWD: return m->last.fwd.d3f;
        case ALQ_INFO_D3D_BWD: return m->last.bwd.d3b;
        case ALQ_INFO_F3D_FWD: return m->last.fwd.f3f;
        case ALQ_INFO_C3D_BWD_FORM: return m->last.bwd.c3_bwd ? m->sw.c3_bwd_rows : 0;
        case ALQ_INFO_HOST_PACK_ELEMS: return m->host_pack_elems > 0x7fffffffll ? 0x7fffffff : (int)m->host_pack_elems;      // saturates
        case ALQ_INFO_LSUM: return m->last.lsum;
        case ALQ_INFO_DCP_FORM: return m->last.fwd.dcp;
        case ALQ_INFO_E3D_BWD_FORM: return m->last.bwd.e3b_form;
        case ALQ_INFO_C3D_BWD_WAVES: return m->last.bwd.c3_bwd ? (m->sw.c3_bwd_rows == 7 ? m->sw.c3_bwd_waves : 1) : 0;
        case ALQ_INFO_C3D_BWD_GRID: return m->last.bwd.c3_bwd ? m->last.bwd.c3b_grid : 0;
        default: break;      // 4 and 18 are unused
    }
    set_error("alq_model_engine_info: bad argument");
    return ALQ_EINVAL;
}

int alq_debug_set(int key, int value) {
    ALQ_REQUIRE(key >= 0 && key < ALQ_NKNOBS, ALQ_EINVAL, "alq_debug_set: bad key");
    // an explicit override of every model's snapshot; 0 restores "whatever the model was created with" for the keys
    // whose environment default is 0 (all of them unless the ALQ_* diagnostics variables were set at creation)
    g_knob_override[key] = value > 0 ? value : -1;
    g_dbg_knobs[key] = value;
    return ALQ_OK;
}

int alq_debug_set_stamp_buffer(void *d_buf) {
    g_igemm2_dbg = reinterpret_cast<unsigned long long *>(d_buf);
    return ALQ_OK;
}

}  // extern "C"
