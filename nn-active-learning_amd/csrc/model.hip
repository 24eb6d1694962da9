// Model plan + orchestration behind the C ABI: shapes, activation / cotangent workspaces (concat skips = channel slices of
// one buffer), engine routing, the forward pass and the fused Fisher backward sweep, with their entry points and the debug hooks.
// The structures are in model_types.h; weights reach the engines' packed forms in weights.hip; the general gradient path is grads.hip,
// everything that takes no model (contexts, profiling, the pass-through entry points) ctx.hip.
#include <algorithm>
#include <cmath>
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
enum GemmRoute { ROUTE_DIRECT, ROUTE_FCGEMM, ROUTE_IGEMM4, ROUTE_IGEMM3, ROUTE_IGEMM2, ROUTE_IGEMM };
static GemmRoute gemm_route(const Gemm &g, const View &in, const View &out, int accumulate, const Igemm2Fuse *fuse) {
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

// [layer][max_batch] derived per-patch output bounds, allocated by the first pass that wants them
static int ensure_bounds(alq_model *m) {
    if (m->bound_all) return ALQ_OK;
    const int nl = (int)m->layers.size();
    ALQ_TRY(m->dalloc(&m->bound_all, (size_t)nl * m->max_batch));
    for (int k = 0; k < nl; ++k) m->layers[k].bound_fwd = m->bound_all + (size_t)k * m->max_batch;
    return ALQ_OK;
}

// per-(patch, tile) maxima of one launch: at least `len` per patch
static int ensure_amax_tiles(alq_model *m, size_t len) {
    if (len <= m->amax_tiles_len) return ALQ_OK;
    ALQ_TRY(m->dalloc(&m->amax_tiles, (size_t)m->max_batch * len));
    m->amax_tiles_len = len;
    return ALQ_OK;
}

// every layer's out = in * L + B (and its second input, if any) for k_fwd_bounds
static FwdBoundsArgs fwd_bounds_args(const alq_model *m) {
    const int nl = (int)m->layers.size();
    FwdBoundsArgs ba;
    ba.nl = nl;
    for (int k = 0; k < nl && k < 16; ++k) {
        const Layer &lk = m->layers[k];
        const bool par = lk.pidx >= 0 && lk.spec.type != ALQ_FC;
        ba.L[k] = par ? lk.out_l1 : 1.f;
        ba.B[k] = par ? lk.out_bmax : 0.f;
        ba.src2[k] = lk.spec.skip_src;
    }
    return ba;
}

// ---- forward routes: "engine X runs layer i in this pass".  `prod` / `cons`: the layers that report / read per-patch input maxima
// (run_forward); `fuse`: the launch's epilogue request as far as the pass has filled it, or null; `light`: a forward-only pass that keeps no activation

// layer i = first conv, fused with the pool behind it (direct_conv_pool_launch)
static bool dcp_applies(const alq_model *m, int i, const DropSpec *drop) {
    if (i != 0 || m->layers.size() < 2) return false;
    const Layer &ly = m->layers[0], &nx = m->layers[1];
    const alq_layer_t &sp = ly.spec;
    const View &in = ly.in;
    return ly.spec.type == ALQ_CONV && nx.spec.type == ALQ_POOL && ly.fwd[0].pd.ok && ly.fwd[0].pd.d_W && in.C == 1 && in.cs == 1 &&
           sp.cout == 8 && sp.k[0] == 3 && sp.k[1] == 3 && sp.k[2] == 3 && ly.lo[0] == 1 && ly.lo[1] == 1 && ly.lo[2] == 1 &&
           nx.spec.k[0] == 2 && nx.spec.k[1] == 2 && nx.spec.k[2] == 2 && nx.lo[0] == 0 && nx.lo[1] == 0 && nx.lo[2] == 0 &&
           in.D % 2 == 0 && in.H % 2 == 0 && in.W % 2 == 0 && nx.out.D * 2 == in.D && nx.out.H * 2 == in.H &&
           nx.out.W * 2 == in.W && ((ly.out.cs | ly.out.c0 | nx.out.cs | nx.out.c0) & 3) == 0 && !g_dbg_knobs[KNOB_NO_CONV_POOL] &&
           !(drop && (drop->on(0) || drop->on(1)));       // a dropped layer 0 output cannot share a kernel with the pool
}

// flip-safe head: only where the launch will contract with the fp16x2 split (input maxima known) and the
// sign bits are wanted (Fisher pass); stride-1 conv on one dense tensor or a split concat of two
static bool flipfix_applies(const alq_model *m, const Layer &ly, const Layer &nx, const View &in, const Igemm2Fuse &fz, bool with_sums) {
    const alq_layer_t &sp = ly.spec;
    return with_sums && fz.fc_bits && fz.in_amax && !g_no_f16x2 && !m->sw.no_flipfix && ly.d_W32 && ly.fwd_l1 > 0.f &&
           sp.s[0] == 1 && sp.s[1] == 1 && sp.s[2] == 1 && in.c0 == 0 && nx.F % 64 == 0 &&      // (whole 16-byte words of sign bytes per patch)
           ((in.split == 0 && in.cs == in.C) || (in.split > 0 && in.cs == in.split && in.C == 2 * in.split));
}

// the conv under the fused head on the plane-sweep engine (c3d.hip): where its geometry applies and both per-patch input maxima are known
static bool c3d_fwd_applies(const alq_model *m, const Layer &ly, const Layer &nx, const Igemm2Fuse &fz) {
    return ly.c3f.ok && ly.c3f.d_W && nx.c3_part && fz.in_amax && fz.in_amax2 && !g_no_f16x2 && !m->sw.no_c3d;
}

// the row-sweep engine (d3d.hip) where its geometry applies, both per-patch input bounds are known and nothing but the tensor,
// its channel sums and its sign field is wanted
// (round 6: forward-only passes too - the entropy filter over a pool is most of a query round - without sums / sign field)
static bool d3d_fwd_applies(const alq_model *m, int i, const View &in, const Igemm2Fuse *fuse, const std::vector<char> &prod, bool with_sums,
                            bool light, const DropSpec *drop) {
    const Layer &ly = m->layers[i];
    return fuse && ly.d3f.ok && ly.d3f.d_Whi && !m->sw.no_d3d && fuse->in_amax && fuse->in_amax2 && !prod[i] && !g_no_f16x2 && two_slot_allowed() &&
           ((with_sums && fuse->osumA) || (light && !m->sw.no_light_kernels)) && in.split == 16 && !(drop && drop->on(i));
}

// enc2 + the pool behind it in one launch (f3d.hip): fp16 pairs under the first layer's measured maximum
static bool f3d_fwd_applies(const alq_model *m, int i, const View &in, const Igemm2Fuse *fuse, const std::vector<char> &prod,
                            const std::vector<char> &cons, bool with_sums, bool light, const DropSpec *drop) {
    const Layer &ly = m->layers[i];
    const Layer *nx = i + 1 < (int)m->layers.size() ? &m->layers[i + 1] : nullptr;
    return fuse && ly.f3f.ok && ly.f3f.d_Whi && !m->sw.no_f3d && cons[i] == 2 && fuse->in_amax && !fuse->in_amax2 && !prod[i] && !g_no_f16x2 && two_slot_allowed() &&
           ((with_sums && fuse->osumA) || (light && !m->sw.no_light_kernels)) && ly.spec.relu && in.split == 0 && !(drop && (drop->on(i) || drop->on(i + 1))) && nx && nx->spec.type == ALQ_POOL &&
           nx->spec.k[0] == 2 && nx->spec.k[1] == 2 && nx->spec.k[2] == 2 && nx->lo[0] == 0 && nx->lo[1] == 0 && nx->lo[2] == 0 && nx->out.D == 8 && nx->out.H == 8 &&
           nx->out.W == 8 && nx->out.C == 16 && nx->out.cs == 16 && nx->out.c0 == 0 && !nx->out.split && nx->argmax && !prod[i + 1];
}

// the row-sweep engine (t3d.hip): bf16 triples like the two-slot launch it replaces, nothing but the tensor, its channel
// sums and its per-patch maximum to produce (no ReLU behind a conv_transpose of this geometry: no sign field)
static bool t3d_fwd_applies(const alq_model *m, int i, const std::vector<char> &prod, const std::vector<char> &cons, bool with_sums,
                            const DropSpec *drop) {
    const Layer &ly = m->layers[i];
    return ly.t3f.ok && ly.t3f.d_W && !m->sw.no_t3d && !g_dbg_knobs[KNOB_NO_FWD_FUSE] && two_slot_allowed() && !cons[i] && !ly.spec.relu &&
           !(drop && drop->on(i)) && (!with_sums || ly.osum) && !(ly.t3f.kind == 8 && prod[i]);
}

// ------------------------------------------------------------------------------------------
// keep_all (forward-only calls): every activation stays readable (a feature layer was asked for); otherwise the fc
// head of a two-class net is fused into the last conv in forward-only calls too (no channel sums, no sign bytes)
int run_forward(alq_model *m, const float *d_x, int N, bool with_sums, bool keep_all, const DropSpec *drop) {
    alq_ctx *ctx = m->ctx;
    const int nl = (int)m->layers.size();
    bool skip_next = false;      // this layer's outputs were produced by the previous layer's kernel
    bool fc_head_fused = false;  // the logits partials of the fc head came out of the previous conv's epilogue
    bool c3_head = false;        // ... of the plane-sweep engine: one partial per (patch, wave), the head's input sum likewise
    m->last.fwd = {};
    // A conv / conv_transpose launch contracts with the fp16x2 split if it knows max |x| per patch of (every part of)
    // its input ahead of time: the launches that produce those tensors report them (`prod`), the consumers (`cons`)
    // read one scale per tile.  Producers: the first conv + pool kernel and one-patch-per-tile igemm4 launches.
    const bool no16 = g_no_f16x2 != 0;
    std::vector<char> prod(nl, 0), cons(nl, 0);
    const bool light = !with_sums && !keep_all;       // forward-only: fuse objects only for the launches of the fused head
    if ((with_sums || light) && !no16 && !g_dbg_knobs[KNOB_NO_FWD_FUSE] && two_slot_allowed()) {
        auto prod_ok = [&](int p) {
            if (p < 0) return false;
            const Layer &l = m->layers[p];
            if (p == 0 && dcp_applies(m, 0, drop)) return true;
            if (!l.osum) return false;
            if (l.spec.type == ALQ_CONV) return l.fwd[0].p4.ok && !l.fwd[0].pd.ok && !l.fwd[0].pfc.ok && l.fwd[0].p4.a.PT == 1;
            if (l.spec.type == ALQ_CONVT) return l.fwd_all.ok && l.fwd_all.a.PT == 1;
            return false;
        };
        size_t need = 0;
        for (int j = 1; j < nl; ++j) {
            const Layer &l = m->layers[j];
            if (l.dense_head) continue;
            const Igemm4Plan *pl = l.spec.type == ALQ_CONV ? &l.fwd[0].p4 : (l.spec.type == ALQ_CONVT ? &l.fwd_all : nullptr);
            if (!pl || !pl->ok || !pl->d_W16 || pl->multi || pl->a.PT != 1 || !l.osum) continue;
            if (l.spec.type == ALQ_CONV && (l.fwd[0].pd.ok || l.fwd[0].pfc.ok)) continue;
            // Forward launches: only the conv under the fused fc head.  The fp16x2 split rounds at 2^-22 instead of 2^-24; in
            // the forward pass that noise reaches ReLU decisions (measured: with dec1 or up1 on the split one patch in ~12
            // had a ReLU input of a later layer land on the other side of zero, moving two layer scores by 1 % - the same
            // event any two fp32 implementations produce, four times as often).  The head conv has one ReLU behind it;
            // backward launches have none (the masks are fixed by then), so they take the split wherever a variant exists.
            const int s_ = l.spec.skip_src;
            // ... and the conv whose output reaches the head conv through the (linear) conv_transpose only (NET-C's dec1): its
            // input maxima are not measured (an epilogue in two producer launches cost what the split gave) but DERIVED per patch
            // from the first layer's measured maximum through the layers' L1 norms (k_fwd_bounds) - the fp16 pairs keep their 22
            // bits under a bound that is loose by orders of magnitude.  Measured (profiles/r04al_*): bench +2.6 % same-box, launch
            // 1148 -> 875 us; on a 2000-patch batch against the exact-fp32 engine 129 patches with a flipped fragile unit instead
            // of 115 (bf16x3 everywhere: 109; each engine has its own set against fp64).  Default since round 5 (the round-4
            // verdict: a faster, equally accurate path is not withheld for an accounting ratio); ALQ_NO_F16_DERIVED=1 is the A/B arm.
            if (m->sw.f16_fwd_mask < 0 && !m->sw.no_f16_derived && nl <= 16 && ((m->f16_fwd_derived >> j) & 1) && l.spec.type == ALQ_CONV && dcp_applies(m, 0, drop) &&
                (s_ >= 0) == (l.in.split != 0) && !(drop && drop->layers)) {
                cons[j] = 2;
                prod[0] = 1;
                continue;
            }
            if (!(j == nl - 2 && m->layers[nl - 1].fc_part2 && l.spec.type == ALQ_CONV) && m->sw.f16_fwd_mask < 0) continue;
            if (l.spec.type == ALQ_CONVT && !pl->fic) continue;                 // MULTI has no F16 variant
            if (!prod_ok(j - 1) || (s_ >= 0 && !prod_ok(s_))) continue;
            if ((s_ >= 0) != (l.in.split != 0)) continue;                       // two parts <-> a split view
            if (m->sw.f16_fwd_mask >= 0 && !((m->sw.f16_fwd_mask >> j) & 1)) continue;      // diagnostics: consumers by layer bit
            cons[j] = 1; prod[j - 1] = 1;
            if (s_ >= 0) prod[s_] = 1;
        }
        for (int p = 0; p < nl; ++p) {
            if (!prod[p]) continue;
            Layer &l = m->layers[p];
            if (!l.amax_fwd) ALQ_TRY(m->dalloc(&l.amax_fwd, (size_t)m->max_batch));
            if (l.spec.type == ALQ_CONV && !(p == 0 && dcp_applies(m, 0, drop))) need = std::max(need, (size_t)l.fwd[0].p4.a.tpg * 4);
            if (l.spec.type == ALQ_CONVT) need = std::max(need, (size_t)l.fwd_all.a.tpg * (l.fwd_all.multi ? l.fwd_all.a.ngr : 1) * 4);
            if (l.spec.type == ALQ_CONVT && l.t3f.ok) need = std::max(need, (size_t)16);      // row-sweep engine: one maximum per input plane
        }
        ALQ_TRY(ensure_amax_tiles(m, need));
    }
    bool any_derived = false;
    for (int j = 0; j < nl; ++j) any_derived = any_derived || cons[j] == 2;
    m->last.fwd.f16_derived = any_derived;
    if (any_derived) ALQ_TRY(ensure_bounds(m));
    // Forward launches that stay on igemm3 (no two-slot plan: NET-B's conv1 .. conv3) on fp16 pairs, one scale per patch: the
    // measured maximum of every patch of the network input, pushed through the layers' L1 norms, bounds every layer's input.
    // Fisher passes and forward-only passes; not the passes that keep every activation for training, not under dropout.
    const bool v3f16 = m->v3_fwd_f16 && (with_sums || light) && !no16 && !drop && !any_derived && !dcp_applies(m, 0, drop) && nl <= 16 &&
                       !g_dbg_knobs[KNOB_NO_FWD_FUSE] && two_slot_allowed() && m->layers[0].in.split == 0 && m->layers[0].in.cs == m->layers[0].in.C;
    if (v3f16) {
        if (!m->in_amax) ALQ_TRY(m->dalloc(&m->in_amax, (size_t)m->max_batch));
        ALQ_TRY(ensure_bounds(m));
        ALQ_TRY(k_rowmax_abs(ctx, d_x, N, (long long)m->layers[0].in.vox() * m->layers[0].in.C, m->in_amax));
        FwdBoundsArgs ba = fwd_bounds_args(m);
        ba.from_input = 1;
        ALQ_TRY(k_fwd_bounds(ctx, m->in_amax, N, m->max_batch, ba, m->bound_all));
    }
    auto take_amax = [&](Igemm2Fuse &fz, int j) {      // the input maxima of consumer j
        if (!cons[j]) return;
        const bool dv = cons[j] == 2;
        fz.in_amax = dv ? m->layers[j - 1].bound_fwd : m->layers[j - 1].amax_fwd;
        if (m->layers[j].spec.skip_src >= 0) {
            const Layer &sl = m->layers[m->layers[j].spec.skip_src];
            fz.in_amax2 = dv ? sl.bound_fwd : sl.amax_fwd;
        }
    };
    for (Layer &l : m->layers) l.signs_ready = false;
    // Sign fields (View::sg): in a Fisher pass a forward launch of the two-slot engine also writes one byte per 4 channels
    // with the signs of its ReLU'd output; the backward launches read those instead of the fp32 activations (1/16 of the bytes)
    for (int i = 0; i < nl; ++i) {
        Layer &ly = m->layers[i];
        ALQ_REQUIRE(ly.pidx < 0 || ly.weights_set, ALQ_EINVAL, "weights of parameterised layer %d not set", ly.pidx);
        if (ly.dense_head) break;      // the caller runs the head (dense_forward_head): posteriors straight from its input
        if (skip_next) { skip_next = false; continue; }
        View in = ly.in;
        if (i == 0) in.p = const_cast<float *>(d_x);
        // channel sums of every spatial layer's output ride on the producing kernel's epilogue when it
        // can; they are the `asum` fields of the layers that consume it
        Igemm2Fuse fz;
        fz.osumA = with_sums ? ly.osum : nullptr;
        const bool head_conv = i + 2 == nl && m->layers[nl - 1].fc_part2 && ly.spec.type == ALQ_CONV;
        const bool light_here = light && (prod[i] || cons[i] || head_conv);
        const Igemm2Fuse *fuse = ((with_sums || light_here) && ly.osum && !g_dbg_knobs[KNOB_NO_FWD_FUSE]) ? &fz : nullptr;
        bool fused = false;
        switch (ly.spec.type) {
            case ALQ_CONV: {
                // first conv + the pool behind it in one kernel (one input channel, 3x3x3 -> 8, 2x2x2 windows)
                Layer *nx = i + 1 < nl ? &m->layers[i + 1] : nullptr;
                const alq_layer_t &sp = ly.spec;
                if (dcp_applies(m, i, drop)) {
                    if (prod[i]) ALQ_HIP(hipMemsetAsync(ly.amax_fwd, 0, (size_t)N * sizeof(unsigned), ctx->stream));
                    // (the sign field of the full-resolution output: what the last conv's backward launch reads as its ReLU mask)
                    const bool sg_here = with_sums && !m->sw.no_signs && !m->sw.no_signs0 && sp.relu && ly.out.sg != nullptr;
                    ALQ_TRY(direct_conv_pool_launch(ctx, ly.fwd[0].pd.d_W, in, ly.out, nx->out, ly.d_bias, sp.relu, nx->argmax,
                                                    with_sums ? ly.osum : nullptr, with_sums ? nx->osum : nullptr, N,
                                                    ly.fwd[0].pd.flops_per_patch, prod[i] ? ly.amax_fwd : nullptr,
                                                    sg_here ? ly.out.sg : nullptr, (sg_here && nx->out.sg) ? nx->out.sg : nullptr));
                    m->last.fwd.dcp = g_dcp_last_form;
                    ly.signs_ready = sg_here;
                    nx->signs_ready = sg_here && nx->out.sg != nullptr;      // (the pool's output: sign of the window maximum)
                    if (any_derived)      // per-patch bounds on every later layer's output from this layer's measured maximum
                        ALQ_TRY(k_fwd_bounds(ctx, ly.amax_fwd, N, m->max_batch, fwd_bounds_args(m), m->bound_all));
                    fused = true;
                    skip_next = true;
                    break;
                }
                if (fuse && nx && i + 2 == nl && nx->fc_part2 && two_slot_allowed()) {
                    // the fc head is this layer's only consumer in a Fisher pass: logits partials + sign bytes from the
                    // epilogue, the tensor itself is not stored
                    fz.fc_W = nx->fc_wv; fz.fc_F = nx->F; fz.fc_part = nx->fc_part2; fz.fc_bits = with_sums ? nx->fc_maskbits : nullptr;
                    take_amax(fz, i);
                    const bool flipfix = flipfix_applies(m, ly, *nx, in, fz, with_sums);
                    if (flipfix) {
                        if (!m->flip_list) {
                            m->flip_cap = flip_list_len(m->max_batch);      // kernels.hip: per-patch segments of FLIP_PER_BLOCK slots
                            ALQ_TRY(m->dalloc(&m->flip_cnt, (size_t)flip_segments(m->max_batch)));
                            ALQ_TRY(m->dalloc(&m->flip_list, (size_t)m->flip_cap));
                            ALQ_TRY(m->dalloc(&m->flip_overflow, (size_t)1));
                            ALQ_HIP(hipMemsetAsync(m->flip_overflow, 0, sizeof(unsigned), ctx->stream));
                        }
                        fz.flip_cnt = m->flip_cnt; fz.flip_list = m->flip_list; fz.flip_cap = m->flip_cap; fz.flip_l1 = ly.fwd_l1; fz.flip_bias_nonzero = ly.out_bmax > 0.f;
                    }
                    c3_head = c3d_fwd_applies(m, ly, *nx, fz);
                    if (c3_head)
                        ALQ_TRY(c3d_fwd_launch(ctx, ly.c3f, in, ly.d_bias, N, fz.in_amax, fz.in_amax2, nx->fc_wv, nx->c3_part,
                                               with_sums ? nx->c3_asum : nullptr, reinterpret_cast<unsigned char *>(fz.fc_bits),
                                               flipfix ? std::ldexp(ly.fwd_l1, -24) : 0.f));
                    else
                        ALQ_TRY(igemm4_launch(ctx, ly.fwd[0].p4, in, ly.out, ly.d_bias, ly.spec.relu, 0, N, PROF_IGEMM3_FWD, &fz));
                    if (flipfix)
                        ALQ_TRY(k_flip_fix(ctx, m->flip_list, m->flip_cnt, m->flip_cap, N, in.p, in.split ? in.p + in.delta : nullptr,
                                           in.split ? in.split : in.C, in.split ? in.C - in.split : 0, in.D, in.H, in.W, sp.k[0], sp.k[1], sp.k[2],
                                           ly.lo[0], ly.lo[1], ly.lo[2], ly.d_W32, ly.d_bias, sp.cout,
                                           reinterpret_cast<unsigned char *>(nx->fc_maskbits), nx->F, m->flip_overflow));
                    fused = true;
                    fc_head_fused = true;
                    m->last.fwd.head_fused = true;
                    m->last.fwd.c3 = c3_head;
                    break;
                }
                if (fuse) take_amax(fz, i);
                if (d3d_fwd_applies(m, i, in, fuse, prod, with_sums, light, drop)) {
                    const bool sgd = with_sums && !m->sw.no_signs && ly.spec.relu && ly.out.sg;
                    ALQ_TRY(d3d_fwd_launch(ctx, ly.d3f, N, in.p, in.p + in.delta, fz.in_amax, fz.in_amax2, ly.d_bias, ly.spec.relu ? 1 : 0, ly.out.p,
                                           sgd ? ly.out.sg : nullptr, fz.osumA));
                    ly.signs_ready = sgd;
                    fused = true;
                    m->last.fwd.d3f = 1;
                    break;
                }
                if (f3d_fwd_applies(m, i, in, fuse, prod, cons, with_sums, light, drop)) {
                    const bool sgd = with_sums && !m->sw.no_signs && ly.out.sg;
                    ALQ_TRY(f3d_fwd_launch(ctx, ly.f3f, N, in.p, fz.in_amax, ly.d_bias, ly.out.p, sgd ? ly.out.sg : nullptr, fz.osumA, nx->out.p, nx->argmax,
                                           with_sums ? nx->osum : nullptr));
                    ly.signs_ready = sgd;
                    nx->signs_ready = false;
                    fused = true;
                    skip_next = true;
                    m->last.fwd.f3f = 1;
                    break;
                }
                if (fuse && prod[i]) fz.out_amax = m->amax_tiles;
                if (!ly.fwd_co.empty() && !prod[i] && !cons[i] && two_slot_allowed()) {
                    // a wide conv as launches over slices of its output channels (no epilogue fusion: channel sums and ReLU masks the plain way)
                    // (round 6) with per-patch bounds on the input at hand (v3f16: igemm3's forward launches above this layer asked for
                    // them) the slices take the two-slot engine's fp16-pair form too: one scale per patch, three products
                    Igemm2Fuse sz;
                    const bool s16 = v3f16 && i >= 1 && in.split == 0 && ly.spec.skip_src < 0 && !m->sw.no_co_split_f16;
                    if (s16) sz.in_amax = m->layers[i - 1].bound_fwd;
                    for (size_t j = 0; j < ly.fwd_co.size(); ++j) {
                        View oj = ly.out;
                        oj.c0 = ly.out.c0 + (int)j * ly.fwd_co_w;
                        oj.C = ly.fwd_co_w;
                        bool f1 = false;
                        ALQ_TRY(gemm_launch(ctx, ly.fwd_co[j], in, oj, ly.d_bias + j * ly.fwd_co_w, ly.spec.relu, 0, N, PROF_IGEMM_FWD, s16 ? &sz : nullptr, &f1));
                    }
                    fused = false;
                    ly.signs_ready = false;
                    break;
                }
                const bool sg_here = with_sums && fuse && !m->sw.no_signs && ly.spec.relu && ly.out.sg && gemm_route(ly.fwd[0], in, ly.out, 0, fuse) == ROUTE_IGEMM4;
                if (sg_here) fz.sign_out = ly.out.sg;
                {
                    // igemm3's fp16-pair instantiation for a forward launch without a two-slot plan (NET-B's conv1 .. conv3): one scale per
                    // patch from the bound on this layer's input (measured maximum of the network input pushed through the L1 norms)
                    Igemm2Fuse hz;
                    const Igemm2Fuse *fu = fuse;
                    if (v3f16 && !ly.fwd[0].p4.ok && !ly.fwd[0].pd.ok && !ly.fwd[0].pfc.ok && ly.fwd[0].p3.ok && ly.fwd[0].p3.d_W16 && ly.fwd[0].p2.a.PT == 1 &&
                        in.split == 0 && ly.spec.skip_src < 0) {
                        if (fuse) hz = *fuse;
                        hz.in_amax = i == 0 ? m->in_amax : m->layers[i - 1].bound_fwd;
                        hz.in_amax2 = nullptr;
                        fu = &hz;
                    }
                    bool f2 = false;
                    ALQ_TRY(gemm_launch(ctx, ly.fwd[0], in, ly.out, ly.d_bias, ly.spec.relu, 0, N, PROF_IGEMM_FWD, fu, &f2));
                    fused = fuse ? f2 : false;
                }
                ly.signs_ready = sg_here;
                if (fuse && prod[i]) ALQ_TRY(k_rowmax_u32(ctx, m->amax_tiles, ly.fwd[0].p4.a.tpg * 4, N, ly.amax_fwd));
                break;
            }
            case ALQ_CONVT: {
                if (t3d_fwd_applies(m, i, prod, cons, with_sums, drop)) {
                    const bool want_amax = prod[i] != 0;
                    ALQ_TRY(t3d_fwd_launch(ctx, ly.t3f, in, ly.out, ly.d_bias, N, with_sums ? ly.osum : nullptr, want_amax ? m->amax_tiles : nullptr));
                    if (want_amax) ALQ_TRY(k_rowmax_u32(ctx, m->amax_tiles, 16, N, ly.amax_fwd));
                    ly.signs_ready = false;
                    fused = true;
                    m->last.fwd.t3f += 1;
                    break;
                }
                if (ly.fwd_all.ok && two_slot_allowed()) {
                    const bool want_amax = fuse && prod[i];
                    if (fuse) take_amax(fz, i);
                    if (want_amax) fz.out_amax = m->amax_tiles;
                    const bool sg_here = with_sums && fuse && !m->sw.no_signs && ly.spec.relu && ly.out.sg;
                    if (sg_here) fz.sign_out = ly.out.sg;
                    ALQ_TRY(igemm4_launch(ctx, ly.fwd_all, in, ly.out, ly.d_bias, ly.spec.relu, 0, N, PROF_IGEMM3_FWD, fuse));
                    ly.signs_ready = sg_here;
                    if (want_amax)
                        ALQ_TRY(k_rowmax_u32(ctx, m->amax_tiles, ly.fwd_all.a.tpg * (ly.fwd_all.multi ? ly.fwd_all.a.ngr : 1) * 4, N, ly.amax_fwd));
                    fused = fuse != nullptr;
                    break;
                }
                bool all = true;
                for (auto &p : ly.fwd) {
                    bool f1 = false;
                    ALQ_TRY(gemm_launch(ctx, p, in, ly.out, ly.d_bias, ly.spec.relu, 0, N, PROF_IGEMM_FWD, fuse, &f1));
                    all = all && f1;
                }
                fused = all;
                break;
            }
            case ALQ_POOL:
                ALQ_TRY(k_pool_fwd(ctx, in, ly.out, ly.argmax, ly.spec.k, ly.lo, N, with_sums ? ly.osum : nullptr, &fused));
                break;
            case ALQ_FC:
                if (with_sums) {
                    // sum of all inputs of the fc layer, per patch
                    const bool prev_spatial = i > 0 && m->layers[i - 1].osum != nullptr;
                    if (c3_head) ALQ_TRY(k_rowsum_field(ctx, ly.c3_asum, 4, N, ly.asum));
                    else if (prev_spatial) ALQ_TRY(k_rowsum_field(ctx, m->layers[i - 1].osum, m->layers[i - 1].out.vox(), N, ly.asum));
                    else ALQ_TRY(k_chansum(ctx, flat_view(in), ly.asum, N));
                }
                if (ly.dense_fc_small && fc_head_fused) {      // the plane-sweep engine leaves one partial per (patch, wave)
                    ALQ_TRY(k_fc_small_finish_diff(ctx, c3_head ? ly.c3_part : ly.fc_part2, c3_head ? 4 : ly.fc_slices2, ly.d_bias, N, ly.out.p));
                } else if (ly.dense_fc_small) {
                    ALQ_TRY(k_fc_small_fwd(ctx, in.p, ly.F, ly.d_Wp, ly.spec.cout, N, ly.fc_partials, ly.fc_slices,
                                           with_sums ? ly.fc_maskbits : nullptr));
                    ALQ_TRY(k_fc_small_finish(ctx, ly.fc_partials, ly.fc_slices, ly.d_bias, ly.spec.cout,
                                              ly.spec.relu, N, ly.out.p));
                } else {
                    ALQ_TRY(gemm_launch(ctx, ly.fwd[0], flat_view(in), ly.out, ly.d_bias, ly.spec.relu, 0, N,
                                        PROF_IGEMM_FWD));
                }
                break;
        }
        if (drop && drop->on(i)) {
            ALQ_REQUIRE(keep_all && !with_sums, ALQ_EINVAL, "dropout only in passes that keep every activation");
            ALQ_TRY(k_dropout(ctx, ly.spec.type == ALQ_FC ? flat_view(ly.out) : ly.out, N, drop->first_sample, drop->seed, i, drop->keep_prob));
        }
        if (with_sums && ly.osum && !fused) ALQ_TRY(k_chansum(ctx, ly.out, ly.osum, N));
        if (with_sums && i == 0 && ly.pidx == 0 && ly.spec.type != ALQ_FC && in.C > 1)
            ALQ_TRY(k_chansum(ctx, in, ly.asum, N));     // channel sums of the network input
    }
    return ALQ_OK;
}

// While one of these lives, launches through ctx go to the side stream, ordered after everything already on the main
// stream.  Without a side stream (or when the fork fails) they simply stay on the main stream.
struct SideStream {
    alq_ctx *c;
    hipStream_t main;
    bool on = false;
    explicit SideStream(alq_ctx *ctx) : c(ctx), main(ctx->stream) {
        if (!c->side || c->side_off) return;
        if (hipEventRecord(c->ev_fork, main) != hipSuccess || hipStreamWaitEvent(c->side, c->ev_fork, 0) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        c->stream = c->side;
        c->side_used = true;
        on = true;
    }
    ~SideStream() { if (on) c->stream = main; }
    SideStream(const SideStream &) = delete;
    SideStream &operator=(const SideStream &) = delete;
};

// the main stream waits for what the side stream was given since the last join
static int side_join(alq_ctx *c) {
    if (!c->side || !c->side_used) return ALQ_OK;
    c->side_used = false;
    ALQ_HIP(hipEventRecord(c->ev_join, c->side));
    ALQ_HIP(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return ALQ_OK;
}

// ---- backward routes of a Fisher pass.  `fuse`: the launch's epilogue request (null when nothing below wants one); `acc`: the launch
// accumulates into a slice the skip destination wrote; `hand`: it hands per-patch maxima of what it stores to the launch below

// a pool whose producer is the first parameterised layer: 2x2(x2) windows tiling the input exactly
static bool pool_first_ok(const Layer &pl, const Layer &src) {
    return pl.spec.type == ALQ_POOL && src.pidx == 0 && src.spec.type != ALQ_FC && pl.spec.k[1] == 2 && pl.spec.k[2] == 2 &&
           (pl.spec.k[0] == 1 || pl.spec.k[0] == 2) && pl.lo[0] == 0 && pl.lo[1] == 0 && pl.lo[2] == 0 &&
           src.out.D == pl.out.D * pl.spec.k[0] && src.out.H == pl.out.H * 2 && src.out.W == pl.out.W * 2 &&
           (pl.out.C == 4 || pl.out.C == 8 || pl.out.C == 16) && ((pl.dout.cs | pl.dout.c0 | pl.out.cs | pl.out.c0) & 3) == 0 &&
           src.spec.relu && !g_dbg_knobs[KNOB_NO_POOL_FIRST];
}

// [pool (i)] <- [ReLU conv (i - 1), a skip source whose consumer wrote its cotangent] <- [pool (i - 2)] <- [first conv (i - 3)]: one
// launch produces both channel-sum fields (e3d.hip); the conv's own box-filter dot product runs as usual when the loop gets there
static bool e3d_bwd_applies(const alq_model *m, int i, bool prev_is_src) {
    const Layer &ly = m->layers[i];
    if (!(ly.spec.type == ALQ_POOL && i >= 3 && !m->sw.no_e3d && two_slot_allowed() && !g_no_f16x2 && !m->sw.no_bound16 && !m->sw.no_signs &&
          !g_dbg_knobs[KNOB_NO_BWD_FUSE] && !g_dbg_knobs[KNOB_NO_POOL_FIRST]))
        return false;
    const Layer &cv = m->layers[i - 1], &p1 = m->layers[i - 2], &c0 = m->layers[i - 3];
    return cv.spec.type == ALQ_CONV && cv.e3b.ok && cv.e3b.d_Whi && cv.spec.relu && cv.signs_ready && cv.out.sg && prev_is_src &&
           p1.spec.type == ALQ_POOL && pool_first_ok(p1, c0) && c0.dsum_partial && p1.signs_ready && p1.out.sg && p1.spec.k[0] == 2 &&
           ly.spec.k[0] == 2 && ly.spec.k[1] == 2 && ly.spec.k[2] == 2 && ly.lo[0] == 0 && ly.lo[1] == 0 && ly.lo[2] == 0 &&
           ly.dout.D == 8 && ly.dout.H == 8 && ly.dout.W == 8 && ly.dout.C == 16 && ly.dout.cs == 16 && ly.dout.c0 == 0 && !ly.dout.split &&
           cv.dout.cs == 16 && cv.dout.c0 == 0 && !cv.dout.split && cv.out.cs == 16 && cv.out.c0 == 0 && p1.out.cs == 8 && p1.out.c0 == 0 &&
           p1.out.C == 8 && c0.out.D == 32 && cv.dout_bound > 0.f && cv.dsum && c0.dsum;
}

// the two-class head (layer i) over a ReLU conv: every patch has the same head cotangent (the unit cotangent), so nothing of
// the size of the conv's output is written; the conv's backward contraction reads [sign] * wv (wv = W0 - W1, set with the weights)
static bool head_bits_apply(const alq_model *m, int i, bool prev_param, bool prev_is_src) {
    const Layer &ly = m->layers[i];
    const Layer *prev = i > 0 ? &m->layers[i - 1] : nullptr;
    return ly.dense_fc_small && ly.fc_maskbits && prev_param && prev->out.cs == prev->out.C &&
           prev->out.c0 == 0 && two_slot_allowed() && prev->bwd.p4.ok && prev->bwd.p4.NTW == 1 && !prev->bwd.p4.multi &&
           prev->bwd.p4.a.PT == 1 && !prev->dout.split && !prev_is_src &&
           // ... and that launch must not accumulate (a skip source right below the conv): the
           // accumulating instantiations of the engine are the plain ones
           !(i >= 2 && m->layers[i - 2].out_is_skip_src && prev->spec.skip_src < 0);
}

// the head conv's backward on the plane-sweep engine (c3d.hip): the NET-C pattern - channels 0..7 = the skip source (first conv,
// ReLU: masked by its sign field and only summed), channels 8..15 = a layer without ReLU (stored and summed)
static bool c3d_bwd_applies(const alq_model *m, const Layer &ly, const unsigned short *vec16c, const Igemm2Fuse *fuse, int acc) {
    return ly.c3b.ok && ly.c3b.d_W && vec16c && !m->sw.no_c3d && !g_no_f16x2 && fuse && !acc && fuse->in_vec_amax > 0.f &&
           fuse->split == 8 && fuse->store_from == 8 && fuse->mask_bits && fuse->mask_from == 0 && fuse->mask_to == 8 && fuse->osumA && fuse->osumB &&
           ly.din.split == 8 && ly.din.cs == 8 && ly.din.C == 16;
}

// the row-sweep engine (t3d.hip) for the backward-data pass of a stride-2 conv_transpose: fp16 pairs under the static
// bound like the two-slot launch it replaces; the producer below is a ReLU conv whose sign field masks the result
static bool t3d_bwd_applies(const alq_model *m, const Layer &ly, const Igemm2Fuse *fuse, int acc, bool hand, bool prev_param) {
    return ly.spec.type == ALQ_CONVT && ly.t3b.ok && ly.t3b.d_W && !m->sw.no_t3d && two_slot_allowed() && !g_no_f16x2 && !acc && fuse && !hand &&
           fuse->in_bound > 0.f && !fuse->in_amax && fuse->split == 0 && fuse->store_from == 0 && fuse->osumA && !fuse->osumB && fuse->mask_from == 0 &&
           (!fuse->mask || fuse->mask_bits) && !ly.dout.split && !ly.din.split && prev_param;
}

// the plane-sweep kernel of d3d.hip for the backward-data pass of the conv over a split concat (NET-C's dec1): fp16 pairs under the static
// bound like the two-slot launch it replaces; channels [0, 16) = the skip source's cotangent (stored), [16, 32) = the producer's (stored + summed)
static bool d3d_bwd_applies(const alq_model *m, const Layer &ly, const Igemm2Fuse *fuse, int acc, bool hand) {
    return ly.spec.type == ALQ_CONV && ly.d3f.ok && ly.d3f.d_Bhi && !m->sw.no_d3d && !m->sw.no_d3b && two_slot_allowed() && !g_no_f16x2 && !acc && fuse && !hand &&
           fuse->in_bound > 0.f && !fuse->in_amax && fuse->split == 16 && fuse->store_from == 0 && !fuse->mask && !fuse->osumA && fuse->osumB &&
           !ly.dout.split && ly.dout.cs == 16 && ly.dout.c0 == 0 && ly.din.split == 16 && ly.din.cs == 16 && ly.din.c0 == 0 && ly.din.C == 32;
}

static int run_backward_main(alq_model *m, const float *d_x, int N);
static int run_backward(alq_model *m, const float *d_x, int N) {
    const int rc = run_backward_main(m, d_x, N);
    const int rj = side_join(m->ctx);       // also after a failure: nothing may still run beside the caller's next step
    return rc != ALQ_OK ? rc : rj;
}

static int run_backward_main(alq_model *m, const float *d_x, int N) {
    alq_ctx *ctx = m->ctx;
    const int nl = (int)m->layers.size();
    ALQ_REQUIRE(m->nclass == 2, ALQ_EUNSUPPORTED, "Fisher scoring is binary (PW_NNAL.py:766), got %d classes", m->nclass);
    ALQ_TRY(k_fill_unit_cotangent(ctx, m->dlogits, N));
    for (Layer &l : m->layers) { l.delta_ready = false; l.dsum_partial = false; l.dout_bits = nullptr; l.dout_vec = nullptr; l.dout_vec16 = nullptr; l.dout_vec16c = nullptr; l.dout_amax = nullptr; }
    m->last.bwd = {};
    {   // bounds on every layer's output cotangent under the unit cotangent (+1, -1): |d out| of the head = 1; a two-class
        // head hands max |W0 - W1| down, a conv / conv_transpose its L1 bound, a pool passes the bound on, a ReLU mask
        // cannot raise it; a tensor with several consumers (skip source) collects the sum.  One fp16x2 scale per LAUNCH
        // follows from it (igemm4: Igemm2Fuse::in_bound) - no per-patch maxima, no extra pass, batch-invariant results.
        for (Layer &l : m->layers) l.dout_bound = 0.f;
        m->layers[nl - 1].dout_bound = 1.f;
        for (int i = nl - 1; i >= 1; --i) {
            const Layer &ly = m->layers[i];
            double inb = ly.dout_bound;
            if (ly.spec.type == ALQ_FC)      // the head: max |W0 - W1|; a hidden fc layer: its L1 bound like a conv's (set with the weights)
                inb = (ly.spec.cout == 2 && ly.fc_wv_amax > 0.f && i == nl - 1) ? (double)ly.fc_wv_amax : (i < nl - 1 ? ly.bwd_l1 * ly.dout_bound : 0.0);
            else if (ly.spec.type != ALQ_POOL) inb = ly.bwd_l1 * ly.dout_bound;
            if (!(inb > 0.0) || ly.dout_bound <= 0.f) inb = 0.0;       // unknown upstream: no bound below either
            auto add = [&](Layer &p) { p.dout_bound = (p.dout_bound < 0.f || inb <= 0.0) ? -1.f : p.dout_bound + (float)(inb * (1.0 + 1e-6)); };
            add(m->layers[i - 1]);
            if (ly.spec.skip_src >= 0) add(m->layers[ly.spec.skip_src]);
        }
    }
    int e3_conv = -1;      // the conv whose backward ran fused with the pool backward steps around it (e3d.hip), or -1
    for (int i = nl - 1; i >= 0; --i) {
        Layer &ly = m->layers[i];
        const bool prev_is_src = (i > 0 && m->layers[i - 1].out_is_skip_src && ly.spec.skip_src < 0);
        if (e3d_bwd_applies(m, i, prev_is_src)) {
            Layer &cv = m->layers[i - 1], &p1 = m->layers[i - 2], &c0 = m->layers[i - 3];
            ALQ_TRY(e3d_bwd_launch(ctx, cv.e3b, N, cv.dout.p, ly.dout.p, ly.argmax, cv.out.sg, p1.argmax, p1.out.sg, cv.dsum, c0.dsum, cv.dout_bound, m->sw.e3d_rows != 0));
            m->last.bwd.e3b_form = m->sw.e3d_rows ? 1 : 2;
            cv.delta_ready = true;
            c0.delta_ready = true;
            e3_conv = i - 1;
            m->last.bwd.e3b = 1;
            continue;
        }
        if (e3_conv >= 0 && i == e3_conv - 1) continue;      // the pool below the fused conv: done
        // Every backward op is the LAST writer of its direct input's cotangent (a skip destination
        // wrote its slice earlier), so it can finish that tensor: ReLU-grad mask + channel sums.
        Layer *prev = i > 0 ? &m->layers[i - 1] : nullptr;
        const bool prev_param = prev && prev->pidx >= 0 && prev->spec.type != ALQ_FC;
        if (ly.spec.type == ALQ_POOL && i == 0) break;      // a pool on the network input: nothing below takes a cotangent (as in grads.hip)
        if (ly.spec.type == ALQ_POOL && prev_param && pool_first_ok(ly, *prev) && (prev->dsum_partial || !prev_is_src)) {
            ALQ_TRY(k_pool_bwd_first(ctx, ly.dout, ly.out, ly.argmax, ly.spec.k, prev->out.D, prev->out.H, prev->out.W, N,
                                     prev->dsum, prev->dsum_partial ? 1 : 0, ly.signs_ready ? 1 : 0));
            prev->delta_ready = true;
            continue;
        }
        if (ly.spec.type == ALQ_POOL) {
            bool fused = false;
            ALQ_TRY(k_pool_bwd(ctx, ly.dout, ly.din, ly.argmax, ly.spec.k, ly.lo, N, prev_is_src ? 1 : 0,
                               (prev_param && prev->spec.relu) ? &prev->out : nullptr, prev_param ? prev->dsum : nullptr,
                               &fused, /*store_din=*/!(prev_param && prev->pidx == 0),      // layer 0 only needs the sums
                               /*use_signs=*/(prev_param && prev->signs_ready) ? 1 : 0));
            if (prev_param && fused) prev->delta_ready = true;
            continue;
        }
        // cotangent w.r.t. the pre-activation + its channel sum (unless the producer already did it)
        const bool isfc = ly.spec.type == ALQ_FC;
        if (!ly.delta_ready) {
            View dv = isfc ? flat_view(ly.dout) : ly.dout;
            View av = isfc ? flat_view(ly.out) : ly.out;
            ALQ_TRY(k_mask_chansum(ctx, dv, ly.spec.relu ? &av : nullptr, ly.dsum, N));
        }
        // channel sums of the layer input: the producers' osum fields (two for a concat input)
        const float *as1 = ly.asum, *as2 = nullptr;
        if (!isfc) {
            if (i == 0) as1 = ly.in.C == 1 ? d_x : ly.asum;
            else as1 = m->layers[i - 1].osum;
            if (ly.spec.skip_src >= 0) as2 = m->layers[ly.spec.skip_src].osum;
        }
        double *Sdst = m->Spart + (size_t)ly.pidx * m->max_batch * m->nslab_max;
        {   // reads this layer's sums, writes its own slice of Spart: beside the contraction launched below
            SideStream beside(ctx);
            if (ly.spec.type == ALQ_CONVT) {
                ALQ_TRY(k_boxdot_convT(ctx, ly.dsum, as1, as2, ly.in.D, ly.in.H, ly.in.W, ly.spec.k, ly.spec.s, ly.lo, N, Sdst, m->nslab_max));
            } else if (isfc) {
                const int one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
                ALQ_TRY(k_boxdot_conv(ctx, ly.dsum, ly.asum, nullptr, 1, 1, 1, one, zero, N, Sdst, m->nslab_max));
            } else {
                ALQ_TRY(k_boxdot_conv(ctx, ly.dsum, as1, as2, ly.out.D, ly.out.H, ly.out.W, ly.spec.k, ly.lo, N, Sdst, m->nslab_max));
            }
        }
        if (ly.pidx == 0) break;   // nothing upstream needs a cotangent
        if (i == e3_conv) continue;      // its backward-data pass ran inside the fused launch
        const int acc = prev_is_src ? 1 : 0;   // the skip destination has already written this slice
        bool fused = false;
        if (isfc) {
            ALQ_REQUIRE(!acc, ALQ_EUNSUPPORTED, "layer %d: fc consumer of a skip source", i);
            if (head_bits_apply(m, i, prev_param, prev_is_src)) {
                {   // the sums feed only the layer's box-filter dot products (same stream, later)
                    SideStream beside(ctx);
                    ALQ_TRY(k_fc_small_dsum_bits(ctx, ly.fc_maskbits, ly.fc_wv, ly.F, N, prev->dsum));
                }
                prev->dout_bits = ly.fc_maskbits;
                prev->dout_vec = ly.fc_wv;
                prev->dout_vec16 = ly.fc_wv16;
                prev->dout_vec16c = ly.fc_wv16c;
                prev->dout_vec_amax = ly.spec.cout == 2 ? ly.fc_wv_amax : 0.f;
                fused = true;
            } else if (ly.dense_fc_small) {
                const bool can = prev_param && prev->out.cs == prev->out.C;
                ALQ_TRY(k_fc_small_bwd(ctx, ly.dout.p, ly.spec.cout, ly.d_Wp, ly.F, N, ly.din.p,
                                       (can && prev->spec.relu) ? prev->out.p : nullptr, can ? prev->dsum : nullptr,
                                       can ? prev->out.C : 0, &fused));
            } else {
                // a wide fc layer's backward GEMM on fp16 pairs under the static bound on its input cotangent (fcgemm.hip, F16)
                ALQ_TRY(gemm_launch(ctx, ly.bwd, ly.dout, flat_view(ly.din), nullptr, 0, 0, N, PROF_IGEMM_BWD, nullptr, nullptr,
                                    (ly.dout_bound > 0.f && !m->sw.no_bound16) ? ly.dout_bound : 0.f));
            }
        } else {
            Igemm2Fuse fz;
            const Igemm2Fuse *fuse = nullptr;
            if (prev_param && !g_dbg_knobs[KNOB_NO_BWD_FUSE]) {
                const int Cs = ly.spec.skip_src >= 0 ? m->layers[ly.spec.skip_src].out.C : 0;   // concat: [src | prev]
                if (prev->spec.relu) {
                    fz.mask = prev->out.p; fz.mask_cs = prev->out.cs; fz.mask_c0 = prev->out.c0; fz.mask_from = Cs;
                    if (prev->signs_ready) fz.mask_bits = prev->out.sg;
                }
                if (Cs > 0) { fz.split = Cs; fz.osumB = prev->dsum; } else { fz.osumA = prev->dsum; }
                // the skip source is the first parameterised layer and sits in front of a pool: nothing needs its
                // cotangent except the channel sums, so mask and sum its columns here and do not store them
                if (Cs > 0 && (two_slot_allowed() || ly.din.split) && ly.bwd.p4.ok) {
                    Layer &sl = m->layers[ly.spec.skip_src];
                    const bool next_pool = ly.spec.skip_src + 1 < nl && pool_first_ok(m->layers[ly.spec.skip_src + 1], sl);
                    const bool sliced = sl.out.p == prev->out.p && sl.out.cs == prev->out.cs && prev->out.c0 == sl.out.c0 + Cs;
                    const bool splitv = ly.in.split == Cs && sl.out.p == ly.in.p;
                    if (next_pool && (sliced || splitv) && (Cs & 3) == 0) {
                        fz.mask = sl.out.p; fz.mask_cs = sl.out.cs; fz.mask_c0 = sl.out.c0; fz.mask_from = 0;
                        fz.mask_bits = (sl.signs_ready && (!prev->spec.relu || prev->signs_ready)) ? sl.out.sg : nullptr;
                        if (splitv) { fz.mask_split = Cs; fz.mask_delta = ly.in.delta; }
                        if (!prev->spec.relu) fz.mask_to = Cs;
                        fz.osumA = sl.dsum; fz.store_from = Cs;
                        sl.dsum_partial = true;
                    }
                }
                fuse = &fz;
            }
            if (ly.dout_bits) {       // the cotangent of this layer's output exists only as mask bits and one vector
                fz.in_bits = ly.dout_bits; fz.in_vec = ly.dout_vec; fz.in_vec_amax = ly.dout_vec_amax;
                fz.in_vec16 = m->sw.no_presplit ? nullptr : ly.dout_vec16;
                const unsigned short *vec16c = ly.dout_vec16c;
                ly.dout_bits = nullptr; ly.dout_vec = nullptr; ly.dout_vec16 = nullptr; ly.dout_vec16c = nullptr;
                const bool honoured = fuse != nullptr;
                const bool c3 = c3d_bwd_applies(m, ly, vec16c, fuse, acc);
                m->last.bwd.c3_bwd = c3;
                if (c3) {
                    int ex = 0;
                    (void)std::frexp(fz.in_vec_amax, &ex);
                    ALQ_TRY(c3d_bwd_launch(ctx, ly.c3b, N, reinterpret_cast<const unsigned char *>(fz.in_bits), vec16c, 14 - ex, fz.mask_bits,
                                           ly.din.p + ly.din.delta, fz.osumA, fz.osumB, m->sw.c3_bwd_rows, m->sw.c3_bwd_waves, &m->last.bwd.c3b_grid));
                } else {
                    ALQ_TRY(igemm4_launch(ctx, ly.bwd.p4, ly.dout, ly.din, nullptr, 0, acc, N, PROF_IGEMM3_BWD, &fz));
                }
                fused = honoured;
            } else {
                // Hand the per-patch maxima of what this launch stores to the backward launch below it when that one has
                // an fp16x2 variant (two column tiles, or one with the prefetch on the contracting side).  Not from the
                // mask-bit launch above: its staging side is the critical one and the maxima cost more than they gave.
                const bool p4_here = fuse && two_slot_allowed() && ly.bwd.p4.ok && !ly.bwd.p4.multi && ly.bwd.p4.a.PT == 1 && !g_no_f16x2;
                bool hand = false;
                // (with a static bound for the launch below, nothing needs to be measured here)
                if (p4_here && prev_param && !acc && !(prev->dout_bound > 0.f && !m->sw.no_bound16) && prev->pidx > 0 && prev->bwd.p4.ok && !prev->bwd.p4.multi && prev->bwd.p4.a.PT == 1 &&
                    prev->bwd.p4.d_W16 && !prev->dout.split &&
                    ((prev->bwd.p4.NTW == 1 && prev->bwd.p4.fic) || prev->bwd.p4.NTW == 2)) {
                    const size_t len = (size_t)ly.bwd.p4.a.tpg * 4;
                    if (!m->amax_a) { ALQ_TRY(m->dalloc(&m->amax_a, (size_t)m->max_batch)); ALQ_TRY(m->dalloc(&m->amax_b, (size_t)m->max_batch)); }
                    ALQ_TRY(ensure_amax_tiles(m, len));
                    fz.out_amax = m->amax_tiles;
                    fz.amax_from = fz.split > 0 && fz.split < (1 << 29) ? fz.split : 0;       // the slice the layer below reads
                    hand = true;
                }
                // (not for an accumulating launch - a conv right behind a skip source: those run the plain bf16x3 instantiation,
                // igemm4_launch_impl's `no16`, and must not be routed to an fp16x2-only twin plan)
                if (p4_here && !acc && ly.dout_amax) fz.in_amax = ly.dout_amax;
                if (p4_here && !acc && !fz.in_amax && ly.dout_bound > 0.f && !m->sw.no_bound16) fz.in_bound = ly.dout_bound;
                // a launch without an epilogue request (nothing parameterised below it to mask or sum for) still gets its
                // fp16x2 scale: an otherwise empty request carries the bound (no mask, no sums: the plain epilogue runs)
                if (!fuse && !acc && two_slot_allowed() && ly.bwd.p4.ok && !ly.bwd.p4.multi && ly.bwd.p4.a.PT == 1 && !g_no_f16x2 && !ly.dout_amax &&
                    ly.dout_bound > 0.f && !m->sw.no_bound16 && !g_dbg_knobs[KNOB_NO_BWD_FUSE]) {
                    fz = Igemm2Fuse();
                    fz.in_bound = ly.dout_bound;
                    fuse = &fz;
                }
                // the same bound for a launch that runs on igemm3's fp16-pair instantiation (no two-slot plan)
                if (!ly.bwd.p4.ok && ly.bwd.p3.ok && ly.bwd.p3.d_W16 && !acc && !g_no_f16x2 && ly.dout_bound > 0.f && !m->sw.no_bound16 && !g_dbg_knobs[KNOB_NO_BWD_FUSE] &&
                    two_slot_allowed() && !ly.bwd.pd.ok && !ly.bwd.pfc.ok) {
                    if (!fuse) { fz = Igemm2Fuse(); fuse = &fz; }
                    fz.in_bound = ly.dout_bound;
                }
                const unsigned *mine = ly.dout_amax;
                ly.dout_amax = nullptr;
                if (t3d_bwd_applies(m, ly, fuse, acc, hand, prev_param)) {
                    ALQ_TRY(t3d_bwd_launch(ctx, ly.t3b, ly.dout, ly.din, N, fz.in_bound, fz.mask ? fz.mask_bits : nullptr, fz.osumA));
                    fused = true;
                    m->last.bwd.t3b += 1;
                } else if (d3d_bwd_applies(m, ly, fuse, acc, hand)) {
                    ALQ_TRY(d3d_bwd_launch(ctx, ly.d3f, N, ly.dout.p, fz.in_bound, ly.din.p, ly.din.p + ly.din.delta, fz.osumB));
                    fused = true;
                    m->last.bwd.d3b = 1;
                } else
                ALQ_TRY(gemm_launch(ctx, ly.bwd, ly.dout, ly.din, nullptr, 0, acc, N, PROF_IGEMM_BWD, fuse, &fused));
                if (hand) {
                    // two buffers alternate down the chain: this launch may have read the other one
                    unsigned *dst = mine == m->amax_a ? m->amax_b : m->amax_a;
                    ALQ_TRY(k_rowmax_u32(ctx, m->amax_tiles, ly.bwd.p4.a.tpg * 4, N, dst));
                    prev->dout_amax = dst;
                }
            }
        }
        if (prev_param && fused) prev->delta_ready = true;
    }
    return ALQ_OK;
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
    ALQ_REQUIRE(layer_idx >= 0 && layer_idx < (int)m->layers.size(), ALQ_EINVAL, "bad layer index");
    const Layer &ly = m->layers[layer_idx];
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
            ALQ_REQUIRE(v.sg && ly.signs_ready && ((v.C | v.cs | v.c0) & 3) == 0 && ((int64_t)N * v.vox() * v.cs) % 16 == 0, ALQ_EUNSUPPORTED,
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
