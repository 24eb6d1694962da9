// The two pass drivers behind the entry points: run_forward (Fisher, forward-only and keep-all passes) and run_backward, the fused
// backward sweep of a Fisher pass.  A route is a plain function holding its own condition and its launch; the drivers try them in the order
// below and the first one that applies takes the layer.  The state of one pass lives in FwdPass / BwdPass, locals of the drivers; what
// outlives a driver is in PassInfo (model_types.h).  Plans, gemm_route / gemm_launch and the C ABI are in model.hip.
//   run_forward, per layer:
//     conv            fwd_conv_pool     the first conv + the pool behind it in one kernel (direct.hip)
//                     fwd_head_conv     the conv under the fused two-class head: c3d.hip or igemm4, flip-fix behind either
//                     fwd_conv_d3d      row sweep over a split concat (d3d.hip; NET-C's dec1)
//                     fwd_conv_f3d      conv + the pool behind it under the first layer's measured maximum (f3d.hip; NET-C's enc2)
//                     fwd_conv_sliced   a wide conv as launches over slices of its output channels
//                     fwd_conv_gemm     gemm_launch (igemm3 on fp16 pairs where the pass has bounds on its input)
//     conv_transpose  fwd_convt         t3d.hip, or one igemm4 launch for all classes, or one gemm_launch per class
//     pool            k_pool_fwd
//     fc              fwd_fc            input sums; finish of the fused head, or the skinny fc kernels, or gemm_launch
//   run_backward, per layer from the head down:
//     pool            bwd_pool          e3d.hip (pool, conv and pool below it in one launch), or pool-first, or the plain pool backward
//     other layers    bwd_boxdot        mask + sums where no launch above left them, box-filter dot products on the side stream
//                     bwd_fc            head as mask bits, or skinny fc, or wide fc
//                     bwd_epilogue_request, then bwd_bits_launch (c3d.hip or igemm4 from mask bits)
//                                       or bwd_data_launch (scale choice, hand-off of maxima; t3d.hip, d3d.hip or gemm_launch)
#include <algorithm>
#include <cmath>

#include "model_types.h"

using namespace alq;

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

// ---- the forward pass ----------------------------------------------------------------------
// keep_all (forward-only calls): every activation stays readable (a feature layer was asked for); otherwise the fc head of a two-class
// net is fused into the last conv in forward-only calls too (no channel sums, no sign bytes).  light: a forward-only pass that keeps no
// activation (fuse objects only for the launches of the fused head).  prod / cons: the layers that report / read per-patch input maxima
// (plan_input_scales; cons == 2: derived bounds instead of measured maxima).
struct FwdPass {
    alq_model *m;
    const float *d_x;
    int N;
    bool with_sums, keep_all, light;
    const DropSpec *drop;
    bool dcp;                    // layer 0 = first conv, fused with the pool behind it (dcp_applies)
    std::vector<char> prod, cons;
    bool any_derived = false;    // some consumer takes derived bounds
    bool v3f16 = false;          // igemm3's forward launches take fp16 pairs under bounds derived from the measured input maxima
    bool skip_next = false;      // this layer's outputs were produced by the previous layer's kernel
    bool fc_head_fused = false;  // the logits partials of the fc head came out of the previous conv's epilogue
    bool c3_head = false;        // ... of the plane-sweep engine: one partial per (patch, wave), the head's input sum likewise
};
// one layer of it.  fz: the launch's epilogue request as far as the pass has filled it; fuse: &fz or null; fused: the launch produced
// the channel sums of its output
struct FwdStep {
    int i;
    View in;
    Igemm2Fuse fz;
    const Igemm2Fuse *fuse = nullptr;
    bool fused = false;
};

// the first conv, fused with the pool behind it (direct_conv_pool_launch)
static bool dcp_applies(const alq_model *m, const DropSpec *drop) {
    if (m->layers.size() < 2) return false;
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
static bool flipfix_applies(const FwdPass &P, int i, const Igemm2Fuse *fz) {
    const Layer &ly = P.m->layers[i], &nx = P.m->layers[i + 1];
    const alq_layer_t &sp = ly.spec;
    const View &in = ly.in;
    return P.with_sums && fz->fc_bits && fz->in_amax && !g_no_f16x2 && !P.m->sw.no_flipfix && ly.d_W32 && ly.fwd_l1 > 0.f &&
           sp.s[0] == 1 && sp.s[1] == 1 && sp.s[2] == 1 && in.c0 == 0 && nx.F % 64 == 0 &&      // (whole 16-byte words of sign bytes per patch)
           ((in.split == 0 && in.cs == in.C) || (in.split > 0 && in.cs == in.split && in.C == 2 * in.split));
}

// the conv under the fused head on the plane-sweep engine (c3d.hip): where its geometry applies and both per-patch input maxima are known
static bool c3d_fwd_applies(const FwdPass &P, int i, const Igemm2Fuse *fz) {
    const Layer &ly = P.m->layers[i], &nx = P.m->layers[i + 1];
    return ly.c3f.ok && ly.c3f.d_W && nx.c3_part && fz->in_amax && fz->in_amax2 && !g_no_f16x2 && !P.m->sw.no_c3d;
}

// the row-sweep engine (d3d.hip) where its geometry applies, both per-patch input bounds are known and nothing but the tensor,
// its channel sums and its sign field is wanted
// (round 6: forward-only passes too - the entropy filter over a pool is most of a query round - without sums / sign field)
static bool d3d_fwd_applies(const FwdPass &P, int i, const Igemm2Fuse *fuse) {
    const alq_model *m = P.m;
    const Layer &ly = m->layers[i];
    return fuse && ly.d3f.ok && ly.d3f.d_Whi && !m->sw.no_d3d && fuse->in_amax && fuse->in_amax2 && !P.prod[i] && !g_no_f16x2 && two_slot_allowed() &&
           ((P.with_sums && fuse->osumA) || (P.light && !m->sw.no_light_kernels)) && ly.in.split == 16 && !(P.drop && P.drop->on(i));
}

// enc2 + the pool behind it in one launch (f3d.hip): fp16 pairs under the first layer's measured maximum
static bool f3d_fwd_applies(const FwdPass &P, int i, const Igemm2Fuse *fuse) {
    const alq_model *m = P.m;
    const DropSpec *drop = P.drop;
    const Layer &ly = m->layers[i];
    const Layer *nx = i + 1 < (int)m->layers.size() ? &m->layers[i + 1] : nullptr;
    return fuse && ly.f3f.ok && ly.f3f.d_Whi && !m->sw.no_f3d && P.cons[i] == 2 && fuse->in_amax && !fuse->in_amax2 && !P.prod[i] && !g_no_f16x2 && two_slot_allowed() &&
           ((P.with_sums && fuse->osumA) || (P.light && !m->sw.no_light_kernels)) && ly.spec.relu && ly.in.split == 0 && !(drop && (drop->on(i) || drop->on(i + 1))) && nx && nx->spec.type == ALQ_POOL &&
           nx->spec.k[0] == 2 && nx->spec.k[1] == 2 && nx->spec.k[2] == 2 && nx->lo[0] == 0 && nx->lo[1] == 0 && nx->lo[2] == 0 && nx->out.D == 8 && nx->out.H == 8 &&
           nx->out.W == 8 && nx->out.C == 16 && nx->out.cs == 16 && nx->out.c0 == 0 && !nx->out.split && nx->argmax && !P.prod[i + 1];
}

// the row-sweep engine (t3d.hip): bf16 triples like the two-slot launch it replaces, nothing but the tensor, its channel
// sums and its per-patch maximum to produce (no ReLU behind a conv_transpose of this geometry: no sign field)
static bool t3d_fwd_applies(const FwdPass &P, int i) {
    const alq_model *m = P.m;
    const Layer &ly = m->layers[i];
    return ly.t3f.ok && ly.t3f.d_W && !m->sw.no_t3d && !g_dbg_knobs[KNOB_NO_FWD_FUSE] && two_slot_allowed() && !P.cons[i] && !ly.spec.relu &&
           !(P.drop && P.drop->on(i)) && (!P.with_sums || ly.osum) && !(ly.t3f.kind == 8 && P.prod[i]);
}

// A conv / conv_transpose launch contracts with the fp16x2 split if it knows max |x| per patch of (every part of)
// its input ahead of time: the launches that produce those tensors report them (`prod`), the consumers (`cons`)
// read one scale per tile.  Producers: the first conv + pool kernel and one-patch-per-tile igemm4 launches.
static int plan_input_scales(FwdPass &P) {
    alq_model *m = P.m;
    const DropSpec *drop = P.drop;
    const int nl = (int)m->layers.size();
    const bool no16 = g_no_f16x2 != 0;
    std::vector<char> &prod = P.prod, &cons = P.cons;
    prod.assign(nl, 0);
    cons.assign(nl, 0);
    if ((P.with_sums || P.light) && !no16 && !g_dbg_knobs[KNOB_NO_FWD_FUSE] && two_slot_allowed()) {
        auto prod_ok = [&](int p) {
            if (p < 0) return false;
            const Layer &l = m->layers[p];
            if (p == 0 && P.dcp) return true;
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
            if (m->sw.f16_fwd_mask < 0 && !m->sw.no_f16_derived && nl <= 16 && ((m->f16_fwd_derived >> j) & 1) && l.spec.type == ALQ_CONV && P.dcp &&
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
            if (l.spec.type == ALQ_CONV && !(p == 0 && P.dcp)) need = std::max(need, (size_t)l.fwd[0].p4.a.tpg * 4);
            if (l.spec.type == ALQ_CONVT) need = std::max(need, (size_t)l.fwd_all.a.tpg * (l.fwd_all.multi ? l.fwd_all.a.ngr : 1) * 4);
            if (l.spec.type == ALQ_CONVT && l.t3f.ok) need = std::max(need, (size_t)16);      // row-sweep engine: one maximum per input plane
        }
        ALQ_TRY(ensure_amax_tiles(m, need));
    }
    for (int j = 0; j < nl; ++j) P.any_derived = P.any_derived || cons[j] == 2;
    m->last.fwd.f16_derived = P.any_derived;
    for (int p = 0; p < nl && p < 64; ++p) m->last.fwd.amax_asked[p] = prod[p] != 0;
    if (P.any_derived) ALQ_TRY(ensure_bounds(m));
    // Forward launches that stay on igemm3 (no two-slot plan: NET-B's conv1 .. conv3) on fp16 pairs, one scale per patch: the
    // measured maximum of every patch of the network input, pushed through the layers' L1 norms, bounds every layer's input.
    // Fisher passes and forward-only passes; not the passes that keep every activation for training, not under dropout.
    P.v3f16 = m->v3_fwd_f16 && (P.with_sums || P.light) && !no16 && !drop && !P.any_derived && !P.dcp && nl <= 16 &&
              !g_dbg_knobs[KNOB_NO_FWD_FUSE] && two_slot_allowed() && m->layers[0].in.split == 0 && m->layers[0].in.cs == m->layers[0].in.C;
    m->last.fwd.v3f16 = P.v3f16;
    if (P.v3f16) {
        if (!m->in_amax) ALQ_TRY(m->dalloc(&m->in_amax, (size_t)m->max_batch));
        ALQ_TRY(ensure_bounds(m));
        ALQ_TRY(k_rowmax_abs(m->ctx, P.d_x, P.N, (long long)m->layers[0].in.vox() * m->layers[0].in.C, m->in_amax));
        FwdBoundsArgs ba = fwd_bounds_args(m);
        ba.from_input = 1;
        ALQ_TRY(k_fwd_bounds(m->ctx, m->in_amax, P.N, m->max_batch, ba, m->bound_all));
    }
    return ALQ_OK;
}

// the input maxima of consumer j
static void fwd_take_amax(const FwdPass &P, Igemm2Fuse &fz, int j) {
    const alq_model *m = P.m;
    if (!P.cons[j]) return;
    const bool dv = P.cons[j] == 2;
    fz.in_amax = dv ? m->layers[j - 1].bound_fwd : m->layers[j - 1].amax_fwd;
    if (m->layers[j].spec.skip_src >= 0) {
        const Layer &sl = m->layers[m->layers[j].spec.skip_src];
        fz.in_amax2 = dv ? sl.bound_fwd : sl.amax_fwd;
    }
}

// Sign fields (View::sg): in a Fisher pass a forward launch of the two-slot engine also writes one byte per 4 channels
// with the signs of its ReLU'd output; the backward launches read those instead of the fp32 activations (1/16 of the bytes).
// PassInfo::Fwd::signs_ready says which layers' fields the pass wrote.

// first conv + the pool behind it in one kernel (one input channel, 3x3x3 -> 8, 2x2x2 windows)
static int fwd_conv_pool(FwdPass &P, FwdStep &s, bool *took) {
    if (!(s.i == 0 && P.dcp)) return ALQ_OK;
    alq_model *m = P.m;
    alq_ctx *ctx = m->ctx;
    Layer &ly = m->layers[0], &nx = m->layers[1];
    const alq_layer_t &sp = ly.spec;
    const bool with_sums = P.with_sums;
    if (P.prod[0]) ALQ_HIP(hipMemsetAsync(ly.amax_fwd, 0, (size_t)P.N * sizeof(unsigned), ctx->stream));
    // (the sign field of the full-resolution output: what the last conv's backward launch reads as its ReLU mask)
    const bool sg_here = with_sums && !m->sw.no_signs && !m->sw.no_signs0 && sp.relu && ly.out.sg != nullptr;
    ALQ_TRY(direct_conv_pool_launch(ctx, ly.fwd[0].pd.d_W, s.in, ly.out, nx.out, ly.d_bias, sp.relu, nx.argmax,
                                    with_sums ? ly.osum : nullptr, with_sums ? nx.osum : nullptr, P.N,
                                    ly.fwd[0].pd.flops_per_patch, P.prod[0] ? ly.amax_fwd : nullptr,
                                    sg_here ? ly.out.sg : nullptr, (sg_here && nx.out.sg) ? nx.out.sg : nullptr));
    m->last.fwd.dcp = g_dcp_last_form;
    m->last.fwd.signs_ready[0] = sg_here;
    m->last.fwd.signs_ready[1] = sg_here && nx.out.sg != nullptr;      // (the pool's output: sign of the window maximum)
    if (P.any_derived)      // per-patch bounds on every later layer's output from this layer's measured maximum
        ALQ_TRY(k_fwd_bounds(ctx, ly.amax_fwd, P.N, m->max_batch, fwd_bounds_args(m), m->bound_all));
    s.fused = true;
    P.skip_next = true;
    *took = true;
    return ALQ_OK;
}

// the fc head is this layer's only consumer in a Fisher pass: logits partials + sign bytes from the
// epilogue, the tensor itself is not stored
static int fwd_head_conv(FwdPass &P, FwdStep &s, bool *took) {
    alq_model *m = P.m;
    alq_ctx *ctx = m->ctx;
    const int nl = (int)m->layers.size(), i = s.i, N = P.N;
    if (!(s.fuse && i + 2 == nl && m->layers[nl - 1].fc_part2 && two_slot_allowed())) return ALQ_OK;
    Layer &ly = m->layers[i], &nx = m->layers[i + 1];
    const alq_layer_t &sp = ly.spec;
    const View &in = s.in;
    Igemm2Fuse &fz = s.fz;
    fz.fc_W = nx.fc_wv; fz.fc_F = nx.F; fz.fc_part = nx.fc_part2; fz.fc_bits = P.with_sums ? nx.fc_maskbits : nullptr;
    fwd_take_amax(P, fz, i);
    const bool flipfix = flipfix_applies(P, i, &fz);
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
    P.c3_head = c3d_fwd_applies(P, i, &fz);
    if (P.c3_head)
        ALQ_TRY(c3d_fwd_launch(ctx, ly.c3f, in, ly.d_bias, N, fz.in_amax, fz.in_amax2, nx.fc_wv, nx.c3_part,
                               P.with_sums ? nx.c3_asum : nullptr, reinterpret_cast<unsigned char *>(fz.fc_bits),
                               flipfix ? std::ldexp(ly.fwd_l1, -24) : 0.f));
    else
        ALQ_TRY(igemm4_launch(ctx, ly.fwd[0].p4, in, ly.out, ly.d_bias, ly.spec.relu, 0, N, PROF_IGEMM3_FWD, &fz));
    if (flipfix)
        ALQ_TRY(k_flip_fix(ctx, m->flip_list, m->flip_cnt, m->flip_cap, N, in.p, in.split ? in.p + in.delta : nullptr,
                           in.split ? in.split : in.C, in.split ? in.C - in.split : 0, in.D, in.H, in.W, sp.k[0], sp.k[1], sp.k[2],
                           ly.lo[0], ly.lo[1], ly.lo[2], ly.d_W32, ly.d_bias, sp.cout,
                           reinterpret_cast<unsigned char *>(nx.fc_maskbits), nx.F, m->flip_overflow));
    s.fused = true;
    P.fc_head_fused = true;
    m->last.fwd.head_fused = true;
    m->last.fwd.c3 = P.c3_head;
    *took = true;
    return ALQ_OK;
}

static int fwd_conv_d3d(FwdPass &P, FwdStep &s, bool *took) {
    if (!d3d_fwd_applies(P, s.i, s.fuse)) return ALQ_OK;
    alq_model *m = P.m;
    Layer &ly = m->layers[s.i];
    const bool sgd = P.with_sums && !m->sw.no_signs && ly.spec.relu && ly.out.sg;
    ALQ_TRY(d3d_fwd_launch(m->ctx, ly.d3f, P.N, s.in.p, s.in.p + s.in.delta, s.fz.in_amax, s.fz.in_amax2, ly.d_bias, ly.spec.relu ? 1 : 0, ly.out.p,
                           sgd ? ly.out.sg : nullptr, s.fz.osumA));
    m->last.fwd.signs_ready[s.i] = sgd;
    m->last.fwd.d3f = 1;
    s.fused = true;
    *took = true;
    return ALQ_OK;
}

static int fwd_conv_f3d(FwdPass &P, FwdStep &s, bool *took) {
    if (!f3d_fwd_applies(P, s.i, s.fuse)) return ALQ_OK;
    alq_model *m = P.m;
    Layer &ly = m->layers[s.i], &nx = m->layers[s.i + 1];
    const bool sgd = P.with_sums && !m->sw.no_signs && ly.out.sg;
    ALQ_TRY(f3d_fwd_launch(m->ctx, ly.f3f, P.N, s.in.p, s.fz.in_amax, ly.d_bias, ly.out.p, sgd ? ly.out.sg : nullptr, s.fz.osumA, nx.out.p, nx.argmax,
                           P.with_sums ? nx.osum : nullptr));
    m->last.fwd.signs_ready[s.i] = sgd;      // (none for the pool's output)
    m->last.fwd.f3f = 1;
    s.fused = true;
    P.skip_next = true;
    *took = true;
    return ALQ_OK;
}

// a wide conv as launches over slices of its output channels (no epilogue fusion: channel sums and ReLU masks the plain way)
// (round 6) with per-patch bounds on the input at hand (v3f16: igemm3's forward launches above this layer asked for
// them) the slices take the two-slot engine's fp16-pair form too: one scale per patch, three products
static int fwd_conv_sliced(FwdPass &P, FwdStep &s, bool *took) {
    alq_model *m = P.m;
    const int i = s.i;
    Layer &ly = m->layers[i];
    if (!(!ly.fwd_co.empty() && !P.prod[i] && !P.cons[i] && two_slot_allowed())) return ALQ_OK;
    Igemm2Fuse sz;
    const bool s16 = P.v3f16 && i >= 1 && s.in.split == 0 && ly.spec.skip_src < 0 && !m->sw.no_co_split_f16;
    if (s16) sz.in_amax = m->layers[i - 1].bound_fwd;
    for (size_t j = 0; j < ly.fwd_co.size(); ++j) {
        View oj = ly.out;
        oj.c0 = ly.out.c0 + (int)j * ly.fwd_co_w;
        oj.C = ly.fwd_co_w;
        bool f1 = false;
        ALQ_TRY(gemm_launch(m->ctx, ly.fwd_co[j], s.in, oj, ly.d_bias + j * ly.fwd_co_w, ly.spec.relu, 0, P.N, PROF_IGEMM_FWD, s16 ? &sz : nullptr, &f1));
    }
    s.fused = false;
    *took = true;
    return ALQ_OK;
}

static int fwd_conv_gemm(FwdPass &P, FwdStep &s) {
    alq_model *m = P.m;
    const int i = s.i;
    Layer &ly = m->layers[i];
    const Igemm2Fuse *fuse = s.fuse;
    const bool sg_here = P.with_sums && fuse && !m->sw.no_signs && ly.spec.relu && ly.out.sg && gemm_route(ly.fwd[0], s.in, ly.out, 0, fuse) == ROUTE_IGEMM4;
    if (sg_here) s.fz.sign_out = ly.out.sg;
    // igemm3's fp16-pair instantiation for a forward launch without a two-slot plan (NET-B's conv1 .. conv3): one scale per
    // patch from the bound on this layer's input (measured maximum of the network input pushed through the L1 norms)
    Igemm2Fuse hz;
    const Igemm2Fuse *fu = fuse;
    if (P.v3f16 && !ly.fwd[0].p4.ok && !ly.fwd[0].pd.ok && !ly.fwd[0].pfc.ok && ly.fwd[0].p3.ok && ly.fwd[0].p3.d_W16 && ly.fwd[0].p2.a.PT == 1 &&
        s.in.split == 0 && ly.spec.skip_src < 0) {
        if (fuse) hz = *fuse;
        hz.in_amax = i == 0 ? m->in_amax : m->layers[i - 1].bound_fwd;
        hz.in_amax2 = nullptr;
        fu = &hz;
    }
    bool f2 = false;
    ALQ_TRY(gemm_launch(m->ctx, ly.fwd[0], s.in, ly.out, ly.d_bias, ly.spec.relu, 0, P.N, PROF_IGEMM_FWD, fu, &f2));
    s.fused = fuse ? f2 : false;
    m->last.fwd.signs_ready[i] = sg_here;
    if (fuse && P.prod[i]) ALQ_TRY(k_rowmax_u32(m->ctx, m->amax_tiles, ly.fwd[0].p4.a.tpg * 4, P.N, ly.amax_fwd));
    return ALQ_OK;
}

static int fwd_convt(FwdPass &P, FwdStep &s) {
    alq_model *m = P.m;
    alq_ctx *ctx = m->ctx;
    const int i = s.i, N = P.N;
    Layer &ly = m->layers[i];
    const Igemm2Fuse *fuse = s.fuse;
    if (t3d_fwd_applies(P, i)) {
        const bool want_amax = P.prod[i] != 0;
        ALQ_TRY(t3d_fwd_launch(ctx, ly.t3f, s.in, ly.out, ly.d_bias, N, P.with_sums ? ly.osum : nullptr, want_amax ? m->amax_tiles : nullptr));
        if (want_amax) ALQ_TRY(k_rowmax_u32(ctx, m->amax_tiles, 16, N, ly.amax_fwd));
        s.fused = true;
        m->last.fwd.t3f += 1;
        return ALQ_OK;
    }
    if (ly.fwd_all.ok && two_slot_allowed()) {
        const bool want_amax = fuse && P.prod[i];
        if (fuse) fwd_take_amax(P, s.fz, i);
        if (want_amax) s.fz.out_amax = m->amax_tiles;
        const bool sg_here = P.with_sums && fuse && !m->sw.no_signs && ly.spec.relu && ly.out.sg;
        if (sg_here) s.fz.sign_out = ly.out.sg;
        ALQ_TRY(igemm4_launch(ctx, ly.fwd_all, s.in, ly.out, ly.d_bias, ly.spec.relu, 0, N, PROF_IGEMM3_FWD, fuse));
        m->last.fwd.signs_ready[i] = sg_here;
        if (want_amax)
            ALQ_TRY(k_rowmax_u32(ctx, m->amax_tiles, ly.fwd_all.a.tpg * (ly.fwd_all.multi ? ly.fwd_all.a.ngr : 1) * 4, N, ly.amax_fwd));
        s.fused = fuse != nullptr;
        return ALQ_OK;
    }
    bool all = true;
    for (auto &p : ly.fwd) {
        bool f1 = false;
        ALQ_TRY(gemm_launch(ctx, p, s.in, ly.out, ly.d_bias, ly.spec.relu, 0, N, PROF_IGEMM_FWD, fuse, &f1));
        all = all && f1;
    }
    s.fused = all;
    return ALQ_OK;
}

static int fwd_fc(FwdPass &P, FwdStep &s) {
    alq_model *m = P.m;
    alq_ctx *ctx = m->ctx;
    const int i = s.i, N = P.N;
    Layer &ly = m->layers[i];
    if (P.with_sums) {
        // sum of all inputs of the fc layer, per patch
        const bool prev_spatial = i > 0 && m->layers[i - 1].osum != nullptr;
        if (P.c3_head) ALQ_TRY(k_rowsum_field(ctx, ly.c3_asum, 4, N, ly.asum));
        else if (prev_spatial) ALQ_TRY(k_rowsum_field(ctx, m->layers[i - 1].osum, m->layers[i - 1].out.vox(), N, ly.asum));
        else ALQ_TRY(k_chansum(ctx, flat_view(s.in), ly.asum, N));
    }
    if (ly.dense_fc_small && P.fc_head_fused) {      // the plane-sweep engine leaves one partial per (patch, wave)
        ALQ_TRY(k_fc_small_finish_diff(ctx, P.c3_head ? ly.c3_part : ly.fc_part2, P.c3_head ? 4 : ly.fc_slices2, ly.d_bias, N, ly.out.p));
    } else if (ly.dense_fc_small) {
        ALQ_TRY(k_fc_small_fwd(ctx, s.in.p, ly.F, ly.d_Wp, ly.spec.cout, N, ly.fc_partials, ly.fc_slices,
                               P.with_sums ? ly.fc_maskbits : nullptr));
        ALQ_TRY(k_fc_small_finish(ctx, ly.fc_partials, ly.fc_slices, ly.d_bias, ly.spec.cout,
                                  ly.spec.relu, N, ly.out.p));
    } else {
        ALQ_TRY(gemm_launch(ctx, ly.fwd[0], flat_view(s.in), ly.out, ly.d_bias, ly.spec.relu, 0, N,
                            PROF_IGEMM_FWD));
    }
    return ALQ_OK;
}

int run_forward(alq_model *m, const float *d_x, int N, bool with_sums, bool keep_all, const DropSpec *drop) {
    alq_ctx *ctx = m->ctx;
    const int nl = (int)m->layers.size();
    m->last.fwd = {};
    FwdPass P{m, d_x, N, with_sums, keep_all, /*light=*/!with_sums && !keep_all, drop, dcp_applies(m, drop)};
    ALQ_TRY(plan_input_scales(P));
    for (int i = 0; i < nl; ++i) {
        Layer &ly = m->layers[i];
        ALQ_REQUIRE(ly.pidx < 0 || ly.weights_set, ALQ_EINVAL, "weights of parameterised layer %d not set", ly.pidx);
        if (ly.dense_head) break;      // the caller runs the head (dense_forward_head): posteriors straight from its input
        if (P.skip_next) { P.skip_next = false; continue; }
        FwdStep s;
        s.i = i;
        s.in = ly.in;
        if (i == 0) s.in.p = const_cast<float *>(d_x);
        // channel sums of every spatial layer's output ride on the producing kernel's epilogue when it
        // can; they are the `asum` fields of the layers that consume it
        s.fz.osumA = with_sums ? ly.osum : nullptr;
        const bool head_conv = i + 2 == nl && m->layers[nl - 1].fc_part2 && ly.spec.type == ALQ_CONV;
        const bool light_here = P.light && (P.prod[i] || P.cons[i] || head_conv);
        if ((with_sums || light_here) && ly.osum && !g_dbg_knobs[KNOB_NO_FWD_FUSE]) s.fuse = &s.fz;
        switch (ly.spec.type) {
            case ALQ_CONV: {      // the first route that applies takes the layer: the order is part of the conditions
                bool took = false;
                ALQ_TRY(fwd_conv_pool(P, s, &took));
                if (!took) ALQ_TRY(fwd_head_conv(P, s, &took));
                if (!took && s.fuse) fwd_take_amax(P, s.fz, i);      // (the head conv has taken its own)
                if (!took) ALQ_TRY(fwd_conv_d3d(P, s, &took));
                if (!took) ALQ_TRY(fwd_conv_f3d(P, s, &took));
                if (!took && s.fuse && P.prod[i]) s.fz.out_amax = m->amax_tiles;      // (the sweep kernels report no maxima)
                if (!took) ALQ_TRY(fwd_conv_sliced(P, s, &took));
                if (!took) ALQ_TRY(fwd_conv_gemm(P, s));
                break;
            }
            case ALQ_CONVT: ALQ_TRY(fwd_convt(P, s)); break;
            case ALQ_POOL: ALQ_TRY(k_pool_fwd(ctx, s.in, ly.out, ly.argmax, ly.spec.k, ly.lo, N, with_sums ? ly.osum : nullptr, &s.fused)); break;
            case ALQ_FC: ALQ_TRY(fwd_fc(P, s)); break;
        }
        if (drop && drop->on(i)) {
            ALQ_REQUIRE(keep_all && !with_sums, ALQ_EINVAL, "dropout only in passes that keep every activation");
            ALQ_TRY(k_dropout(ctx, ly.spec.type == ALQ_FC ? flat_view(ly.out) : ly.out, N, drop->first_sample, drop->seed, i, drop->keep_prob));
        }
        if (with_sums && ly.osum && !s.fused) ALQ_TRY(k_chansum(ctx, ly.out, ly.osum, N));
        if (with_sums && i == 0 && ly.pidx == 0 && ly.spec.type != ALQ_FC && s.in.C > 1)
            ALQ_TRY(k_chansum(ctx, s.in, ly.asum, N));     // channel sums of the network input
    }
    return ALQ_OK;
}

// ---- the side stream -----------------------------------------------------------------------
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

// ---- the backward sweep of a Fisher pass ---------------------------------------------------
struct BwdPass {
    alq_model *m;
    const float *d_x;
    int N;
    struct PerLayer {
        bool delta_ready = false;            // the cotangent of the layer's output is already masked and dsum is filled
        bool dsum_partial = false;           // first layer: the skip destination has written its share of dsum
        float dout_bound = 0.f;              // static bound on max |cotangent of the layer's output| under the unit cotangent (bwd_bounds)
        const unsigned *dout_amax = nullptr; // per-patch max |cotangent of the layer's output|, measured by the launch above, or null
    };
    std::vector<PerLayer> st;
    // from the two-class head to the conv below it: the cotangent of that conv's output exists only as mask bits and one vector
    struct HeadBits {
        const unsigned *bits = nullptr;
        const float *vec = nullptr;
        const unsigned *vec16 = nullptr;
        const unsigned short *vec16c = nullptr;
        float vec_amax = 0.f;
    } head;
    int e3_conv = -1;      // the conv whose backward ran fused with the pool backward steps around it (e3d.hip), or -1
    bool signs(int i) const { return m->last.fwd.signs_ready[i]; }      // the forward pass wrote layer i's sign field
};

// one layer of it.  acc: the launch accumulates into a slice the skip destination wrote; fused: it masked and summed its output
struct BwdStep {
    int i;
    bool prev_is_src, prev_param;
    int acc = 0;
    bool fused = false;
};

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
static bool e3d_bwd_applies(const BwdPass &B, int i, bool prev_is_src) {
    const alq_model *m = B.m;
    const Layer &ly = m->layers[i];
    if (!(ly.spec.type == ALQ_POOL && i >= 3 && !m->sw.no_e3d && two_slot_allowed() && !g_no_f16x2 && !m->sw.no_bound16 && !m->sw.no_signs &&
          !g_dbg_knobs[KNOB_NO_BWD_FUSE] && !g_dbg_knobs[KNOB_NO_POOL_FIRST]))
        return false;
    const Layer &cv = m->layers[i - 1], &p1 = m->layers[i - 2], &c0 = m->layers[i - 3];
    return cv.spec.type == ALQ_CONV && cv.e3b.ok && cv.e3b.d_Whi && cv.spec.relu && B.signs(i - 1) && cv.out.sg && prev_is_src &&
           p1.spec.type == ALQ_POOL && pool_first_ok(p1, c0) && B.st[i - 3].dsum_partial && B.signs(i - 2) && p1.out.sg && p1.spec.k[0] == 2 &&
           ly.spec.k[0] == 2 && ly.spec.k[1] == 2 && ly.spec.k[2] == 2 && ly.lo[0] == 0 && ly.lo[1] == 0 && ly.lo[2] == 0 &&
           ly.dout.D == 8 && ly.dout.H == 8 && ly.dout.W == 8 && ly.dout.C == 16 && ly.dout.cs == 16 && ly.dout.c0 == 0 && !ly.dout.split &&
           cv.dout.cs == 16 && cv.dout.c0 == 0 && !cv.dout.split && cv.out.cs == 16 && cv.out.c0 == 0 && p1.out.cs == 8 && p1.out.c0 == 0 &&
           p1.out.C == 8 && c0.out.D == 32 && B.st[i - 1].dout_bound > 0.f && cv.dsum && c0.dsum;
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

// `hand` (both below): the launch hands per-patch maxima of what it stores to the launch below it
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

// bounds on every layer's output cotangent under the unit cotangent (+1, -1): |d out| of the head = 1; a two-class
// head hands max |W0 - W1| down, a conv / conv_transpose its L1 bound, a pool passes the bound on, a ReLU mask
// cannot raise it; a tensor with several consumers (skip source) collects the sum.  One fp16x2 scale per LAUNCH
// follows from it (igemm4: Igemm2Fuse::in_bound) - no per-patch maxima, no extra pass, batch-invariant results.
static void bwd_bounds(BwdPass &B) {
    const alq_model *m = B.m;
    const int nl = (int)m->layers.size();
    B.st[nl - 1].dout_bound = 1.f;
    for (int i = nl - 1; i >= 1; --i) {
        const Layer &ly = m->layers[i];
        const float bound = B.st[i].dout_bound;
        double inb = bound;
        if (ly.spec.type == ALQ_FC)      // the head: max |W0 - W1|; a hidden fc layer: its L1 bound like a conv's (set with the weights)
            inb = (ly.spec.cout == 2 && ly.fc_wv_amax > 0.f && i == nl - 1) ? (double)ly.fc_wv_amax : (i < nl - 1 ? ly.bwd_l1 * bound : 0.0);
        else if (ly.spec.type != ALQ_POOL) inb = ly.bwd_l1 * bound;
        if (!(inb > 0.0) || bound <= 0.f) inb = 0.0;       // unknown upstream: no bound below either
        // a conv / conv_transpose over a concat: each producer's cotangent under the norm of its own channels (conv_bwd_l1_slices)
        auto add = [&](float &b, double part_l1) {
            const double v = (inb > 0.0 && part_l1 > 0.0 && ly.spec.type != ALQ_FC && ly.spec.type != ALQ_POOL) ? part_l1 * bound : inb;
            b = (b < 0.f || v <= 0.0) ? -1.f : b + (float)(v * (1.0 + 1e-6));
        };
        add(B.st[i - 1].dout_bound, ly.bwd_l1_part[1]);
        if (ly.spec.skip_src >= 0) add(B.st[ly.spec.skip_src].dout_bound, ly.bwd_l1_part[0]);
    }
}

// a pool layer (not on the network input)
static int bwd_pool(BwdPass &B, const BwdStep &s) {
    alq_model *m = B.m;
    alq_ctx *ctx = m->ctx;
    const int i = s.i, N = B.N;
    Layer &ly = m->layers[i];
    if (e3d_bwd_applies(B, i, s.prev_is_src)) {
        Layer &cv = m->layers[i - 1], &p1 = m->layers[i - 2], &c0 = m->layers[i - 3];
        ALQ_TRY(e3d_bwd_launch(ctx, cv.e3b, N, cv.dout.p, ly.dout.p, ly.argmax, cv.out.sg, p1.argmax, p1.out.sg, cv.dsum, c0.dsum, B.st[i - 1].dout_bound, m->sw.e3d_rows != 0));
        m->last.bwd.e3b_form = m->sw.e3d_rows ? 1 : 2;
        B.st[i - 1].delta_ready = true;
        B.st[i - 3].delta_ready = true;
        B.e3_conv = i - 1;
        m->last.bwd.e3b = 1;
        return ALQ_OK;
    }
    if (B.e3_conv >= 0 && i == B.e3_conv - 1) return ALQ_OK;      // the pool below the fused conv: done
    // Every backward op is the LAST writer of its direct input's cotangent (a skip destination
    // wrote its slice earlier), so it can finish that tensor: ReLU-grad mask + channel sums.
    Layer *prev = &m->layers[i - 1];
    BwdPass::PerLayer &pst = B.st[i - 1];
    if (s.prev_param && pool_first_ok(ly, *prev) && (pst.dsum_partial || !s.prev_is_src)) {
        ALQ_TRY(k_pool_bwd_first(ctx, ly.dout, ly.out, ly.argmax, ly.spec.k, prev->out.D, prev->out.H, prev->out.W, N,
                                 prev->dsum, pst.dsum_partial ? 1 : 0, B.signs(i) ? 1 : 0));
        pst.delta_ready = true;
        return ALQ_OK;
    }
    bool fused = false;
    ALQ_TRY(k_pool_bwd(ctx, ly.dout, ly.din, ly.argmax, ly.spec.k, ly.lo, N, s.prev_is_src ? 1 : 0,
                       (s.prev_param && prev->spec.relu) ? &prev->out : nullptr, s.prev_param ? prev->dsum : nullptr,
                       &fused, /*store_din=*/!(s.prev_param && prev->pidx == 0),      // layer 0 only needs the sums
                       /*use_signs=*/(s.prev_param && B.signs(i - 1)) ? 1 : 0));
    if (s.prev_param && fused) pst.delta_ready = true;
    return ALQ_OK;
}

// cotangent w.r.t. the pre-activation + its channel sum (unless the producer already did it), then the layer's box-filter dot products
static int bwd_boxdot(BwdPass &B, const BwdStep &s) {
    alq_model *m = B.m;
    alq_ctx *ctx = m->ctx;
    const int i = s.i, N = B.N;
    Layer &ly = m->layers[i];
    const bool isfc = ly.spec.type == ALQ_FC;
    if (!B.st[i].delta_ready) {
        View dv = isfc ? flat_view(ly.dout) : ly.dout;
        View av = isfc ? flat_view(ly.out) : ly.out;
        ALQ_TRY(k_mask_chansum(ctx, dv, ly.spec.relu ? &av : nullptr, ly.dsum, N));
    }
    // channel sums of the layer input: the producers' osum fields (two for a concat input)
    const float *as1 = ly.asum, *as2 = nullptr;
    if (!isfc) {
        if (i == 0) as1 = ly.in.C == 1 ? B.d_x : ly.asum;
        else as1 = m->layers[i - 1].osum;
        if (ly.spec.skip_src >= 0) as2 = m->layers[ly.spec.skip_src].osum;
    }
    double *Sdst = m->Spart + (size_t)ly.pidx * m->max_batch * m->nslab_max;
    // reads this layer's sums, writes its own slice of Spart: beside the contraction launched below
    SideStream beside(ctx);
    if (ly.spec.type == ALQ_CONVT) {
        ALQ_TRY(k_boxdot_convT(ctx, ly.dsum, as1, as2, ly.in.D, ly.in.H, ly.in.W, ly.spec.k, ly.spec.s, ly.lo, N, Sdst, m->nslab_max));
    } else if (isfc) {
        const int one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
        ALQ_TRY(k_boxdot_conv(ctx, ly.dsum, ly.asum, nullptr, 1, 1, 1, one, zero, N, Sdst, m->nslab_max));
    } else {
        ALQ_TRY(k_boxdot_conv(ctx, ly.dsum, as1, as2, ly.out.D, ly.out.H, ly.out.W, ly.spec.k, ly.lo, N, Sdst, m->nslab_max));
    }
    return ALQ_OK;
}

static int bwd_fc(BwdPass &B, BwdStep &s) {
    alq_model *m = B.m;
    alq_ctx *ctx = m->ctx;
    const int i = s.i, N = B.N;
    Layer &ly = m->layers[i];
    Layer *prev = i > 0 ? &m->layers[i - 1] : nullptr;
    ALQ_REQUIRE(!s.acc, ALQ_EUNSUPPORTED, "layer %d: fc consumer of a skip source", i);
    if (head_bits_apply(m, i, s.prev_param, s.prev_is_src)) {
        {   // the sums feed only the layer's box-filter dot products (same stream, later)
            SideStream beside(ctx);
            ALQ_TRY(k_fc_small_dsum_bits(ctx, ly.fc_maskbits, ly.fc_wv, ly.F, N, prev->dsum));
        }
        B.head = {ly.fc_maskbits, ly.fc_wv, ly.fc_wv16, ly.fc_wv16c, ly.spec.cout == 2 ? ly.fc_wv_amax : 0.f};
        s.fused = true;
    } else if (ly.dense_fc_small) {
        const bool can = s.prev_param && prev->out.cs == prev->out.C;
        ALQ_TRY(k_fc_small_bwd(ctx, ly.dout.p, ly.spec.cout, ly.d_Wp, ly.F, N, ly.din.p,
                               (can && prev->spec.relu) ? prev->out.p : nullptr, can ? prev->dsum : nullptr,
                               can ? prev->out.C : 0, &s.fused));
    } else {
        // a wide fc layer's backward GEMM on fp16 pairs under the static bound on its input cotangent (fcgemm.hip, F16)
        const float bound = B.st[i].dout_bound;
        ALQ_TRY(gemm_launch(ctx, ly.bwd, ly.dout, flat_view(ly.din), nullptr, 0, 0, N, PROF_IGEMM_BWD, nullptr, nullptr,
                            (bound > 0.f && !m->sw.no_bound16) ? bound : 0.f));
    }
    return ALQ_OK;
}

// the epilogue request of a conv / conv_transpose above a parameterised layer: mask and sum that layer's cotangent; false: nothing to ask for
static bool bwd_epilogue_request(BwdPass &B, const BwdStep &s, Igemm2Fuse &fz) {
    alq_model *m = B.m;
    const int nl = (int)m->layers.size(), i = s.i;
    Layer &ly = m->layers[i];
    Layer *prev = &m->layers[i - 1];
    if (!(s.prev_param && !g_dbg_knobs[KNOB_NO_BWD_FUSE])) return false;
    const int Cs = ly.spec.skip_src >= 0 ? m->layers[ly.spec.skip_src].out.C : 0;   // concat: [src | prev]
    if (prev->spec.relu) {
        fz.mask = prev->out.p; fz.mask_cs = prev->out.cs; fz.mask_c0 = prev->out.c0; fz.mask_from = Cs;
        if (B.signs(i - 1)) fz.mask_bits = prev->out.sg;
    }
    if (Cs > 0) { fz.split = Cs; fz.osumB = prev->dsum; } else { fz.osumA = prev->dsum; }
    // the skip source is the first parameterised layer and sits in front of a pool: nothing needs its
    // cotangent except the channel sums, so mask and sum its columns here and do not store them
    if (Cs > 0 && (two_slot_allowed() || ly.din.split) && ly.bwd.p4.ok) {
        const int si = ly.spec.skip_src;
        Layer &sl = m->layers[si];
        const bool next_pool = si + 1 < nl && pool_first_ok(m->layers[si + 1], sl);
        const bool sliced = sl.out.p == prev->out.p && sl.out.cs == prev->out.cs && prev->out.c0 == sl.out.c0 + Cs;
        const bool splitv = ly.in.split == Cs && sl.out.p == ly.in.p;
        if (next_pool && (sliced || splitv) && (Cs & 3) == 0) {
            fz.mask = sl.out.p; fz.mask_cs = sl.out.cs; fz.mask_c0 = sl.out.c0; fz.mask_from = 0;
            fz.mask_bits = (B.signs(si) && (!prev->spec.relu || B.signs(i - 1))) ? sl.out.sg : nullptr;
            if (splitv) { fz.mask_split = Cs; fz.mask_delta = ly.in.delta; }
            if (!prev->spec.relu) fz.mask_to = Cs;
            fz.osumA = sl.dsum; fz.store_from = Cs;
            B.st[si].dsum_partial = true;
        }
    }
    return true;
}

// the cotangent of this layer's output exists only as mask bits and one vector (BwdPass::head)
static int bwd_bits_launch(BwdPass &B, BwdStep &s, Igemm2Fuse &fz, const Igemm2Fuse *fuse) {
    alq_model *m = B.m;
    Layer &ly = m->layers[s.i];
    fz.in_bits = B.head.bits; fz.in_vec = B.head.vec; fz.in_vec_amax = B.head.vec_amax;
    fz.in_vec16 = m->sw.no_presplit ? nullptr : B.head.vec16;
    const unsigned short *vec16c = B.head.vec16c;
    B.head = {};
    const bool c3 = c3d_bwd_applies(m, ly, vec16c, fuse, s.acc);
    m->last.bwd.c3_bwd = c3;
    if (c3) {
        int ex = 0;
        (void)std::frexp(fz.in_vec_amax, &ex);
        ALQ_TRY(c3d_bwd_launch(m->ctx, ly.c3b, B.N, reinterpret_cast<const unsigned char *>(fz.in_bits), vec16c, 14 - ex, fz.mask_bits,
                               ly.din.p + ly.din.delta, fz.osumA, fz.osumB, m->sw.c3_bwd_rows, m->sw.c3_bwd_waves, &m->last.bwd.c3b_grid));
    } else {
        ALQ_TRY(igemm4_launch(m->ctx, ly.bwd.p4, ly.dout, ly.din, nullptr, 0, s.acc, B.N, PROF_IGEMM3_BWD, &fz));
    }
    s.fused = fuse != nullptr;
    return ALQ_OK;
}

// "this launch can take the fp16 split on the two-slot engine": two-slot allowed, plan ok, one patch per tile, not multi, fp16 not disabled
static bool bwd_split16_ok(const Layer &ly) {
    return two_slot_allowed() && ly.bwd.p4.ok && !ly.bwd.p4.multi && ly.bwd.p4.a.PT == 1 && !g_no_f16x2;
}

// Which fp16x2 scale the backward-data launch of layer i gets: the per-patch maxima the launch above measured, the static bound of the
// pass, or none (bf16 triples).  `requested`: the launch has an epilogue request; a static bound without one travels in an otherwise
// empty request (no mask, no sums: the plain epilogue runs), which the fusion knob must allow.  Measured maxima are read by a launch
// that has a request only.  Never for an accumulating launch - a conv right behind a skip source: those run the plain bf16x3
// instantiation, igemm4_launch_impl's `no16`, and must not be routed to an fp16x2-only twin plan.
enum BwdScale { SCALE_NONE, SCALE_MEASURED, SCALE_BOUND };
static BwdScale bwd_scale_choice(const BwdPass &B, const BwdStep &s, bool requested) {
    const Layer &ly = B.m->layers[s.i];
    const BwdPass::PerLayer &st = B.st[s.i];
    const bool bound_ok = st.dout_bound > 0.f && !B.m->sw.no_bound16;
    const bool may_request = requested || !g_dbg_knobs[KNOB_NO_BWD_FUSE];
    if (s.acc) return SCALE_NONE;
    if (bwd_split16_ok(ly)) {
        if (st.dout_amax) return requested ? SCALE_MEASURED : SCALE_NONE;
        return bound_ok && may_request ? SCALE_BOUND : SCALE_NONE;
    }
    // a launch that runs on igemm3's fp16-pair instantiation (no two-slot plan): the same bound
    const bool v3 = !ly.bwd.p4.ok && ly.bwd.p3.ok && ly.bwd.p3.d_W16 && !g_no_f16x2 && two_slot_allowed() && !ly.bwd.pd.ok && !ly.bwd.pfc.ok;
    return v3 && bound_ok && !g_dbg_knobs[KNOB_NO_BWD_FUSE] ? SCALE_BOUND : SCALE_NONE;
}

static int bwd_data_launch(BwdPass &B, BwdStep &s, Igemm2Fuse &fz, const Igemm2Fuse *fuse) {
    alq_model *m = B.m;
    alq_ctx *ctx = m->ctx;
    const int i = s.i, N = B.N, acc = s.acc;
    Layer &ly = m->layers[i];
    Layer *prev = &m->layers[i - 1];
    // Hand the per-patch maxima of what this launch stores to the backward launch below it when that one has
    // an fp16x2 variant (two column tiles, or one with the prefetch on the contracting side).  Not from the
    // mask-bit launch above: its staging side is the critical one and the maxima cost more than they gave.
    // (with a static bound for the launch below, nothing needs to be measured here)
    const bool hand = fuse && bwd_split16_ok(ly) && s.prev_param && !acc && !(B.st[i - 1].dout_bound > 0.f && !m->sw.no_bound16) && prev->pidx > 0 &&
                      prev->bwd.p4.ok && !prev->bwd.p4.multi && prev->bwd.p4.a.PT == 1 && prev->bwd.p4.d_W16 && !prev->dout.split &&
                      ((prev->bwd.p4.NTW == 1 && prev->bwd.p4.fic) || prev->bwd.p4.NTW == 2);
    if (hand) {
        if (!m->amax_a) { ALQ_TRY(m->dalloc(&m->amax_a, (size_t)m->max_batch)); ALQ_TRY(m->dalloc(&m->amax_b, (size_t)m->max_batch)); }
        ALQ_TRY(ensure_amax_tiles(m, (size_t)ly.bwd.p4.a.tpg * 4));
        fz.out_amax = m->amax_tiles;
        fz.amax_from = fz.split > 0 && fz.split < (1 << 29) ? fz.split : 0;       // the slice the layer below reads
    }
    const unsigned *mine = B.st[i].dout_amax;
    const BwdScale scale = bwd_scale_choice(B, s, fuse != nullptr);
    if (scale != SCALE_NONE && !fuse) { fz = Igemm2Fuse(); fuse = &fz; }
    if (scale == SCALE_MEASURED) fz.in_amax = mine;
    if (scale == SCALE_BOUND) fz.in_bound = B.st[i].dout_bound;
    if (t3d_bwd_applies(m, ly, fuse, acc, hand, s.prev_param)) {
        ALQ_TRY(t3d_bwd_launch(ctx, ly.t3b, ly.dout, ly.din, N, fz.in_bound, fz.mask ? fz.mask_bits : nullptr, fz.osumA));
        s.fused = true;
        m->last.bwd.t3b += 1;
    } else if (d3d_bwd_applies(m, ly, fuse, acc, hand)) {
        ALQ_TRY(d3d_bwd_launch(ctx, ly.d3f, N, ly.dout.p, fz.in_bound, ly.din.p, ly.din.p + ly.din.delta, fz.osumB));
        s.fused = true;
        m->last.bwd.d3b = 1;
    } else {
        ALQ_TRY(gemm_launch(ctx, ly.bwd, ly.dout, ly.din, nullptr, 0, acc, N, PROF_IGEMM_BWD, fuse, &s.fused));
    }
    if (hand) {
        // two buffers alternate down the chain: this launch may have read the other one
        unsigned *dst = mine == m->amax_a ? m->amax_b : m->amax_a;
        ALQ_TRY(k_rowmax_u32(ctx, m->amax_tiles, ly.bwd.p4.a.tpg * 4, N, dst));
        B.st[i - 1].dout_amax = dst;
    }
    return ALQ_OK;
}

static int run_backward_main(alq_model *m, const float *d_x, int N) {
    const int nl = (int)m->layers.size();
    ALQ_REQUIRE(m->nclass == 2, ALQ_EUNSUPPORTED, "Fisher scoring is binary (PW_NNAL.py:766), got %d classes", m->nclass);
    ALQ_TRY(k_fill_unit_cotangent(m->ctx, m->dlogits, N));
    m->last.bwd = {};
    BwdPass B{m, d_x, N};
    B.st.resize(nl);
    bwd_bounds(B);
    m->last.bwd.nbounds = nl < 64 ? nl : 64;
    for (int i = 0; i < m->last.bwd.nbounds; ++i) m->last.bwd.dout_bound[i] = B.st[i].dout_bound;
    for (int i = nl - 1; i >= 0; --i) {
        Layer &ly = m->layers[i];
        BwdStep s;
        s.i = i;
        s.prev_is_src = i > 0 && m->layers[i - 1].out_is_skip_src && ly.spec.skip_src < 0;
        s.prev_param = i > 0 && m->layers[i - 1].pidx >= 0 && m->layers[i - 1].spec.type != ALQ_FC;
        if (ly.spec.type == ALQ_POOL) {
            if (i == 0) break;      // a pool on the network input: nothing below takes a cotangent (as in grads.hip)
            ALQ_TRY(bwd_pool(B, s));
            continue;
        }
        ALQ_TRY(bwd_boxdot(B, s));
        if (ly.pidx == 0) break;   // nothing upstream needs a cotangent
        if (i == B.e3_conv) continue;      // its backward-data pass ran inside the fused launch
        s.acc = s.prev_is_src ? 1 : 0;   // the skip destination has already written this slice
        if (ly.spec.type == ALQ_FC) {
            ALQ_TRY(bwd_fc(B, s));
        } else {
            Igemm2Fuse fz;
            const Igemm2Fuse *fuse = bwd_epilogue_request(B, s, fz) ? &fz : nullptr;
            if (B.head.bits) ALQ_TRY(bwd_bits_launch(B, s, fz, fuse));
            else ALQ_TRY(bwd_data_launch(B, s, fz, fuse));
        }
        if (s.prev_param && s.fused) B.st[i - 1].delta_ready = true;
    }
    return ALQ_OK;
}

int run_backward(alq_model *m, const float *d_x, int N) {
    const int rc = run_backward_main(m, d_x, N);
    const int rj = side_join(m->ctx);       // also after a failure: nothing may still run beside the caller's next step
    return rc != ALQ_OK ? rc : rj;
}
