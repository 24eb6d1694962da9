// Stand-alone driver of csrc/model_plan.h, the host arithmetic of model creation.  The standard input is a sequence of commands:
//   pads <in> <k> <s>                              -> "<out> <lo>"                                               (same_pads)
//   plan <max_batch> <D> <H> <W> <C> <n> <descs>   then n lines "<type> <cout> <k x3> <s x3> <relu> <skip_src>"  (plan_shapes)
//     -> "rc <code> <last message of set_error, empty if none>"; for ALQ_OK also
//        "model <L> <dense> <V> <nclass> <max_batch>" and per layer
//        "layer <i> <in D H W C> <out D H W C> <lo x3> <pidx> <w_elems> <b_elems> <F> <src_of> <dest_of>";
//        descs != 0: every descriptor builder's result for every conv, conv_transpose and fc layer,
//        "desc <name> <i> <ID IH IW Ci> <OD OH OW Co> <MD MH MW> <sm> <so> <ooff x3> <ntaps> {<tz> <ty> <tx>} [<class tap index>...]"
//        "geom <name> <i> <kind> <cls x3> <ID IH IW Ci> <OD OH OW Co> <k x3> <s x3> <lo x3> <flipped>"
// tests/test_model_plan_host.py compares the output with restatements in Python.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "model_plan.h"

static char g_msg[1024];

namespace alq {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
}
}  // namespace alq

static void need(bool ok) {
    if (!ok) std::exit(3);
}

static std::vector<long long> read_ints(std::istream &in) {
    std::vector<long long> a;
    for (long long v; in >> v;) a.push_back(v);
    return a;
}

static void print_desc(const char *name, int i, const alq::ConvDesc &d, const std::vector<int> *cls_taps = nullptr) {
    std::printf("desc %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu", name, i, d.ID, d.IH, d.IW, d.Ci, d.OD, d.OH, d.OW, d.Co,
                d.MD, d.MH, d.MW, d.sm, d.so, d.ooff[0], d.ooff[1], d.ooff[2], d.tz.size());
    need(d.ty.size() == d.tz.size() && d.tx.size() == d.tz.size() && (!cls_taps || cls_taps->size() == d.tz.size()));
    for (size_t t = 0; t < d.tz.size(); ++t) std::printf(" %d %d %d", d.tz[t], d.ty[t], d.tx[t]);
    if (cls_taps)
        for (int t : *cls_taps) std::printf(" %d", t);
    std::printf("\n");
}

static void print_geom(const char *name, int i, const alq::G4Geom &g) {
    need(g.flops_per_patch == 0);
    std::printf("geom %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", name, i, g.kind, g.cls[0], g.cls[1], g.cls[2],
                g.ID, g.IH, g.IW, g.Ci, g.OD, g.OH, g.OW, g.Co, g.k[0], g.k[1], g.k[2], g.s[0], g.s[1], g.s[2], g.lo[0], g.lo[1], g.lo[2],
                (int)g.flipped);
}

static void print_descs(const std::vector<alq_layer_t> &specs, const alq::ModelShape &ms) {
    for (size_t li = 0; li < specs.size(); ++li) {
        const alq_layer_t &sp = specs[li];
        const alq::LayerShape &ls = ms.layers[li];
        const int i = (int)li;
        if (sp.type == ALQ_CONV) {
            print_desc("conv_fwd", i, alq::conv_fwd_desc(ls.in, ls.out, sp, ls.lo));
            print_geom("conv_fwd", i, alq::conv_fwd_geom(ls.in, ls.out, sp, ls.lo));
            print_desc("conv_bwd", i, alq::conv_bwd_desc(ls.in, ls.out, sp, ls.lo));
            print_geom("conv_bwd", i, alq::conv_bwd_geom(ls.in, ls.out, sp, ls.lo));
        } else if (sp.type == ALQ_CONVT) {
            for (int cz = 0; cz < alq::convt_classes_z(ls.in, sp); ++cz)
                for (int cy = 0; cy < sp.s[1]; ++cy)
                    for (int cx = 0; cx < sp.s[2]; ++cx) {
                        std::vector<int> taps;
                        const alq::ConvDesc d = alq::convt_class_desc(ls.in, ls.out, sp, ls.lo, cz, cy, cx, &taps);
                        print_desc("convt_class", i, d, &taps);
                        print_geom("convt_class", i, alq::convt_class_geom(ls.in, ls.out, sp, ls.lo, cz, cy, cx));
                    }
            print_geom("convt_all", i, alq::convt_all_geom(ls.in, ls.out, sp, ls.lo, 2));
            print_geom("convt_all", i, alq::convt_all_geom(ls.in, ls.out, sp, ls.lo, 4));
            print_desc("convt_bwd", i, alq::convt_bwd_desc(ls.in, ls.out, sp, ls.lo));
            print_geom("convt_bwd", i, alq::convt_bwd_geom(ls.in, ls.out, sp, ls.lo));
        } else if (sp.type == ALQ_FC) {
            print_desc("fc_fwd", i, alq::fc_fwd_desc(ls.F, sp.cout));
            print_desc("fc_bwd", i, alq::fc_bwd_desc(ls.F, sp.cout));
        }
    }
}

int main() {
    std::string line;
    int commands = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name;
        in >> name;
        const std::vector<long long> a = read_ints(in);
        if (name == "pads") {
            need(a.size() == 3);
            int out = -1, lo = -1;
            alq::same_pads((int)a[0], (int)a[1], (int)a[2], &out, &lo);
            std::printf("%d %d\n", out, lo);
        } else if (name == "plan") {
            need(a.size() == 7 && a[5] >= 0 && a[5] <= 64);
            const int32_t in_dims[4] = {(int32_t)a[1], (int32_t)a[2], (int32_t)a[3], (int32_t)a[4]};
            std::vector<alq_layer_t> specs((size_t)a[5]);
            for (alq_layer_t &sp : specs) {
                need((bool)std::getline(std::cin, line));
                std::istringstream ls(line);
                const std::vector<long long> v = read_ints(ls);
                need(v.size() == 10);
                sp.type = (int32_t)v[0]; sp.cout = (int32_t)v[1];
                for (int q = 0; q < 3; ++q) { sp.k[q] = (int32_t)v[2 + q]; sp.s[q] = (int32_t)v[5 + q]; }
                sp.relu = (int32_t)v[8]; sp.skip_src = (int32_t)v[9];
            }
            g_msg[0] = 0;
            alq::ModelShape ms;
            const int rc = alq::plan_shapes(specs.data(), (int)specs.size(), in_dims, a[1] * a[2] * a[3] * a[4], (int)a[0], &ms);
            std::printf("rc %d %s\n", rc, g_msg);
            if (rc == ALQ_OK) {
                std::printf("model %d %d %lld %d %d\n", ms.L, (int)ms.dense, (long long)ms.V, ms.nclass, ms.max_batch);
                need(ms.layers.size() == specs.size() && ms.src_of.size() == specs.size() && ms.dest_of.size() == specs.size());
                for (size_t i = 0; i < specs.size(); ++i) {
                    const alq::LayerShape &l = ms.layers[i];
                    std::printf("layer %zu %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %d %d\n", i, l.in.D, l.in.H, l.in.W, l.in.C, l.out.D,
                                l.out.H, l.out.W, l.out.C, l.lo[0], l.lo[1], l.lo[2], l.pidx, (long long)l.w_elems, (long long)l.b_elems,
                                (long long)l.F, ms.src_of[i], ms.dest_of[i]);
                }
                if (a[6]) print_descs(specs, ms);
            }
        } else {
            return 4;
        }
        ++commands;
    }
    return commands ? 0 : 1;
}
