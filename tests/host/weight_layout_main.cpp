// Stand-alone driver of csrc/weight_layout.h, the host arithmetic of weight setting.  The standard input is a sequence of
// commands: one line "<name> <ints...>", then the command's float arrays, one per line, as 8-digit hex bit patterns:
//   conv <transposed> <ntaps> <Ci> <Co> | W | b      -> "<bwd_l1 16 hex> <out_l1> <out_bmax>"                    (conv_norms)
//   taps <R> <C> <ntaps> [<tap> ...]    | W          -> the array of transpose_taps (no tap list: all taps)
//   slice <K> <Co> <j> <w>              | B          -> the array of column_slice
//   fc <Co> <D> <H> <W> <C>             | W          -> Wp (fc_to_mem_order), B (transpose_taps of Wp as one tap), "<fc_col_l1 16 hex>";
//                                                       Co = 2: wv, "<amax>" (head_wv); amax > 0 and F % 4 == 0: "e <e>", the words of head_wv16
// tests/test_weight_layout_host.py compares the output with a NumPy restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "weight_layout.h"

static std::vector<float> read_floats() {
    std::string line, tok;
    std::vector<float> w;
    if (!std::getline(std::cin, line)) std::exit(2);
    std::istringstream in(line);
    while (in >> tok) {
        const unsigned bits = (unsigned)std::strtoul(tok.c_str(), nullptr, 16);
        float f;
        std::memcpy(&f, &bits, 4);
        w.push_back(f);
    }
    return w;
}

static unsigned f32_bits(float f) {
    unsigned b;
    std::memcpy(&b, &f, 4);
    return b;
}

static unsigned long long f64_bits(double d) {
    unsigned long long b;
    std::memcpy(&b, &d, 8);
    return b;
}

static void print_floats(const std::vector<float> &v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %08x" : "%08x", f32_bits(v[i]));
    std::printf("\n");
}

static void need(bool ok) {
    if (!ok) std::exit(3);
}

int main() {
    std::string line;
    int commands = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name;
        in >> name;
        std::vector<int> a;
        for (int v; in >> v;) a.push_back(v);
        if (name == "conv") {
            need(a.size() == 4);
            const std::vector<float> W = read_floats(), b = read_floats();
            need(W.size() == (size_t)a[1] * a[2] * a[3] && b.size() == (size_t)a[3]);
            double bwd_l1 = -1;
            float out_l1 = -1.f, out_bmax = -1.f;
            alq::conv_norms(W.data(), b.data(), a[1], a[2], a[3], a[0] != 0, &bwd_l1, &out_l1, &out_bmax);
            std::printf("%016llx %08x %08x\n", f64_bits(bwd_l1), f32_bits(out_l1), f32_bits(out_bmax));
        } else if (name == "taps") {
            need(a.size() >= 3);
            const std::vector<float> W = read_floats();
            const std::vector<int> taps(a.begin() + 3, a.end());
            need(taps.empty() ? W.size() == (size_t)a[0] * a[1] * a[2] : taps.size() == (size_t)a[2]);
            for (int t : taps) need(t >= 0 && (size_t)(t + 1) * a[0] * a[1] <= W.size());
            print_floats(alq::transpose_taps(W.data(), a[0], a[1], a[2], taps.empty() ? nullptr : taps.data()));
        } else if (name == "slice") {
            need(a.size() == 4);
            const std::vector<float> B = read_floats();
            need(B.size() == (size_t)a[0] * a[1] && (a[2] + 1) * a[3] <= a[1]);
            print_floats(alq::column_slice(B, a[0], a[1], a[2], a[3]));
        } else if (name == "fc") {
            need(a.size() == 5);
            const std::vector<float> W = read_floats();
            const int Co = a[0];
            const int64_t F = (int64_t)a[1] * a[2] * a[3] * a[4];
            need(W.size() == (size_t)Co * F);
            const std::vector<float> Wp = alq::fc_to_mem_order(W.data(), Co, a[1], a[2], a[3], a[4]);
            print_floats(Wp);
            print_floats(alq::transpose_taps(Wp.data(), Co, (int)F, 1));
            std::printf("%016llx\n", f64_bits(alq::fc_col_l1(W.data(), Co, F)));
            if (Co == 2) {
                float amax = -1.f;
                const std::vector<float> wv = alq::head_wv(Wp.data(), F, &amax);
                print_floats(wv);
                std::printf("%08x\n", f32_bits(amax));
                if (amax > 0.f && F % 4 == 0) {
                    int e = 0;
                    const std::vector<unsigned> sp = alq::head_wv16(wv, amax, &e);
                    std::printf("e %d\n", e);
                    for (size_t i = 0; i < sp.size(); ++i) std::printf(i ? " %08x" : "%08x", sp[i]);
                    std::printf("\n");
                }
            }
        } else {
            return 4;
        }
        ++commands;
    }
    return commands ? 0 : 1;
}
