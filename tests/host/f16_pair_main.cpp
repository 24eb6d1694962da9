// Stand-alone driver of csrc/f16_pair.h, the arithmetic of the layer kernels' host weight packers.  Every line of the standard
// input is one array of floats, written as 8-digit hex bit patterns.  Per array the program prints "e <exponent>"
// (f16_pair_exp) and per element "<hi> <lo> <hi> <lo>": the hex bits of f16_pair_split at that exponent for lo_shift 0, then 11.
// tests/test_f16_pair_host.py compares the output with a NumPy restatement of the packers' statement sequence.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "f16_pair.h"

int main() {
    std::string line;
    int arrays = 0;
    while (std::getline(std::cin, line)) {
        std::vector<float> w;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            const unsigned bits = (unsigned)std::strtoul(tok.c_str(), nullptr, 16);
            float f;
            std::memcpy(&f, &bits, 4);
            w.push_back(f);
        }
        const int e = alq::f16_pair_exp(w.data(), w.size());
        std::printf("e %d\n", e);
        for (float x : w) {
            unsigned short h0, l0, h11, l11;
            alq::f16_pair_split(x, e, 0, &h0, &l0);
            alq::f16_pair_split(x, e, 11, &h11, &l11);
            std::printf("%04x %04x %04x %04x\n", h0, l0, h11, l11);
        }
        ++arrays;
    }
    return arrays ? 0 : 1;
}
