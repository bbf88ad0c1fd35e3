// grad_fixed.h on the host (tests/test_radiance_grad_api.py): reads commands from stdin, one per line, doubles as 16 hex
// digits of their bit pattern.
//   S x0 x1 ...   the sum of the doubles in this order: prints the rounded sum's bits, or "nan" when fix_from_double
//                 refused one of them (what a row's NaN flag records)
//   C x           the conversion of one double: prints "ok w2 w1 w0" (hex limbs) or "refused"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "grad_fixed.h"

static double from_hex(const std::string& s) {
    const uint64_t b = std::strtoull(s.c_str(), nullptr, 16);
    double x;
    std::memcpy(&x, &b, sizeof x);
    return x;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        in >> cmd;
        if (cmd == "S") {
            art::Fix192 sum{{0, 0, 0}};
            bool bad = false;
            while (in >> tok) {
                art::Fix192 f;
                if (art::fix_from_double(from_hex(tok), f)) art::fix_add(sum, f);
                else bad = true;
            }
            const double r = art::fix_to_double(sum);
            uint64_t b;
            std::memcpy(&b, &r, sizeof b);
            if (bad) std::printf("nan\n");
            else std::printf("%016" PRIx64 "\n", b);
        } else if (cmd == "C") {
            in >> tok;
            art::Fix192 f;
            if (art::fix_from_double(from_hex(tok), f)) std::printf("ok %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", f.w[2], f.w[1], f.w[0]);
            else std::printf("refused\n");
        }
    }
    return 0;
}
