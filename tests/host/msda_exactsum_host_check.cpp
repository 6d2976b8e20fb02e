// csrc/msda_exactsum.h on the host: the fixed-point accumulator behind the exact MSDA backward, driven from stdin so that
// tests/test_msda_exact_ref.py can compare it bit for bit with a Fraction model.  One request per line, fp32 bit patterns in hex:
//   S b1 b2 ...       one accumulator, the numbers added in the order given
//   M k b1 b2 ...     k accumulators, number i goes to accumulator i % k, then accumulators k-1 .. 1 are merged into 0
// Answer per line: the bits of round_to_float(), 8 hex digits.  The last line printed is "msda_exactsum_host_check: ok".
// No HIP, no GPU: tools/msda_exactsum_host_check.sh builds it (by default under AddressSanitizer + UBSan).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "msda_exactsum.h"

int main()
{
    using semidetr_exact::ExactSum;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        size_t k = 1;
        if (op == "M") {
            if (!(in >> k) || k == 0 || k > 4096) {
                std::fprintf(stderr, "bad accumulator count in: %s\n", line.c_str());
                return 2;
            }
        } else if (op != "S") {
            std::fprintf(stderr, "unknown request: %s\n", line.c_str());
            return 2;
        }
        std::vector<ExactSum> acc(k);
        for (auto &a : acc) a.clear();
        std::string tok;
        size_t i = 0;
        while (in >> tok) {
            const uint32_t bits = (uint32_t)std::strtoul(tok.c_str(), nullptr, 16);
            acc[i++ % k].add(semidetr_exact::bits_float(bits));
        }
        for (size_t j = k - 1; j >= 1; --j) acc[0].merge(acc[j]);
        std::printf("%08x\n", semidetr_exact::float_bits(acc[0].round_to_float()));
    }
    std::printf("msda_exactsum_host_check: ok\n");
    return 0;
}
