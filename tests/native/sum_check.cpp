// Host-only run of bf_sum.h (tests/test_exact_sum_host.py).  Input, per set: a line "n_cells n", then n lines "cell bits" (the fp32
// bit pattern as a decimal integer); output: the resolved bit pattern of every cell, one per line.
#include <cstdio>
#include <vector>

#include "../../beifong_amd/csrc/bf_sum.h"

int main() {
    unsigned n_cells, n;
    while (std::scanf("%u %u", &n_cells, &n) == 2) {
        std::vector<int64_t> limbs((size_t) n_cells * bfs::kLimbs, 0);
        for (unsigned i = 0; i < n; ++i) {
            unsigned cell, bits;
            if (std::scanf("%u %u", &cell, &bits) != 2 || cell >= n_cells || !bfs::finite_bits(bits)) return 1;
            bfs::add(&limbs[(size_t) cell * bfs::kLimbs], bits);
        }
        for (unsigned c = 0; c < n_cells; ++c) std::printf("%u\n", bfs::resolve(&limbs[(size_t) c * bfs::kLimbs]).bits);
    }
    return 0;
}
