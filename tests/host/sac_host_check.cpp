// sac_host_check.cpp — the plane search's sampler and plane of three points (rgbd360_amd/csrc/host/sac_sample.h) as plain
// C++: a stand-alone program, built by tests/test_sac_host.py with g++ -ffp-contract=off under the address and
// undefined-behaviour sanitizers.  It reads requests from standard input and answers one line each:
//   s <seed> <p> <h> <m>          ->  <a> <b> <c>                 three pool positions
//   t <9 float32 bit patterns>    ->  <nx> <ny> <nz> <d>          hex floats, or "degenerate"
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "host/sac_sample.h"

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 's') {
            uint64_t seed, m;
            uint32_t p, h;
            if (scanf("%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu64, &seed, &p, &h, &m) != 4 || m < 3) return 2;
            uint64_t pos[3];
            sac_sample3(seed, p, h, m, pos);
            for (int k = 0; k < 3; ++k)
                if (pos[k] >= m) return 3;
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", pos[0], pos[1], pos[2]);
        } else if (kind == 't') {
            float q[3][3];
            for (int i = 0; i < 9; ++i) {
                uint32_t bits;
                if (scanf("%" SCNx32, &bits) != 1) return 2;
                memcpy(&q[i / 3][i % 3], &bits, 4);
            }
            double c[4];
            if (sac_plane3(q[0], q[1], q[2], c)) printf("%a %a %a %a\n", c[0], c[1], c[2], c[3]);
            else printf("degenerate\n");
        } else {
            return 2;
        }
    }
    return 0;
}
