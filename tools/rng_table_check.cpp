// rng_table_check.cpp — csrc/rng_table_host.h on the host alone: the size of the table of scatter draws
// (option rng_table) at its edges and against the option rng_table_mb cap.  It has no HIP
// in it, so it also runs under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I 3d-ray-tracer-vulkan_amd/csrc tools/rng_table_check.cpp -o rng_table_check && ./rng_table_check
#include <climits>
#include <cstdio>

#include "rng_table_host.h"

using namespace rtamd;

static int failures = 0;
#define EXPECT(c)                                                       \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("rng_table_check: line %d: %s\n", __LINE__, #c); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

int main() {
    // the sizes the documents quote
    EXPECT(rng_table_bytes(1920, 1080, 2) == 66355200ull);
    EXPECT(rng_table_bytes(3840, 2160, 2) == 265420800ull);
    EXPECT(rng_table_bytes(1, 1, 1) == 16ull);
    EXPECT(rng_table_bytes(203, 77, 64) == 203ull * 77 * 64 * 16);
    // no table: a side or k below 1, k past the range
    EXPECT(rng_table_bytes(0, 5, 1) == 0 && rng_table_bytes(5, 0, 1) == 0 && rng_table_bytes(5, 5, 0) == 0);
    EXPECT(rng_table_bytes(-3, 5, 1) == 0 && rng_table_bytes(5, -3, 1) == 0 && rng_table_bytes(5, 5, -1) == 0);
    EXPECT(rng_table_bytes(5, 5, kRngTableMaxK) == 5ull * 5 * kRngTableMaxK * 16);
    EXPECT(rng_table_bytes(5, 5, kRngTableMaxK + 1) == 0);
    // the pixel cap, from both sides, and products that would wrap 32 bits or a signed 64
    EXPECT(rng_table_bytes(1 << 14, 1 << 13, kRngTableMaxK) == (1ull << 27) * kRngTableMaxK * 16);
    EXPECT(rng_table_bytes((1 << 14) + 1, 1 << 13, 1) == 0);
    EXPECT(rng_table_bytes(1 << 16, 1 << 16, 1) == 0);
    EXPECT(rng_table_bytes(INT_MAX, INT_MAX, kRngTableMaxK) == 0);
    EXPECT(rng_table_bytes(INT_MAX, 1, 1) == 0 && rng_table_bytes(1, INT_MAX, 1) == 0);
    EXPECT(rng_table_bytes(INT_MIN, INT_MIN, INT_MIN) == 0);
    // every plane's byte size fits the 32-bit buffer range the kernels read it through
    EXPECT(kRngTableMaxPixels * 16 <= (1ull << 31));
    // the cap, in MiB
    EXPECT(!rng_table_fits(0, 512));
    EXPECT(!rng_table_fits(16, 0) && !rng_table_fits(16, -1));
    EXPECT(rng_table_fits(1ull << 20, 1) && !rng_table_fits((1ull << 20) + 16, 1));
    EXPECT(rng_table_fits(66355200ull, 64) && !rng_table_fits(66355200ull, 63));
    EXPECT(rng_table_fits(265420800ull, 512) && !rng_table_fits(265420800ull, 253));
    EXPECT(rng_table_fits((1ull << 27) * kRngTableMaxK * 16, kRngTableMaxMb));
    EXPECT(rng_table_fits(~0ull, INT_MAX) == false);
    if (failures) return 1;
    std::printf("rng_table_check: OK\n");
    return 0;
}
