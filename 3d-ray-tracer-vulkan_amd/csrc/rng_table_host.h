// rng_table_host.h — the size of the table of scatter draws (option rng_table; rt_rng.h).
// Plain C++ with no HIP in it, so that tools/rng_table_check.cpp runs it under the sanitizers.
//
// The table, planes by bounce: entry k * width * height + s0 holds the point rnd_in_sphere returns for the
// (k + 1)-th scatter of the path whose first seed is s0 = y * width + x (.xyz) and the bits of the seed
// after that call (.w).  The seed before k = 0 is s0 after the primary ray's two draws.  A frame kernel
// reads plane k through a buffer resource over that plane alone, with the 32-bit byte offset s0 << 4: a
// plane holds at most kRngTableMaxPixels entries (2 GB), so the offset never wraps for a pixel of the
// frame, and the hardware's range check covers anything else.
#pragma once
#include <cstdint>

namespace rtamd {

constexpr int kRngTableMaxK = 64;                       // option rng_table's range (max_bounces is not bounded)
constexpr uint64_t kRngTableMaxPixels = 1ull << 27;
constexpr int kRngTableMaxMb = 1 << 20;                 // option rng_table_mb's range (MiB)

// Bytes of the table for a width x height frame and k planes; 0 when there is none (k or a side below 1,
// k above kRngTableMaxK, or more pixels than kRngTableMaxPixels).  64-bit arithmetic: nothing wraps (the
// product of two ints is below 2^62, the result at most 2^27 x 64 x 16 = 2^37).
inline uint64_t rng_table_bytes(int width, int height, int k) {
    if (width < 1 || height < 1 || k < 1 || k > kRngTableMaxK) return 0;
    const uint64_t px = (uint64_t)width * (uint64_t)height;
    if (px > kRngTableMaxPixels) return 0;
    return px * (uint64_t)k * 16u;
}

// Whether a table of `bytes` bytes (> 0) fits under option rng_table_mb (MiB, 0..kRngTableMaxMb).
inline bool rng_table_fits(uint64_t bytes, int cap_mb) {
    return bytes > 0 && cap_mb > 0 && bytes <= (uint64_t)cap_mb << 20;
}

}  // namespace rtamd
