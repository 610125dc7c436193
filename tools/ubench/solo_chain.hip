// solo_chain.hip — microbenchmark (analysis aid for option solo_lanes, DESIGN.md
// §7): the latency of ONE ray's dependent record chain on gfx950, the next
// record's index coming from the record just read, when the record comes
//   s32 / s64: through the constant address space (scalar cache), one or two
//              32-B scalar loads per step (a box / a leaf of the accel records);
//   v32 / v64: by 2 or 4 16-B buffer loads of a single active lane;
// each alone (one chain wave in 32 one-wave workgroups, the others idle), with
// the other 31 workgroups running ta_cost.hip's divergent 16-B load loop, which
// keeps every CU's texture addresser busy, and crowded (all 32 workgroups chain
// waves of the same arm: every wave slot of a CU on the same path).  Tables of
// 2, 8 and 64 MB of 64-B records, linked in one full cycle (an LCG), so a chain
// never returns to a record it has read.  Prints ns per step over the chain
// waves (mean, min, max) and how long the busy waves ran (they must outlast
// the chains).
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/solo_chain.hip -o tools/ubench/solo_chain
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

constexpr int kBusyTable = 16384;   // float4 entries: 256 KB (ta_cost.hip)
constexpr int kGroup = 32;          // one chain wave per 32 one-wave workgroups

typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x8 srec(const uint32_t* t, unsigned byte) {
    typedef const __attribute__((address_space(4))) char* cbytes;
    return *(const __attribute__((address_space(4))) u32x8*)((cbytes)t + byte);
}

__device__ __forceinline__ unsigned sum4(u32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ unsigned sum8(u32x8 v) {
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// ARM 0: s32, 1: s64, 2: v32, 3: v64.  tab: 64-B records at a 32-B aligned
// (not 64-B aligned) address, as a leaf of the accel records may lie: the two
// halves of a record then come by two 32-B scalar loads, not one of 64 B.
template <int ARM>
__global__ __launch_bounds__(64) void chain(const uint32_t* __restrict__ tab, unsigned mask, int steps,
                                            const float4* __restrict__ busy_t, int busy_iters, int group,
                                            unsigned long long* out, unsigned long long* busy_out, float* sink) {
    const int lane = threadIdx.x;
    if (blockIdx.x % group != 0) {
        if (busy_iters == 0) return;
        // ta_cost.hip, width 16, lane stride 64 B: 8 independent loads per round
        const unsigned long long t0 = wall_clock64();
        float acc = 0.f;
        unsigned base = (blockIdx.x * 977u) & (kBusyTable - 1);
        for (int i = 0; i < busy_iters; ++i) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                unsigned j = (base + (unsigned)(i * 8 + k) * 67u + ((unsigned)lane << 2)) & (kBusyTable - 1);
                const float4 v = busy_t[j];
                acc += (v.x + v.y) + (v.z + v.w);
            }
        }
        if (lane == 0 && blockIdx.x % group == 1) busy_out[blockIdx.x / group] = wall_clock64() - t0;
        if (acc == 12345.f) sink[0] = acc;
        return;
    }
    unsigned i = (blockIdx.x * 7919u + 12345u) & mask;
    unsigned acc = 0;
    const unsigned long long t0 = wall_clock64();
    if (ARM < 2) {
        // (as in solo_walk, whether the second half is read is known from the
        // record before: a flag in the data, always set, so the two loads stay two)
        bool leaf = ARM == 1;
        for (int s = 0; s < steps; ++s) {
            const u32x8 r = srec(tab, i << 6);
            acc += sum8(r);
            if (leaf) {
                const u32x8 q = srec(tab, (i << 6) + 32u);
                acc += sum8(q);
            }
            i = r[1] & mask;                      // the next record comes from the data
            leaf = ARM == 1 && (r[2] & 1u) != 0u;
        }
    } else if (lane == 0) {
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(tab), 0, (int)((mask + 1u) << 6), 0x00020000);
        for (int s = 0; s < steps; ++s) {
            const int off = (int)(i << 6);
            const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
            const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 0);
            acc += sum4(a) + sum4(b);
            if (ARM == 3) {
                const u32x4 c = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 32, 0, 0);
                const u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 48, 0, 0);
                acc += sum4(c) + sum4(d);
            }
            i = a[1] & mask;
        }
    }
    const unsigned long long t1 = wall_clock64();
    if (lane == 0) out[blockIdx.x / group] = t1 - t0;
    if (acc == 0x12345678u) sink[1] = (float)acc;
}

int main(int argc, char** argv) {
    const int steps = argc > 1 ? std::atoi(argv[1]) : 2000;
    const int busy_iters = argc > 2 ? std::atoi(argv[2]) : 4000;
    int dev = 0, n_cu = 0, khz = 0;
    CHECK(hipGetDevice(&dev));
    CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
    const int groups = n_cu;                       // one chain wave per CU on average
    float4* busy_t = nullptr;
    float* sink = nullptr;
    unsigned long long *out = nullptr, *busy_out = nullptr;
    CHECK(hipMalloc(&busy_t, kBusyTable * sizeof(float4)));
    CHECK(hipMemset(busy_t, 0, kBusyTable * sizeof(float4)));
    CHECK(hipMalloc(&sink, 64));
    CHECK(hipMalloc(&out, groups * kGroup * 8));
    CHECK(hipMalloc(&busy_out, groups * kGroup * 8));
    const char* names[4] = {"s32 (1 scalar x8)", "s64 (2 scalar x8)", "v32 (2 buffer x4)", "v64 (4 buffer x4)"};
    for (size_t mb : {2, 8, 64}) {
        const unsigned n_rec = (unsigned)(mb * 1024 * 1024 / 64);
        std::vector<uint32_t> h((size_t)n_rec * 16 + 16, 1u);   // (+ 64 B: the records start 32 B in)
        for (size_t r = 0; r < n_rec; ++r)
            h[8 + r * 16 + 1] = (uint32_t)((r * 1664525ull + 1013904223ull) % n_rec);   // full period: n_rec = 2^k
        uint32_t* d = nullptr;
        CHECK(hipMalloc(&d, h.size() * 4));
        CHECK(hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        for (int busy : {0, 1, 2})                              // alone, TA busy, crowded
            for (int arm = 0; arm < 4; ++arm) {
                const int group = busy == 2 ? 1 : kGroup, waves = groups * kGroup / group;
                std::vector<unsigned long long> t(waves), b(waves);
                for (int rep = 0; rep < 2; ++rep) {            // the second launch is reported
                    CHECK(hipMemset(busy_out, 0, groups * kGroup * 8));
                    auto k = arm == 0 ? chain<0> : arm == 1 ? chain<1> : arm == 2 ? chain<2> : chain<3>;
                    hipLaunchKernelGGL(k, dim3(groups * kGroup), dim3(64), 0, 0, d + 8, n_rec - 1, steps, busy_t,
                                       busy == 1 ? busy_iters : 0, group, out, busy_out, sink);
                    CHECK(hipDeviceSynchronize());
                }
                CHECK(hipMemcpy(t.data(), out, waves * 8, hipMemcpyDeviceToHost));
                CHECK(hipMemcpy(b.data(), busy_out, waves * 8, hipMemcpyDeviceToHost));
                const double ns = 1e6 / khz / steps;
                double sum = 0, bsum = 0;
                for (int g = 0; g < waves; ++g) { sum += (double)t[g]; bsum += (double)b[g]; }
                std::printf("table %2zu MB  %s  %s: %6.0f ns/step (min %.0f max %.0f); chain %.2f ms, busy waves %.2f ms\n",
                            mb, busy == 2 ? "crowded" : busy ? "TA busy" : "alone  ", names[arm], sum / waves * ns,
                            (double)*std::min_element(t.begin(), t.end()) * ns,
                            (double)*std::max_element(t.begin(), t.end()) * ns, sum / waves / khz,
                            bsum / waves / khz);
            }
        CHECK(hipFree(d));
    }
    return 0;
}
