// vanilla_blocked_check.hip -- the blocked fp32 vanilla kernel outside the library (tests/test_vanilla_blocked_isa.py):
//   * compiled for the device alone (-S) it holds vanilla_f32_blocked_kernel<false / true> and nothing else: the listing the
//     instruction counts are read from;
//   * compiled as a program it prints what csrc/mc_launch_shape.hpp's vanilla_blocking decides for a list of segments, one line
//     per case "unit_lo n_units stride -> head sweeps extra blocked rest_trips".  Host code only; nothing is launched.
#include <cstdio>
#include <cstdlib>

#include "mc_launch_shape.hpp"

namespace mc {
template __global__ void vanilla_f32_blocked_kernel<false>(const Tail, const VanillaF32, const Work, const VanillaBlocking);
template __global__ void vanilla_f32_blocked_kernel<true>(const Tail, const VanillaF32, const Work, const VanillaBlocking);
}  // namespace mc

int main(int argc, char **argv)
{
    for (int i = 1; i + 2 < argc; i += 3) {
        const uint32_t lo = (uint32_t)strtoull(argv[i], nullptr, 10), n = (uint32_t)strtoull(argv[i + 1], nullptr, 10),
                       stride = (uint32_t)strtoull(argv[i + 2], nullptr, 10);
        const mc::VanillaBlocking b = mc::vanilla_blocking(lo, n, stride);
        printf("%u %u %u -> %u %u %u %u %u\n", lo, n, stride, b.head, b.sweeps, b.extra, b.blocked, b.rest_trips);
    }
    return 0;
}
