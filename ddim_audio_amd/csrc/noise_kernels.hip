// Seeded device noise (ddim_audio_amd/noise.py): fills a [B][per_sample] buffer from the counter-based stream of noise.h.
//
// The value of element i of global sample s at draw k is a pure function of (seed, s, k, i): no state, no atomics, no LDS, no
// dependence on the grid or on B.  The draw index is draw_base + step[0], read when the launch RUNS, so one captured launch
// serves every replay of a sampler step (the device step counter the coefficient tables use).  The grid is (blocks per sample, B)
// like inpaint_update_kernel's: every block belongs to one sample, whose groups of four it walks grid-stride, consecutive threads
// on consecutive groups; one Philox call and one 16-byte store per thread and trip.  Plain cacheable stores: the update kernel
// reads the buffer next.
#include "noise_kernels.h"
#include "noise.h"

namespace ddimx {

template <int KIND>
__global__ void __launch_bounds__(kNoiseThreads) noise_fill_kernel(void* __restrict__ out, long long n4, unsigned k0, unsigned k1,
                                                                   unsigned first_sample, const int* __restrict__ step,
                                                                   unsigned draw_base, unsigned tag) {
    const unsigned sample = first_sample + blockIdx.y;
    const unsigned draw = draw_base + (step ? (unsigned)step[0] : 0u);
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kNoiseThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kNoiseThreads) {
        if (KIND == kNoiseWords) {
            unsigned c[4] = {(unsigned)i, sample, draw, tag};
            philox4x32_10(c, k0, k1);
            ((uint4*)out)[base + (size_t)i] = make_uint4(c[0], c[1], c[2], c[3]);
        } else {
            float z[4];
            noise_normals4((unsigned)i, sample, draw, tag, k0, k1, z);
            store4((float*)out, base + (size_t)i, z);
        }
    }
}

hipError_t noise_fill_launch(void* out, int B, long long per_sample, unsigned long long seed, unsigned first_sample, const int* step,
                             unsigned draw_base, unsigned tag, int kind, hipStream_t s) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4) return hipErrorInvalidValue;
    const long long n4 = per_sample / 4;
    if (n4 > (1LL << 32) || (unsigned long long)first_sample + (unsigned long long)B > (1ULL << 32)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kNoiseThreads);
    const unsigned k0 = (unsigned)(seed & 0xffffffffULL), k1 = (unsigned)(seed >> 32);
    if (kind == kNoiseNormals)
        hipLaunchKernelGGL((noise_fill_kernel<kNoiseNormals>), grid, block, 0, s, out, n4, k0, k1, first_sample, step, draw_base, tag);
    else if (kind == kNoiseWords)
        hipLaunchKernelGGL((noise_fill_kernel<kNoiseWords>), grid, block, 0, s, out, n4, k0, k1, first_sample, step, draw_base, tag);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace ddimx
