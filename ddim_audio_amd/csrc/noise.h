// The seeded noise stream, version 1 (ddim_audio_amd/noise.py): Philox4x32-10 (Salmon et al., SC'11)
// and the transform of its four 32-bit words into four fp32 normals.  The only copy of both, and of their composition
// (noise_normals4): noise_kernels.hip fills buffers from it, sde_kernels.hip and pool_kernels.hip draw a step's noise in place.
//
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (q, s, k, tag): q = group of four consecutive elements of one sample, s = global sample index, k = draw index,
//             tag = purpose (0 = the noise a sampler step adds, 1 = the initial x_T)
//   normals = Box-Muller on the word pairs (w0, w1) and (w2, w3), every operation rounded on its own:
//             u = ((wa >> 8) + 1) 2^-24 in (0, 1], v = (wb >> 8) 2^-23 in [0, 2) (both exact), r = sqrtf(-2 logf(u)),
//             outputs r cospi(v), r sinpi(v).  |z| <= sqrt(48 ln 2) = 5.77: the tails are cut there.
// The words are the contract (bit exact); the normals follow logf / sincospif of the ROCm release to their last bit.
#pragma once
#include "common.h"

namespace ddimx {

constexpr unsigned kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;  // round multipliers
constexpr unsigned kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;  // key increments

// ten rounds on the counter c[0..3] in place
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(kPhiloxM0, c[0]), lo0 = kPhiloxM0 * c[0];
        const unsigned hi1 = __umulhi(kPhiloxM1, c[2]), lo1 = kPhiloxM1 * c[2];
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
}

// one word pair -> two normals (accurate logf / sincospif: __logf loses all relative accuracy near u = 1)
__device__ __forceinline__ void noise_pair(unsigned wa, unsigned wb, float& z0, float& z1) {
    const float u = __fmul_rn((float)((wa >> 8) + 1u), 0x1p-24f);
    const float v = __fmul_rn((float)(wb >> 8), 0x1p-23f);
    const float r = sqrtf(__fmul_rn(-2.f, logf(u)));
    float sn, cs;
    sincospif(v, &sn, &cs);
    z0 = __fmul_rn(r, cs);
    z1 = __fmul_rn(r, sn);
}

// the four normals of group q of global sample `sample` at draw `draw`: what noise_fill_kernel<kNoiseNormals> stores there, and
// what a kernel that draws in place adds -- one function, so the two cannot differ
__device__ __forceinline__ void noise_normals4(unsigned q, unsigned sample, unsigned draw, unsigned tag, unsigned k0, unsigned k1,
                                               float z[4]) {
    unsigned w[4] = {q, sample, draw, tag};
    philox4x32_10(w, k0, k1);
    noise_pair(w[0], w[1], z[0], z[1]);
    noise_pair(w[2], w[3], z[2], z[3]);
}

// the Rademacher probe of the likelihood (likelihood_kernels.hip, include/features/lkx_likelihood.h): the four signs of group q of
// global sample `sample` for probe index `probe`, +1 where bit 31 of the word is clear.  The fill and the update both call this.
constexpr unsigned kNoiseTagProbe = 3u;  // tags 0 to 2: a step's noise, the initial x_T, the Brownian path
__device__ __forceinline__ float probe_sign(unsigned word) { return (word >> 31) ? -1.f : 1.f; }
__device__ __forceinline__ void probe_signs4(unsigned q, unsigned sample, unsigned probe, unsigned k0, unsigned k1, float r[4]) {
    unsigned w[4] = {q, sample, probe, kNoiseTagProbe};
    philox4x32_10(w, k0, k1);
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = probe_sign(w[j]);
}

}  // namespace ddimx
