// Philox4x32-10 (Salmon et al., SC'11; the counter-based generator torch and cuRAND use): ten rounds on a 128-bit counter under a 64-bit
// key.  Shared by the in-launch latent draw of the lagged form (role32.hpp latents32) and the latent-set generator (latents.hip).
// Host and device: tests/latents_host.hip runs the generator's work items on the CPU.
#pragma once

__host__ __device__ inline void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (unsigned)p1; c[2] = n2; c[3] = (unsigned)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
