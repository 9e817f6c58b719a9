// l2a_philox.h - Philox4x32-10 (Salmon et al., SC'11) for the device-RNG controller step: host AND device evaluate the same
// integer rounds and the same fp32 map, so the host can recompute any candidate's action from (seed, element index) - the winner's
// first action needs no gather launch and no device-to-host copy.  (l2a_cem.hip keeps its own copy for the CEM normals; the uniform
// stream carries another domain word, the two never collide.)
#pragma once

__host__ __device__ inline void l2a_philox4x32_10(unsigned long long seed, unsigned long long ctr, unsigned int domain,
                                                  unsigned int (&c)[4]) {
    c[0] = (unsigned int)ctr; c[1] = (unsigned int)(ctr >> 32); c[2] = domain; c[3] = 0u;
    unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned int hi0 = (unsigned int)(p0 >> 32), lo0 = (unsigned int)p0;
        const unsigned int hi1 = (unsigned int)(p1 >> 32), lo1 = (unsigned int)p1;
        c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

#define L2A_PHILOX_UNIFORM 0x756e6966u      // 'unif'

// word -> low + range * u, u = (word >> 8) / 2^24 in [0, 1): exact conversions and ONE fused multiply-add (v_fma_f32 on the device,
// libm's correctly rounded fmaf on the host): the same bits on both sides
__host__ __device__ inline float l2a_uniform_from_word(unsigned int w, float low, float range) {
    const float u = (float)(w >> 8) * (1.0f / 16777216.0f);
    return fmaf(range, u, low);
}

// element e of the stream that starts at `offset` (both in elements; four elements share a Philox block)
__host__ __device__ inline float l2a_philox_uniform(unsigned long long seed, unsigned long long e, float low, float range) {
    unsigned int c[4];
    l2a_philox4x32_10(seed, e >> 2, L2A_PHILOX_UNIFORM, c);
    return l2a_uniform_from_word(c[e & 3ull], low, range);
}

#define L2A_PHILOX_PERM 0x7065726du         // 'perm' .. 'perm' + 3: the TS1 particle shuffle's four word groups
#define L2A_PERM_MAX_E 16
#define L2A_PERM_SLOT_LIMIT (1ull << 33)    // (step, env) slots: the slot fills the counter's 33 bits above the candidate's 31

// The permutation of 0 .. E - 1 (1 <= E <= 16) of horizon boundary `slot` = offset + t m + i and candidate gj < 2^31, packed four
// bits per entry: entry e - bits 4 e .. 4 e + 3 - is the block the particle that lands in block e comes from.  Fisher-Yates from
// the identity, k = E - 1 down to 1: r = (word (k + 1)) >> 32 (64-bit product), entries k and r change places.  Draw d = E - 1 - k
// is word d & 3 of l2a_philox4x32_10(seed, slot << 31 | gj, L2A_PHILOX_PERM + (d >> 2)).  A 32-bit word leaves r a bias of at most
// k / 2^32 against the uniform draw.  Fully unrolled: the words and the table stay in registers.
__host__ __device__ inline unsigned long long l2a_particle_perm_pack(unsigned long long seed, unsigned long long slot,
                                                                     unsigned int gj, int E) {
    unsigned long long p = 0xfedcba9876543210ull;
    const unsigned long long ctr = (slot << 31) | (unsigned long long)gj;
#pragma unroll
    for (int q = 0; q < (L2A_PERM_MAX_E - 1 + 3) / 4; ++q) {
        if (4 * q >= E - 1) break;
        unsigned int c[4];
        l2a_philox4x32_10(seed, ctr, L2A_PHILOX_PERM + (unsigned int)q, c);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int k = E - 1 - (4 * q + w);
            if (k >= 1) {
                const int r = (int)(((unsigned long long)c[w] * (unsigned long long)(k + 1)) >> 32);
                const unsigned long long x = ((p >> (4 * k)) ^ (p >> (4 * r))) & 15ull;
                p ^= (x << (4 * k)) | (x << (4 * r));
            }
        }
    }
    return p;
}
