// l2a_philox.h - Philox4x32-10 (Salmon et al., SC'11) for the device-RNG controller step: host AND device evaluate the same
// integer rounds and the same fp32 map, so the host can recompute any candidate's action from (seed, element index) - the winner's
// first action needs no gather launch and no device-to-host copy.  The planners' normal stream (l2a_philox_normal) is built on the
// same rounds; the streams carry different domain words and never collide.
#pragma once

// One round; the caller bumps the key (k0 += 0x9E3779B9u, k1 += 0xBB67AE85u) between rounds.
__host__ __device__ __forceinline__ void l2a_philox_round(unsigned int (&c)[4], unsigned int k0, unsigned int k1) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned int hi0 = (unsigned int)(p0 >> 32), lo0 = (unsigned int)p0;
    const unsigned int hi1 = (unsigned int)(p1 >> 32), lo1 = (unsigned int)p1;
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
}

__host__ __device__ inline void l2a_philox4x32_10(unsigned long long seed, unsigned long long ctr, unsigned int domain,
                                                  unsigned int (&c)[4]) {
    c[0] = (unsigned int)ctr; c[1] = (unsigned int)(ctr >> 32); c[2] = domain; c[3] = 0u;
    unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        l2a_philox_round(c, k0, k1);
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

#define L2A_PHILOX_NORMAL 0x4c32614du       // 'L2aM'

// The planners' standard normal (l2a_cem.hip, l2a_mppi.hip, l2a_icem.hip, l2a_policy.hip): Box-Muller on two uniforms in (0, 1] of
// block `index` - a pure function of (seed, index), so all ranks of a sharded plan generate the same numbers without talking.
// MAINTENANCE: this function carries no contraction pragma of its own - it is compiled as the including unit is at the point of
// the #include.  l2a_cem.hip and l2a_icem.hip contract (hipcc's default), and their streams are bit-equal; -ffp-contract=off
// (l2a_mppi.hip, l2a_policy.hip) also keeps the math library's multiply-adds inside logf / cosf from fusing, which moves a normal
// by an ulp here and there.  So l2a_cem.hip, l2a_icem.hip and l2a_mppi.hip include this header ABOVE every `#pragma clang fp
// contract(off)` of theirs, and in l2a_icem.hip EVERYTHING ELSE that does floating-point arithmetic - every kernel body, every
// device helper a kernel calls, the host arithmetic that forms `c` in l2a_icem_sample - MUST open with that pragma: the unit's
// flags do not switch contraction off, and a helper without it would fuse silently.
__device__ __forceinline__ float l2a_philox_normal(unsigned long long seed, unsigned long long index) {
    unsigned int c[4] = {(unsigned int)index, (unsigned int)(index >> 32), L2A_PHILOX_NORMAL, 0u};
    unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
#pragma unroll          // (l2a_philox4x32_10's own loop is left to the optimiser, which keeps it rolled in these kernels)
    for (int r = 0; r < 10; ++r) {
        l2a_philox_round(c, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const float u1 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

#define L2A_PHILOX_PERM 0x7065726du        // 'perm' .. 'perm' + 3: the TS1 particle shuffle's four word groups
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
