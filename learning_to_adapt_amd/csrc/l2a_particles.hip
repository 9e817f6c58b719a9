// l2a_particles.hip - trajectory-sampling ("particle") plans of a mean ensemble (include/l2a.h: l2a_plan_rs_particles): the two
// kernels around the rollout.  Every member of an E-set ensemble rolls every candidate out as a trajectory of its own - ONE
// per-block request of E blocks per env on the model's packed weight sets, the rollout kernels unchanged - and a candidate's
// score is the mean of its E returns minus lambda times their (biased) standard deviation.
//
//   l2a_particle_expand_k   in front of the rollout: obs0 [m, O] and actions [h, m n, A] -> the per-block requests' inputs, env
//                           major: obs_x [m][E][O], act_x [m][h][E n][A] (request i reads a contiguous [h, E n, A]; particle
//                           row e n + j of request i is particle (i E + e) n + j of the plan).  A pure copy: every source word
//                           is read once and written E times.
//   l2a_particle_score_k    behind it: member_returns [m, E, n] -> score [m, n], spread [m, n], arg-max keys [m].
//
// The scorer's arithmetic is fixed by the header so that a host restates it bit for bit (tests/particle_reference.py): this
// unit is compiled with contraction off (the pragma below and -ffp-contract=off in build.py), and the division and sqrtf are
// the correctly rounded ones hipcc emits by default (see the head of l2a_score.hip).  No float atomics: a thread owns one
// (env, candidate) and sums its members in ascending order, so the bits depend on neither the grid nor the run; the keys are
// integers under max, which no order changes.
#pragma clang fp contract(off)

#include "l2a_host.h"
#include "l2a_kernels.h"
#include "l2a_philox.h"

#include <cmath>
#include <cstdint>
#include <string>

#define L2A_PART_THREADS 256

struct L2AParticleExpandParams {
    const float* obs0;      // [m, O]
    const float* actions;   // [h, m n, A]
    float* obs_x;           // [m, E, O]
    float* act_x;           // [m, h, E n, A]
    long long obs_total;    // m E O
    long long work;         // h m L words of the source actions, L = n A floats (vec: L / 4 f32x4)
    int L;                  // words per (step, env) run of the source, in the unit of `work`
    int m, E, h, O;
    int vec;                // 1: f32x4 words (L = n A / 4; both action pointers 16-byte aligned), 0: floats
};

// Thread g copies word g of the source actions - the source is one contiguous run, so the loads of a wave are 256 B or 1 KiB
// back to back - into its E places, each of which is contiguous over the wave too; the first m E O threads also place one
// observation value.
__global__ __launch_bounds__(L2A_PART_THREADS) void l2a_particle_expand_k(const L2AParticleExpandParams p) {
    const long long g = (long long)blockIdx.x * L2A_PART_THREADS + threadIdx.x;
    if (g < p.obs_total) {
        const long long ie = g / p.O;
        const int k = (int)(g - ie * p.O);
        p.obs_x[g] = p.obs0[(ie / p.E) * p.O + k];
    }
    if (g >= p.work) return;
    const long long c = g / p.L;                // run c = t m + i of the source
    const int w = (int)(g - c * p.L);
    const long long t = c / p.m;
    const long long i = c - t * p.m;
    const long long d0 = ((i * p.h + t) * p.E) * p.L + w;
    if (p.vec) {
        const f32x4 v = reinterpret_cast<const f32x4*>(p.actions)[g];
        f32x4* dst = reinterpret_cast<f32x4*>(p.act_x) + d0;
        for (int e = 0; e < p.E; ++e) dst[(long long)e * p.L] = v;
    } else {
        const float v = p.actions[g];
        float* dst = p.act_x + d0;
        for (int e = 0; e < p.E; ++e) dst[(long long)e * p.L] = v;
    }
}

struct L2AParticleScoreParams {
    const float* member_returns;    // [m, E, n]
    float* score;                   // [m, n] or null
    float* spread;                  // [m, n] or null
    unsigned long long* best_key;   // [m] or null
    float lambda;
    int E, n, cand_offset;
    int bpe;                        // workgroups per env: ceil(n / 256)
};

// One thread per (env, candidate): lane j of a wave reads member e's return of candidate j - consecutive words - for e ascending,
// twice (the second pass hits the cache).  A workgroup's keys are reduced in registers and LDS to one atomicMax per workgroup.
__global__ __launch_bounds__(L2A_PART_THREADS) void l2a_particle_score_k(const L2AParticleScoreParams p) {
    __shared__ unsigned long long wkey[L2A_PART_THREADS / 64];
    const int env = (int)blockIdx.x / p.bpe;
    const int j = ((int)blockIdx.x - env * p.bpe) * L2A_PART_THREADS + (int)threadIdx.x;
    unsigned long long key = 0ull;              // below every packed key: the packed index field is never zero
    if (j < p.n) {
        const float* R = p.member_returns + (size_t)env * p.E * p.n + j;
        const float fe = (float)p.E;
        float s = R[0];
        for (int e = 1; e < p.E; ++e) s = s + R[(size_t)e * p.n];
        const float mean = s / fe;
        float score = mean;
        if (p.spread || p.lambda != 0.0f) {
            float v = 0.0f;
            for (int e = 0; e < p.E; ++e) {
                const float d = R[(size_t)e * p.n] - mean;
                v = v + d * d;
            }
            const float sd = sqrtf(v / fe);
            if (p.spread) p.spread[(size_t)env * p.n + j] = sd;
            if (p.lambda != 0.0f) score = mean - p.lambda * sd;
        }
        if (p.score) p.score[(size_t)env * p.n + j] = score;
        key = l2a_key_pack(score, p.cand_offset + j);
    }
    if (!p.best_key) return;
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = (o > key) ? o : key;
    }
    if ((threadIdx.x & 63) == 0) wkey[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < L2A_PART_THREADS / 64; ++w) key = (wkey[w] > key) ? wkey[w] : key;
        atomicMax(p.best_key + env, key);
    }
}

// ---- TS1: the shuffle between two horizon steps ----------------------------------------------------------------------------------
// A workgroup owns L2A_SHUF_CANDS consecutive candidates of one env.  Its first threads work the candidates' permutations out - one
// thread per (env, candidate), ONCE: Philox and Fisher-Yates in registers (l2a_philox.h), or the injected row, clamped - park them
// in LDS as sixteen 4-bit fields of one 64-bit word, and move the candidate's E returns.  Behind the barrier the whole workgroup
// copies the states: within every member block the workgroup's candidates are ONE contiguous run of cnt * O words at the same
// offset in source and destination, so thread w moves word w of that run for e = 0 .. E - 1 from block pi(e) to block e - the
// stores of a wave are 256 contiguous bytes, its loads contiguous within each candidate's row.  Words move as 32-bit integers:
// no float operation ever sees them.
#define L2A_SHUF_CANDS 32

struct L2AParticleShuffleParams {
    const unsigned int* state_in;   // [m][E n][O]
    const unsigned int* ret_in;     // [m][E][n]
    unsigned int* state_out;
    unsigned int* ret_out;
    const unsigned char* perm;      // [m, n, E] or null
    unsigned long long seed;
    unsigned long long slot0;       // offset + t m: env i's slot is slot0 + i
    int E, n, O, cand_offset;
    int bpe;                        // workgroups per env: ceil(n / L2A_SHUF_CANDS)
};

__global__ __launch_bounds__(L2A_PART_THREADS) void l2a_particle_shuffle_k(const L2AParticleShuffleParams p) {
    __shared__ unsigned long long tab[L2A_SHUF_CANDS];
    const int env = (int)blockIdx.x / p.bpe;
    const int j0 = ((int)blockIdx.x - env * p.bpe) * L2A_SHUF_CANDS;
    const int cnt = (p.n - j0 < L2A_SHUF_CANDS) ? p.n - j0 : L2A_SHUF_CANDS;
    if ((int)threadIdx.x < cnt) {
        const int j = j0 + (int)threadIdx.x;
        unsigned long long pk;
        if (p.perm) {
            const unsigned char* row = p.perm + ((size_t)env * p.n + j) * p.E;
            pk = 0ull;
            for (int e = 0; e < p.E; ++e) {
                const unsigned int v = row[e];
                pk |= (unsigned long long)(v < (unsigned int)p.E ? v : (unsigned int)p.E - 1u) << (4 * e);
            }
        } else {
            pk = l2a_particle_perm_pack(p.seed, p.slot0 + (unsigned long long)env, (unsigned int)(p.cand_offset + j), p.E);
        }
        tab[threadIdx.x] = pk;
        const unsigned int* __restrict__ ri = p.ret_in + (size_t)env * p.E * p.n + j;
        unsigned int* __restrict__ ro = p.ret_out + (size_t)env * p.E * p.n + j;
        for (int e = 0; e < p.E; ++e) ro[(size_t)e * p.n] = ri[(size_t)((pk >> (4 * e)) & 15ull) * p.n];
    }
    __syncthreads();
    const size_t block_words = (size_t)p.n * p.O;                   // one member block of one env
    const size_t base = (size_t)env * p.E * block_words + (size_t)j0 * p.O;
    const unsigned int* __restrict__ si = p.state_in + base;
    unsigned int* __restrict__ so = p.state_out + base;
    const int words = cnt * p.O;
    for (int w = (int)threadIdx.x; w < words; w += L2A_PART_THREADS) {
        const unsigned long long pk = tab[w / p.O];
        for (int e = 0; e < p.E; ++e) so[(size_t)e * block_words + w] = si[(size_t)((pk >> (4 * e)) & 15ull) * block_words + w];
    }
}

// The expansion launch's geometry for source actions at `actions` and a destination at `act_x`: f32x4 words when a (step, env)
// run is a multiple of four floats and both pointers are 16-byte aligned, else floats.  L2A_EINVAL when a run or the launch's
// thread count does not fit 32 bits.
static int expand_geometry(l2a_ctx* ctx, const float* actions, const float* act_x, int m, int E, int n, int h, int obs_dim,
                           int act_dim, L2AParticleExpandParams* p) {
    const long long run = (long long)n * act_dim;       // floats of one (step, env) run
    p->obs_total = (long long)m * E * obs_dim;
    p->vec = (run % 4 == 0 && (((uintptr_t)actions | (uintptr_t)act_x) & 15) == 0) ? 1 : 0;
    const long long L = p->vec ? run / 4 : run;
    if (L > 0x7fffffffLL) return l2a_fail(ctx, L2A_EINVAL, "particle plan: one horizon step of an env's actions is too large");
    p->L = (int)L;
    p->work = (long long)h * m * L;
    p->m = m; p->E = E; p->h = h; p->O = obs_dim;
    const long long threads = p->work > p->obs_total ? p->work : p->obs_total;
    if (threads > 0xffffffffLL - L2A_PART_THREADS)      // (a launch's global size is a 32-bit count of threads)
        return l2a_fail(ctx, L2A_EINVAL, "particle plan: too many action words for one expansion launch");
    return L2A_OK;
}

extern "C" {

int l2a_particle_expand_check(l2a_ctx* ctx, const float* actions, int m, int E, int n, int h, int obs_dim, int act_dim) {
    L2AParticleExpandParams p;
    return expand_geometry(ctx, actions, nullptr, m, E, n, h, obs_dim, act_dim, &p);    // (the model's buffer is 16-byte aligned)
}

int l2a_particle_expand(l2a_ctx* ctx, const float* obs0, const float* actions, int m, int E, int n, int h, int obs_dim, int act_dim,
                        float* obs_x, float* act_x, hipStream_t stream) {
    L2AParticleExpandParams p;
    const int rc = expand_geometry(ctx, actions, act_x, m, E, n, h, obs_dim, act_dim, &p);
    if (rc != L2A_OK) return rc;
    p.obs0 = obs0; p.actions = actions; p.obs_x = obs_x; p.act_x = act_x;
    const long long threads = p.work > p.obs_total ? p.work : p.obs_total;
    const long long blocks = (threads + L2A_PART_THREADS - 1) / L2A_PART_THREADS;
    hipLaunchKernelGGL(l2a_particle_expand_k, dim3((unsigned)blocks), dim3(L2A_PART_THREADS), 0, stream, p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

int l2a_particle_score(l2a_ctx* ctx, const float* member_returns, int m, int E, int n, float lambda, int cand_offset,
                       float* score_out, float* spread_out, unsigned long long* best_key, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if (!member_returns) return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_score: null member_returns");
    if (!score_out && !spread_out && !best_key)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_score: nothing to write (score_out, spread_out and best_key are null)");
    if (m < 1 || E < 1 || n < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_score: m, E and n must be >= 1");
    if (!std::isfinite(lambda)) return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_score: lambda must be finite");
    if ((long long)m * E * n > 0x3fffffffLL || cand_offset < 0 || (long long)cand_offset + n > 0x7fffffffLL)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_score: too many candidates");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    if (best_key) L2A_HIP(ctx, hipMemsetAsync(best_key, 0, sizeof(unsigned long long) * (size_t)m, stream));
    L2AParticleScoreParams p;
    p.member_returns = member_returns; p.score = score_out; p.spread = spread_out; p.best_key = best_key;
    p.lambda = lambda; p.E = E; p.n = n; p.cand_offset = cand_offset;
    p.bpe = l2a_ceil_div(n, L2A_PART_THREADS);
    hipLaunchKernelGGL(l2a_particle_score_k, dim3((unsigned)((long long)m * p.bpe)), dim3(L2A_PART_THREADS), 0, stream, p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

// every slot offset + t m + i, i < m, below 2^33?  (offset <= 2^33 is tested first: nothing below overflows 64 bits)
static bool slots_fit(unsigned long long offset, int t, int m, long long i_end) {
    if (offset > L2A_PERM_SLOT_LIMIT) return false;
    return offset + (unsigned long long)t * (unsigned long long)m + (unsigned long long)i_end <= L2A_PERM_SLOT_LIMIT;
}

int l2a_particle_perm(unsigned long long seed, unsigned long long offset, int t, int m, int i_first, int i_count, int cand_first,
                      int cand_count, int E, unsigned char* out_host) {
    if (!out_host || E < 1 || E > L2A_PERM_MAX_E) return L2A_EINVAL;
    if (t < 0 || m < 1 || i_first < 0 || i_count < 0 || cand_first < 0 || cand_count < 0) return L2A_EINVAL;
    if ((long long)i_first + i_count > m || (long long)cand_first + cand_count > 0x7fffffffLL) return L2A_EINVAL;
    if (!slots_fit(offset, t, m, (long long)i_first + i_count)) return L2A_EINVAL;
    const unsigned long long slot0 = offset + (unsigned long long)t * (unsigned long long)m;
    for (int i = 0; i < i_count; ++i)
        for (int j = 0; j < cand_count; ++j) {
            const unsigned long long pk = l2a_particle_perm_pack(seed, slot0 + (unsigned long long)(i_first + i),
                                                                 (unsigned int)(cand_first + j), E);
            unsigned char* row = out_host + ((size_t)i * cand_count + j) * E;
            for (int e = 0; e < E; ++e) row[e] = (unsigned char)((pk >> (4 * e)) & 15ull);
        }
    return L2A_OK;
}

int l2a_particle_shuffle(l2a_ctx* ctx, const float* state_in, const float* ret_in, float* state_out, float* ret_out,
                         const unsigned char* perm, unsigned long long seed, unsigned long long offset, int t, int m, int E, int n,
                         int obs_dim, int cand_offset, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if (!state_in || !ret_in || !state_out || !ret_out) return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_shuffle: null buffer");
    if (m < 1 || E < 1 || n < 1 || obs_dim < 1 || t < 0) return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_shuffle: m, E, n and obs_dim must be >= 1, t >= 0");
    if (E > L2A_PERM_MAX_E) return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_shuffle: at most 16 members");
    if ((long long)m * E * n > 0x3fffffffLL || cand_offset < 0 || (long long)cand_offset + n > 0x7fffffffLL)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_shuffle: too many candidates");
    if ((long long)L2A_SHUF_CANDS * obs_dim > 0x7fffffffLL) return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_shuffle: obs_dim too large");
    if (!slots_fit(offset, t, m, m)) return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_shuffle: offset + t * m + i must stay below 2^33");
    const size_t rets = (size_t)m * E * n, states = rets * (size_t)obs_dim;
    auto overlap = [](const float* a, const float* b, size_t count) { return a < b + count && b < a + count; };
    if (overlap(state_in, state_out, states) || overlap(ret_in, ret_out, rets))
        return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_shuffle: the shuffle is out of place (an output overlaps its input)");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    L2AParticleShuffleParams p;
    p.state_in = reinterpret_cast<const unsigned int*>(state_in); p.ret_in = reinterpret_cast<const unsigned int*>(ret_in);
    p.state_out = reinterpret_cast<unsigned int*>(state_out); p.ret_out = reinterpret_cast<unsigned int*>(ret_out);
    p.perm = perm; p.seed = seed; p.slot0 = offset + (unsigned long long)t * (unsigned long long)m;
    p.E = E; p.n = n; p.O = obs_dim; p.cand_offset = cand_offset;
    p.bpe = l2a_ceil_div(n, L2A_SHUF_CANDS);
    hipLaunchKernelGGL(l2a_particle_shuffle_k, dim3((unsigned)((long long)m * p.bpe)), dim3(L2A_PART_THREADS), 0, stream, p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

}  // extern "C"
