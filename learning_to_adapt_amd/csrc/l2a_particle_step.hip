// l2a_particle_step.hip - TS1 particle plans of envs whose reward is a program or a reward model (include/l2a.h:
// l2a_particle_step): ONE kernel per horizon step that takes the step's reward of every particle, adds it to the particle's
// return and deals states and returns anew over the member blocks - l2a_particle_shuffle_k (l2a_particles.hip) with the step's
// reward taken in the launch that moves the particles, BEFORE anything moves: at that boundary a particle's pre-state, its action
// and its post-state still lie in one row of HBM each.
//
// A unit of its own so that the code objects of l2a_particles.hip and l2a_score.hip stay what they are.  The arithmetic is
// l2a_score_traj_k's, restated here operation by operation (RewardProgram.evaluate_f32 restates it bit for bit on the host): this
// unit is compiled with contraction off (the pragma below and -ffp-contract=off in build.py), sqrtf is the correctly rounded one.
#pragma clang fp contract(off)

#include "l2a_host.h"
#include "l2a_kernels.h"
#include "l2a_philox.h"

#include <cstdint>
#include <string>

#define L2A_PSTEP_THREADS 256
#define L2A_PSTEP_CANDS 32                  // candidates per workgroup: l2a_particles.hip's L2A_SHUF_CANDS
#define L2A_PSTEP_LDS_MAX (61 * 1024)       // dynamic LDS of the program mode's staging: 64 KiB less the 2304 static bytes below

struct L2AParticleStepParams {
    const unsigned int* pre;        // [m][E][O] (pre_per_row 0) or [m][E n][O]
    const unsigned int* post;       // [m][E n][O]
    const float* actions;           // env i's slab [E n][A] at actions + i * act_env_stride
    const float* rewards;           // [m][E][n], or null: the program
    const float* ret_in;            // [m][E][n], or null: every return is the literal 0.0f
    unsigned int* state_out;        // [m][E n][O], or null: the last step, nothing is dealt
    float* ret_out;                 // [m][E][n]
    const unsigned char* perm;      // [m, n, E] or null
    unsigned long long seed;
    unsigned long long slot0;       // offset + t m: env i's slot is slot0 + i
    long long act_env_stride;
    double disc;                    // discount ** t, the host's repeated product
    int pre_per_row;
    int E, n, O, A, cand_offset;
    int bpe;                        // workgroups per env: ceil(n / L2A_PSTEP_CANDS)
    int rpp;                        // program mode: particle rows staged per pass, a multiple of 64, at most 256
    l2a_reward_program prog;        // by value in the kernel arguments: uniform, read through scalar loads only
};

// Element j of a term's source vector for this lane's particle (l2a_score.hip: l2a_score_fetch).
__device__ __forceinline__ float l2a_pstep_fetch(int source, int j, const float* o, const float* nx, const float* a) {
    switch (source) {
        case L2A_SRC_OBS: return o[j];
        case L2A_SRC_ACT: return a[j];
        case L2A_SRC_NEXT: return nx[j];
        default: return nx[j] - o[j];
    }
}

// One step's reward of one particle: l2a_score_traj_k's operation sequence - the same term order, s = s + d * d, sqrtf,
// r = r + coef * v, INRANGE of a NaN gives 0.
__device__ __forceinline__ float l2a_pstep_reward(const l2a_reward_program& prog, const float* o, const float* nx, const float* a) {
    float r = prog.bias;
    for (int ti = 0; ti < prog.n_terms; ++ti) {
        const int kind = prog.terms[ti].kind, source = prog.terms[ti].source;
        const int index = prog.terms[ti].index, len = prog.terms[ti].len, target = prog.terms[ti].target;
        float v;
        if (kind == L2A_TERM_LINEAR) {
            v = l2a_pstep_fetch(source, index, o, nx, a);
        } else if (kind == L2A_TERM_INRANGE) {
            const float x = l2a_pstep_fetch(source, index, o, nx, a);
            v = (x >= prog.terms[ti].lo && x <= prog.terms[ti].hi) ? 1.0f : 0.0f;
        } else {
            float s = 0.0f;
            for (int k = 0; k < len; ++k) {
                const float tk = (target >= 0) ? prog.consts[target + k] : 0.0f;
                const float d = l2a_pstep_fetch(source, index + k, o, nx, a) - tk;
                s = s + d * d;
            }
            v = (kind == L2A_TERM_NORM) ? sqrtf(s) : s;
        }
        r = r + prog.terms[ti].coef * v;
    }
    return r;
}

// Particle rows q0 .. q0 + rows - 1 of the workgroup (particle q = e * cnt + c: candidate j0 + c of member block e) into LDS rows
// `stride` apart.  Within a member block the workgroup's rows are one contiguous run of cnt * dim words: a wave's loads are
// contiguous within each run, its LDS writes consecutive words (a gap of at most one at a row's end).  block_rows 0: a member
// block holds ONE row, which every particle of the block reads (the expansion's obs_x).
__device__ __forceinline__ void l2a_pstep_stage(unsigned int* dst, const unsigned int* __restrict__ src, int q0, int rows, int cnt,
                                                int dim, int stride, size_t block_rows, int j0) {
    for (int w = (int)threadIdx.x; w < rows * dim; w += L2A_PSTEP_THREADS) {
        const int i = w / dim, k = w - i * dim;
        const int q = q0 + i, e = q / cnt, c = q - e * cnt;
        const size_t row = block_rows ? (size_t)e * block_rows + (size_t)(j0 + c) : (size_t)e;
        dst[i * stride + k] = src[row * (size_t)dim + k];
    }
}

// The shuffle's geometry: a workgroup owns up to L2A_PSTEP_CANDS consecutive candidates of one env across all E member blocks -
// everything a candidate's permutation touches.  (1) its first threads work the permutations out, as the shuffle does;  (2) every
// particle's R' = R + (float)disc * r goes to LDS - r from the program on rows staged at an ODD stride (lane i reads word
// i * stride + k: 32 lanes on 32 banks), at most 256 particles per pass, or from the given rewards;  (3) ret_out[e] = R'[pi(e)];
// (4) state_out[e] = post[pi(e)] as 32-bit integer words, the shuffle's copy loop.  Without state_out nothing is dealt.
__global__ __launch_bounds__(L2A_PSTEP_THREADS) void l2a_particle_step_k(const L2AParticleStepParams p) {
    extern __shared__ unsigned int lds[];
    __shared__ unsigned long long tab[L2A_PSTEP_CANDS];
    __shared__ float racc[L2A_PERM_MAX_E * L2A_PSTEP_CANDS];
    const int tid = (int)threadIdx.x;
    const int env = (int)blockIdx.x / p.bpe;
    const int j0 = ((int)blockIdx.x - env * p.bpe) * L2A_PSTEP_CANDS;
    const int cnt = (p.n - j0 < L2A_PSTEP_CANDS) ? p.n - j0 : L2A_PSTEP_CANDS;
    const int total = p.E * cnt;
    const size_t ret_base = (size_t)env * p.E * p.n + j0;             // + e * n + c: particle (e, c)'s return
    if (tid < cnt && p.state_out) {
        const int j = j0 + tid;
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
        tab[tid] = pk;
    }
    const float disc = (float)p.disc;
    if (p.rewards) {
        for (int q = tid; q < total; q += L2A_PSTEP_THREADS) {
            const int e = q / cnt, c = q - e * cnt;
            const size_t at = ret_base + (size_t)e * p.n + c;
            const float R = p.ret_in ? p.ret_in[at] : 0.0f;
            racc[q] = R + disc * p.rewards[at];
        }
    } else {
        const int so = p.O | 1, sa = p.A | 1;
        unsigned int* const obuf = lds;
        unsigned int* const nbuf = lds + p.rpp * so;
        unsigned int* const abuf = lds + 2 * p.rpp * so;
        const size_t env_rows = (size_t)env * p.E * p.n;
        const unsigned int* pre = p.pre + (p.pre_per_row ? env_rows : (size_t)env * p.E) * p.O;
        const unsigned int* post = p.post + env_rows * p.O;
        const unsigned int* act = reinterpret_cast<const unsigned int*>(p.actions + (size_t)env * (size_t)p.act_env_stride);
        for (int q0 = 0; q0 < total; q0 += p.rpp) {
            const int rows = (total - q0 < p.rpp) ? total - q0 : p.rpp;
            l2a_pstep_stage(obuf, pre, q0, rows, cnt, p.O, so, p.pre_per_row ? (size_t)p.n : 0, j0);
            l2a_pstep_stage(nbuf, post, q0, rows, cnt, p.O, so, (size_t)p.n, j0);
            l2a_pstep_stage(abuf, act, q0, rows, cnt, p.A, sa, (size_t)p.n, j0);
            __syncthreads();
            if (tid < rows) {
                const int q = q0 + tid, e = q / cnt, c = q - e * cnt;
                const float r = l2a_pstep_reward(p.prog, reinterpret_cast<const float*>(obuf) + tid * so,
                                                 reinterpret_cast<const float*>(nbuf) + tid * so,
                                                 reinterpret_cast<const float*>(abuf) + tid * sa);
                const float R = p.ret_in ? p.ret_in[ret_base + (size_t)e * p.n + c] : 0.0f;
                racc[q] = R + disc * r;
            }
            __syncthreads();        // the next pass's staging overwrites this pass's rows
        }
    }
    __syncthreads();
    for (int q = tid; q < total; q += L2A_PSTEP_THREADS) {
        const int e = q / cnt, c = q - e * cnt;
        const int from = p.state_out ? (int)((tab[c] >> (4 * e)) & 15ull) : e;
        p.ret_out[ret_base + (size_t)e * p.n + c] = racc[from * cnt + c];
    }
    if (!p.state_out) return;
    const size_t block_words = (size_t)p.n * p.O;                   // one member block of one env
    const size_t base = (size_t)env * p.E * block_words + (size_t)j0 * p.O;
    const unsigned int* __restrict__ si = p.post + base;
    unsigned int* __restrict__ so_ = p.state_out + base;
    const int words = cnt * p.O;
    for (int w = tid; w < words; w += L2A_PSTEP_THREADS) {
        const unsigned long long pk = tab[w / p.O];
        for (int e = 0; e < p.E; ++e) so_[(size_t)e * block_words + w] = si[(size_t)((pk >> (4 * e)) & 15ull) * block_words + w];
    }
}

// Bytes of one staged particle: its pre-state and post-state rows and its action row, each at an odd stride.
static long long pstep_row_bytes(int obs_dim, int act_dim) { return 4LL * (2LL * (obs_dim | 1) + (act_dim | 1)); }

// Particle rows staged per pass: what fits the LDS in whole waves, at most one row per thread; below 64 nothing fits.
static int pstep_rows_per_pass(int obs_dim, int act_dim) {
    const long long rows = L2A_PSTEP_LDS_MAX / pstep_row_bytes(obs_dim, act_dim) / 64 * 64;
    return rows > L2A_PSTEP_THREADS ? L2A_PSTEP_THREADS : (int)rows;
}

extern "C" {

int l2a_particle_step_lds_check(l2a_ctx* ctx, int obs_dim, int act_dim) {
    if (pstep_rows_per_pass(obs_dim, act_dim) >= 64) return L2A_OK;
    return l2a_fail(ctx, L2A_EINVAL, "l2a_particle_step: 64 rows of obs_dim " + std::to_string(obs_dim) + " / act_dim " +
                    std::to_string(act_dim) + " do not fit the LDS");
}

int l2a_particle_step(l2a_ctx* ctx, const float* pre, int pre_per_row, const float* post, const float* actions,
                      long long act_env_stride, const float* rewards, const l2a_reward_program* program, double disc_t,
                      const float* ret_in, float* state_out, float* ret_out, const unsigned char* perm, unsigned long long seed,
                      unsigned long long offset, int t, int m, int E, int n, int obs_dim, int act_dim, int cand_offset,
                      void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    const std::string who("l2a_particle_step: ");
    if (!pre || !post || !actions || !ret_out) return l2a_fail(ctx, L2A_EINVAL, who + "null buffer");
    if ((rewards != nullptr) == (program != nullptr))
        return l2a_fail(ctx, L2A_EINVAL, who + "exactly one of rewards and program is given");
    if (m < 1 || E < 1 || n < 1 || obs_dim < 1 || act_dim < 1 || t < 0)
        return l2a_fail(ctx, L2A_EINVAL, who + "m, E, n, obs_dim and act_dim must be >= 1, t >= 0");
    if (E > L2A_PERM_MAX_E) return l2a_fail(ctx, L2A_EINVAL, who + "at most 16 members");
    if ((long long)m * E * n > 0x3fffffffLL || cand_offset < 0 || (long long)cand_offset + n > 0x7fffffffLL)
        return l2a_fail(ctx, L2A_EINVAL, who + "too many candidates");
    if ((long long)L2A_PSTEP_CANDS * obs_dim > 0x7fffffffLL || (long long)L2A_PSTEP_THREADS * act_dim > 0x7fffffffLL)
        return l2a_fail(ctx, L2A_EINVAL, who + "obs_dim or act_dim too large");
    if (offset > L2A_PERM_SLOT_LIMIT ||
        offset + (unsigned long long)t * (unsigned long long)m + (unsigned long long)m > L2A_PERM_SLOT_LIMIT)
        return l2a_fail(ctx, L2A_EINVAL, who + "offset + t * m + i must stay below 2^33");
    const long long slab = (long long)E * n * act_dim;              // one env's actions of the step
    if (act_env_stride < 0 || (m > 1 && act_env_stride < slab) || act_env_stride > (1LL << 40))
        return l2a_fail(ctx, L2A_EINVAL, who + "act_env_stride must be at least E * n * act_dim floats");
    int rpp = 0;
    long long lds_bytes = 0;
    if (program) {
        const int rc = l2a_reward_program_check(program, obs_dim, act_dim);
        if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
        rpp = pstep_rows_per_pass(obs_dim, act_dim);
        if (rpp < 64) return l2a_particle_step_lds_check(ctx, obs_dim, act_dim);
        lds_bytes = rpp * pstep_row_bytes(obs_dim, act_dim);
    }
    // out of place throughout: no output may overlap an input or the other output
    const size_t rets = (size_t)m * E * n, states = rets * (size_t)obs_dim;
    struct span { const void* p; size_t bytes; };
    const span ins[] = {{pre, 4 * (pre_per_row ? states : (size_t)m * E * obs_dim)}, {post, 4 * states},
                        {actions, 4 * ((size_t)(m - 1) * (size_t)act_env_stride + (size_t)slab)}, {rewards, 4 * rets},
                        {ret_in, 4 * rets}, {state_out ? perm : nullptr, rets}};     // (the last step reads no table)
    const span outs[] = {{state_out, 4 * states}, {ret_out, 4 * rets}};
    auto overlap = [](const span& a, const span& b) {
        if (!a.p || !b.p) return false;
        const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
        return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
    };
    for (const span& o : outs)
        for (const span& i : ins)
            if (overlap(o, i)) return l2a_fail(ctx, L2A_EINVAL, who + "the step is out of place (an output overlaps an input)");
    if (overlap(outs[0], outs[1])) return l2a_fail(ctx, L2A_EINVAL, who + "state_out overlaps ret_out");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    L2AParticleStepParams p{};
    p.pre =reinterpret_cast<const unsigned int*>(pre); p.post = reinterpret_cast<const unsigned int*>(post);
    p.actions = actions; p.rewards = rewards; p.ret_in = ret_in;
    p.state_out = reinterpret_cast<unsigned int*>(state_out); p.ret_out = ret_out;
    p.perm = perm; p.seed = seed; p.slot0 = offset + (unsigned long long)t * (unsigned long long)m;
    p.act_env_stride = act_env_stride; p.disc = disc_t; p.pre_per_row = pre_per_row ? 1 : 0;
    p.E = E; p.n = n; p.O = obs_dim; p.A = act_dim; p.cand_offset = cand_offset;
    p.bpe = l2a_ceil_div(n, L2A_PSTEP_CANDS);
    p.rpp = rpp;
    if (program) p.prog = *program;
    hipLaunchKernelGGL(l2a_particle_step_k, dim3((unsigned)((long long)m * p.bpe)), dim3(L2A_PSTEP_THREADS), (size_t)lds_bytes,
                       stream, p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

}  // extern "C"
