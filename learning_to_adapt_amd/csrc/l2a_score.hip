// l2a_score.hip - reward programs (include/l2a.h: l2a_reward_program): the host-only validator and the
// trajectory-scoring kernel behind l2a_score_trajectory / l2a_plan_rs_program; and termination programs (l2a_termination):
// their validator and the kernel behind l2a_score_trajectory_term / l2a_plan_rs_term, which stops a candidate's return at its
// first step whose next observation fails a guard.
//
// The rollout kernels fuse ONE reward formula (l2a_reward).  An env with any other closed-form reward plans through
// l2a_plan_rs_program instead: the rollout kernels - unchanged - write every candidate's state out step by step
// (their carry launch), and the kernel here scores those trajectories with a general list of terms.  It moves
// h x rows x (obs_dim + act_dim) floats once (BASELINE config 2: 6 MB) - never the long pole of a plan.
//
// The arithmetic is fixed by the header so that envs/reward_spec.py (RewardProgram.evaluate_f32) restates it bit for
// bit: this unit is compiled with contraction off (the pragma below and -ffp-contract=off in build.py - HIP's
// __fmul_rn / __fadd_rn are plain operators that the default -ffp-contract=fast would fuse), and the square root is
// sqrtf, which hipcc rounds correctly by default (HIP's __fsqrt_rn is the native, approximate one).
#pragma clang fp contract(off)

#include "l2a_host.h"
#include "l2a_kernels.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#define L2A_SCORE_ROWS 64        // candidates per workgroup: one lane of wave 0 each
#define L2A_SCORE_THREADS 256    // all four waves stage, wave 0 scores
#define L2A_SCORE_LDS_MAX (63 * 1024)

struct L2AScoreParams {
    const float* obs0;              // [m, obs_dim]
    const float* traj;              // [h, rows, obs_dim]
    const float* actions;           // [h, rows, act_dim]
    float* returns_out;             // [rows] or null
    unsigned long long* best_key;   // [m] or null
    double discount;
    int rows, n, h;                 // rows = m * n
    int obs_dim, act_dim;
    int cand_offset;
    l2a_reward_program prog;        // by value in the kernel arguments: uniform, read through scalar loads only
};

// `count` floats at `src` - whole rows of `dim` floats, back to back as they lie in memory - into LDS rows `stride` apart.
// wide: 16-byte loads (count is a multiple of 4 and src 16-byte aligned: a whole block of an aligned step), else dwords.
__device__ __forceinline__ void l2a_score_stage(float* dst, const float* __restrict__ src, int count, int dim, int stride,
                                                bool wide) {
    if (wide) {
        const f32x4* src4 = reinterpret_cast<const f32x4*>(src);
        for (int q = threadIdx.x; q < (count >> 2); q += L2A_SCORE_THREADS) {
            const f32x4 v = src4[q];
            int i = (4 * q) / dim, k = 4 * q - i * dim;
            dst[i * stride + k] = v.x; if (++k == dim) { k = 0; ++i; }
            dst[i * stride + k] = v.y; if (++k == dim) { k = 0; ++i; }
            dst[i * stride + k] = v.z; if (++k == dim) { k = 0; ++i; }
            dst[i * stride + k] = v.w;
        }
    } else {
        for (int e = threadIdx.x; e < count; e += L2A_SCORE_THREADS) {
            const int i = e / dim, k = e - i * dim;
            dst[i * stride + k] = src[e];
        }
    }
}

// Element j of a term's source vector for this lane's row (o / nx / a: the row's obs, next obs and action in LDS).
__device__ __forceinline__ float l2a_score_fetch(int source, int j, const float* o, const float* nx, const float* a) {
    switch (source) {
        case L2A_SRC_OBS: return o[j];
        case L2A_SRC_ACT: return a[j];
        case L2A_SRC_NEXT: return nx[j];
        default: return nx[j] - o[j];
    }
}

// One workgroup = 64 consecutive rows (candidates) over the whole horizon.  Per step the block's next observations and
// actions - contiguous in memory, because rows are - are staged into LDS rows of an ODD stride (lane i reads word
// i * stride + k: 32 lanes on 32 banks), and the step's `next` block stays where it is as the following step's `obs`.
__global__ __launch_bounds__(L2A_SCORE_THREADS) void l2a_score_traj_k(const L2AScoreParams p) {
    extern __shared__ float lds[];
    __shared__ unsigned long long skey[L2A_SCORE_ROWS];
    __shared__ int senv[L2A_SCORE_ROWS];
    const int tid = threadIdx.x;
    const int so = p.obs_dim | 1, sa = p.act_dim | 1;
    const int obuf_floats = L2A_SCORE_ROWS * so;       // two observation blocks: step t reads (t & 1) as obs, (t + 1) & 1 as next
    float* const abuf = lds + 2 * L2A_SCORE_ROWS * so;
    const int r0 = (int)blockIdx.x * L2A_SCORE_ROWS;
    const int nr = min(L2A_SCORE_ROWS, p.rows - r0);
    const bool whole = (nr == L2A_SCORE_ROWS);

    for (int e = tid; e < nr * p.obs_dim; e += L2A_SCORE_THREADS) {     // obs of step 0: obs0[env of the row]
        const int i = e / p.obs_dim, k = e - i * p.obs_dim;
        lds[i * so + k] = p.obs0[(size_t)((r0 + i) / p.n) * p.obs_dim + k];
    }
    float R = 0.0f;
    double disc = 1.0;
    for (int t = 0; t < p.h; ++t) {
        const float* nsrc = p.traj + ((size_t)t * p.rows + r0) * p.obs_dim;
        const float* asrc = p.actions + ((size_t)t * p.rows + r0) * p.act_dim;
        l2a_score_stage(lds + ((t + 1) & 1) * obuf_floats, nsrc, nr * p.obs_dim, p.obs_dim, so, whole && ((uintptr_t)nsrc & 15) == 0);
        l2a_score_stage(abuf, asrc, nr * p.act_dim, p.act_dim, sa, whole && ((uintptr_t)asrc & 15) == 0);
        __syncthreads();
        if (tid < nr) {
            const float* o = lds + (t & 1) * obuf_floats + tid * so;
            const float* nx = lds + ((t + 1) & 1) * obuf_floats + tid * so;
            const float* a = abuf + tid * sa;
            float r = p.prog.bias;
            for (int ti = 0; ti < p.prog.n_terms; ++ti) {
                const int kind = p.prog.terms[ti].kind, source = p.prog.terms[ti].source;
                const int index = p.prog.terms[ti].index, len = p.prog.terms[ti].len, target = p.prog.terms[ti].target;
                float v;
                if (kind == L2A_TERM_LINEAR) {
                    v = l2a_score_fetch(source, index, o, nx, a);
                } else if (kind == L2A_TERM_INRANGE) {
                    const float x = l2a_score_fetch(source, index, o, nx, a);
                    v = (x >= p.prog.terms[ti].lo && x <= p.prog.terms[ti].hi) ? 1.0f : 0.0f;
                } else {
                    float s = 0.0f;
                    for (int k = 0; k < len; ++k) {
                        const float tk = (target >= 0) ? p.prog.consts[target + k] : 0.0f;
                        const float d = l2a_score_fetch(source, index + k, o, nx, a) - tk;
                        s = s + d * d;
                    }
                    v = (kind == L2A_TERM_NORM) ? sqrtf(s) : s;
                }
                r = r + p.prog.terms[ti].coef * v;
            }
            R = R + (float)disc * r;
        }
        disc *= p.discount;
        __syncthreads();        // the next step's staging overwrites this step's obs and actions
    }

    if (tid < nr) {
        const int row = r0 + tid, env = row / p.n;
        if (p.returns_out) p.returns_out[row] = R;
        skey[tid] = l2a_key_pack(R, p.cand_offset + (row - env * p.n));
        senv[tid] = env;
    }
    __syncthreads();
    // one atomic per (workgroup, env touched): the first row of every env's run in this block reduces the run
    if (p.best_key && tid < nr && (tid == 0 || senv[tid - 1] != senv[tid])) {
        unsigned long long best = skey[tid];
        for (int i = tid + 1; i < nr && senv[i] == senv[tid]; ++i) best = (skey[i] > best) ? skey[i] : best;
        atomicMax(p.best_key + senv[tid], best);
    }
}

// ---- termination programs (include/l2a.h: l2a_termination) ----------------------------------------------------------
struct L2ATermParams {
    const float* obs0;              // [m, obs_dim]; not read in step_rewards mode
    const float* traj;              // [h, rows, obs_dim]
    const float* actions;           // [h, rows, act_dim]; not read in step_rewards mode
    const float* step_rewards;      // [h, rows], or null: the reward program scores every step
    const float* terminal_values;   // [rows] or null
    float* returns_out;             // [rows] or null
    int* steps_alive;               // [rows] or null
    unsigned long long* best_key;   // [m] or null
    double discount;
    float w;                        // fp32(value_coef * discount ** h), as l2a_value_terminal
    int rows, n, h;
    int obs_dim, act_dim;
    int cand_offset;
    l2a_termination term;           // both by value in the kernel arguments: uniform, read through scalar loads only
    l2a_reward_program prog;
};

// l2a_score_traj_k's step reward of one row, operation by operation (that kernel keeps its own copy: it is not to change).
__device__ __forceinline__ float l2a_score_reward(const l2a_reward_program& prog, const float* o, const float* nx, const float* a) {
    float r = prog.bias;
    for (int ti = 0; ti < prog.n_terms; ++ti) {
        const int kind = prog.terms[ti].kind, source = prog.terms[ti].source;
        const int index = prog.terms[ti].index, len = prog.terms[ti].len, target = prog.terms[ti].target;
        float v;
        if (kind == L2A_TERM_LINEAR) {
            v = l2a_score_fetch(source, index, o, nx, a);
        } else if (kind == L2A_TERM_INRANGE) {
            const float x = l2a_score_fetch(source, index, o, nx, a);
            v = (x >= prog.terms[ti].lo && x <= prog.terms[ti].hi) ? 1.0f : 0.0f;
        } else {
            float s = 0.0f;
            for (int k = 0; k < len; ++k) {
                const float tk = (target >= 0) ? prog.consts[target + k] : 0.0f;
                const float d = l2a_score_fetch(source, index + k, o, nx, a) - tk;
                s = s + d * d;
            }
            v = (kind == L2A_TERM_NORM) ? sqrtf(s) : s;
        }
        r = r + prog.terms[ti].coef * v;
    }
    return r;
}

// l2a_score_traj_k's geometry - 64 consecutive rows per workgroup, all four waves stage, one lane of wave 0 per row, LDS rows of
// an odd stride - with a per-row `alive` flag: a row is scored up to and including its first step whose next observation
// fails a guard, and nothing of it is looked at afterwards (a selection: a dead lane skips the step's arithmetic).  With
// step_rewards only the next observations pass through LDS (one block; the guards read nothing else) and a row's reward of
// the step is one coalesced dword load by its own lane.
__global__ __launch_bounds__(L2A_SCORE_THREADS) void l2a_score_term_k(const L2ATermParams p) {
    extern __shared__ float lds[];
    __shared__ unsigned long long skey[L2A_SCORE_ROWS];
    __shared__ int senv[L2A_SCORE_ROWS];
    const int tid = threadIdx.x;
    const bool given = (p.step_rewards != nullptr);
    const int so = p.obs_dim | 1, sa = p.act_dim | 1;
    const int obuf_floats = L2A_SCORE_ROWS * so;
    float* const abuf = lds + 2 * L2A_SCORE_ROWS * so;
    const int r0 = (int)blockIdx.x * L2A_SCORE_ROWS;
    const int nr = min(L2A_SCORE_ROWS, p.rows - r0);
    const bool whole = (nr == L2A_SCORE_ROWS);

    if (!given) {
        for (int e = tid; e < nr * p.obs_dim; e += L2A_SCORE_THREADS) {     // obs of step 0: obs0[env of the row]
            const int i = e / p.obs_dim, k = e - i * p.obs_dim;
            lds[i * so + k] = p.obs0[(size_t)((r0 + i) / p.n) * p.obs_dim + k];
        }
    }
    float R = 0.0f;
    double disc = 1.0;
    bool alive = (tid < nr);
    int steps = p.h;
    for (int t = 0; t < p.h; ++t) {
        float* const nbuf = given ? lds : lds + ((t + 1) & 1) * obuf_floats;
        const float* nsrc = p.traj + ((size_t)t * p.rows + r0) * p.obs_dim;
        l2a_score_stage(nbuf, nsrc, nr * p.obs_dim, p.obs_dim, so, whole && ((uintptr_t)nsrc & 15) == 0);
        float r = 0.0f;
        if (given) {
            if (tid < nr) r = p.step_rewards[(size_t)t * p.rows + r0 + tid];
        } else {
            const float* asrc = p.actions + ((size_t)t * p.rows + r0) * p.act_dim;
            l2a_score_stage(abuf, asrc, nr * p.act_dim, p.act_dim, sa, whole && ((uintptr_t)asrc & 15) == 0);
        }
        __syncthreads();
        if (alive) {
            const float* nx = nbuf + tid * so;
            if (!given) r = l2a_score_reward(p.prog, lds + (t & 1) * obuf_floats + tid * so, nx, abuf + tid * sa);
            const float d = (float)disc;
            R = R + d * r;
            bool ok = true;
            for (int g = 0; g < p.term.n_guards; ++g) {
                const int index = p.term.guards[g].index, len = p.term.guards[g].len;
                const float lo = p.term.guards[g].lo, hi = p.term.guards[g].hi;
                for (int k = 0; k < len; ++k) {
                    const float x = nx[index + k];
                    ok = ok && (x >= lo && x <= hi);        // a NaN is outside
                }
            }
            if (!ok) {
                if (p.term.terminal_reward != 0.0f) R = R + d * p.term.terminal_reward;
                alive = false;
                steps = t + 1;
            }
        }
        disc *= p.discount;
        __syncthreads();        // the next step's staging overwrites this step's obs and actions
    }

    if (tid < nr) {
        const int row = r0 + tid, env = row / p.n;
        if (alive && p.terminal_values && p.w != 0.0f) R = R + p.w * p.terminal_values[row];
        if (p.returns_out) p.returns_out[row] = R;
        if (p.steps_alive) p.steps_alive[row] = steps;
        skey[tid] = l2a_key_pack(R, p.cand_offset + (row - env * p.n));
        senv[tid] = env;
    }
    __syncthreads();
    // one atomic per (workgroup, env touched): the first row of every env's run in this block reduces the run
    if (p.best_key && tid < nr && (tid == 0 || senv[tid - 1] != senv[tid])) {
        unsigned long long best = skey[tid];
        for (int i = tid + 1; i < nr && senv[i] == senv[tid]; ++i) best = (skey[i] > best) ? skey[i] : best;
        atomicMax(p.best_key + senv[tid], best);
    }
}

extern "C" {

int l2a_reward_program_check(const l2a_reward_program* pg, int obs_dim, int act_dim) {
    if (!pg) return l2a_fail(nullptr, L2A_EINVAL, "reward program: null program");
    if (obs_dim < 1 || act_dim < 1) return l2a_fail(nullptr, L2A_EINVAL, "reward program: obs_dim and act_dim must be >= 1");
    if (pg->n_terms < 0 || pg->n_terms > L2A_PROGRAM_MAX_TERMS)
        return l2a_fail(nullptr, L2A_EINVAL, "reward program: " + std::to_string(pg->n_terms) + " terms (at most " +
                        std::to_string(L2A_PROGRAM_MAX_TERMS) + ")");
    if (pg->n_consts < 0 || pg->n_consts > L2A_PROGRAM_MAX_CONSTS)
        return l2a_fail(nullptr, L2A_EINVAL, "reward program: " + std::to_string(pg->n_consts) + " constants (at most " +
                        std::to_string(L2A_PROGRAM_MAX_CONSTS) + ")");
    for (int i = 0; i < pg->n_terms; ++i) {
        const l2a_reward_term& t = pg->terms[i];
        const std::string who = "reward program: term " + std::to_string(i) + ": ";
        if (t.kind < L2A_TERM_LINEAR || t.kind > L2A_TERM_INRANGE) return l2a_fail(nullptr, L2A_EINVAL, who + "unknown kind");
        if (t.source < L2A_SRC_OBS || t.source > L2A_SRC_DELTA) return l2a_fail(nullptr, L2A_EINVAL, who + "unknown source");
        if ((t.kind == L2A_TERM_LINEAR || t.kind == L2A_TERM_INRANGE) && t.len != 1)
            return l2a_fail(nullptr, L2A_EINVAL, who + "LINEAR and INRANGE read one element (len must be 1)");
        const int dim = (t.source == L2A_SRC_ACT) ? act_dim : obs_dim;
        if (t.len < 1 || t.index < 0 || t.index >= dim || t.len > dim - t.index)
            return l2a_fail(nullptr, L2A_EINVAL, who + "range outside its source vector");
        if (t.target != -1 && (t.target < 0 || t.target >= pg->n_consts || t.len > pg->n_consts - t.target))
            return l2a_fail(nullptr, L2A_EINVAL, who + "target range outside the constant table");
    }
    return L2A_OK;
}

int l2a_score_trajectory(l2a_ctx* ctx, const float* obs0, const float* traj, const float* actions, int m, int n, int h,
                         int obs_dim, int act_dim, double discount, const l2a_reward_program* program, int cand_offset,
                         float* returns_out, unsigned long long* best_key, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    const int rc = l2a_reward_program_check(program, obs_dim, act_dim);
    if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
    if (!obs0 || !traj || !actions) return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory: null obs0/traj/actions");
    if (!best_key && !returns_out)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory: nothing to write (best_key and returns_out are null)");
    if (m < 1 || n < 1 || h < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory: m, n and h must be >= 1");
    if ((long long)m * n > 0x3fffffffLL || cand_offset < 0 || (long long)cand_offset + n > 0x7fffffffLL)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory: too many candidates");
    const long long lds_bytes = 4LL * L2A_SCORE_ROWS * (2LL * (obs_dim | 1) + (act_dim | 1));
    if (lds_bytes > L2A_SCORE_LDS_MAX)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory: 64 rows of obs_dim " + std::to_string(obs_dim) + " / act_dim " +
                        std::to_string(act_dim) + " do not fit the LDS");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    if (best_key) L2A_HIP(ctx, hipMemsetAsync(best_key, 0, sizeof(unsigned long long) * (size_t)m, stream));
    L2AScoreParams p;
    p.obs0 = obs0; p.traj = traj; p.actions = actions; p.returns_out = returns_out; p.best_key = best_key;
    p.discount = discount;
    p.rows = m * n; p.n = n; p.h = h; p.obs_dim = obs_dim; p.act_dim = act_dim; p.cand_offset = cand_offset;
    p.prog = *program;
    const int blocks = l2a_ceil_div(p.rows, L2A_SCORE_ROWS);
    hipLaunchKernelGGL(l2a_score_traj_k, dim3(blocks), dim3(L2A_SCORE_THREADS), (size_t)lds_bytes, stream, p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

int l2a_termination_check(const l2a_termination* tm, int obs_dim) {
    if (!tm) return l2a_fail(nullptr, L2A_EINVAL, "termination program: null program");
    if (obs_dim < 1) return l2a_fail(nullptr, L2A_EINVAL, "termination program: obs_dim must be >= 1");
    if (tm->n_guards < 1 || tm->n_guards > L2A_TERMINATION_MAX_GUARDS)
        return l2a_fail(nullptr, L2A_EINVAL, "termination program: " + std::to_string(tm->n_guards) + " guards (1 .. " +
                        std::to_string(L2A_TERMINATION_MAX_GUARDS) + ")");
    if (!std::isfinite(tm->terminal_reward)) return l2a_fail(nullptr, L2A_EINVAL, "termination program: terminal_reward must be finite");
    for (int i = 0; i < tm->n_guards; ++i) {
        const l2a_guard& g = tm->guards[i];
        const std::string who = "termination program: guard " + std::to_string(i) + ": ";
        if (g.len < 1 || g.index < 0 || g.index >= obs_dim || g.len > obs_dim - g.index)
            return l2a_fail(nullptr, L2A_EINVAL, who + "range outside the observation");
        if (std::isnan(g.lo) || std::isnan(g.hi)) return l2a_fail(nullptr, L2A_EINVAL, who + "a bound is NaN");
        if (g.lo > g.hi) return l2a_fail(nullptr, L2A_EINVAL, who + "lo > hi");
    }
    return L2A_OK;
}

int l2a_score_trajectory_term(l2a_ctx* ctx, const float* obs0, const float* traj, const float* actions, const float* step_rewards,
                              int m, int n, int h, int obs_dim, int act_dim, double discount, const l2a_reward_program* program,
                              const l2a_termination* termination, const float* terminal_values, double value_coef,
                              int cand_offset, float* returns_out, int* steps_alive_out, unsigned long long* best_key,
                              void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if ((program != nullptr) == (step_rewards != nullptr))
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_term: exactly one of program and step_rewards must be given");
    if (obs_dim < 1 || act_dim < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_term: obs_dim and act_dim must be >= 1");
    int rc = program ? l2a_reward_program_check(program, obs_dim, act_dim) : L2A_OK;
    if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
    rc = l2a_termination_check(termination, obs_dim);
    if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
    if (!traj || (program && (!obs0 || !actions))) return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_term: null obs0/traj/actions");
    if (!best_key && !returns_out && !steps_alive_out)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_term: nothing to write (best_key, returns_out and steps_alive_out are null)");
    if (m < 1 || n < 1 || h < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_term: m, n and h must be >= 1");
    if (!std::isfinite(discount) || !std::isfinite(value_coef))
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_term: discount and value_coef must be finite");
    if ((long long)m * n > 0x3fffffffLL || cand_offset < 0 || (long long)cand_offset + n > 0x7fffffffLL)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_term: too many candidates");
    const long long lds_bytes = 4LL * L2A_SCORE_ROWS * (program ? 2LL * (obs_dim | 1) + (act_dim | 1) : (long long)(obs_dim | 1));
    if (lds_bytes > L2A_SCORE_LDS_MAX)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_term: 64 rows of obs_dim " + std::to_string(obs_dim) + " / act_dim " +
                        std::to_string(act_dim) + " do not fit the LDS");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    if (best_key) L2A_HIP(ctx, hipMemsetAsync(best_key, 0, sizeof(unsigned long long) * (size_t)m, stream));
    double d = 1.0;     // discount ** h by the rollout kernels' own recurrence, as l2a_value_terminal
    for (int t = 0; t < h; ++t) d *= discount;
    L2ATermParams p;
    std::memset(&p, 0, sizeof(p));
    p.obs0 = obs0; p.traj = traj; p.actions = actions; p.step_rewards = step_rewards; p.terminal_values = terminal_values;
    p.returns_out = returns_out; p.steps_alive = steps_alive_out; p.best_key = best_key;
    p.discount = discount; p.w = (float)(value_coef * d);
    p.rows = m * n; p.n = n; p.h = h; p.obs_dim = obs_dim; p.act_dim = act_dim; p.cand_offset = cand_offset;
    p.term = *termination;
    if (program) p.prog = *program;
    const int blocks = l2a_ceil_div(p.rows, L2A_SCORE_ROWS);
    hipLaunchKernelGGL(l2a_score_term_k, dim3(blocks), dim3(L2A_SCORE_THREADS), (size_t)lds_bytes, stream, p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

}  // extern "C"
