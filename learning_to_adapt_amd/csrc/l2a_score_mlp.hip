// l2a_score_mlp.hip - learned reward models (include/l2a.h: l2a_reward_model): the host-only eligibility check, the model
// object, and the matrix-core kernel that scores trajectories with it (l2a_score_trajectory_model,
// l2a_plan_rs_reward_model) or evaluates it row by row (l2a_reward_model_predict).
//
// Semantics.  Per (step, candidate) row, all fp32:
//   x = [ (obs - mu_obs) * inv_obs | (act - mu_act) * inv_act | ((next - obs) - mu_delta) * inv_delta ],  inv = fp32(1 / (sd + 1e-10))
//   z = MLP(x): n_hidden = 1 .. 3 hidden layers (widths multiples of 64 up to 512, one of the five L2A_ACT_*), linear scalar output
//   r = z * fp32(sd_r + 1e-10) + fp32(mu_r);  r = NaN when any of the row's obs / act / next values is not finite
//   R = R + fp32(disc) * r, disc carried in float64 (disc *= discount), t = 0 .. h - 1 in order - as l2a_score_traj_k.
// This unit is compiled with contraction off: no multiply-add outside the MFMAs is fused.
//
// Kernel.  D = W^T-tile x activations on v_mfma_f32_16x16x4_f32 with the fragment scheme of the rollout kernels (l2a_kernels.h:
// the packed A fragments, the D fragment of one layer = the B fragment of the next).  A workgroup (4 waves) owns CT tiles of 16
// candidates for the whole horizon and takes S steps of them per pass: RT = CT * S row tiles of 16 rows.  The pass's activations
// live in ONE LDS image [row tile][k-group][lane] of f32x4, overwritten in place layer by layer: wave w computes unit tiles
// [w * TPW, (w + 1) * TPW) of a layer (TPW = width / 64) for all RT row tiles with TPW x RT accumulators in registers, so each
// A fragment (one 16-byte load per lane from L2, prefetched one k-group ahead) feeds 16 * RT rows and is fetched by exactly one
// wave of the workgroup.  RT is 8 up to width 256 and 4 above (accumulators: 128 registers; LDS image: 128 KiB) - more rows per
// fragment do not fit a CU: the image alone is rows x width x 4 bytes.
//
// A row's reward bits depend on the row's inputs only: every output element is ONE accumulator chain over k in the order
// k-group 0, 1, .. and inside a group MFMA 0 .. 3, i.e. (l2a_kernels.h) features 16g + 4kk + ii for ii = 0 .. 3 (outer), kk = 0 .. 3
// (inside the instruction) - whichever row tile, workgroup geometry (RT, CT, S), shard or cand_offset the row falls into.  K is
// padded with zeros to a multiple of 16.  The scalar output layer is the same chain on a unit tile whose rows 1 .. 15 are zero.
// No float atomics.  The descriptor, the hidden-layer routine and the output chain are shared with the value and policy kernels
// (l2a_rm_layer.h), the model object with their models (l2a_rm_net.hip); the pass prologue, the discounted sum, the keys and the
// geometry search are this unit's own.
#pragma clang fp contract(off)

#include "l2a_host.h"
#include "l2a_kernels.h"
#include "l2a_rm_net.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

struct L2ARMParams {
    L2ARmNet net;                   // d_in = 2 * obs_dim + act_dim
    int obs_dim, act_dim;
    float sr, mur;                  // fp32(sd_r + 1e-10), fp32(mu_r)
    const float* obs0;              // [m, obs_dim], or [rows, obs_dim] when obs_per_row
    const float* traj;              // [h, rows, obs_dim]
    const float* actions;           // [h, rows, act_dim]
    float* returns_out;             // [rows] or null
    unsigned long long* best_key;   // [m] or null
    double discount;
    int rows, n, h, obs_per_row, cand_offset;
    int CT, S;                      // candidate tiles per workgroup, steps per pass; CT * S = RT
};

// One workgroup = 16 * CT consecutive candidates (rows r of [0, m * n)) over the whole horizon, S steps per pass.
// Row tile rt = ct * S + s of a pass holds candidates r0 + 16 ct + 0 .. 15 at step t0 + s.
template <int RT>
__global__ __launch_bounds__(L2A_RM_THREADS) void l2a_score_mlp_k(const L2ARMParams p) {
    extern __shared__ f32x4 act[];                      // [RT][kgs][64]
    __shared__ float sz[L2A_RM_MAX_ROWS];               // the pass's network outputs
    __shared__ int sbad[L2A_RM_MAX_ROWS];               // row holds a non-finite input
    __shared__ unsigned long long skey[L2A_RM_MAX_ROWS];
    __shared__ int senv[L2A_RM_MAX_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int CT = p.CT, S = p.S;
    const int r0 = (int)blockIdx.x * 16 * CT;
    const int nr = min(16 * CT, p.rows - r0);           // candidates of this workgroup
    const float* __restrict__ mu = p.net.wblk + p.net.nm;
    const float* __restrict__ inv = mu + 16 * p.net.KG0;
    const int kpad = 16 * p.net.KG0;
    float* actf = reinterpret_cast<float*>(act);

    if (tid < L2A_RM_MAX_ROWS) sbad[tid] = 0;
    __syncthreads();
    float R = 0.0f;
    double disc = 1.0;
    for (int t0 = 0; t0 < p.h; t0 += S) {
        unsigned live = 0;
        for (int rt = 0; rt < RT; ++rt)
            if (16 * (rt / S) < nr && t0 + rt % S < p.h) live |= 1u << rt;
        // ---- features of the pass into the image (zero rows and zero padding where there is nothing) ----
        for (int e = tid; e < 16 * RT * kpad; e += L2A_RM_THREADS) {
            const int i = e / kpad, k = e - i * kpad;
            const int rt = i >> 4, j = i & 15;
            const int ci = 16 * (rt / S) + j, t = t0 + rt % S;
            float x = 0.0f;
            if (ci < nr && t < p.h && k < p.net.d_in) {
                const size_t r = (size_t)(r0 + ci);
                const float* o = p.obs_per_row ? p.obs0 + r * p.obs_dim
                                 : (t == 0)    ? p.obs0 + (r / (size_t)p.n) * p.obs_dim
                                               : p.traj + ((size_t)(t - 1) * p.rows + r) * p.obs_dim;
                const size_t q = (size_t)t * p.rows + r;
                float v;
                bool fin;
                if (k < p.obs_dim) {
                    v = o[k];
                    fin = isfinite(v);
                } else if (k < p.obs_dim + p.act_dim) {
                    v = p.actions[q * p.act_dim + (k - p.obs_dim)];
                    fin = isfinite(v);
                } else {
                    const int d = k - p.obs_dim - p.act_dim;
                    const float nx = p.traj[q * p.obs_dim + d];
                    v = nx - o[d];
                    fin = isfinite(nx);
                }
                if (!fin) sbad[i] = 1;
                x = (v - mu[k]) * inv[k];
            }
            actf[l2a_rm_image_index(rt, p.net.kgs, k, j)] = x;
        }
        __syncthreads();
        // ---- hidden layers, in place ----
        int KGin = p.net.KG0;
        for (int l = 0; l < p.net.n_hidden; ++l) KGin = l2a_rm_hidden_layer<RT>(p.net, l, KGin, act, live, tid, wave, lane);
        // ---- the scalar output layer: row tiles dealt to the waves; unit 0 = register 0 of lanes 0 .. 15 ----
        {
            const float bo = p.net.wblk[p.net.bias[p.net.n_hidden]];
#pragma unroll
            for (int q = 0; q < (RT + 3) / 4; ++q) {
                const int rt = wave + 4 * q;
                if (rt < RT && ((live >> rt) & 1u)) {
                    const f32x4 acc = l2a_rm_out_chain(p.net, act, rt, KGin, lane);
                    if (lane < 16) sz[rt * 16 + lane] = acc.x + bo;
                }
            }
        }
        __syncthreads();
        // ---- the pass's steps of this thread's candidate, in order ----
        if (tid < nr) {
            const int ct = tid >> 4, j = tid & 15;
            for (int s = 0; s < S && t0 + s < p.h; ++s) {
                const int i = (ct * S + s) * 16 + j;
                float r = sz[i] * p.sr + p.mur;
                if (sbad[i]) { r = __builtin_nanf(""); sbad[i] = 0; }
                R = R + (float)disc * r;
                disc *= p.discount;
            }
        }
        __syncthreads();        // the next pass overwrites the image, sz and sbad
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

struct l2a_reward_model : l2a_rm_core {          // d_in = 2 * obs_dim + act_dim, one output
    int obs_dim = 0, act_dim = 0;
    float sr = 1.0f, mur = 0.0f;
};

namespace {

// Launch geometry: RT row tiles per pass (accumulator and LDS budget), of them S steps x CT candidate tiles.  Any choice gives
// the same bits; this one minimises (rounds of workgroups) x (passes) x (pass cost ~ RT + 2).  Plain integers, no context and
// no HIP call: launch() and l2a_reward_model_geometry share it.  False (outputs untouched) when no RT fits the LDS.
bool choose_geometry(int n_hidden, const int* hidden, int obs_dim, int act_dim, long long rows, int h, int num_cu,
                     int lds_per_block, int* rt_out, int* ct_out, int* s_out) {
    int tpw_max = 1;
    for (int l = 0; l < n_hidden; ++l) tpw_max = hidden[l] / 64 > tpw_max ? hidden[l] / 64 : tpw_max;
    const int kgs = l2a_rm_kgs(n_hidden, hidden, 2 * obs_dim + act_dim);
    const int cus = num_cu > 0 ? num_cu : 256;
    long long best_cost = -1;
    for (int rt = 8; rt >= 1; rt >>= 1) {
        if (rt * tpw_max > L2A_RM_MAX_ACC) continue;
        if ((long long)rt * kgs * 1024 + 4096 > lds_per_block) continue;
        for (int s = rt; s >= 1; s >>= 1) {
            if (s > 1 && s / 2 >= h) continue;          // steps per pass beyond the horizon are empty tiles
            const int ct = rt / s;
            const long long wgs = (rows + 16 * ct - 1) / (16 * ct);
            const long long cost = ((wgs + cus - 1) / cus) * ((h + s - 1) / s) * (rt + 2);
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; *rt_out = rt; *ct_out = ct; *s_out = s; }
        }
    }
    return best_cost >= 0;
}

int launch(l2a_reward_model* rm, L2ARMParams& p, hipStream_t stream) {
    l2a_rm_core_net(rm, &p.net);
    p.obs_dim = rm->obs_dim; p.act_dim = rm->act_dim;
    p.sr = rm->sr; p.mur = rm->mur;
    int rt = 1, ct = 1, s = 1;
    (void)choose_geometry(rm->n_hidden, rm->hidden, rm->obs_dim, rm->act_dim, p.rows, p.h, rm->ctx->num_cu, rm->ctx->lds_per_block,
                          &rt, &ct, &s);
    p.CT = ct; p.S = s;
    const unsigned blocks = (unsigned)(((long long)p.rows + 16 * ct - 1) / (16 * ct));
    return L2A_RM_LAUNCH_RT(l2a_score_mlp_k, L2ARMParams, rm, rt, p, blocks, stream);
}

}  // namespace

extern "C" {

int l2a_reward_model_check(int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act) {
    return l2a_rm_check("reward model: ", obs_dim, &act_dim, "1 .. 16", n_hidden, hidden, hidden_act);
}

int l2a_reward_model_geometry(int obs_dim, int act_dim, int n_hidden, const int* hidden, long long rows, int h, int num_cu,
                              int lds_per_block, int* out) {
    if (!out || rows < 1 || h < 1) return L2A_EINVAL;
    const int rc = l2a_reward_model_check(obs_dim, act_dim, n_hidden, hidden, L2A_ACT_RELU);
    if (rc != L2A_OK) return rc;
    int rt = 1, ct = 1, s = 1;
    if (!choose_geometry(n_hidden, hidden, obs_dim, act_dim, rows, h, num_cu, lds_per_block, &rt, &ct, &s))
        return l2a_fail(nullptr, L2A_EINVAL, "reward model: no launch geometry fits " + std::to_string(lds_per_block) + " bytes of LDS");
    const long long wgs = (rows + 16 * ct - 1) / (16 * ct);
    if (wgs > 0x7fffffffLL) return l2a_fail(nullptr, L2A_EINVAL, "reward model: too many rows");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = rt; out[1] = ct; out[2] = s;
    out[3] = (int)wgs;
    out[4] = (h + s - 1) / s;
    out[5] = rt * l2a_rm_kgs(n_hidden, hidden, 2 * obs_dim + act_dim) * 1024;
    return L2A_OK;
}

int l2a_reward_model_create(l2a_ctx* ctx, int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act,
                            l2a_reward_model** out) {
    if (!ctx || !out) return L2A_EINVAL;
    const int rc = l2a_reward_model_check(obs_dim, act_dim, n_hidden, hidden, hidden_act);
    if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
    l2a_reward_model* rm = new l2a_reward_model();
    rm->obs_dim = obs_dim; rm->act_dim = act_dim;
    l2a_device_guard guard(ctx->device);
    int rc_c = l2a_rm_core_create(rm, ctx, "l2a_reward_model_create", 2 * obs_dim + act_dim, 1, n_hidden, hidden, hidden_act, 0);
    // identity statistics until l2a_reward_model_set_norm is called (on the null stream, drained here)
    if (rc_c == L2A_OK)
        rc_c = l2a_reward_model_set_norm(rm, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc_c == L2A_OK && hipStreamSynchronize(nullptr) != hipSuccess)
        rc_c = l2a_fail(ctx, L2A_EHIP, "l2a_reward_model_create: hipStreamSynchronize failed");
    if (rc_c == L2A_OK) *out = rm;
    else l2a_reward_model_destroy(rm);
    return rc_c;
}

void l2a_reward_model_destroy(l2a_reward_model* rm) {
    if (!rm) return;
    l2a_rm_core_free(rm);
    delete rm;
}

int l2a_reward_model_set_weights(l2a_reward_model* rm, const void* const* device_ptrs, void* stream_v) {
    return l2a_rm_core_set_weights(rm, "l2a_reward_model_set_weights", device_ptrs, stream_v);
}

int l2a_reward_model_set_norm(l2a_reward_model* rm, const double* mean_obs, const double* std_obs, const double* mean_act,
                              const double* std_act, const double* mean_delta, const double* std_delta, const double* mean_r,
                              const double* std_r, void* stream_v) {
    if (!rm) return L2A_EINVAL;
    l2a_ctx* ctx = rm->ctx;
    const int n_null = !mean_obs + !std_obs + !mean_act + !std_act + !mean_delta + !std_delta + !mean_r + !std_r;
    if (n_null != 0 && n_null != 8)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_reward_model_set_norm: pass all eight statistics, or none for identity");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    float* mu = nullptr;
    const int rc = l2a_rm_core_norm_stage(rm, stream, &mu);
    if (rc != L2A_OK) return rc;
    float* inv = mu + 16 * rm->KG0;
    const double eps = 1e-10;
    for (int k = 0; k < rm->d_in; ++k) {
        if (n_null) { mu[k] = 0.0f; inv[k] = 1.0f; continue; }
        const int oa = rm->obs_dim + rm->act_dim;
        const double m_ = k < rm->obs_dim ? mean_obs[k] : k < oa ? mean_act[k - rm->obs_dim] : mean_delta[k - oa];
        const double s_ = k < rm->obs_dim ? std_obs[k] : k < oa ? std_act[k - rm->obs_dim] : std_delta[k - oa];
        mu[k] = (float)m_;
        inv[k] = (float)(1.0 / (s_ + eps));
    }
    rm->mur = n_null ? 0.0f : (float)*mean_r;
    rm->sr = n_null ? 1.0f : (float)(*std_r + eps);
    return l2a_rm_core_norm_upload(rm, stream);
}

int l2a_reward_model_predict(l2a_reward_model* rm, const float* obs, const float* act, const float* next_obs, int rows,
                             float* rewards_out, void* stream_v) {
    if (!rm) return L2A_EINVAL;
    l2a_ctx* ctx = rm->ctx;
    if (!obs || !act || !next_obs || !rewards_out) return l2a_fail(ctx, L2A_EINVAL, "l2a_reward_model_predict: null pointer");
    if (rows < 1 || rows > 0x3fffffff) return l2a_fail(ctx, L2A_EINVAL, "l2a_reward_model_predict: rows must be 1 .. 2^30 - 1");
    if (!rm->weights_set) return l2a_fail(ctx, L2A_ESTATE, "the reward model's weights were never set");
    l2a_device_guard guard(ctx->device);
    L2ARMParams p;
    std::memset(&p, 0, sizeof(p));
    p.obs0 = obs; p.traj = next_obs; p.actions = act; p.returns_out = rewards_out; p.best_key = nullptr;
    p.discount = 1.0; p.rows = rows; p.n = rows; p.h = 1; p.obs_per_row = 1; p.cand_offset = 0;
    return launch(rm, p, reinterpret_cast<hipStream_t>(stream_v));
}

int l2a_score_trajectory_model(l2a_reward_model* rm, const float* obs0, const float* traj, const float* actions, int m, int n,
                               int h, double discount, int cand_offset, float* returns_out, unsigned long long* best_key,
                               void* stream_v) {
    if (!rm) return L2A_EINVAL;
    l2a_ctx* ctx = rm->ctx;
    if (!obs0 || !traj || !actions) return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_model: null obs0/traj/actions");
    if (!best_key && !returns_out)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_model: nothing to write (best_key and returns_out are null)");
    if (m < 1 || n < 1 || h < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_model: m, n and h must be >= 1");
    if ((long long)m * n > 0x3fffffffLL || cand_offset < 0 || (long long)cand_offset + n > 0x7fffffffLL)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_score_trajectory_model: too many candidates");
    if (!rm->weights_set) return l2a_fail(ctx, L2A_ESTATE, "the reward model's weights were never set");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    if (best_key) L2A_HIP(ctx, hipMemsetAsync(best_key, 0, sizeof(unsigned long long) * (size_t)m, stream));
    L2ARMParams p;
    std::memset(&p, 0, sizeof(p));
    p.obs0 = obs0; p.traj = traj; p.actions = actions; p.returns_out = returns_out; p.best_key = best_key;
    p.discount = discount; p.rows = m * n; p.n = n; p.h = h; p.obs_per_row = 0; p.cand_offset = cand_offset;
    return launch(rm, p, stream);
}

void l2a_reward_model_facts(const l2a_reward_model* rm, l2a_ctx** ctx, int* obs_dim, int* act_dim) {
    if (ctx) *ctx = rm->ctx;
    if (obs_dim) *obs_dim = rm->obs_dim;
    if (act_dim) *act_dim = rm->act_dim;
}

}  // extern "C"
