// l2a_value.hip - learned terminal values (include/l2a.h: l2a_value_model): the host-only eligibility check, the model object,
// and the matrix-core kernel that evaluates it on the m * n last predicted states of a plan and folds it into the returns and
// the arg-max keys (l2a_value_terminal), or evaluates it row by row (l2a_value_model_predict).
//
// Semantics.  Per row (one candidate's state after the last horizon step), all fp32:
//   x  = (s_h - mu_obs) * inv_obs,  inv = fp32(1 / (sd + 1e-10))
//   z  = MLP(x): n_hidden = 1 .. 3 hidden layers (widths multiples of 64 up to 512, one of the five L2A_ACT_*), linear scalar output
//   v  = z * fp32(sd_v + 1e-10) + fp32(mu_v);  v = NaN when any value of the row's state is not finite
//   w  = fp32(value_coef * d_h), d_h = discount ** h in float64 by h multiplications from 1.0 (the rollout's recurrence), rounded ONCE
//   R' = R + w * v   a multiply and an add;  w == 0 leaves R' = R bit for bit (v is not looked at)
// This unit is compiled with contraction off: no multiply-add outside the MFMAs is fused.
//
// Kernel.  The network descriptor, the hidden-layer routine, the output tile's chain, the fragment scheme and the k order are shared with
// the reward-model scorer and the policy kernel (l2a_rm_layer.h); the model object is l2a_rm_net.hip's core.  One LDS image
// [row tile][k-group][lane] of f32x4 overwritten in place layer by layer, every output element ONE accumulator chain over k, K
// padded with zeros to a multiple of 16 - a row's value bits depend on the row's state only.  This unit keeps what is its own: the
// prologue (normalised states), the epilogue (the fold and the per-env keys) and the public entry points.
// There is one "step": a workgroup (4 waves) owns RT consecutive row tiles of 16 rows, once.  The epilogue computes v and R',
// stores the row and reduces the packed keys per env: __shfl_xor inside a wave, one LDS word per (env, wave), ONE integer
// atomicMax per workgroup per env it touches (a workgroup's rows may straddle env boundaries).  No float atomics.
#pragma clang fp contract(off)

#include "l2a_host.h"
#include "l2a_kernels.h"
#include "l2a_rm_net.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

struct L2AVParams {
    L2ARmNet net;                   // d_in = obs_dim
    float sv, muv;                  // fp32(sd_v + 1e-10), fp32(mu_v)
    const float* states;            // [rows, d_in]
    const float* returns_in;        // [rows], or null: predict (values_out = v)
    float* out;                     // [rows] or null: R' (fold) or v (predict)
    unsigned long long* best_key;   // [m] or null
    float w;                        // fp32(value_coef * discount ** h)
    int rows, n, cand_offset;
};

// One workgroup = rows [16 RT b, 16 RT (b + 1)) of the m * n; row tile rt holds rows r0 + 16 rt + 0 .. 15.
template <int RT>
__global__ __launch_bounds__(L2A_RM_THREADS) void l2a_value_mlp_k(const L2AVParams p) {
    extern __shared__ f32x4 act[];                      // [RT][kgs][64]
    __shared__ float sz[L2A_RM_MAX_ROWS];               // the network outputs
    __shared__ int sbad[L2A_RM_MAX_ROWS];               // row holds a non-finite input
    __shared__ unsigned long long swk[L2A_RM_MAX_ROWS][2];      // per env of this workgroup (at most one per row): the two row waves' maxima
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = (int)blockIdx.x * 16 * RT;
    const int nr = min(16 * RT, p.rows - r0);           // rows of this workgroup
    const float* __restrict__ mu = p.net.wblk + p.net.nm;
    const float* __restrict__ inv = mu + 16 * p.net.KG0;
    const int kpad = 16 * p.net.KG0;
    float* actf = reinterpret_cast<float*>(act);

    if (tid < L2A_RM_MAX_ROWS) { sbad[tid] = 0; swk[tid][0] = 0ull; swk[tid][1] = 0ull; }
    __syncthreads();
    unsigned live = 0;
    for (int rt = 0; rt < RT; ++rt)
        if (16 * rt < nr) live |= 1u << rt;
    // ---- prologue: the normalised states into the image (zero rows and zero padding where there is nothing) ----
    for (int e = tid; e < 16 * RT * kpad; e += L2A_RM_THREADS) {
        const int i = e / kpad, k = e - i * kpad;
        const int rt = i >> 4, j = i & 15;
        float x = 0.0f;
        if (i < nr && k < p.net.d_in) {
            const float v = p.states[(size_t)(r0 + i) * p.net.d_in + k];
            if (!isfinite(v)) sbad[i] = 1;
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
    // ---- epilogue: v, R', the row's store and key ----
    unsigned long long key = 0ull;      // (below every real key: l2a_key_pack's ordered -inf is 0x007fffff << 31)
    int env = -1;
    if (tid < nr) {
        const int row = r0 + tid;
        float v = sz[tid] * p.sv + p.muv;
        if (sbad[tid]) v = __builtin_nanf("");
        if (!p.returns_in) {
            p.out[row] = v;
        } else {
            float R = p.returns_in[row];
            if (p.w != 0.0f) R = R + p.w * v;
            if (p.out) p.out[row] = R;
            env = row / p.n;
            key = l2a_key_pack(R, p.cand_offset + (row - env * p.n));
        }
    }
    if (!p.best_key || !p.returns_in) return;           // (uniform over the workgroup)
    // rows live in waves 0 and 1 (16 RT <= 128): each reduces the envs ITS rows touch - a wave-uniform range - into swk[env][wave]
    const int env_lo = r0 / p.n;
    if (wave < 2 && 64 * wave < nr) {
        const int e0 = (r0 + 64 * wave) / p.n, e1 = (r0 + min(64 * wave + 63, nr - 1)) / p.n;
        for (int e = e0; e <= e1; ++e) {
            unsigned long long k = (env == e) ? key : 0ull;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long o = __shfl_xor(k, d, 64);
                k = (o > k) ? o : k;
            }
            if (lane == 0) swk[e - env_lo][wave] = k;
        }
    }
    __syncthreads();
    const int n_env = (r0 + nr - 1) / p.n - env_lo + 1;
    if (tid < n_env) {
        const unsigned long long a = swk[tid][0], b = swk[tid][1];
        atomicMax(p.best_key + env_lo + tid, (a > b) ? a : b);
    }
}

struct l2a_value_model : l2a_rm_core {           // d_in = obs_dim, one output
    float sv = 1.0f, muv = 0.0f;
};

namespace {

int launch(l2a_value_model* vm, L2AVParams& p, hipStream_t stream) {
    l2a_rm_core_net(vm, &p.net);
    p.sv = vm->sv; p.muv = vm->muv;
    const int rt = l2a_rm_choose_rt(vm->n_hidden, vm->hidden, vm->d_in, p.rows, vm->ctx->num_cu, vm->ctx->lds_per_block);
    if (rt < 1) return l2a_fail(vm->ctx, L2A_EINVAL, "value model: no launch geometry fits the device's LDS");
    const unsigned blocks = (unsigned)(((long long)p.rows + 16 * rt - 1) / (16 * rt));
    return L2A_RM_LAUNCH_RT(l2a_value_mlp_k, L2AVParams, vm, rt, p, blocks, stream);
}

}  // namespace

extern "C" {

int l2a_value_model_check(int obs_dim, int n_hidden, const int* hidden, int hidden_act) {
    return l2a_rm_check("value model: ", obs_dim, nullptr, nullptr, n_hidden, hidden, hidden_act);
}

int l2a_value_model_geometry(int obs_dim, int n_hidden, const int* hidden, long long rows, int num_cu, int lds_per_block, int* out) {
    if (!out || rows < 1) return L2A_EINVAL;
    const int rc = l2a_value_model_check(obs_dim, n_hidden, hidden, L2A_ACT_RELU);
    if (rc != L2A_OK) return rc;
    return l2a_rm_rt_geometry("value model: ", n_hidden, hidden, obs_dim, rows, num_cu, lds_per_block, out);
}

int l2a_value_model_create(l2a_ctx* ctx, int obs_dim, int n_hidden, const int* hidden, int hidden_act, l2a_value_model** out) {
    if (!ctx || !out) return L2A_EINVAL;
    const int rc = l2a_value_model_check(obs_dim, n_hidden, hidden, hidden_act);
    if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
    l2a_value_model* vm = new l2a_value_model();
    l2a_device_guard guard(ctx->device);
    int rc_c = l2a_rm_core_create(vm, ctx, "l2a_value_model_create", obs_dim, 1, n_hidden, hidden, hidden_act, 0);
    // identity statistics until l2a_value_model_set_norm is called (on the null stream, drained here)
    if (rc_c == L2A_OK) rc_c = l2a_value_model_set_norm(vm, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc_c == L2A_OK && hipStreamSynchronize(nullptr) != hipSuccess)
        rc_c = l2a_fail(ctx, L2A_EHIP, "l2a_value_model_create: hipStreamSynchronize failed");
    if (rc_c == L2A_OK) *out = vm;
    else l2a_value_model_destroy(vm);
    return rc_c;
}

void l2a_value_model_destroy(l2a_value_model* vm) {
    if (!vm) return;
    l2a_rm_core_free(vm);
    delete vm;
}

int l2a_value_model_set_weights(l2a_value_model* vm, const void* const* device_ptrs, void* stream_v) {
    return l2a_rm_core_set_weights(vm, "l2a_value_model_set_weights", device_ptrs, stream_v);
}

int l2a_value_model_set_norm(l2a_value_model* vm, const double* mean_obs, const double* std_obs, const double* mean_v,
                             const double* std_v, void* stream_v) {
    if (!vm) return L2A_EINVAL;
    l2a_ctx* ctx = vm->ctx;
    const int n_null = !mean_obs + !std_obs + !mean_v + !std_v;
    if (n_null != 0 && n_null != 4)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_value_model_set_norm: pass all four statistics, or none for identity");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    float* mu = nullptr;
    const int rc = l2a_rm_core_norm_stage(vm, stream, &mu);
    if (rc != L2A_OK) return rc;
    float* inv = mu + 16 * vm->KG0;
    const double eps = 1e-10;
    for (int k = 0; k < vm->d_in; ++k) {
        if (n_null) { mu[k] = 0.0f; inv[k] = 1.0f; continue; }
        mu[k] = (float)mean_obs[k];
        inv[k] = (float)(1.0 / (std_obs[k] + eps));
    }
    vm->muv = n_null ? 0.0f : (float)*mean_v;
    vm->sv = n_null ? 1.0f : (float)(*std_v + eps);
    return l2a_rm_core_norm_upload(vm, stream);
}

int l2a_value_model_predict(l2a_value_model* vm, const float* states, int rows, float* values_out, void* stream_v) {
    if (!vm) return L2A_EINVAL;
    l2a_ctx* ctx = vm->ctx;
    if (!states || !values_out) return l2a_fail(ctx, L2A_EINVAL, "l2a_value_model_predict: null pointer");
    if (rows < 1 || rows > 0x3fffffff) return l2a_fail(ctx, L2A_EINVAL, "l2a_value_model_predict: rows must be 1 .. 2^30 - 1");
    if (!vm->weights_set) return l2a_fail(ctx, L2A_ESTATE, "the value model's weights were never set");
    l2a_device_guard guard(ctx->device);
    L2AVParams p;
    std::memset(&p, 0, sizeof(p));
    p.states = states; p.returns_in = nullptr; p.out = values_out; p.best_key = nullptr;
    p.w = 0.0f; p.rows = rows; p.n = rows; p.cand_offset = 0;
    return launch(vm, p, reinterpret_cast<hipStream_t>(stream_v));
}

int l2a_value_terminal(l2a_value_model* vm, const float* final_state, const float* returns_in, int m, int n, int h, double discount,
                       double value_coef, int cand_offset, float* returns_out, unsigned long long* best_key, void* stream_v) {
    if (!vm) return L2A_EINVAL;
    l2a_ctx* ctx = vm->ctx;
    if (!final_state || !returns_in) return l2a_fail(ctx, L2A_EINVAL, "l2a_value_terminal: null final_state/returns_in");
    if (!best_key && !returns_out)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_value_terminal: nothing to write (best_key and returns_out are null)");
    if (m < 1 || n < 1 || h < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_value_terminal: m, n and h must be >= 1");
    if (!std::isfinite(discount) || !std::isfinite(value_coef))
        return l2a_fail(ctx, L2A_EINVAL, "l2a_value_terminal: discount and value_coef must be finite");
    if ((long long)m * n > 0x3fffffffLL || cand_offset < 0 || (long long)cand_offset + n > 0x7fffffffLL)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_value_terminal: too many candidates");
    if (!vm->weights_set) return l2a_fail(ctx, L2A_ESTATE, "the value model's weights were never set");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    if (best_key) L2A_HIP(ctx, hipMemsetAsync(best_key, 0, sizeof(unsigned long long) * (size_t)m, stream));
    double d = 1.0;     // discount ** h by the rollout kernels' own recurrence
    for (int t = 0; t < h; ++t) d *= discount;
    L2AVParams p;
    std::memset(&p, 0, sizeof(p));
    p.states = final_state; p.returns_in = returns_in; p.out = returns_out; p.best_key = best_key;
    p.w = (float)(value_coef * d); p.rows = m * n; p.n = n; p.cand_offset = cand_offset;
    return launch(vm, p, stream);
}

void l2a_value_model_facts(const l2a_value_model* vm, l2a_ctx** ctx, int* obs_dim) {
    if (ctx) *ctx = vm->ctx;
    if (obs_dim) *obs_dim = vm->d_in;
}

}  // extern "C"
