// l2a_policy.hip - learned policy priors (include/l2a.h: l2a_policy_model): the host-only eligibility check, the model object and
// the matrix-core kernel that evaluates the policy on a batch of states and writes clipped, optionally noisy actions
// (l2a_policy_act; the steps of l2a_policy_propose, l2a_api.hip, go through the same launcher).
//
// Semantics.  Per row, all fp32, nothing contracted:
//   x   = (s - mu_obs) * inv_obs,  inv = fp32(1 / (sd + 1e-10))
//   y   = MLP(x): n_hidden = 1 .. 3 hidden layers (widths multiples of 64 up to 512, one of the five L2A_ACT_*), a linear output layer
//         of act_dim <= 16 units
//   a_k = y_k * fp32(sd_a,k + 1e-10) + fp32(mu_a,k)
//   a_k = a_k + sigma_k * z_k       a multiply and an add; skipped where sigma_k == 0 (no z is read or drawn then)
//   a_k = min(max(a_k, low_k), high_k), NaN propagating;  every a_k = NaN when any value of the row's state is not finite
// z is given, or the Philox4x32-10 + Box-Muller normal of l2a_cem.hip / l2a_mppi.hip (l2a_philox_normal, l2a_philox.h).
//
// Kernel.  l2a_value_mlp_k's frame (the shared descriptor, hidden-layer routine and output chain of l2a_rm_layer.h; the model object is
// l2a_rm_net.hip's core): 4 waves, RT row tiles of 16 rows, one LDS image [row tile][k-group][lane] of
// f32x4 overwritten in place, every output element ONE accumulator chain over k, K padded with zeros to a multiple of 16.  The
// output layer is ONE 16-unit tile - the same single MFMA chain per row tile as the value kernel's scalar output: unit u of row r
// is register u & 3 of lane 16 (u >> 2) + r.  The tile goes through LDS - the image itself, dead after the last hidden layer - as
// [row][20 words]: a lane stores its four units with one 16-byte write, and the 8 consecutive lanes a 16-byte write is served in
// are 8 rows at a stride of 20 words = 8 different 4-bank slots of the 32 banks (20 r mod 32 = 0, 20, 8, 28, 16, 4, 24, 12): no
// conflict.  Thread e of the epilogue then owns element (row e / act_dim, dimension e % act_dim): consecutive threads read
// consecutive words of a row, and a row's act_dim words are stored contiguously.  No keys, no atomics.
#pragma clang fp contract(off)

#include "l2a_host.h"
#include "l2a_kernels.h"
#include "l2a_philox.h"
#include "l2a_rm_net.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#define L2A_PM_OSTRIDE 20           // words between the rows of the transposed output tile

struct L2APParams {
    L2ARmNet net;                   // d_in = obs_dim; nm: [mu KG0*16][inv KG0*16][sd_a 16][mu_a 16]
    int act_dim;
    const float* states;            // [rows, obs_dim], or [m, obs_dim] (state_per_row == 0: env i's row for all its candidates)
    int state_per_row;
    int rows;                       // m * npl
    int npl;                        // proposal rows per env in this launch (row = i * npl + j)
    int m, n, n_pi, h, t, cand_offset;      // the noise / seq / mirror indexing (global candidate gj = cand_offset + j)
    const float* z;                 // [h, m, n_pi, act_dim] or null (draw)
    unsigned long long seed, offset;
    const float* sigma;             // [act_dim]
    const float* low;
    const float* high;
    float* out;                     // [rows, act_dim]
    float* seq;                     // [h, m * n, act_dim] or null
    float* mirror;                  // [n_total, m, h * act_dim] or null
};

namespace {

// min that propagates NaN from either side, as l2a_max_nan does for max
__device__ __forceinline__ float pm_min_nan(float x, float f) { return __builtin_elementwise_minimum(x, f); }

}  // namespace

// One workgroup = rows [16 RT b, 16 RT (b + 1)); row tile rt holds rows r0 + 16 rt + 0 .. 15.
template <int RT>
__global__ __launch_bounds__(L2A_RM_THREADS) void l2a_policy_mlp_k(const L2APParams p) {
    extern __shared__ f32x4 act[];                      // [RT][kgs][64]
    __shared__ int sbad[L2A_RM_MAX_ROWS];               // row holds a non-finite input
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = (int)blockIdx.x * 16 * RT;
    const int nr = min(16 * RT, p.rows - r0);           // rows of this workgroup
    const float* __restrict__ mu = p.net.wblk + p.net.nm;
    const float* __restrict__ inv = mu + 16 * p.net.KG0;
    const float* __restrict__ sda = inv + 16 * p.net.KG0;
    const float* __restrict__ mua = sda + 16;
    const int kpad = 16 * p.net.KG0;
    float* actf = reinterpret_cast<float*>(act);

    if (tid < L2A_RM_MAX_ROWS) sbad[tid] = 0;
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
            const int srow = p.state_per_row ? r0 + i : (r0 + i) / p.npl;
            const float v = p.states[(size_t)srow * p.net.d_in + k];
            if (!isfinite(v)) sbad[i] = 1;
            x = (v - mu[k]) * inv[k];
        }
        actf[l2a_rm_image_index(rt, p.net.kgs, k, j)] = x;
    }
    __syncthreads();
    // ---- hidden layers, in place ----
    int KGin = p.net.KG0;
    for (int l = 0; l < p.net.n_hidden; ++l) KGin = l2a_rm_hidden_layer<RT>(p.net, l, KGin, act, live, tid, wave, lane);
    // ---- the output tile: row tiles dealt to the waves; unit 4 (lane >> 4) + c of row lane & 15 = register c ----
    f32x4 yo[(RT + 3) / 4];
    {
        const f32x4 bo = *reinterpret_cast<const f32x4*>(p.net.wblk + p.net.bias[p.net.n_hidden] + 4 * (lane >> 4));
#pragma unroll
        for (int q = 0; q < (RT + 3) / 4; ++q) {
            const int rt = wave + 4 * q;
            f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (rt < RT && ((live >> rt) & 1u)) acc = l2a_rm_out_chain(p.net, act, rt, KGin, lane);
            yo[q] = acc + bo;
        }
    }
    __syncthreads();            // every wave has read the last hidden layer: the image becomes the transposed output tile
    float* sy = actf;           // [16 RT rows][L2A_PM_OSTRIDE words]: 1280 RT bytes of the image's >= 4096 RT
#pragma unroll
    for (int q = 0; q < (RT + 3) / 4; ++q) {
        const int rt = wave + 4 * q;
        if (rt < RT && ((live >> rt) & 1u))
            *reinterpret_cast<f32x4*>(sy + (rt * 16 + (lane & 15)) * L2A_PM_OSTRIDE + 4 * (lane >> 4)) = yo[q];
    }
    __syncthreads();
    // ---- epilogue: element e = (row, dimension); a row's words are consecutive threads' ----
    const int A = p.act_dim;
    for (int e = tid; e < nr * A; e += L2A_RM_THREADS) {
        const int lr = e / A, k = e - lr * A;
        const int row = r0 + lr;
        const int i = row / p.npl, j = row - i * p.npl;
        const long long gj = (long long)p.cand_offset + j;
        float a = sy[lr * L2A_PM_OSTRIDE + k] * sda[k] + mua[k];
        const float sg = p.sigma[k];
        if (sg != 0.0f) {
            const unsigned long long ze = ((unsigned long long)((long long)p.t * p.m + i) * (unsigned long long)p.n_pi +
                                           (unsigned long long)gj) * (unsigned long long)A + (unsigned long long)k;
            const float z = p.z ? p.z[ze] : l2a_philox_normal(p.seed, p.offset + ze);
            const float nz = sg * z;
            a = a + nz;
        }
        a = pm_min_nan(l2a_max_nan(a, p.low[k]), p.high[k]);
        if (sbad[lr]) a = __builtin_nanf("");
        p.out[(size_t)row * A + k] = a;
        if (p.seq) p.seq[((size_t)p.t * ((size_t)p.m * p.n) + (size_t)i * p.n + j) * A + k] = a;
        if (p.mirror) p.mirror[(((size_t)gj * p.m + i) * p.h + p.t) * A + k] = a;
    }
}

struct l2a_policy_model : l2a_rm_core {};       // d_in = obs_dim, n_out = act_dim

namespace {

int launch(l2a_policy_model* pm, L2APParams& p, hipStream_t stream) {
    l2a_rm_core_net(pm, &p.net);
    p.act_dim = pm->n_out;
    const int rt = l2a_rm_choose_rt(pm->n_hidden, pm->hidden, pm->d_in, p.rows, pm->ctx->num_cu, pm->ctx->lds_per_block);
    if (rt < 1) return l2a_fail(pm->ctx, L2A_EINVAL, "policy model: no launch geometry fits the device's LDS");
    const unsigned blocks = (unsigned)(((long long)p.rows + 16 * rt - 1) / (16 * rt));
    return L2A_RM_LAUNCH_RT(l2a_policy_mlp_k, L2APParams, pm, rt, p, blocks, stream);
}

}  // namespace

extern "C" {

int l2a_policy_model_check(int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act) {
    return l2a_rm_check("policy model: ", obs_dim, &act_dim, "1 .. 16: one output tile", n_hidden, hidden, hidden_act);
}

int l2a_policy_model_geometry(int obs_dim, int act_dim, int n_hidden, const int* hidden, long long rows, int num_cu, int lds_per_block,
                              int* out) {
    if (!out || rows < 1) return L2A_EINVAL;
    const int rc = l2a_policy_model_check(obs_dim, act_dim, n_hidden, hidden, L2A_ACT_RELU);
    if (rc != L2A_OK) return rc;
    return l2a_rm_rt_geometry("policy model: ", n_hidden, hidden, obs_dim, rows, num_cu, lds_per_block, out);
}

int l2a_policy_model_create(l2a_ctx* ctx, int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act,
                            l2a_policy_model** out) {
    if (!ctx || !out) return L2A_EINVAL;
    const int rc = l2a_policy_model_check(obs_dim, act_dim, n_hidden, hidden, hidden_act);
    if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
    l2a_policy_model* pm = new l2a_policy_model();
    l2a_device_guard guard(ctx->device);
    int rc_c = l2a_rm_core_create(pm, ctx, "l2a_policy_model_create", obs_dim, act_dim, n_hidden, hidden, hidden_act, 32);
    // identity statistics until l2a_policy_model_set_norm is called (on the null stream, drained here)
    if (rc_c == L2A_OK) rc_c = l2a_policy_model_set_norm(pm, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc_c == L2A_OK && hipStreamSynchronize(nullptr) != hipSuccess)
        rc_c = l2a_fail(ctx, L2A_EHIP, "l2a_policy_model_create: hipStreamSynchronize failed");
    if (rc_c == L2A_OK) *out = pm;
    else l2a_policy_model_destroy(pm);
    return rc_c;
}

void l2a_policy_model_destroy(l2a_policy_model* pm) {
    if (!pm) return;
    l2a_rm_core_free(pm);
    delete pm;
}

int l2a_policy_model_set_weights(l2a_policy_model* pm, const void* const* device_ptrs, void* stream_v) {
    return l2a_rm_core_set_weights(pm, "l2a_policy_model_set_weights", device_ptrs, stream_v);
}

int l2a_policy_model_set_norm(l2a_policy_model* pm, const double* mean_obs, const double* std_obs, const double* mean_act,
                              const double* std_act, void* stream_v) {
    if (!pm) return L2A_EINVAL;
    l2a_ctx* ctx = pm->ctx;
    const int n_null = !mean_obs + !std_obs + !mean_act + !std_act;
    if (n_null != 0 && n_null != 4)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_policy_model_set_norm: pass all four statistics, or none for identity");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    float* mu = nullptr;
    const int rc = l2a_rm_core_norm_stage(pm, stream, &mu);
    if (rc != L2A_OK) return rc;
    float* inv = mu + 16 * pm->KG0;
    float* sda = inv + 16 * pm->KG0;
    float* mua = sda + 16;
    const double eps = 1e-10;
    for (int k = 0; k < pm->d_in; ++k) {
        if (n_null) { mu[k] = 0.0f; inv[k] = 1.0f; continue; }
        mu[k] = (float)mean_obs[k];
        inv[k] = (float)(1.0 / (std_obs[k] + eps));
    }
    for (int k = 0; k < pm->n_out; ++k) {
        sda[k] = n_null ? 1.0f : (float)(std_act[k] + eps);
        mua[k] = n_null ? 0.0f : (float)mean_act[k];
    }
    return l2a_rm_core_norm_upload(pm, stream);
}

void l2a_policy_model_facts(const l2a_policy_model* pm, l2a_ctx** ctx, int* obs_dim, int* act_dim) {
    if (ctx) *ctx = pm->ctx;
    if (obs_dim) *obs_dim = pm->d_in;
    if (act_dim) *act_dim = pm->n_out;
}

// One launch of the kernel for horizon step t of a proposal (l2a_policy_propose, l2a_api.hip: arguments validated there).
int l2a_policy_step_launch(l2a_policy_model* pm, const float* states, int state_per_row, int m, int npl, int n, int n_pi, int h, int t,
                           int cand_offset, const float* z, unsigned long long seed, unsigned long long offset, const float* sigma,
                           const float* low, const float* high, float* out, float* seq, float* mirror, hipStream_t stream) {
    l2a_ctx* ctx = pm->ctx;
    if (!pm->weights_set) return l2a_fail(ctx, L2A_ESTATE, "the policy model's weights were never set");
    L2APParams p;
    std::memset(&p, 0, sizeof(p));
    p.states = states; p.state_per_row = state_per_row; p.rows = m * npl; p.npl = npl;
    p.m = m; p.n = n; p.n_pi = n_pi; p.h = h; p.t = t; p.cand_offset = cand_offset;
    p.z = z; p.seed = seed; p.offset = offset; p.sigma = sigma; p.low = low; p.high = high;
    p.out = out; p.seq = seq; p.mirror = mirror;
    return launch(pm, p, stream);
}

int l2a_policy_act(l2a_policy_model* pm, const float* states, int rows, const float* z, unsigned long long seed,
                   unsigned long long offset, const float* sigma, const float* low, const float* high, float* actions_out,
                   void* stream_v) {
    if (!pm) return L2A_EINVAL;
    l2a_ctx* ctx = pm->ctx;
    if (!states || !sigma || !low || !high || !actions_out) return l2a_fail(ctx, L2A_EINVAL, "l2a_policy_act: null pointer");
    if (rows < 1 || rows > 0x3fffffff) return l2a_fail(ctx, L2A_EINVAL, "l2a_policy_act: rows must be 1 .. 2^30 - 1");
    l2a_device_guard guard(ctx->device);
    // one "env" of `rows` candidates at step 0 of a one-step plan: the counter of element (row, k) is offset + row * act_dim + k
    return l2a_policy_step_launch(pm, states, 1, 1, rows, rows, rows, 1, 0, 0, z, seed, offset, sigma, low, high, actions_out, nullptr,
                                  nullptr, reinterpret_cast<hipStream_t>(stream_v));
}

}  // extern "C"
