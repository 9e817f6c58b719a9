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
// Kernel.  The layer routine, the fragment scheme and the k order are the reward-model scorer's (l2a_rm_layer.h,
// l2a_score_mlp.hip): one LDS image [row tile][k-group][lane] of f32x4 overwritten in place layer by layer, every output element
// ONE accumulator chain over k, K padded with zeros to a multiple of 16 - a row's value bits depend on the row's state only.
// There is one "step": a workgroup (4 waves) owns RT consecutive row tiles of 16 rows, once.  The epilogue computes v and R',
// stores the row and reduces the packed keys per env: __shfl_xor inside a wave, one LDS word per (env, wave), ONE integer
// atomicMax per workgroup per env it touches (a workgroup's rows may straddle env boundaries).  No float atomics.
#pragma clang fp contract(off)

#include "l2a_host.h"
#include "l2a_kernels.h"
#include "l2a_rm_layer.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

struct L2AVParams {
    const float* wblk;              // the model's device block
    long long pk[L2A_RM_MAX_HIDDEN + 1];    // packed kernels (floats from wblk); [n_hidden] = the output layer
    long long bias[L2A_RM_MAX_HIDDEN + 1];  // biases
    long long nm;                   // [mu KG0*16][inv KG0*16]
    int tpw[L2A_RM_MAX_HIDDEN];     // hidden width / 64
    int n_hidden, obs_dim, KG0, kgs;        // kgs: k-groups between the row tiles of the LDS image
    int act;
    float sv, muv;                  // fp32(sd_v + 1e-10), fp32(mu_v)
    const float* states;            // [rows, obs_dim]
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
    const float* __restrict__ mu = p.wblk + p.nm;
    const float* __restrict__ inv = mu + 16 * p.KG0;
    const int kpad = 16 * p.KG0;
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
        if (i < nr && k < p.obs_dim) {
            const float v = p.states[(size_t)(r0 + i) * p.obs_dim + k];
            if (!isfinite(v)) sbad[i] = 1;
            x = (v - mu[k]) * inv[k];
        }
        actf[(((rt * p.kgs + (k >> 4)) * 64) + ((k >> 2) & 3) * 16 + j) * 4 + (k & 3)] = x;
    }
    __syncthreads();
    // ---- hidden layers, in place ----
    int KGin = p.KG0;
    const float floor = (p.act == L2A_ACT_RELU) ? 0.0f : -__builtin_inff();
    for (int l = 0; l < p.n_hidden; ++l) {
        l2a_rm_layer_any<RT>(p.tpw[l], reinterpret_cast<const f32x4*>(p.wblk + p.pk[l]), p.wblk + p.bias[l], KGin, p.kgs, act,
                             floor, live, wave, lane);
        KGin = 4 * p.tpw[l];
        if (p.act != L2A_ACT_RELU && p.act != L2A_ACT_IDENTITY) {       // tanh / sigmoid / swish: elementwise over the live tiles
            for (int e = tid; e < RT * KGin * 64; e += L2A_RM_THREADS) {
                const int rt = e / (KGin * 64);
                if ((live >> rt) & 1u) {
                    f32x4* q = act + (rt * p.kgs) * 64 + (e - rt * KGin * 64);
                    f32x4 v = *q;
                    v.x = l2a_act1(v.x, p.act); v.y = l2a_act1(v.y, p.act); v.z = l2a_act1(v.z, p.act); v.w = l2a_act1(v.w, p.act);
                    *q = v;
                }
            }
            __syncthreads();
        }
    }
    // ---- the scalar output layer: row tiles dealt to the waves; unit 0 = register 0 of lanes 0 .. 15 ----
    {
        const f32x4* wo = reinterpret_cast<const f32x4*>(p.wblk + p.pk[p.n_hidden]) + lane;
        const float bo = p.wblk[p.bias[p.n_hidden]];
#pragma unroll
        for (int q = 0; q < (RT + 3) / 4; ++q) {
            const int rt = wave + 4 * q;
            if (rt < RT && ((live >> rt) & 1u)) {
                f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                for (int g = 0; g < KGin; ++g) {
                    const f32x4 a = wo[g * 64];
                    const f32x4 b = act[(rt * p.kgs + g) * 64 + lane];
                    acc = L2A_MFMA(a.x, b.x, acc);
                    acc = L2A_MFMA(a.y, b.y, acc);
                    acc = L2A_MFMA(a.z, b.z, acc);
                    acc = L2A_MFMA(a.w, b.w, acc);
                }
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

struct l2a_value_model {
    l2a_ctx* ctx = nullptr;
    int obs_dim = 0, KG0 = 0, kgs = 0;
    int n_hidden = 0, hidden[L2A_RM_MAX_HIDDEN] = {0}, act = L2A_ACT_RELU;
    float* wblk = nullptr;
    long long blk_floats = 0;
    long long pk[L2A_RM_MAX_HIDDEN + 1] = {0}, bias[L2A_RM_MAX_HIDDEN + 1] = {0}, nm = 0;
    float sv = 1.0f, muv = 0.0f;
    bool weights_set = false;
    std::vector<float> norm_stage;              // host staging, kept alive for the async H2D
};

namespace {

int vm_kgs(int n_hidden, const int* hidden, int obs_dim) {
    int kgs = l2a_ceil_div(obs_dim, 16);
    for (int l = 0; l < n_hidden; ++l) kgs = hidden[l] / 16 > kgs ? hidden[l] / 16 : kgs;
    return kgs;
}

// Launch geometry: RT row tiles per workgroup.  There is one step and the launch is latency-sized, so the smallest RT that
// brings the launch down to about min(row tiles, CUs) workgroups - every CU takes its rows in ONE round where the budgets allow -
// capped by the accumulators (TPW x RT <= 32) and the LDS image, as the scorer's RT is.  Any choice gives the same bits.  Plain
// integers, no context and no HIP call: launch() and l2a_value_model_geometry share it.  0 when no RT fits the LDS.
int choose_rt(int n_hidden, const int* hidden, int obs_dim, long long rows, int num_cu, int lds_per_block) {
    int tpw_max = 1;
    for (int l = 0; l < n_hidden; ++l) tpw_max = hidden[l] / 64 > tpw_max ? hidden[l] / 64 : tpw_max;
    const int kgs = vm_kgs(n_hidden, hidden, obs_dim);
    const int cus = num_cu > 0 ? num_cu : 256;
    const long long tiles = (rows + 15) / 16;
    int best = 0;
    for (int rt = 1; rt <= 8; rt <<= 1) {
        if (rt * tpw_max > L2A_RM_MAX_ACC) break;
        if ((long long)rt * kgs * 1024 + 4096 > lds_per_block) break;
        best = rt;
        if ((tiles + rt - 1) / rt <= cus) break;
    }
    return best;
}

// The function attribute is per (device, instance), not per model: raised ONCE to all the LDS a workgroup may take.
template <int RT>
int launch_rt(l2a_value_model* vm, const L2AVParams& p, unsigned blocks, hipStream_t stream) {
    static bool allowed[64] = {false};
    const size_t bytes = (size_t)RT * vm->kgs * 1024;
    const int dev = vm->ctx->device;
    if (bytes > 48 * 1024 && !(dev >= 0 && dev < 64 && allowed[dev])) {
        L2A_HIP(vm->ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_value_mlp_k<RT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, vm->ctx->lds_per_block - 4096));
        if (dev >= 0 && dev < 64) allowed[dev] = true;
    }
    hipLaunchKernelGGL(l2a_value_mlp_k<RT>, dim3(blocks), dim3(L2A_RM_THREADS), bytes, stream, p);
    L2A_HIP(vm->ctx, hipGetLastError());
    return L2A_OK;
}

int launch(l2a_value_model* vm, L2AVParams& p, hipStream_t stream) {
    p.wblk = vm->wblk;
    for (int l = 0; l <= vm->n_hidden; ++l) { p.pk[l] = vm->pk[l]; p.bias[l] = vm->bias[l]; }
    p.nm = vm->nm;
    for (int l = 0; l < L2A_RM_MAX_HIDDEN; ++l) p.tpw[l] = l < vm->n_hidden ? vm->hidden[l] / 64 : 0;
    p.n_hidden = vm->n_hidden; p.obs_dim = vm->obs_dim; p.KG0 = vm->KG0; p.kgs = vm->kgs;
    p.act = vm->act; p.sv = vm->sv; p.muv = vm->muv;
    const int rt = choose_rt(vm->n_hidden, vm->hidden, vm->obs_dim, p.rows, vm->ctx->num_cu, vm->ctx->lds_per_block);
    if (rt < 1) return l2a_fail(vm->ctx, L2A_EINVAL, "value model: no launch geometry fits the device's LDS");
    const unsigned blocks = (unsigned)(((long long)p.rows + 16 * rt - 1) / (16 * rt));
    switch (rt) {
        case 8: return launch_rt<8>(vm, p, blocks, stream);
        case 4: return launch_rt<4>(vm, p, blocks, stream);
        case 2: return launch_rt<2>(vm, p, blocks, stream);
        default: return launch_rt<1>(vm, p, blocks, stream);
    }
}

}  // namespace

extern "C" {

int l2a_value_model_check(int obs_dim, int n_hidden, const int* hidden, int hidden_act) {
    const std::string who = "value model: ";
    if (obs_dim < 1 || obs_dim > 16 * L2A_OTMAX)
        return l2a_fail(nullptr, L2A_EINVAL, who + "obs_dim " + std::to_string(obs_dim) + " (1 .. " + std::to_string(16 * L2A_OTMAX) + ")");
    if (n_hidden < 1 || n_hidden > L2A_RM_MAX_HIDDEN)
        return l2a_fail(nullptr, L2A_EINVAL, who + std::to_string(n_hidden) + " hidden layers (1 .. " + std::to_string(L2A_RM_MAX_HIDDEN) + ")");
    if (!hidden) return l2a_fail(nullptr, L2A_EINVAL, who + "null hidden sizes");
    for (int l = 0; l < n_hidden; ++l)
        if (hidden[l] < 64 || hidden[l] > 512 || hidden[l] % 64 != 0)
            return l2a_fail(nullptr, L2A_EINVAL, who + "hidden width " + std::to_string(hidden[l]) + " (a multiple of 64 up to 512)");
    if (hidden_act < L2A_ACT_IDENTITY || hidden_act > L2A_ACT_SWISH)
        return l2a_fail(nullptr, L2A_EINVAL, who + "unknown activation " + std::to_string(hidden_act));
    return L2A_OK;
}

int l2a_value_model_geometry(int obs_dim, int n_hidden, const int* hidden, long long rows, int num_cu, int lds_per_block, int* out) {
    if (!out || rows < 1) return L2A_EINVAL;
    const int rc = l2a_value_model_check(obs_dim, n_hidden, hidden, L2A_ACT_RELU);
    if (rc != L2A_OK) return rc;
    const int rt = choose_rt(n_hidden, hidden, obs_dim, rows, num_cu, lds_per_block);
    if (rt < 1)
        return l2a_fail(nullptr, L2A_EINVAL, "value model: no launch geometry fits " + std::to_string(lds_per_block) + " bytes of LDS");
    const long long wgs = (rows + 16 * rt - 1) / (16 * rt);
    if (wgs > 0x7fffffffLL) return l2a_fail(nullptr, L2A_EINVAL, "value model: too many rows");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = rt;
    out[1] = (int)wgs;
    out[2] = rt * vm_kgs(n_hidden, hidden, obs_dim) * 1024;
    return L2A_OK;
}

int l2a_value_model_create(l2a_ctx* ctx, int obs_dim, int n_hidden, const int* hidden, int hidden_act, l2a_value_model** out) {
    if (!ctx || !out) return L2A_EINVAL;
    const int rc = l2a_value_model_check(obs_dim, n_hidden, hidden, hidden_act);
    if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
    l2a_value_model* vm = new l2a_value_model();
    vm->ctx = ctx;
    vm->obs_dim = obs_dim; vm->KG0 = l2a_ceil_div(obs_dim, 16);
    vm->n_hidden = n_hidden; vm->act = hidden_act;
    vm->kgs = vm_kgs(n_hidden, hidden, obs_dim);
    long long off = 0;
    int kg = vm->KG0;
    for (int l = 0; l <= n_hidden; ++l) {
        const int n_out = l < n_hidden ? hidden[l] : 1;
        if (l < n_hidden) vm->hidden[l] = hidden[l];
        vm->pk[l] = off;
        off += (long long)l2a_ceil_div(n_out, 16) * kg * 256;
        vm->bias[l] = off;
        off += (n_out + 63) / 64 * 64;
        kg = n_out / 16;
    }
    vm->nm = off;
    off += 32 * vm->KG0;
    vm->blk_floats = off;
    l2a_device_guard guard(ctx->device);
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&vm->wblk), (size_t)off * sizeof(float));
    if (e != hipSuccess) {
        delete vm;
        return l2a_fail(ctx, L2A_EHIP, std::string("l2a_value_model_create: hipMalloc: ") + hipGetErrorString(e));
    }
    // identity statistics until l2a_value_model_set_norm is called (on the null stream, drained here)
    const int rc_n = l2a_value_model_set_norm(vm, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc_n == L2A_OK && hipStreamSynchronize(nullptr) == hipSuccess) { *out = vm; return L2A_OK; }
    l2a_value_model_destroy(vm);
    return rc_n != L2A_OK ? rc_n : l2a_fail(ctx, L2A_EHIP, "l2a_value_model_create: hipStreamSynchronize failed");
}

void l2a_value_model_destroy(l2a_value_model* vm) {
    if (!vm) return;
    l2a_device_guard guard(vm->ctx->device);
    if (vm->wblk) (void)hipFree(vm->wblk);
    delete vm;
}

int l2a_value_model_set_weights(l2a_value_model* vm, const void* const* device_ptrs, void* stream_v) {
    if (!vm) return L2A_EINVAL;
    l2a_ctx* ctx = vm->ctx;
    if (!device_ptrs) return l2a_fail(ctx, L2A_EINVAL, "l2a_value_model_set_weights: null pointer table");
    for (int i = 0; i < 2 * (vm->n_hidden + 1); ++i)
        if (!device_ptrs[i]) return l2a_fail(ctx, L2A_EINVAL, "l2a_value_model_set_weights: null parameter " + std::to_string(i));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    int k_in = vm->obs_dim, kg = vm->KG0;
    for (int l = 0; l <= vm->n_hidden; ++l) {
        const int n_out = l < vm->n_hidden ? vm->hidden[l] : 1;
        const long long total = (long long)l2a_ceil_div(n_out, 16) * kg * 256;
        hipLaunchKernelGGL(l2a_rm_pack_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                           static_cast<const float*>(device_ptrs[2 * l]), k_in, n_out, kg, total, vm->wblk + vm->pk[l]);
        L2A_HIP(ctx, hipGetLastError());
        L2A_HIP(ctx, hipMemcpyAsync(vm->wblk + vm->bias[l], device_ptrs[2 * l + 1], sizeof(float) * (size_t)n_out,
                                    hipMemcpyDeviceToDevice, stream));
        k_in = n_out;
        kg = n_out / 16;
    }
    vm->weights_set = true;
    return L2A_OK;
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
    // a previous async copy from the staging buffer must have drained before it is overwritten
    if (!vm->norm_stage.empty()) L2A_HIP(ctx, hipStreamSynchronize(stream));
    vm->norm_stage.assign((size_t)32 * vm->KG0, 0.0f);
    float* mu = vm->norm_stage.data();
    float* inv = mu + 16 * vm->KG0;
    const double eps = 1e-10;
    for (int k = 0; k < vm->obs_dim; ++k) {
        if (n_null) { mu[k] = 0.0f; inv[k] = 1.0f; continue; }
        mu[k] = (float)mean_obs[k];
        inv[k] = (float)(1.0 / (std_obs[k] + eps));
    }
    vm->muv = n_null ? 0.0f : (float)*mean_v;
    vm->sv = n_null ? 1.0f : (float)(*std_v + eps);
    L2A_HIP(ctx, hipMemcpyAsync(vm->wblk + vm->nm, mu, vm->norm_stage.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    return L2A_OK;
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
    if (obs_dim) *obs_dim = vm->obs_dim;
}

}  // extern "C"
