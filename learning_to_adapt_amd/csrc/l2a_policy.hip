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
// z is given, or the Philox4x32-10 + Box-Muller normal of l2a_cem.hip / l2a_mppi.hip (restated below; those files keep their own).
//
// Kernel.  l2a_value_mlp_k's frame (l2a_rm_layer.h): 4 waves, RT row tiles of 16 rows, one LDS image [row tile][k-group][lane] of
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
#include "l2a_rm_layer.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#define L2A_PM_OSTRIDE 20           // words between the rows of the transposed output tile

struct L2APParams {
    const float* wblk;              // the model's device block
    long long pk[L2A_RM_MAX_HIDDEN + 1];    // packed kernels (floats from wblk); [n_hidden] = the output layer
    long long bias[L2A_RM_MAX_HIDDEN + 1];  // biases
    long long nm;                   // [mu KG0*16][inv KG0*16][sd_a 16][mu_a 16]
    int tpw[L2A_RM_MAX_HIDDEN];     // hidden width / 64
    int n_hidden, obs_dim, act_dim, KG0, kgs;       // kgs: k-groups between the row tiles of the LDS image
    int act;
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

// ---- Philox4x32-10 + Box-Muller: l2a_cem.hip's normal stream restated (l2a_cem.hip and l2a_mppi.hip keep their own copies; the
//      three must stay the same function of (seed, index): tests/test_policy_model_gpu.py holds this one to l2a_mppi_sample) ------
__device__ __forceinline__ void pm_philox_round(unsigned int (&c)[4], unsigned int k0, unsigned int k1) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned int hi0 = (unsigned int)(p0 >> 32), lo0 = (unsigned int)p0;
    const unsigned int hi1 = (unsigned int)(p1 >> 32), lo1 = (unsigned int)p1;
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
}

__device__ __forceinline__ float pm_philox_normal(unsigned long long seed, unsigned long long index) {
    unsigned int c[4] = {(unsigned int)index, (unsigned int)(index >> 32), 0x4c32614du, 0u};
    unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        pm_philox_round(c, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    // Box-Muller on two uniforms in (0, 1]
    const float u1 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

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
    const float* __restrict__ mu = p.wblk + p.nm;
    const float* __restrict__ inv = mu + 16 * p.KG0;
    const float* __restrict__ sda = inv + 16 * p.KG0;
    const float* __restrict__ mua = sda + 16;
    const int kpad = 16 * p.KG0;
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
        if (i < nr && k < p.obs_dim) {
            const int srow = p.state_per_row ? r0 + i : (r0 + i) / p.npl;
            const float v = p.states[(size_t)srow * p.obs_dim + k];
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
    // ---- the output tile: row tiles dealt to the waves; unit 4 (lane >> 4) + c of row lane & 15 = register c ----
    f32x4 yo[(RT + 3) / 4];
    {
        const f32x4* wo = reinterpret_cast<const f32x4*>(p.wblk + p.pk[p.n_hidden]) + lane;
        const f32x4 bo = *reinterpret_cast<const f32x4*>(p.wblk + p.bias[p.n_hidden] + 4 * (lane >> 4));
#pragma unroll
        for (int q = 0; q < (RT + 3) / 4; ++q) {
            const int rt = wave + 4 * q;
            f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (rt < RT && ((live >> rt) & 1u)) {
                for (int g = 0; g < KGin; ++g) {
                    const f32x4 a = wo[g * 64];
                    const f32x4 b = act[(rt * p.kgs + g) * 64 + lane];
                    acc = L2A_MFMA(a.x, b.x, acc);
                    acc = L2A_MFMA(a.y, b.y, acc);
                    acc = L2A_MFMA(a.z, b.z, acc);
                    acc = L2A_MFMA(a.w, b.w, acc);
                }
            }
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
            const float z = p.z ? p.z[ze] : pm_philox_normal(p.seed, p.offset + ze);
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

struct l2a_policy_model {
    l2a_ctx* ctx = nullptr;
    int obs_dim = 0, act_dim = 0, KG0 = 0, kgs = 0;
    int n_hidden = 0, hidden[L2A_RM_MAX_HIDDEN] = {0}, act = L2A_ACT_RELU;
    float* wblk = nullptr;
    long long blk_floats = 0;
    long long pk[L2A_RM_MAX_HIDDEN + 1] = {0}, bias[L2A_RM_MAX_HIDDEN + 1] = {0}, nm = 0;
    bool weights_set = false;
    std::vector<float> norm_stage;              // host staging, kept alive for the async H2D
};

namespace {

int pm_kgs(int n_hidden, const int* hidden, int obs_dim) {
    int kgs = l2a_ceil_div(obs_dim, 16);
    for (int l = 0; l < n_hidden; ++l) kgs = hidden[l] / 16 > kgs ? hidden[l] / 16 : kgs;
    return kgs;
}

// Launch geometry: l2a_value.hip's rule on the same caps - the smallest RT that brings the launch down to about
// min(row tiles, CUs) workgroups, capped by the accumulators (TPW x RT <= 32) and the LDS image.  Any choice gives the same bits.  0 when no RT fits the LDS.
int choose_rt(int n_hidden, const int* hidden, int obs_dim, long long rows, int num_cu, int lds_per_block) {
    int tpw_max = 1;
    for (int l = 0; l < n_hidden; ++l) tpw_max = hidden[l] / 64 > tpw_max ? hidden[l] / 64 : tpw_max;
    const int kgs = pm_kgs(n_hidden, hidden, obs_dim);
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
int launch_rt(l2a_policy_model* pm, const L2APParams& p, unsigned blocks, hipStream_t stream) {
    static bool allowed[64] = {false};
    const size_t bytes = (size_t)RT * pm->kgs * 1024;
    const int dev = pm->ctx->device;
    if (bytes > 48 * 1024 && !(dev >= 0 && dev < 64 && allowed[dev])) {
        L2A_HIP(pm->ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_policy_mlp_k<RT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, pm->ctx->lds_per_block - 4096));
        if (dev >= 0 && dev < 64) allowed[dev] = true;
    }
    hipLaunchKernelGGL(l2a_policy_mlp_k<RT>, dim3(blocks), dim3(L2A_RM_THREADS), bytes, stream, p);
    L2A_HIP(pm->ctx, hipGetLastError());
    return L2A_OK;
}

int launch(l2a_policy_model* pm, L2APParams& p, hipStream_t stream) {
    p.wblk = pm->wblk;
    for (int l = 0; l <= pm->n_hidden; ++l) { p.pk[l] = pm->pk[l]; p.bias[l] = pm->bias[l]; }
    p.nm = pm->nm;
    for (int l = 0; l < L2A_RM_MAX_HIDDEN; ++l) p.tpw[l] = l < pm->n_hidden ? pm->hidden[l] / 64 : 0;
    p.n_hidden = pm->n_hidden; p.obs_dim = pm->obs_dim; p.act_dim = pm->act_dim; p.KG0 = pm->KG0; p.kgs = pm->kgs;
    p.act = pm->act;
    const int rt = choose_rt(pm->n_hidden, pm->hidden, pm->obs_dim, p.rows, pm->ctx->num_cu, pm->ctx->lds_per_block);
    if (rt < 1) return l2a_fail(pm->ctx, L2A_EINVAL, "policy model: no launch geometry fits the device's LDS");
    const unsigned blocks = (unsigned)(((long long)p.rows + 16 * rt - 1) / (16 * rt));
    switch (rt) {
        case 8: return launch_rt<8>(pm, p, blocks, stream);
        case 4: return launch_rt<4>(pm, p, blocks, stream);
        case 2: return launch_rt<2>(pm, p, blocks, stream);
        default: return launch_rt<1>(pm, p, blocks, stream);
    }
}

}  // namespace

extern "C" {

int l2a_policy_model_check(int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act) {
    const std::string who = "policy model: ";
    if (obs_dim < 1 || obs_dim > 16 * L2A_OTMAX)
        return l2a_fail(nullptr, L2A_EINVAL, who + "obs_dim " + std::to_string(obs_dim) + " (1 .. " + std::to_string(16 * L2A_OTMAX) + ")");
    if (act_dim < 1 || act_dim > 16)
        return l2a_fail(nullptr, L2A_EINVAL, who + "act_dim " + std::to_string(act_dim) + " (1 .. 16: one output tile)");
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

int l2a_policy_model_geometry(int obs_dim, int act_dim, int n_hidden, const int* hidden, long long rows, int num_cu, int lds_per_block,
                              int* out) {
    if (!out || rows < 1) return L2A_EINVAL;
    const int rc = l2a_policy_model_check(obs_dim, act_dim, n_hidden, hidden, L2A_ACT_RELU);
    if (rc != L2A_OK) return rc;
    const int rt = choose_rt(n_hidden, hidden, obs_dim, rows, num_cu, lds_per_block);
    if (rt < 1)
        return l2a_fail(nullptr, L2A_EINVAL, "policy model: no launch geometry fits " + std::to_string(lds_per_block) + " bytes of LDS");
    const long long wgs = (rows + 16 * rt - 1) / (16 * rt);
    if (wgs > 0x7fffffffLL) return l2a_fail(nullptr, L2A_EINVAL, "policy model: too many rows");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = rt;
    out[1] = (int)wgs;
    out[2] = rt * pm_kgs(n_hidden, hidden, obs_dim) * 1024;
    return L2A_OK;
}

int l2a_policy_model_create(l2a_ctx* ctx, int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act,
                            l2a_policy_model** out) {
    if (!ctx || !out) return L2A_EINVAL;
    const int rc = l2a_policy_model_check(obs_dim, act_dim, n_hidden, hidden, hidden_act);
    if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
    l2a_policy_model* pm = new l2a_policy_model();
    pm->ctx = ctx;
    pm->obs_dim = obs_dim; pm->act_dim = act_dim; pm->KG0 = l2a_ceil_div(obs_dim, 16);
    pm->n_hidden = n_hidden; pm->act = hidden_act;
    pm->kgs = pm_kgs(n_hidden, hidden, obs_dim);
    long long off = 0;
    int kg = pm->KG0;
    for (int l = 0; l <= n_hidden; ++l) {
        const int n_out = l < n_hidden ? hidden[l] : act_dim;
        if (l < n_hidden) pm->hidden[l] = hidden[l];
        pm->pk[l] = off;
        off += (long long)l2a_ceil_div(n_out, 16) * kg * 256;
        pm->bias[l] = off;
        off += (n_out + 63) / 64 * 64;
        kg = n_out / 16;
    }
    pm->nm = off;
    off += 32 * pm->KG0 + 32;
    pm->blk_floats = off;
    l2a_device_guard guard(ctx->device);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&pm->wblk), (size_t)off * sizeof(float));
    if (e != hipSuccess) {
        delete pm;
        return l2a_fail(ctx, L2A_EHIP, std::string("l2a_policy_model_create: hipMalloc: ") + hipGetErrorString(e));
    }
    // (the output bias is read as a whole 16-unit tile: the words behind act_dim must be zeros, not what the allocation held)
    e = hipMemsetAsync(pm->wblk, 0, (size_t)off * sizeof(float), nullptr);
    // identity statistics until l2a_policy_model_set_norm is called (on the null stream, drained here)
    const int rc_n = e == hipSuccess ? l2a_policy_model_set_norm(pm, nullptr, nullptr, nullptr, nullptr, nullptr) : L2A_EHIP;
    if (rc_n == L2A_OK && hipStreamSynchronize(nullptr) == hipSuccess) { *out = pm; return L2A_OK; }
    l2a_policy_model_destroy(pm);
    return (rc_n != L2A_OK && e == hipSuccess) ? rc_n : l2a_fail(ctx, L2A_EHIP, "l2a_policy_model_create: clearing the weight block failed");
}

void l2a_policy_model_destroy(l2a_policy_model* pm) {
    if (!pm) return;
    l2a_device_guard guard(pm->ctx->device);
    if (pm->wblk) (void)hipFree(pm->wblk);
    delete pm;
}

int l2a_policy_model_set_weights(l2a_policy_model* pm, const void* const* device_ptrs, void* stream_v) {
    if (!pm) return L2A_EINVAL;
    l2a_ctx* ctx = pm->ctx;
    if (!device_ptrs) return l2a_fail(ctx, L2A_EINVAL, "l2a_policy_model_set_weights: null pointer table");
    for (int i = 0; i < 2 * (pm->n_hidden + 1); ++i)
        if (!device_ptrs[i]) return l2a_fail(ctx, L2A_EINVAL, "l2a_policy_model_set_weights: null parameter " + std::to_string(i));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    int k_in = pm->obs_dim, kg = pm->KG0;
    for (int l = 0; l <= pm->n_hidden; ++l) {
        const int n_out = l < pm->n_hidden ? pm->hidden[l] : pm->act_dim;
        const long long total = (long long)l2a_ceil_div(n_out, 16) * kg * 256;
        hipLaunchKernelGGL(l2a_rm_pack_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                           static_cast<const float*>(device_ptrs[2 * l]), k_in, n_out, kg, total, pm->wblk + pm->pk[l]);
        L2A_HIP(ctx, hipGetLastError());
        L2A_HIP(ctx, hipMemcpyAsync(pm->wblk + pm->bias[l], device_ptrs[2 * l + 1], sizeof(float) * (size_t)n_out,
                                    hipMemcpyDeviceToDevice, stream));
        k_in = n_out;
        kg = n_out / 16;
    }
    pm->weights_set = true;
    return L2A_OK;
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
    // a previous async copy from the staging buffer must have drained before it is overwritten
    if (!pm->norm_stage.empty()) L2A_HIP(ctx, hipStreamSynchronize(stream));
    pm->norm_stage.assign((size_t)32 * pm->KG0 + 32, 0.0f);
    float* mu = pm->norm_stage.data();
    float* inv = mu + 16 * pm->KG0;
    float* sda = inv + 16 * pm->KG0;
    float* mua = sda + 16;
    const double eps = 1e-10;
    for (int k = 0; k < pm->obs_dim; ++k) {
        if (n_null) { mu[k] = 0.0f; inv[k] = 1.0f; continue; }
        mu[k] = (float)mean_obs[k];
        inv[k] = (float)(1.0 / (std_obs[k] + eps));
    }
    for (int k = 0; k < pm->act_dim; ++k) {
        sda[k] = n_null ? 1.0f : (float)(std_act[k] + eps);
        mua[k] = n_null ? 0.0f : (float)mean_act[k];
    }
    L2A_HIP(ctx, hipMemcpyAsync(pm->wblk + pm->nm, mu, pm->norm_stage.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    return L2A_OK;
}

void l2a_policy_model_facts(const l2a_policy_model* pm, l2a_ctx** ctx, int* obs_dim, int* act_dim) {
    if (ctx) *ctx = pm->ctx;
    if (obs_dim) *obs_dim = pm->obs_dim;
    if (act_dim) *act_dim = pm->act_dim;
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
