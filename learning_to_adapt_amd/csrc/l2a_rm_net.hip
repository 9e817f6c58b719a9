// l2a_rm_net.hip - the model core of the matrix-core MLP heads (l2a_rm_net.h): eligibility check, block layout, weight packing,
// the upload of the normalisation statistics, the kernels' network descriptor and the one-step heads' launch geometry.  The
// heads' kernels and public entry points are in l2a_score_mlp.hip, l2a_value.hip and l2a_policy.hip.
#pragma clang fp contract(off)

#include "l2a_rm_net.h"

#include <string>

// A layer's kernel [k_in, n_out] into the A fragments of the MFMA (l2a_kernels.h), zeros in the padding
static __global__ void l2a_rm_pack_k(const float* __restrict__ w, int k_in, int n_out, int KG, long long total, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    int k, u;
    l2a_pack_decode(idx, KG, &k, &u);
    out[idx] = (k < k_in && u < n_out) ? w[(long long)k * n_out + u] : 0.0f;
}

int l2a_rm_kgs(int n_hidden, const int* hidden, int d_in) {
    int kgs = l2a_ceil_div(d_in, 16);
    for (int l = 0; l < n_hidden; ++l) kgs = hidden[l] / 16 > kgs ? hidden[l] / 16 : kgs;
    return kgs;
}

int l2a_rm_check(const char* who_c, int obs_dim, const int* act_dim, const char* act_range, int n_hidden, const int* hidden,
                 int hidden_act) {
    const std::string who = who_c;
    if (obs_dim < 1 || obs_dim > 16 * L2A_OTMAX)
        return l2a_fail(nullptr, L2A_EINVAL, who + "obs_dim " + std::to_string(obs_dim) + " (1 .. " + std::to_string(16 * L2A_OTMAX) + ")");
    if (act_dim && (*act_dim < 1 || *act_dim > 16))
        return l2a_fail(nullptr, L2A_EINVAL, who + "act_dim " + std::to_string(*act_dim) + " (" + act_range + ")");
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

int l2a_rm_choose_rt(int n_hidden, const int* hidden, int d_in, long long rows, int num_cu, int lds_per_block) {
    int tpw_max = 1;
    for (int l = 0; l < n_hidden; ++l) tpw_max = hidden[l] / 64 > tpw_max ? hidden[l] / 64 : tpw_max;
    const int kgs = l2a_rm_kgs(n_hidden, hidden, d_in);
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

int l2a_rm_rt_geometry(const char* who_c, int n_hidden, const int* hidden, int d_in, long long rows, int num_cu, int lds_per_block,
                       int* out) {
    const std::string who = who_c;
    const int rt = l2a_rm_choose_rt(n_hidden, hidden, d_in, rows, num_cu, lds_per_block);
    if (rt < 1) return l2a_fail(nullptr, L2A_EINVAL, who + "no launch geometry fits " + std::to_string(lds_per_block) + " bytes of LDS");
    const long long wgs = (rows + 16 * rt - 1) / (16 * rt);
    if (wgs > 0x7fffffffLL) return l2a_fail(nullptr, L2A_EINVAL, who + "too many rows");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = rt;
    out[1] = (int)wgs;
    out[2] = rt * l2a_rm_kgs(n_hidden, hidden, d_in) * 1024;
    return L2A_OK;
}

int l2a_rm_core_create(l2a_rm_core* c, l2a_ctx* ctx, const char* entry, int d_in, int n_out_last, int n_hidden, const int* hidden,
                       int hidden_act, int norm_tail) {
    c->ctx = ctx;
    c->d_in = d_in; c->n_out = n_out_last; c->KG0 = l2a_ceil_div(d_in, 16);
    c->n_hidden = n_hidden; c->act = hidden_act;
    c->kgs = l2a_rm_kgs(n_hidden, hidden, d_in);
    long long off = 0;
    int kg = c->KG0;
    for (int l = 0; l <= n_hidden; ++l) {
        const int n_out = l < n_hidden ? hidden[l] : n_out_last;
        if (l < n_hidden) c->hidden[l] = hidden[l];
        c->pk[l] = off;
        off += (long long)l2a_ceil_div(n_out, 16) * kg * 256;
        c->bias[l] = off;
        off += (n_out + 63) / 64 * 64;
        kg = n_out / 16;
    }
    c->nm = off;
    c->norm_tail = norm_tail;
    off += 32 * c->KG0 + norm_tail;
    c->blk_floats = off;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->wblk), (size_t)off * sizeof(float));
    if (e != hipSuccess) {
        c->wblk = nullptr;
        return l2a_fail(ctx, L2A_EHIP, std::string(entry) + ": hipMalloc: " + hipGetErrorString(e));
    }
    // (an output bias is read as a whole 16-unit tile: the words behind n_out must be zeros, not what the allocation held)
    e = hipMemsetAsync(c->wblk, 0, (size_t)off * sizeof(float), nullptr);
    if (e != hipSuccess) return l2a_fail(ctx, L2A_EHIP, std::string(entry) + ": clearing the weight block failed");
    return L2A_OK;
}

void l2a_rm_core_free(l2a_rm_core* c) {
    l2a_device_guard guard(c->ctx->device);
    if (c->wblk) (void)hipFree(c->wblk);
    c->wblk = nullptr;
}

int l2a_rm_core_set_weights(l2a_rm_core* c, const char* entry_c, const void* const* device_ptrs, void* stream_v) {
    if (!c) return L2A_EINVAL;
    l2a_ctx* ctx = c->ctx;
    const std::string entry = entry_c;
    if (!device_ptrs) return l2a_fail(ctx, L2A_EINVAL, entry + ": null pointer table");
    for (int i = 0; i < 2 * (c->n_hidden + 1); ++i)
        if (!device_ptrs[i]) return l2a_fail(ctx, L2A_EINVAL, entry + ": null parameter " + std::to_string(i));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    int k_in = c->d_in, kg = c->KG0;
    for (int l = 0; l <= c->n_hidden; ++l) {
        const int n_out = l < c->n_hidden ? c->hidden[l] : c->n_out;
        const long long total = (long long)l2a_ceil_div(n_out, 16) * kg * 256;
        hipLaunchKernelGGL(l2a_rm_pack_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                           static_cast<const float*>(device_ptrs[2 * l]), k_in, n_out, kg, total, c->wblk + c->pk[l]);
        L2A_HIP(ctx, hipGetLastError());
        L2A_HIP(ctx, hipMemcpyAsync(c->wblk + c->bias[l], device_ptrs[2 * l + 1], sizeof(float) * (size_t)n_out,
                                    hipMemcpyDeviceToDevice, stream));
        k_in = n_out;
        kg = n_out / 16;
    }
    c->weights_set = true;
    return L2A_OK;
}

int l2a_rm_core_norm_stage(l2a_rm_core* c, hipStream_t stream, float** stage) {
    // a previous async copy from the staging buffer must have drained before it is overwritten
    if (!c->norm_stage.empty()) L2A_HIP(c->ctx, hipStreamSynchronize(stream));
    c->norm_stage.assign((size_t)32 * c->KG0 + c->norm_tail, 0.0f);
    *stage = c->norm_stage.data();
    return L2A_OK;
}

int l2a_rm_core_norm_upload(l2a_rm_core* c, hipStream_t stream) {
    L2A_HIP(c->ctx, hipMemcpyAsync(c->wblk + c->nm, c->norm_stage.data(), c->norm_stage.size() * sizeof(float), hipMemcpyHostToDevice,
                                   stream));
    return L2A_OK;
}

void l2a_rm_core_net(const l2a_rm_core* c, L2ARmNet* net) {
    net->wblk = c->wblk;
    for (int l = 0; l <= L2A_RM_MAX_HIDDEN; ++l) { net->pk[l] = c->pk[l]; net->bias[l] = c->bias[l]; }
    net->nm = c->nm;
    for (int l = 0; l < L2A_RM_MAX_HIDDEN; ++l) net->tpw[l] = l < c->n_hidden ? c->hidden[l] / 64 : 0;
    net->n_hidden = c->n_hidden; net->d_in = c->d_in; net->KG0 = c->KG0; net->kgs = c->kgs;
    net->act = c->act;
}
