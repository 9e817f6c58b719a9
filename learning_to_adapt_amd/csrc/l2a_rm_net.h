// l2a_rm_net.h - the host side of the matrix-core MLP heads (reward model, terminal value, policy prior): the model core that
// l2a_reward_model, l2a_value_model and l2a_policy_model derive from, and the launcher of their kernels.  Defined in l2a_rm_net.hip;
// internal to libl2a_hip.so.  The public l2a_{reward,value,policy}_model_* entry points are thin wrappers in the heads' own units.
#pragma once

#include "l2a_host.h"
#include "l2a_rm_layer.h"

#include <vector>

// A head's network: d_in features -> n_hidden hidden layers -> n_out linear outputs (one 16-unit tile), and its device block
// [per layer: packed kernel | bias][mu 16 KG0][inv 16 KG0][norm_tail floats of the head's own statistics].
struct l2a_rm_core {
    l2a_ctx* ctx = nullptr;
    int d_in = 0, n_out = 0, KG0 = 0, kgs = 0;
    int n_hidden = 0, hidden[L2A_RM_MAX_HIDDEN] = {0}, act = L2A_ACT_RELU;
    float* wblk = nullptr;
    long long blk_floats = 0;
    long long pk[L2A_RM_MAX_HIDDEN + 1] = {0}, bias[L2A_RM_MAX_HIDDEN + 1] = {0}, nm = 0;
    int norm_tail = 0;
    bool weights_set = false;
    std::vector<float> norm_stage;              // host staging, kept alive for the async H2D
};

// k-groups between the row tiles of the LDS image: the widest layer's input or output
L2A_HIDDEN int l2a_rm_kgs(int n_hidden, const int* hidden, int d_in);
// Host-only eligibility check behind the three *_model_check: `who` prefixes the message; `act_dim` is null for a head without
// actions, else it must be 1 .. 16 and `act_range` is the text between the message's brackets.
L2A_HIDDEN int l2a_rm_check(const char* who, int obs_dim, const int* act_dim, const char* act_range, int n_hidden, const int* hidden,
                            int hidden_act);
// Launch geometry of the one-step heads (value, policy): RT row tiles per workgroup.  The launch is latency-sized, so the
// smallest RT that brings it down to about min(row tiles, CUs) workgroups - every CU takes its rows in ONE round where the
// budgets allow - capped by the accumulators (TPW x RT <= 32) and the LDS image.  Any choice gives the same bits.  Plain integers,
// no context and no HIP call.  0 when no RT fits the LDS.
L2A_HIDDEN int l2a_rm_choose_rt(int n_hidden, const int* hidden, int d_in, long long rows, int num_cu, int lds_per_block);
// Behind l2a_{value,policy}_model_geometry (arguments checked by the caller): out[0 .. 7] = RT, workgroups, LDS bytes, zeros
L2A_HIDDEN int l2a_rm_rt_geometry(const char* who, int n_hidden, const int* hidden, int d_in, long long rows, int num_cu,
                                  int lds_per_block, int* out);
// Lays the block out, allocates and clears it (null stream; the caller holds the device guard and drains).  `entry` names the
// public entry point in the messages.  On failure the core is left for l2a_rm_core_free.
L2A_HIDDEN int l2a_rm_core_create(l2a_rm_core* c, l2a_ctx* ctx, const char* entry, int d_in, int n_out, int n_hidden, const int* hidden,
                                  int hidden_act, int norm_tail);
L2A_HIDDEN void l2a_rm_core_free(l2a_rm_core* c);       // the device block; the caller deletes the object
// [W0, b0, ..., Wout, bout] device pointers, kernels [in, out]: packs them into the block on `stream`
L2A_HIDDEN int l2a_rm_core_set_weights(l2a_rm_core* c, const char* entry, const void* const* device_ptrs, void* stream);
// set_norm in two halves around the head's own fill: _stage drains a previous upload from the staging buffer and hands it out
// zeroed (mu = stage, inv = stage + 16 KG0, tail = stage + 32 KG0); _upload copies it behind the weights on `stream`.
L2A_HIDDEN int l2a_rm_core_norm_stage(l2a_rm_core* c, hipStream_t stream, float** stage);
L2A_HIDDEN int l2a_rm_core_norm_upload(l2a_rm_core* c, hipStream_t stream);
L2A_HIDDEN void l2a_rm_core_net(const l2a_rm_core* c, L2ARmNet* net);

// One launch of a head's kernel instance K on RT row tiles (P: its parameter struct).  The function attribute is per (device,
// instance), not per model: it is raised ONCE to all the LDS a workgroup may take, so that models of different widths do not
// lower it under each other - `allowed` is one flag per instantiation, i.e. per kernel instance.
template <typename P, void (*K)(P)>
L2A_HIDDEN int l2a_rm_launch(const l2a_rm_core* c, int RT, const P& p, unsigned blocks, hipStream_t stream) {
    static bool allowed[64] = {false};
    const size_t bytes = (size_t)RT * c->kgs * 1024;
    const int dev = c->ctx->device;
    if (bytes > 48 * 1024 && !(dev >= 0 && dev < 64 && allowed[dev])) {
        L2A_HIP(c->ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            c->ctx->lds_per_block - 4096));
        if (dev >= 0 && dev < 64) allowed[dev] = true;
    }
    hipLaunchKernelGGL(K, dim3(blocks), dim3(L2A_RM_THREADS), bytes, stream, p);
    L2A_HIP(c->ctx, hipGetLastError());
    return L2A_OK;
}
// The four instances of a head's kernel template KERNEL<RT>, by the chosen rt
#define L2A_RM_LAUNCH_RT(KERNEL, P, c, rt, p, blocks, stream)                                     \
    ((rt) == 8   ? l2a_rm_launch<P, KERNEL<8>>((c), 8, (p), (blocks), (stream))                   \
     : (rt) == 4 ? l2a_rm_launch<P, KERNEL<4>>((c), 4, (p), (blocks), (stream))                   \
     : (rt) == 2 ? l2a_rm_launch<P, KERNEL<2>>((c), 2, (p), (blocks), (stream))                   \
                 : l2a_rm_launch<P, KERNEL<1>>((c), 1, (p), (blocks), (stream)))
