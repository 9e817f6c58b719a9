// l2a_rm_layer.h - the device side of the matrix-core MLP heads: the learned reward model (l2a_score_mlp.hip), the terminal value
// (l2a_value.hip) and the policy prior (l2a_policy.hip).  The network descriptor the three kernels take, the place of an input
// feature in the LDS image, one hidden layer in place in the image with its dispatch on the layer's width and its activation pass, and the
// output tile's accumulator chain.  Each kernel keeps its own prologue (what the features are) and its own consumer of the output
// tile.  The three units are compiled with contraction off and include this header below their `#pragma clang fp contract(off)`.
// The host side of the heads - the model object, its weight block and the launcher - is l2a_rm_net.h / l2a_rm_net.hip.
#pragma once

#include "l2a_kernels.h"

#define L2A_RM_THREADS 256
#define L2A_RM_MAX_HIDDEN 3
#define L2A_RM_MAX_ROWS 128         // 16 * RT, RT <= 8
#define L2A_RM_MAX_ACC 32           // TPW * RT accumulators of four registers per wave

// The network as a kernel sees it (filled by l2a_rm_core_net, l2a_rm_net.hip): plain data, a member of the kernel's parameters.
struct L2ARmNet {
    const float* wblk;              // the model's device block
    long long pk[L2A_RM_MAX_HIDDEN + 1];    // packed kernels (floats from wblk); [n_hidden] = the output layer
    long long bias[L2A_RM_MAX_HIDDEN + 1];  // biases
    long long nm;                   // [mu KG0*16][inv KG0*16] in feature order, then the head's own tail
    int tpw[L2A_RM_MAX_HIDDEN];     // hidden width / 64
    int n_hidden, d_in, KG0, kgs;   // d_in input features in KG0 k-groups; kgs: k-groups between the row tiles of the LDS image
    int act;
};

// Float index of feature k of row j (0 .. 15) of row tile rt in the image [row tile][k-group][lane] of f32x4: the B fragment
__device__ __forceinline__ int l2a_rm_image_index(int rt, int kgs, int k, int j) {
    return (((rt * kgs + (k >> 4)) * 64) + ((k >> 2) & 3) * 16 + j) * 4 + (k & 3);
}

// One hidden layer for the pass's RT row tiles, in place: this wave's TPW unit tiles.  `live`: bit rt = row tile rt holds rows.
// The epilogue applies max(x, floor) - relu (0) or nothing (-inf; the max propagates NaN, l2a_max_nan) - and the other
// activations follow in a pass of their own over the image (l2a_rm_hidden_layer): inlined into every instance here their code
// cost registers (spills at RT = 4) and a minute of compile time.
template <int TPW, int RT>
__device__ __forceinline__ void l2a_rm_layer(const f32x4* __restrict__ wp, const float* __restrict__ bias, int KGin, int kgs,
                                             f32x4* act, float floor, unsigned live, int wave, int lane) {
    if constexpr (TPW * RT <= L2A_RM_MAX_ACC) {
        f32x4 acc[TPW][RT];
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[tp][rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const int c0 = wave * TPW;
        const f32x4* wl = wp + (long long)c0 * KGin * 64 + lane;
        f32x4 a[TPW], an[TPW];
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp) a[tp] = wl[(long long)tp * KGin * 64];
#pragma unroll 1
        for (int g = 0; g < KGin; ++g) {
            const int gn = (g + 1 < KGin) ? g + 1 : g;
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp) an[tp] = wl[((long long)tp * KGin + gn) * 64];
            // (row tiles without rows are computed too - branch-free MFMA stream; only their stores are skipped)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const f32x4 b = act[(rt * kgs + g) * 64 + lane];
#pragma unroll
                for (int tp = 0; tp < TPW; ++tp) acc[tp][rt] = L2A_MFMA(a[tp].x, b.x, acc[tp][rt]);
#pragma unroll
                for (int tp = 0; tp < TPW; ++tp) acc[tp][rt] = L2A_MFMA(a[tp].y, b.y, acc[tp][rt]);
#pragma unroll
                for (int tp = 0; tp < TPW; ++tp) acc[tp][rt] = L2A_MFMA(a[tp].z, b.z, acc[tp][rt]);
#pragma unroll
                for (int tp = 0; tp < TPW; ++tp) acc[tp][rt] = L2A_MFMA(a[tp].w, b.w, acc[tp][rt]);
            }
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp) a[tp] = an[tp];
        }
        __syncthreads();        // every wave has read the layer's input: the image may be overwritten
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 16 * (c0 + tp) + 4 * (lane >> 4));
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
                if ((live >> rt) & 1u) {
                    f32x4 v = acc[tp][rt] + bv;
                    v.x = l2a_max_nan(v.x, floor); v.y = l2a_max_nan(v.y, floor);
                    v.z = l2a_max_nan(v.z, floor); v.w = l2a_max_nan(v.w, floor);
                    act[(rt * kgs + c0 + tp) * 64 + lane] = v;
                }
        }
        __syncthreads();
    }
}

template <int RT>
__device__ __forceinline__ void l2a_rm_layer_any(int tpw, const f32x4* wp, const float* bias, int KGin, int kgs, f32x4* act,
                                                 float floor, unsigned live, int wave, int lane) {
    switch (tpw) {
        case 1: l2a_rm_layer<1, RT>(wp, bias, KGin, kgs, act, floor, live, wave, lane); break;
        case 2: l2a_rm_layer<2, RT>(wp, bias, KGin, kgs, act, floor, live, wave, lane); break;
        case 3: l2a_rm_layer<3, RT>(wp, bias, KGin, kgs, act, floor, live, wave, lane); break;
        case 4: l2a_rm_layer<4, RT>(wp, bias, KGin, kgs, act, floor, live, wave, lane); break;
        case 5: l2a_rm_layer<5, RT>(wp, bias, KGin, kgs, act, floor, live, wave, lane); break;
        case 6: l2a_rm_layer<6, RT>(wp, bias, KGin, kgs, act, floor, live, wave, lane); break;
        case 7: l2a_rm_layer<7, RT>(wp, bias, KGin, kgs, act, floor, live, wave, lane); break;
        default: l2a_rm_layer<8, RT>(wp, bias, KGin, kgs, act, floor, live, wave, lane); break;
    }
}

// Hidden layer l, in place, with its elementwise activation pass: the image holds the layer's input in KGin k-groups on entry
// (every thread's stores made visible by a barrier) and its activations on return.  Returns the next layer's KGin.  The kernels
// keep the loop over l themselves: with the loop inside a shared routine the register allocator schedules the widest
// instances' MFMA loops differently from the loop written out in the kernel (one LDS read in flight instead of eight).
template <int RT>
__device__ __forceinline__ int l2a_rm_hidden_layer(const L2ARmNet& net, int l, int KGin, f32x4* act, unsigned live, int tid, int wave,
                                                   int lane) {
    const float floor = (net.act == L2A_ACT_RELU) ? 0.0f : -__builtin_inff();
    l2a_rm_layer_any<RT>(net.tpw[l], reinterpret_cast<const f32x4*>(net.wblk + net.pk[l]), net.wblk + net.bias[l], KGin, net.kgs,
                         act, floor, live, wave, lane);
    KGin = 4 * net.tpw[l];
    if (net.act != L2A_ACT_RELU && net.act != L2A_ACT_IDENTITY) {       // tanh / sigmoid / swish: elementwise over the live tiles
        for (int e = tid; e < RT * KGin * 64; e += L2A_RM_THREADS) {
            const int rt = e / (KGin * 64);
            if ((live >> rt) & 1u) {
                f32x4* q = act + (rt * net.kgs) * 64 + (e - rt * KGin * 64);
                f32x4 v = *q;
                v.x = l2a_act1(v.x, net.act); v.y = l2a_act1(v.y, net.act); v.z = l2a_act1(v.z, net.act); v.w = l2a_act1(v.w, net.act);
                *q = v;
            }
        }
        __syncthreads();
    }
    return KGin;
}

// The output layer's ONE 16-unit tile for row tile rt, without the bias: the single accumulator chain over k.  Unit 4 (lane >> 4)
// + c of row lane & 15 is register c - a scalar head's unit 0 is .x of lanes 0 .. 15.  The kernels deal the row tiles to the waves.
__device__ __forceinline__ f32x4 l2a_rm_out_chain(const L2ARmNet& net, const f32x4* act, int rt, int KGin, int lane) {
    const f32x4* wo = reinterpret_cast<const f32x4*>(net.wblk + net.pk[net.n_hidden]) + lane;
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int g = 0; g < KGin; ++g) {
        const f32x4 a = wo[g * 64];
        const f32x4 b = act[(rt * net.kgs + g) * 64 + lane];
        acc = L2A_MFMA(a.x, b.x, acc);
        acc = L2A_MFMA(a.y, b.y, acc);
        acc = L2A_MFMA(a.z, b.z, acc);
        acc = L2A_MFMA(a.w, b.w, acc);
    }
    return acc;
}
