// l2a_rm_layer.h - the layer routine of the matrix-core MLP scorers, shared by the reward-model scorer (l2a_score_mlp.hip) and the
// terminal-value kernel (l2a_value.hip): the weight pack kernel, one hidden layer in place in the LDS image, and its dispatch on
// the layer's width.  Both units are compiled with contraction off.  The text is l2a_score_mlp.hip's own, moved here unchanged
// (the pack kernel is `static`, as the pack kernels of l2a_micro_pack.h are: two units of one library hold it).
#pragma once

#include "l2a_kernels.h"

#define L2A_RM_THREADS 256
#define L2A_RM_MAX_HIDDEN 3
#define L2A_RM_MAX_ROWS 128         // 16 * RT, RT <= 8
#define L2A_RM_MAX_ACC 32           // TPW * RT accumulators of four registers per wave

static __global__ void l2a_rm_pack_k(const float* __restrict__ w, int k_in, int n_out, int KG, long long total, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    int k, u;
    l2a_pack_decode(idx, KG, &k, &u);
    out[idx] = (k < k_in && u < n_out) ? w[(long long)k * n_out + u] : 0.0f;
}

// One hidden layer for the pass's RT row tiles, in place: this wave's TPW unit tiles.  `live`: bit rt = row tile rt holds rows.
// The epilogue applies max(x, floor) - relu (0) or nothing (-inf; the max propagates NaN, l2a_max_nan) - and the other
// activations follow in a pass of their own over the image (l2a_score_mlp_k): inlined into every instance here their code
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
