// l2a_mppi.hip - the reward-weighted ("path-integral", MPPI) planner's per-iteration work around the fused rollout, on the device
// (include/l2a.h: l2a_mppi_sample, l2a_mppi_sample_shard, l2a_mppi_update).  gfx950 only, wave64.  Compiled with -ffp-contract=off: the sample arithmetic
// is restated bit for bit on the host (tests/mppi_reference.py: sample_f32), so every operation below rounds once, on its own.
//
// The planner (PDDM's "filtered and reward-weighted refinement", Nagabandi et al. 2019) keeps one fp32 plan mean mu [h, A] per env
// on the device between controller steps.  One iteration:
//
//   l2a_mppi_sample_k : a workgroup per 4 sample rows.  The mean is shifted (shift[i] < 0: zeros; > 0: mu'_t = mu_min(t + 1, h - 1);
//                       0: kept), the normal z (given, or Philox4x32-10 + Box-Muller at counter offset + e - l2a_cem.hip's stream:
//                       same constants, same counter layout) is scaled - every thread takes elements, the transcendentals run in
//                       parallel - and low-pass filtered over the horizon by one thread per (row, action dimension),
//                           u = z * sigma[k];  nz = beta * u + omb * nz;  a = mu' + nz;  c = fminf(fmaxf(a, low[k]), high[k])
//                       (omb = 1.0f - beta, formed once on the host), and c is stored twice: a_clip [n, m, D] (sample row j * m + i)
//                       and the rollout's candidate tensor seq [h, m * n, A] (plan row i * n + j).  The chains of candidate 0 write
//                       the shifted mean out of place (mean_out; every thread reads mean_in only).  The SHARD instance
//                       (l2a_mppi_sample_shard: one rank of a sharded plan) draws, filters and stores a_clip for ALL n candidates
//                       and writes only its window lo <= j < hi of the rollout tensor, as seq_local [h, m * (hi - lo), A] (plan
//                       row i * (hi - lo) + (j - lo)): the same body, one more condition and another row index at the seq store.
//   l2a_mppi_update_k : grid (ceil(D / 32), m), 1024 threads.  Every workgroup of env i stages the env's n returns in LDS, finds the
//                       maximum over the VALID candidates (neither NaN nor -inf; first maximum by index), turns the returns into
//                       weights in place (w = expf(kappa * (R - Rmax)), 0 for an invalid candidate; Rmax = +inf: 1 for the +inf
//                       returns, else 0), sums w and w^2 (thread tid adds candidates tid, tid + 1024, ... in order, a butterfly over
//                       each wave, the 16 waves in order - every workgroup of the env computes the same bits) and then its own 32
//                       dimensions of sum_j w_j a[j, i, d]: 32 candidate slices x 32 dimensions, slice s takes candidates s, s + 32,
//                       ... with four accumulators at +32 / +64 / +96 (128-byte coalesced reads of a_clip rows, four loads in
//                       flight), the slice totals meet in LDS and are added s = 0..31.  mu[i, d] = numerator / sum w.  An env
//                       without a valid candidate keeps its mean.  Workgroup x = 0 writes the env's result row (action | Rmax |
//                       index | ESS | valid count).  No atomics: the same inputs give the same bits on every run.
//
// Longest sequential add chain of l2a_mppi_update_k's sums, L(n) = ceil(n / 128) + 37: an accumulator's ceil(n / 128) fused
// multiply-adds, at most 3 more from the tail loop, 2 adds joining the four accumulators, 32 slice adds (the weight sums' chain,
// ceil(n / 1024) + 6 + 16, is never longer).  tests/mppi_reference.py: sum_chain.
//
// Two launches per iteration instead of the ~15 stock tensor-library launches (randn, mul, a scan over the horizon, add, clamp,
// permute, isfinite, max, sub, mul, exp, two sums, a matrix product, div) and the host round trip of returns and samples.

#include "l2a_host.h"
#include "l2a_philox.h"      // above every `#pragma clang fp contract(off)` of this unit: see the note at l2a_philox_normal

#include <cmath>
#include <cstring>
#include <string>

namespace {

struct MppiSampleParams {
    const float* z;             // [n, m, D] or null (generate)
    unsigned long long seed, offset;
    const float* mean_in;       // [m, D]
    const int* shift;           // [m]
    const float* sigma;         // [act_dim]
    const float* low;           // [act_dim]
    const float* high;
    float beta, omb;
    int n, m, h, act_dim;
    float* mean_out;            // [m, D]
    float* a_clip;              // [n, m, D]
    float* seq;                 // [h, m * n, act_dim] or null; SHARD: [h, m * (hi - lo), act_dim] (null when hi == lo)
    int lo, hi;                 // SHARD: the candidates whose rollout rows this rank keeps
};

// Workgroup = L2A_MPPI_ROWS sample rows (all their D elements), the horizon in passes of as many steps as fit the LDS tiles.  Per pass:
// (1) all 256 threads draw the pass's normals, scale them and fetch the shifted mean of their elements - the Box-Muller
// transcendentals are the cost of this kernel, and a thread per filter chain would evaluate h of them (and wait for h loads of the
// mean) in sequence; (2) the rows' act_dim chains run the recurrence over the tiles, LDS only (the filter state stays in a register
// from pass to pass), and leave the clipped sample in place; (3) all threads store the tile: a row's slice of a_clip is contiguous,
// and so are the rows of one step in seq when m = 1; the rows of candidate 0 store the shifted mean as well.
#define L2A_MPPI_ROWS 4
#define L2A_MPPI_TILE 2048      // floats: L2A_MPPI_ROWS x steps per pass x act_dim (act_dim <= 16: at least 32 steps per pass)

template <bool SHARD>
__global__ void __launch_bounds__(256) l2a_mppi_sample_k(const MppiSampleParams p) {
#pragma clang fp contract(off)
    __shared__ float tile[L2A_MPPI_TILE];       // u = z * sigma, then the clipped sample
    __shared__ float mtile[L2A_MPPI_TILE];      // the shifted mean
    const int tid = threadIdx.x;
    const int A = p.act_dim, D = p.h * A;
    const long long rows = (long long)p.n * p.m;
    const long long g0 = (long long)blockIdx.x * L2A_MPPI_ROWS;     // first flat sample row j * m + i (the draw's [n, m, D] order)
    const int nr = (int)(rows - g0 < L2A_MPPI_ROWS ? rows - g0 : L2A_MPPI_ROWS);
    const int tc = L2A_MPPI_TILE / (L2A_MPPI_ROWS * A);
    // this thread's chain (row cr, action dimension ck), if it has one
    const bool chain = tid < nr * A;
    const int cr = chain ? tid / A : 0, ck = chain ? tid - cr * A : 0;
    const float lo = p.low[ck], hi = p.high[ck];
    float nz = 0.0f;
    for (int t0 = 0; t0 < p.h; t0 += tc) {
        const int nt = p.h - t0 < tc ? p.h - t0 : tc;
        const int span = nt * A, count = nr * span;
        for (int q = tid; q < count; q += 256) {
            const int r = q / span, rem = q - r * span;         // rem = tt * A + k
            const int tt = rem / A, k = rem - tt * A, t = t0 + tt;
            const long long g = g0 + r;
            const int i = (int)(g % p.m);
            const int sh = p.shift[i];
            const int ts = (sh > 0) ? (t + 1 < p.h ? t + 1 : p.h - 1) : t;
            mtile[q] = (sh < 0) ? 0.0f : p.mean_in[(long long)i * D + ts * A + k];
            const long long e = g * D + t0 * A + rem;
            const float z = p.z ? p.z[e] : l2a_philox_normal(p.seed, p.offset + (unsigned long long)e);
            tile[q] = z * p.sigma[k];
        }
        __syncthreads();
        if (chain) {
            int tt = 0;
            for (; tt + 4 <= nt; tt += 4) {     // four steps' operands read ahead of the (sequential) recurrence
                const int q = cr * span + tt * A + ck;
                float u[4], mv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) { u[s] = tile[q + s * A]; mv[s] = mtile[q + s * A]; }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float bu = p.beta * u[s], kn = p.omb * nz;
                    nz = bu + kn;
                    const float a = mv[s] + nz;
                    u[s] = fminf(fmaxf(a, lo), hi);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) tile[q + s * A] = u[s];
            }
            for (; tt < nt; ++tt) {
                const int q = cr * span + tt * A + ck;
                const float u = tile[q];
                const float bu = p.beta * u, kn = p.omb * nz;
                nz = bu + kn;
                const float a = mtile[q] + nz;
                tile[q] = fminf(fmaxf(a, lo), hi);
            }
        }
        __syncthreads();
        for (int q = tid; q < count; q += 256) {
            const int r = q / span, rem = q - r * span;
            const long long g = g0 + r;
            const long long j = g / p.m;
            const int i = (int)(g - j * p.m);
            const float v = tile[q];
            p.a_clip[g * D + t0 * A + rem] = v;
            if (p.seq && (!SHARD || (j >= p.lo && j < p.hi))) {
                // plan row of this candidate (env-major) among the rows of one horizon step: all n candidates, SHARD: the window's
                const long long width = SHARD ? p.hi - p.lo : p.n;
                const long long prow = (long long)i * width + (SHARD ? j - p.lo : j);
                const int tt = rem / A;
                p.seq[((long long)(t0 + tt) * (width * p.m) + prow) * A + (rem - tt * A)] = v;
            }
            if (j == 0) p.mean_out[(long long)i * D + t0 * A + rem] = mtile[q];
        }
        __syncthreads();
    }
}

// The two sample entry points: the argument checks (nothing is written when one fails) and the launch.
template <bool SHARD>
int mppi_sample_launch(l2a_ctx* ctx, const char* who, MppiSampleParams p, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    const std::string w(who);
    if (!p.mean_in || !p.shift || !p.sigma || !p.low || !p.high || !p.mean_out || !p.a_clip) return l2a_fail(ctx, L2A_EINVAL, w + ": null pointer");
    if (p.n < 1 || p.m < 1 || p.h < 1 || p.act_dim < 1 || p.act_dim > 16)
        return l2a_fail(ctx, L2A_EINVAL, w + ": bad n / m / h / act_dim (1 <= act_dim <= 16)");
    if (!(p.beta > 0.0f) || !(p.beta <= 1.0f)) return l2a_fail(ctx, L2A_EINVAL, w + ": beta must lie in (0, 1]");
    if (p.mean_out == p.mean_in) return l2a_fail(ctx, L2A_EINVAL, w + ": mean_out must not alias mean_in");
    const long long total = (long long)p.n * p.m * p.h * p.act_dim;
    if (total > 0x7fffffffLL * 256) return l2a_fail(ctx, L2A_EINVAL, w + ": too many samples");
    if (SHARD) {
        if (p.lo < 0 || p.hi > p.n || p.lo > p.hi) return l2a_fail(ctx, L2A_EINVAL, w + ": the window needs 0 <= lo <= hi <= n");
        if (p.hi > p.lo && !p.seq) return l2a_fail(ctx, L2A_EINVAL, w + ": null seq_local for a window that holds candidates");
        if (p.hi == p.lo) p.seq = nullptr;
    }
    p.omb = 1.0f - p.beta;
    l2a_device_guard guard(ctx->device);
    const long long rows = (long long)p.n * p.m;
    hipLaunchKernelGGL(l2a_mppi_sample_k<SHARD>, dim3((unsigned)((rows + L2A_MPPI_ROWS - 1) / L2A_MPPI_ROWS)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream_v), p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

// ---- the update ---------------------------------------------------------------------------------------------------------------------
// The kernel's static LDS, counted in the entry point's budget next to the n dynamic floats (include/l2a.h states the figure:
// L2A_MPPI_UPDATE_STATIC_LDS).
#define L2A_MPPI_UT 1024        // threads: 32 candidate slices x 32 dimensions, 16 waves
struct MppiUpdateStatic {
    float part[32][33];         // slice totals
    float wa[16], wb[16];       // per wave: maximum, then the sum of w | the sum of w^2
    int wi[16], wc[16];         // per wave: index of the maximum | valid count
};
static_assert(sizeof(MppiUpdateStatic) == L2A_MPPI_UPDATE_STATIC_LDS, "include/l2a.h states l2a_mppi_update_k's static LDS");
#define L2A_MPPI_NONE 0x7fffffff

// (x, c) beats (best, idx): the first maximum by index; L2A_MPPI_NONE = no valid candidate seen
__device__ __forceinline__ bool mppi_better(float x, int c, float best, int idx) {
    return c != L2A_MPPI_NONE && (idx == L2A_MPPI_NONE || x > best || (x == best && c < idx));
}

__global__ void __launch_bounds__(L2A_MPPI_UT) l2a_mppi_update_k(const float* returns, const float* a_clip, int n, int m, int D,
                                                                 int act_dim, float kappa, float* mean, float* out) {
#pragma clang fp contract(off)
    extern __shared__ float w[];                // [n]: the env's returns, then its weights
    __shared__ MppiUpdateStatic st;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = blockIdx.y;
    const float ninf = -__builtin_inff(), pinf = __builtin_inff();

    // returns -> LDS; each thread's best valid candidate (first maximum) and valid count, then the wave's (a butterfly: every
    // lane ends with the same pair), then the 16 waves' in order
    float best = ninf;
    int idx = L2A_MPPI_NONE, cnt = 0;
    for (int c = tid; c < n; c += L2A_MPPI_UT) {
        const float x = returns[(long long)i * n + c];
        w[c] = x;
        if (x != x || x == ninf) continue;
        ++cnt;
        if (mppi_better(x, c, best, idx)) { best = x; idx = c; }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const float x = __shfl_xor(best, o);
        const int c = __shfl_xor(idx, o);
        cnt += __shfl_xor(cnt, o);
        if (mppi_better(x, c, best, idx)) { best = x; idx = c; }
    }
    if (lane == 0) { st.wa[wv] = best; st.wi[wv] = idx; st.wc[wv] = cnt; }
    __syncthreads();
    float rmax = st.wa[0];
    int imax = st.wi[0], valid = st.wc[0];
    for (int v = 1; v < L2A_MPPI_UT / 64; ++v) {
        if (mppi_better(st.wa[v], st.wi[v], rmax, imax)) { rmax = st.wa[v]; imax = st.wi[v]; }
        valid += st.wc[v];
    }
    __syncthreads();                            // (wa is written again below)

    // weights, once, in place; the sums of w and w^2: per thread in index order, a butterfly per wave, the waves in order
    float sw = 0.0f, sq = 0.0f;
    for (int c = tid; c < n; c += L2A_MPPI_UT) {
        const float x = w[c];
        float wt = 0.0f;
        if (!(x != x) && x != ninf) {
            if (rmax == pinf) wt = (x == pinf) ? 1.0f : 0.0f;
            else {
                const float d = x - rmax;       // <= 0; an overflow to -inf gives expf(-inf) = 0
                wt = expf(kappa * d);
            }
        }
        w[c] = wt;
        sw += wt;
        sq = fmaf(wt, wt, sq);
    }
    for (int o = 32; o >= 1; o >>= 1) { sw += __shfl_xor(sw, o); sq += __shfl_xor(sq, o); }
    if (lane == 0) { st.wa[wv] = sw; st.wb[wv] = sq; }
    __syncthreads();
    float S = st.wa[0], Q = st.wb[0];
    for (int v = 1; v < L2A_MPPI_UT / 64; ++v) { S += st.wa[v]; Q += st.wb[v]; }

    // this workgroup's 32 dimensions: slice sl sums candidates sl, sl + 32, ...
    const int dl = tid & 31, sl = tid >> 5;
    const int d = blockIdx.x * 32 + dl;
    const bool live = d < D;
    const float* col = a_clip + (long long)i * D + (live ? d : 0);
    const long long stride = (long long)m * D;  // candidate j's row of env i is sample row j * m + i
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (valid > 0) {
        int q = sl;
        for (; q + 96 < n; q += 128) {
            const float x0 = col[q * stride], x1 = col[(q + 32) * stride];
            const float x2 = col[(q + 64) * stride], x3 = col[(q + 96) * stride];
            s0 = fmaf(w[q], x0, s0); s1 = fmaf(w[q + 32], x1, s1);
            s2 = fmaf(w[q + 64], x2, s2); s3 = fmaf(w[q + 96], x3, s3);
        }
        for (; q < n; q += 32) s0 = fmaf(w[q], col[q * stride], s0);
    }
    st.part[sl][dl] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sl != 0) return;
    float tot = 0.0f;
#pragma unroll
    for (int s = 0; s < 32; ++s) tot += st.part[s][dl];
    float mu = 0.0f;
    if (live) {
        if (valid > 0) { mu = tot / S; mean[(long long)i * D + d] = mu; }
        else mu = mean[(long long)i * D + d];   // no candidate to imitate: the (shifted) mean stays, bit for bit
    }
    if (blockIdx.x != 0) return;
    float* row = out + (long long)i * (act_dim + 4);
    if (dl < act_dim) row[dl] = mu;             // (act_dim <= 16: the first action's dimensions all belong to workgroup 0)
    if (dl == 0) {
        row[act_dim] = (valid > 0) ? returns[(long long)i * n + imax] : __builtin_nanf("");
        row[act_dim + 1] = __int_as_float(valid > 0 ? imax : -1);
        row[act_dim + 2] = (valid > 0) ? (S * S) / Q : 0.0f;
        row[act_dim + 3] = __int_as_float(valid);
    }
}

}  // namespace

extern "C" {

int l2a_mppi_sample(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                    const int* shift, const float* sigma, float beta, const float* low, const float* high, int n, int m, int h,
                    int act_dim, float* mean_out, float* a_clip, float* seq, void* stream_v) {
    MppiSampleParams p;
    std::memset(&p, 0, sizeof(p));
    p.z = z; p.seed = seed; p.offset = offset; p.mean_in = mean_in; p.shift = shift; p.sigma = sigma; p.low = low; p.high = high;
    p.beta = beta; p.n = n; p.m = m; p.h = h; p.act_dim = act_dim; p.mean_out = mean_out; p.a_clip = a_clip; p.seq = seq;
    return mppi_sample_launch<false>(ctx, "l2a_mppi_sample", p, stream_v);
}

int l2a_mppi_sample_shard(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                          const int* shift, const float* sigma, float beta, const float* low, const float* high, int n, int m, int h,
                          int act_dim, int lo, int hi, float* mean_out, float* a_clip, float* seq_local, void* stream_v) {
    MppiSampleParams p;
    std::memset(&p, 0, sizeof(p));
    p.z = z; p.seed = seed; p.offset = offset; p.mean_in = mean_in; p.shift = shift; p.sigma = sigma; p.low = low; p.high = high;
    p.beta = beta; p.n = n; p.m = m; p.h = h; p.act_dim = act_dim; p.mean_out = mean_out; p.a_clip = a_clip; p.seq = seq_local;
    p.lo = lo; p.hi = hi;
    return mppi_sample_launch<true>(ctx, "l2a_mppi_sample_shard", p, stream_v);
}

int l2a_mppi_update(l2a_ctx* ctx, const float* returns, const float* a_clip, int n, int m, int h, int act_dim, float kappa,
                    float* mean, float* out, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if (!returns || !a_clip || !mean || !out) return l2a_fail(ctx, L2A_EINVAL, "l2a_mppi_update: null pointer");
    if (n < 1 || m < 1 || h < 1 || act_dim < 1 || act_dim > 16 || m > 65535)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_mppi_update: bad n / m / h / act_dim (1 <= act_dim <= 16, m <= 65535)");
    if (!(kappa > 0.0f) || !std::isfinite(kappa)) return l2a_fail(ctx, L2A_EINVAL, "l2a_mppi_update: kappa must be positive and finite");
    if ((long long)n * m * h * act_dim > 0x7fffffffLL * 256) return l2a_fail(ctx, L2A_EINVAL, "l2a_mppi_update: too many samples");
    const size_t smem = (size_t)n * sizeof(float);
    if (smem + L2A_MPPI_UPDATE_STATIC_LDS > (size_t)ctx->lds_per_block)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_mppi_update: more candidates than an env's weights fit in LDS");
    l2a_device_guard guard(ctx->device);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    if (smem > 48 * 1024)
        L2A_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_mppi_update_k),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int D = h * act_dim;
    hipLaunchKernelGGL(l2a_mppi_update_k, dim3((unsigned)((D + 31) / 32), (unsigned)m), dim3(L2A_MPPI_UT), (unsigned)smem, stream, returns,
                       a_clip, n, m, D, act_dim, kappa, mean, out);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

}  // extern "C"
