// l2a_icem.hip - the improved cross-entropy-method planner's (iCEM, Pinneri et al. 2020) per-iteration work around the fused rollout,
// on the device (include/l2a.h: l2a_icem_sample, l2a_icem_sample_shard, l2a_icem_refit).  gfx950 only, wave64.  The sample arithmetic is restated bit for bit
// on the host (tests/icem_reference.py: sample_f32), so every operation of the kernels rounds once, on its own: each kernel body
// opens with `#pragma clang fp contract(off)`.  The unit itself is compiled with l2a_cem.hip's flags, NOT with -ffp-contract=off
// as l2a_mppi.hip is: that flag also keeps the math library's internal multiply-adds (logf, cosf) from fusing, and the Box-Muller
// normals then differ from l2a_cem_sample's by an ulp here and there - this planner's stream is CEM's bit for bit.
//
// Per env the planner keeps a plan mean mu [h, A], a spread sd [h, A] and up to Kk kept elite rows [Kk, D] on the device between
// iterations and controller steps.  One iteration:
//
//   l2a_icem_sample_k : a workgroup per 1 - 4 sample rows (l2a_mppi_sample_k's shape; 256 / D rows, so that a thread draws one normal
//                       per pass where the plan is short enough).  Per pass over the horizon all 256 threads fetch
//                       the shifted mean mu' and the spread sd' of their elements (shift[i] < 0: 0 and sigma0; > 0: mu'_t =
//                       mu_min(t + 1, h - 1) and sigma0 again; 0: both kept) and the element's source: the shifted kept row for a
//                       row j < kc', the clipped mean for the mean row (add_mean: row n_it - 1; it wins over a kept row), else the
//                       normal z (given, or Philox4x32-10 + Box-Muller at counter offset + e - l2a_cem.hip's stream: same
//                       constants, same counter layout; the numbering is positional, a kept row's normals are simply not drawn).
//                       One thread per (row, action dimension) then runs the variance-preserving recurrence over the LDS tile,
//                           nz_0 = z_0;  nz_t = rho * nz_(t-1) + c * z_t;  a = mu' + nz_t * sd';  fminf(fmaxf(a, low[k]), high[k])
//                       (c = sqrtf(1 - rho^2), formed once on the host in fp32), and all threads store the tile twice: a_clip
//                       [n_it, m, D] (sample row j * m + i) and the rollout's candidate tensor seq [h, m * n_it, A] (plan row
//                       i * n_it + j).  The rows of candidate 0 write mu' and sd' out of place (mean_out, std_out).
//   l2a_icem_sample_noise_k : the same sample with nz = M z for a given matrix M [h, h] in place of the recurrence (l2a_icem_sample_noise,
//                       l2a_icem_sample_noise_shard; h <= 128, the whole horizon of a row in LDS) - further down, with the power-law
//                       matrix's host builder l2a_icem_noise_matrix.
//   l2a_icem_rank_k  : grid (ceil(n_it / 4) capped at 256, m), 4 waves.  The env's returns are staged in LDS with every invalid one
//                       (NaN, -inf) as -inf; one wave per VALID candidate j counts the candidates that sort before it in the stable
//                       descending order (ballot + popcount per 64, l2a_cem.hip's cem_rank; the count stops at K - such a
//                       candidate is no elite) and, with rank < K, writes j to work[i, rank].  The ranks of the valid candidates
//                       are a permutation of 0 .. valid - 1: exactly the first min(K, valid) entries are written, each once.
//   l2a_icem_stats_k  : grid (ceil(D / 32), m), 1024 threads = 32 dimensions x 32 rank slices.  Counts the env's valid candidates
//                       (Ke = min(K, valid)), stages the elite indices in LDS, and per dimension sums the elite rows of a_clip in
//                       ONE fixed order: slice s takes ranks s, s + 32, ..., rank s + 32 u goes to the slice's accumulator u mod 4
//                       in the order of u, the accumulators join as (s0 + s1) + (s2 + s3), the slice totals are added s = 0..31;
//                       em = total / Ke; the second pass sums (x - em)^2 by fmaf in the same order, es = sqrtf(total / Ke).  A
//                       slice's first eight rows are loaded at once and kept in registers for the second pass.
//                       mu = alpha * mu' + (1 - alpha) * em and sd = alpha * sd' + (1 - alpha) * es in place (two products and a sum,
//                       each rounded); Ke = 0 touches neither.  The values of the first min(Kk, Ke) ranks go to kept_out as they
//                       are loaded; workgroup x = 0 writes kc_out and the env's result row.
//
// Longest sequential add chain of l2a_icem_stats_k's sums, L(Ke) = ceil(Ke / 128) + 34: an accumulator's ceil(Ke / 128) adds, 2 adds
// joining the four accumulators, 32 slice adds.  tests/icem_reference.py: sum_chain.
//
// Why the refit is two launches: the ranking parallelises over candidates (n_it ranks of up to n_it comparisons), the statistics
// over dimensions.  In one launch every dimension block of an env would repeat the env's whole ranking (l2a_mppi_update_k repeats
// its weight pass, which is n operations, not n^2 / 64 ballots).  No atomics anywhere: the same inputs give the same bits.

#include "l2a_host.h"
#include "l2a_philox.h"      // above every `#pragma clang fp contract(off)` of this unit: see the note at l2a_philox_normal

#include <cmath>
#include <cstring>
#include <string>

namespace {

struct IcemSampleParams {
    const float* z;             // [n, m, D] or null (generate)
    unsigned long long seed, offset;
    const float* mean_in;       // [m, D]
    const float* std_in;        // [m, D]
    const float* kept_in;       // [m, Kk, D] (null when Kk == 0)
    const int* kc_in;           // [m] (null when Kk == 0)
    const int* shift;           // [m]
    const float* sigma0;        // [act_dim]
    const float* low;           // [act_dim]
    const float* high;
    float rho, c;
    int n, m, h, act_dim, Kk, add_mean;
    int rpb;                    // sample rows per workgroup, 1 .. L2A_ICEM_ROWS
    float* mean_out;            // [m, D]
    float* std_out;             // [m, D]
    float* a_clip;              // [n, m, D]
    float* seq;                 // [h, m * n, act_dim] or null; SHARD: [h, m * (hi - lo), act_dim] (null when hi == lo)
    int lo, hi;                 // SHARD: the candidates whose rollout rows this rank keeps
};

#define L2A_ICEM_ROWS 4         // at most; the entry point takes fewer on short plans, so that a thread draws one normal where it can
#define L2A_ICEM_TILE 2048      // floats: L2A_ICEM_ROWS x steps per pass x act_dim (act_dim <= 16: at least 32 steps per pass)

// kept rows of env i this call places: none for a fresh env, else the stored count held to 0 .. Kk
__device__ __forceinline__ int icem_kept_count(const IcemSampleParams& p, int i, int sh) {
    if (p.Kk == 0 || sh < 0) return 0;
    const int kc = p.kc_in[i];
    return kc < 0 ? 0 : (kc > p.Kk ? p.Kk : kc);
}

// 0: a drawn row, 1: kept row j, 2: the mean row (it wins over a kept row)
__device__ __forceinline__ int icem_row_kind(const IcemSampleParams& p, long long j, int kc) {
    if (p.add_mean && j == p.n - 1) return 2;
    return j < kc ? 1 : 0;
}

// Workgroup = p.rpb <= L2A_ICEM_ROWS sample rows (all their D elements), the horizon in passes of as many steps as fit the LDS tiles.  Per pass:
// (1) all 256 threads fetch their elements' mu' and sd' and the source value (a normal, a kept element, the clipped mean) - the
// Box-Muller transcendentals are the cost of this kernel and run in parallel; (2) the rows' act_dim chains run the recurrence over
// the tiles, LDS only (the noise state stays in a register from pass to pass), and leave the clipped sample in place; a kept row and
// the mean row are final already; (3) all threads store the tile.  The SHARD instance (l2a_icem_sample_shard: one rank of a sharded
// plan) does all of that for all n rows - a_clip, mean_out and std_out are the same bits - and stores only its window lo <= j < hi of
// the rollout tensor, as seq_local [h, m * (hi - lo), A] (plan row i * (hi - lo) + (j - lo)); a kept row or the mean row inside the
// window is a row like any other.
template <bool SHARD>
__global__ void __launch_bounds__(256) l2a_icem_sample_k(const IcemSampleParams p) {
#pragma clang fp contract(off)
    __shared__ float tile[L2A_ICEM_TILE];       // z (or a final value), then the clipped sample
    __shared__ float mtile[L2A_ICEM_TILE];      // mu'
    __shared__ float stile[L2A_ICEM_TILE];      // sd'
    const int tid = threadIdx.x;
    const int A = p.act_dim, D = p.h * A;
    const long long rows = (long long)p.n * p.m;
    const long long g0 = (long long)blockIdx.x * p.rpb;     // first flat sample row j * m + i (the draw's [n, m, D] order)
    const int nr = (int)(rows - g0 < p.rpb ? rows - g0 : p.rpb);
    const int tc = L2A_ICEM_TILE / (p.rpb * A);
    // this thread's chain (row cr, action dimension ck), if it has one and its row is drawn
    bool chain = tid < nr * A;
    const int cr = chain ? tid / A : 0, ck = chain ? tid - cr * A : 0;
    if (chain) {
        const long long g = g0 + cr, j = g / p.m;
        const int i = (int)(g - j * p.m);
        chain = icem_row_kind(p, j, icem_kept_count(p, i, p.shift[i])) == 0;
    }
    const float lo = p.low[ck], hi = p.high[ck];
    float nz = 0.0f;
    for (int t0 = 0; t0 < p.h; t0 += tc) {
        const int nt = p.h - t0 < tc ? p.h - t0 : tc;
        const int span = nt * A, count = nr * span;
        for (int q = tid; q < count; q += 256) {
            const int r = q / span, rem = q - r * span;         // rem = tt * A + k
            const int tt = rem / A, k = rem - tt * A, t = t0 + tt;
            const long long g = g0 + r, j = g / p.m;
            const int i = (int)(g - j * p.m);
            const int sh = p.shift[i];
            const int ts = (sh > 0) ? (t + 1 < p.h ? t + 1 : p.h - 1) : t;
            const float mv = (sh < 0) ? 0.0f : p.mean_in[(long long)i * D + ts * A + k];
            mtile[q] = mv;
            stile[q] = (sh != 0) ? p.sigma0[k] : p.std_in[(long long)i * D + t * A + k];
            const int kind = icem_row_kind(p, j, icem_kept_count(p, i, sh));
            float v;
            if (kind == 2) v = fminf(fmaxf(mv, p.low[k]), p.high[k]);
            else if (kind == 1) v = p.kept_in[((long long)i * p.Kk + j) * D + ts * A + k];
            else {
                const long long e = g * D + t0 * A + rem;
                v = p.z ? p.z[e] : l2a_philox_normal(p.seed, p.offset + (unsigned long long)e);
            }
            tile[q] = v;
        }
        __syncthreads();
        if (chain) {
            int tt = 0;
            if (t0 == 0) {                      // nz_0 = z_0
                const int q = cr * span + ck;
                nz = tile[q];
                const float s = nz * stile[q];
                const float a = mtile[q] + s;
                tile[q] = fminf(fmaxf(a, lo), hi);
                tt = 1;
            }
            for (; tt + 4 <= nt; tt += 4) {     // four steps' operands read ahead of the (sequential) recurrence
                const int q = cr * span + tt * A + ck;
                float u[4], mv[4], sv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) { u[s] = tile[q + s * A]; mv[s] = mtile[q + s * A]; sv[s] = stile[q + s * A]; }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float rn = p.rho * nz, cz = p.c * u[s];
                    nz = rn + cz;
                    const float sc = nz * sv[s];
                    const float a = mv[s] + sc;
                    u[s] = fminf(fmaxf(a, lo), hi);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) tile[q + s * A] = u[s];
            }
            for (; tt < nt; ++tt) {
                const int q = cr * span + tt * A + ck;
                const float rn = p.rho * nz, cz = p.c * tile[q];
                nz = rn + cz;
                const float sc = nz * stile[q];
                const float a = mtile[q] + sc;
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
            if (j == 0) {
                p.mean_out[(long long)i * D + t0 * A + rem] = mtile[q];
                p.std_out[(long long)i * D + t0 * A + rem] = stile[q];
            }
        }
        __syncthreads();
    }
}

// What l2a_icem_sample and l2a_icem_sample_shard share: the argument checks (nothing is written or launched when one fails), c, the
// rows per workgroup and the launch of the kernel's instance.
template <bool SHARD>
int icem_sample_launch(l2a_ctx* ctx, const char* who, IcemSampleParams p, void* stream_v) {
#pragma clang fp contract(off)
    const std::string w(who);
    if (!p.mean_in || !p.std_in || !p.shift || !p.sigma0 || !p.low || !p.high || !p.mean_out || !p.std_out || !p.a_clip)
        return l2a_fail(ctx, L2A_EINVAL, w + ": null pointer");
    if (p.n < 1 || p.m < 1 || p.h < 1 || p.act_dim < 1 || p.act_dim > 16)
        return l2a_fail(ctx, L2A_EINVAL, w + ": bad n_it / m / h / act_dim (1 <= act_dim <= 16)");
    if (p.Kk < 0 || p.Kk > 8192) return l2a_fail(ctx, L2A_EINVAL, w + ": 0 <= Kk <= 8192");
    if (p.Kk > 0 && (!p.kept_in || !p.kc_in)) return l2a_fail(ctx, L2A_EINVAL, w + ": null kept rows or counts with Kk > 0");
    if (!(p.rho >= 0.0f) || !(p.rho < 1.0f)) return l2a_fail(ctx, L2A_EINVAL, w + ": rho must lie in [0, 1)");
    if (SHARD) {
        if (p.lo < 0 || p.hi > p.n || p.lo > p.hi) return l2a_fail(ctx, L2A_EINVAL, w + ": the window needs 0 <= lo <= hi <= n_it");
        if (p.hi > p.lo && !p.seq) return l2a_fail(ctx, L2A_EINVAL, w + ": null seq_local for a window that holds candidates");
        if (p.hi == p.lo) p.seq = nullptr;
    }
    const void* ins[] = {p.z, p.mean_in, p.std_in, p.kept_in, p.kc_in, p.shift, p.sigma0, p.low, p.high};
    const void* outs[] = {p.mean_out, p.std_out, p.a_clip, p.seq};
    for (size_t a = 0; a < sizeof(outs) / sizeof(outs[0]); ++a) {
        if (!outs[a]) continue;
        for (const void* in : ins)
            if (in == outs[a]) return l2a_fail(ctx, L2A_EINVAL, w + ": an output aliases an input");
        for (size_t b = 0; b < a; ++b)
            if (outs[b] == outs[a]) return l2a_fail(ctx, L2A_EINVAL, w + ": two outputs alias");
    }
    const long long total = (long long)p.n * p.m * p.h * p.act_dim;
    if (total > 0x7fffffffLL * 256 || (long long)p.n * p.m > 0x7fffffffLL) return l2a_fail(ctx, L2A_EINVAL, w + ": too many samples");
    const float r2 = p.rho * p.rho, om = 1.0f - r2;
    p.c = sqrtf(om);
    l2a_device_guard guard(ctx->device);
    // rows per workgroup: as many (up to L2A_ICEM_ROWS) as still leave every thread at most one element per pass
    const long long rows = (long long)p.n * p.m;
    const int D = p.h * p.act_dim;
    p.rpb = 256 / D < 1 ? 1 : (256 / D > L2A_ICEM_ROWS ? L2A_ICEM_ROWS : 256 / D);
    hipLaunchKernelGGL(l2a_icem_sample_k<SHARD>, dim3((unsigned)((rows + p.rpb - 1) / p.rpb)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream_v), p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

// ---- noise given as a matrix (l2a_icem_sample_noise, l2a_icem_sample_noise_shard) -----------------------------------------------------
// nz = M z per (candidate, action dimension) in place of the recurrence: M [h, h] row-major fp32 in global memory, any matrix (the
// power-law one is l2a_icem_noise_matrix's).  The AR(1) kernel above and its parameter block are left exactly as they are: the
// matrix travels in a block of its own around them.
struct IcemNoiseParams {
    IcemSampleParams s;         // (rho, c: unused)
    const float* noise;         // [h, h]
};

// Workgroup = p.s.rpb <= L2A_ICEM_ROWS sample rows with their WHOLE horizon resident (h <= L2A_ICEM_NOISE_MAX_H: rows x D <= the tile),
// so there are no passes and no state between them.  (1) is l2a_icem_sample_k's fetch and draw into LDS - the Box-Muller
// transcendentals in parallel.  (2) every thread owns whole output elements (row, t, k): the h-term sum over the row's normals of
// dimension k in ONE order, s = 0 .. h - 1, a product and an add per term, each rounded on its own - the bits of an element depend on
// nothing but its row of M and its normals, not on the rows per workgroup, the grid or the window -, then scale, add, clip; a kept row
// and the mean row are final as fetched.  (3) the same thread stores the element twice, as l2a_icem_sample_k does (nothing is
// written back to LDS: the normals stay as they are for the other threads' sums).
// M is read from global memory: one workgroup reads each of its h x h entries D / h = act_dim times per sample row, the lanes of
// a wave that share a step t read one address (the 16 lanes of an act_dim = 16 plan), a lane walks its row of M upwards, and the
// matrix - 3.6 KB at h = 30, 64 KB at h = 128 - is shared by every workgroup of the launch, so it is served by L1 / L2.  An LDS
// copy would cost every workgroup those 64 KB of reads again plus, at h = 128, more LDS than the 64 KB a workgroup gets without
// the dynamic-LDS attribute - and one workgroup multiplies at most 2048 x 128 terms.
template <bool SHARD>
__global__ void __launch_bounds__(256) l2a_icem_sample_noise_k(const IcemNoiseParams pn) {
#pragma clang fp contract(off)
    __shared__ float tile[L2A_ICEM_TILE];       // z (or a final value)
    __shared__ float mtile[L2A_ICEM_TILE];      // mu'
    __shared__ float stile[L2A_ICEM_TILE];      // sd'
    const IcemSampleParams& p = pn.s;
    const int tid = threadIdx.x;
    const int h = p.h, A = p.act_dim, D = h * A;
    const long long rows = (long long)p.n * p.m;
    const long long g0 = (long long)blockIdx.x * p.rpb;     // first flat sample row j * m + i (the draw's [n, m, D] order)
    const int nr = (int)(rows - g0 < p.rpb ? rows - g0 : p.rpb);
    const int count = nr * D;                               // <= L2A_ICEM_TILE: the entry point's rpb and its limit on h
    for (int q = tid; q < count; q += 256) {
        const int r = q / D, rem = q - r * D;               // rem = t * A + k
        const int t = rem / A, k = rem - t * A;
        const long long g = g0 + r, j = g / p.m;
        const int i = (int)(g - j * p.m);
        const int sh = p.shift[i];
        const int ts = (sh > 0) ? (t + 1 < h ? t + 1 : h - 1) : t;
        const float mv = (sh < 0) ? 0.0f : p.mean_in[(long long)i * D + ts * A + k];
        mtile[q] = mv;
        stile[q] = (sh != 0) ? p.sigma0[k] : p.std_in[(long long)i * D + t * A + k];
        const int kind = icem_row_kind(p, j, icem_kept_count(p, i, sh));
        float v;
        if (kind == 2) v = fminf(fmaxf(mv, p.low[k]), p.high[k]);
        else if (kind == 1) v = p.kept_in[((long long)i * p.Kk + j) * D + ts * A + k];
        else {
            const long long e = g * D + rem;
            v = p.z ? p.z[e] : l2a_philox_normal(p.seed, p.offset + (unsigned long long)e);
        }
        tile[q] = v;
    }
    __syncthreads();
    for (int q = tid; q < count; q += 256) {
        const int r = q / D, rem = q - r * D;
        const int t = rem / A, k = rem - t * A;
        const long long g = g0 + r, j = g / p.m;
        const int i = (int)(g - j * p.m);
        float v = tile[q];
        if (icem_row_kind(p, j, icem_kept_count(p, i, p.shift[i])) == 0) {
            const float* mrow = pn.noise + (long long)t * h;
            const float* zk = tile + r * D + k;             // this row's normals of dimension k: one per step, A floats apart
            float acc = mrow[0] * zk[0];
            for (int s = 1; s < h; ++s) {
                const float pr = mrow[s] * zk[s * A];
                acc = acc + pr;
            }
            const float sc = acc * stile[q];
            const float a = mtile[q] + sc;
            v = fminf(fmaxf(a, p.low[k]), p.high[k]);
        }
        p.a_clip[g * D + rem] = v;
        if (p.seq && (!SHARD || (j >= p.lo && j < p.hi))) {
            // plan row of this candidate (env-major) among the rows of one horizon step: all n candidates, SHARD: the window's
            const long long width = SHARD ? p.hi - p.lo : p.n;
            const long long prow = (long long)i * width + (SHARD ? j - p.lo : j);
            p.seq[((long long)t * (width * p.m) + prow) * A + k] = v;
        }
        if (j == 0) {
            p.mean_out[(long long)i * D + rem] = mtile[q];
            p.std_out[(long long)i * D + rem] = stile[q];
        }
    }
}

// What l2a_icem_sample_noise and l2a_icem_sample_noise_shard share: icem_sample_launch's checks without rho's, the limit on h, the
// matrix's own, the rows per workgroup (l2a_icem_sample's rule) and the launch.
template <bool SHARD>
int icem_sample_noise_launch(l2a_ctx* ctx, const char* who, IcemNoiseParams pn, void* stream_v) {
    IcemSampleParams& p = pn.s;
    const std::string w(who);
    if (!p.mean_in || !p.std_in || !p.shift || !p.sigma0 || !p.low || !p.high || !p.mean_out || !p.std_out || !p.a_clip || !pn.noise)
        return l2a_fail(ctx, L2A_EINVAL, w + ": null pointer");
    if (p.n < 1 || p.m < 1 || p.h < 1 || p.act_dim < 1 || p.act_dim > 16)
        return l2a_fail(ctx, L2A_EINVAL, w + ": bad n_it / m / h / act_dim (1 <= act_dim <= 16)");
    if (p.h > L2A_ICEM_NOISE_MAX_H) return l2a_fail(ctx, L2A_EINVAL, w + ": h beyond L2A_ICEM_NOISE_MAX_H (a row's whole horizon stays in LDS)");
    if (p.Kk < 0 || p.Kk > 8192) return l2a_fail(ctx, L2A_EINVAL, w + ": 0 <= Kk <= 8192");
    if (p.Kk > 0 && (!p.kept_in || !p.kc_in)) return l2a_fail(ctx, L2A_EINVAL, w + ": null kept rows or counts with Kk > 0");
    if (SHARD) {
        if (p.lo < 0 || p.hi > p.n || p.lo > p.hi) return l2a_fail(ctx, L2A_EINVAL, w + ": the window needs 0 <= lo <= hi <= n_it");
        if (p.hi > p.lo && !p.seq) return l2a_fail(ctx, L2A_EINVAL, w + ": null seq_local for a window that holds candidates");
        if (p.hi == p.lo) p.seq = nullptr;
    }
    const void* ins[] = {p.z, p.mean_in, p.std_in, p.kept_in, p.kc_in, p.shift, p.sigma0, p.low, p.high, pn.noise};
    const void* outs[] = {p.mean_out, p.std_out, p.a_clip, p.seq};
    for (size_t a = 0; a < sizeof(outs) / sizeof(outs[0]); ++a) {
        if (!outs[a]) continue;
        for (const void* in : ins)
            if (in == outs[a]) return l2a_fail(ctx, L2A_EINVAL, w + ": an output aliases an input");
        for (size_t b = 0; b < a; ++b)
            if (outs[b] == outs[a]) return l2a_fail(ctx, L2A_EINVAL, w + ": two outputs alias");
    }
    const long long total = (long long)p.n * p.m * p.h * p.act_dim;
    if (total > 0x7fffffffLL * 256 || (long long)p.n * p.m > 0x7fffffffLL) return l2a_fail(ctx, L2A_EINVAL, w + ": too many samples");
    l2a_device_guard guard(ctx->device);
    const long long rows = (long long)p.n * p.m;
    const int D = p.h * p.act_dim;
    static_assert(L2A_ICEM_NOISE_MAX_H * 16 <= L2A_ICEM_TILE, "one row's whole horizon must fit the LDS tile");
    p.rpb = 256 / D < 1 ? 1 : (256 / D > L2A_ICEM_ROWS ? L2A_ICEM_ROWS : 256 / D);     // rpb * D <= max(256, D) <= L2A_ICEM_TILE
    hipLaunchKernelGGL(l2a_icem_sample_noise_k<SHARD>, dim3((unsigned)((rows + p.rpb - 1) / p.rpb)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream_v), pn);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

// ---- the refit -----------------------------------------------------------------------------------------------------------------------
// Stable descending rank of the valid candidate j among env i's valid returns, counted up to `cap` (rs holds -inf for every invalid
// candidate, and v = rs[j] > -inf: an invalid one is never "before").  One wave per j, l2a_cem.hip's cem_rank, 256 candidates (four
// independent LDS reads) per look at the cap: a look per 64 made every read wait for the one before it.
__device__ __forceinline__ int icem_rank(const float* rs, int n, int j, int lane, int cap) {
    const float v = rs[j];
    int rank = 0;
    for (int c0 = 0; c0 < n && rank < cap; c0 += 256) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + 64 * u + lane;
            const float w = (c < n) ? rs[c] : -__builtin_inff();
            const bool before = (c < n) && (w > v || (w == v && c < j));
            rank += __popcll(__ballot(before));
        }
    }
    return rank;
}

__global__ void __launch_bounds__(256) l2a_icem_rank_k(const float* returns, int n, int K, int* work) {
    extern __shared__ float rs[];               // [n]
    const int i = blockIdx.y;
    for (int c = threadIdx.x; c < n; c += 256) {
        const float x = returns[(long long)i * n + c];
        rs[c] = (x != x) ? -__builtin_inff() : x;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
    for (int j = wave; j < n; j += n_waves) {
        if (rs[j] == -__builtin_inff()) continue;           // invalid: never an elite
        const int rank = icem_rank(rs, n, j, lane, K);
        if (lane == 0 && rank < K) work[(long long)i * K + rank] = j;
    }
}

// The statistics kernel's static LDS, counted in the entry point's budget next to its K dynamic ints (include/l2a.h states the
// figure: L2A_ICEM_REFIT_STATIC_LDS).
#define L2A_ICEM_ST 1024        // threads: 32 rank slices x 32 dimensions, 16 waves
struct IcemStatsStatic {
    float part[32][33];         // slice totals
    int wc[16];                 // valid candidates per wave
};
static_assert(sizeof(IcemStatsStatic) == L2A_ICEM_REFIT_STATIC_LDS, "include/l2a.h states l2a_icem_stats_k's static LDS");

struct IcemStatsParams {
    const float* returns;       // [m, n]
    const float* a_clip;        // [n, m, D]
    const int* work;            // [m, K]
    const float* low;
    const float* high;
    int n, m, D, act_dim, K, Kk;
    float alpha;
    float* mean;                // [m, D]
    float* std;
    float* kept_out;            // [m, Kk, D] (null when Kk == 0)
    int* kc_out;                // [m]
    float* out;                 // [m, act_dim + 4]
};

// one elite value into the slice's accumulator: the sum (pass 0) or the squared deviation from em (pass 1)
__device__ __forceinline__ float icem_acc(float s, float x, float em, int pass) {
#pragma clang fp contract(off)
    if (pass == 0) return s + x;
    const float e = x - em;
    return fmaf(e, e, s);
}

__global__ void __launch_bounds__(L2A_ICEM_ST) l2a_icem_stats_k(const IcemStatsParams p) {
#pragma clang fp contract(off)
    extern __shared__ int erow[];               // [K]: candidate index of rank q
    __shared__ IcemStatsStatic st;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int dl = tid & 31, sl = tid >> 5;
    const int i = blockIdx.y, n = p.n, D = p.D;
    const float ninf = -__builtin_inff();
    const int d0 = blockIdx.x * 32, d = d0 + dl;
    const bool live = d < D;
    const float* col = p.a_clip + (long long)i * D + (live ? d : 0);
    const long long stride = (long long)p.m * D;        // candidate j's row of env i is sample row j * m + i
    const long long e = (long long)i * D + d;

    // one round trip for everything that does not depend on the elite count: the env's valid candidates, the ranking's list (an
    // entry at or beyond Ke was not written: it is held to the rows and never used), this dimension's mu' and sd'
    int cnt = 0;
    for (int c = tid; c < n; c += L2A_ICEM_ST) {
        const float x = p.returns[(long long)i * n + c];
        cnt += (x != x || x == ninf) ? 0 : 1;
    }
    const int kmax = p.K < n ? p.K : n;
    for (int q = tid; q < kmax; q += L2A_ICEM_ST) {
        const int c = p.work[(long long)i * p.K + q];
        erow[q] = c < 0 ? 0 : (c < n ? c : n - 1);
    }
    float mu0 = 0.0f, sd0 = 0.0f;
    if (live && sl == 0) { mu0 = p.mean[e]; sd0 = p.std[e]; }
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) st.wc[wv] = cnt;
    __syncthreads();
    int valid = 0;
#pragma unroll
    for (int v = 0; v < L2A_ICEM_ST / 64; ++v) valid += st.wc[v];
    const int Ke = valid < p.K ? valid : p.K;
    const int kk = p.Kk < Ke ? p.Kk : Ke;
    const bool head = blockIdx.x == 0 && tid == 0;
    float bret = 0.0f;
    if (head && Ke > 0) bret = p.returns[(long long)i * n + erow[0]];

    // Slice sl owns ranks sl, sl + 32, ...; rank sl + 32 u goes to accumulator u mod 4, in the order of u.  The first eight of them
    // are loaded at once and stay in registers for the second pass (Ke <= 256: no second read at all); they also ARE the kept
    // rows and the best candidate's first action, which are stored from the registers.
    float c8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int q = sl + 32 * u;
        c8[u] = (q < Ke) ? col[erow[q] * stride] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int q = sl + 32 * u;
        if (q < kk && live) p.kept_out[((long long)i * p.Kk + q) * D + d] = c8[u];
    }
    float* row = p.out + (long long)i * (p.act_dim + 4);
    // (act_dim <= 16 <= 32: the first action's dimensions all belong to workgroup 0, slice 0, rank 0)
    if (blockIdx.x == 0 && sl == 0 && dl < p.act_dim && Ke > 0) row[dl] = c8[0];

    float em = 0.0f, es = 0.0f;
    const float fk = (float)(Ke > 0 ? Ke : 1);
    for (int pass = 0; pass < 2; ++pass) {
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (sl + 32 * u < Ke) s[u & 3] = icem_acc(s[u & 3], c8[u], em, pass);
        for (int q0 = sl + 256; q0 < Ke; q0 += 128) {
            float x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = (q0 + 32 * u < Ke) ? col[erow[q0 + 32 * u] * stride] : 0.0f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + 32 * u;
                if (q >= Ke) continue;
                s[u] = icem_acc(s[u], x[u], em, pass);
                if (pass == 0 && q < kk && live) p.kept_out[((long long)i * p.Kk + q) * D + d] = x[u];
            }
        }
        st.part[sl][dl] = (s[0] + s[1]) + (s[2] + s[3]);
        __syncthreads();
        float tot = 0.0f;
#pragma unroll
        for (int w = 0; w < 32; ++w) tot += st.part[w][dl];
        __syncthreads();
        if (pass == 0) em = tot / fk; else es = sqrtf(tot / fk);
    }
    if (live && sl == 0 && Ke > 0) {
        const float oma = 1.0f - p.alpha;
        const float km = p.alpha * mu0, nm = oma * em;
        p.mean[e] = km + nm;
        const float ks = p.alpha * sd0, ns = oma * es;
        p.std[e] = ks + ns;
    }
    if (blockIdx.x != 0) return;
    // Ke = 0: the mean stays, and its clipped first step is the action
    if (sl == 0 && dl < p.act_dim && Ke == 0) row[dl] = fminf(fmaxf(mu0, p.low[dl]), p.high[dl]);
    if (head) {
        p.kc_out[i] = kk;
        row[p.act_dim] = (Ke > 0) ? bret : __builtin_nanf("");
        row[p.act_dim + 1] = __int_as_float(Ke > 0 ? erow[0] : -1);
        row[p.act_dim + 2] = __int_as_float(Ke);
        row[p.act_dim + 3] = __int_as_float(valid);
    }
}

}  // namespace

extern "C" {

int l2a_icem_sample(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                    const float* std_in, const float* kept_in, const int* kc_in, const int* shift, const float* sigma0, float rho,
                    const float* low, const float* high, int n_it, int m, int h, int act_dim, int Kk, int add_mean, float* mean_out,
                    float* std_out, float* a_clip, float* seq, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    IcemSampleParams p;
    std::memset(&p, 0, sizeof(p));
    p.z = z; p.seed = seed; p.offset = offset; p.mean_in = mean_in; p.std_in = std_in; p.kept_in = kept_in; p.kc_in = kc_in;
    p.shift = shift; p.sigma0 = sigma0; p.low = low; p.high = high; p.rho = rho;
    p.n = n_it; p.m = m; p.h = h; p.act_dim = act_dim; p.Kk = Kk; p.add_mean = add_mean ? 1 : 0;
    p.mean_out = mean_out; p.std_out = std_out; p.a_clip = a_clip; p.seq = seq;
    return icem_sample_launch<false>(ctx, "l2a_icem_sample", p, stream_v);
}

int l2a_icem_sample_shard(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                          const float* std_in, const float* kept_in, const int* kc_in, const int* shift, const float* sigma0, float rho,
                          const float* low, const float* high, int n_it, int m, int h, int act_dim, int Kk, int add_mean, int lo, int hi,
                          float* mean_out, float* std_out, float* a_clip, float* seq_local, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    IcemSampleParams p;
    std::memset(&p, 0, sizeof(p));
    p.z = z; p.seed = seed; p.offset = offset; p.mean_in = mean_in; p.std_in = std_in; p.kept_in = kept_in; p.kc_in = kc_in;
    p.shift = shift; p.sigma0 = sigma0; p.low = low; p.high = high; p.rho = rho;
    p.n = n_it; p.m = m; p.h = h; p.act_dim = act_dim; p.Kk = Kk; p.add_mean = add_mean ? 1 : 0;
    p.mean_out = mean_out; p.std_out = std_out; p.a_clip = a_clip; p.seq = seq_local;
    p.lo = lo; p.hi = hi;
    return icem_sample_launch<true>(ctx, "l2a_icem_sample_shard", p, stream_v);
}

// The power-law matrix of include/l2a.h, on the host in double precision, rounded once: column 0 the mean, columns 2k - 1 and 2k the
// cosine and the sine of frequency k, the last column of an even h the Nyquist term.  (k t is reduced modulo h in integers before
// it meets pi: the angle stays below 2 pi.)
int l2a_icem_noise_matrix(int h, double beta, float* M_host) {
#pragma clang fp contract(off)
    if (h < 1 || h > L2A_ICEM_NOISE_MAX_H || !std::isfinite(beta) || beta < 0.0 || beta > 8.0 || !M_host) return L2A_EINVAL;
    const int half = h / 2, mid = (h - 1) / 2;
    const bool nyquist = h % 2 == 0 && h > 1;
    double s[L2A_ICEM_NOISE_MAX_H / 2 + 1];
    for (int k = 0; k <= half; ++k) s[k] = std::pow((double)(k > 1 ? k : 1), -0.5 * beta) * std::pow((double)h, 0.5 * beta);
    double sum = s[0] * s[0];
    for (int k = 1; k <= mid; ++k) sum += 2.0 * (s[k] * s[k]);
    if (nyquist) sum += s[half] * s[half];
    const double N = std::sqrt(sum), r2 = std::sqrt(2.0), two_pi = 6.283185307179586476925286766559;
    for (int t = 0; t < h; ++t) {
        float* row = M_host + (size_t)t * h;
        row[0] = (float)(s[0] / N);
        for (int k = 1; k <= mid; ++k) {
            const double ang = two_pi * (double)((k * t) % h) / (double)h;
            row[2 * k - 1] = (float)(r2 * s[k] * std::cos(ang) / N);
            row[2 * k] = (float)(-r2 * s[k] * std::sin(ang) / N);
        }
        if (nyquist) row[h - 1] = (float)((t % 2 ? -s[half] : s[half]) / N);
    }
    return L2A_OK;
}

int l2a_icem_sample_noise(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                          const float* std_in, const float* kept_in, const int* kc_in, const int* shift, const float* sigma0,
                          const float* noise, const float* low, const float* high, int n_it, int m, int h, int act_dim, int Kk,
                          int add_mean, float* mean_out, float* std_out, float* a_clip, float* seq, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    IcemNoiseParams pn;
    std::memset(&pn, 0, sizeof(pn));
    IcemSampleParams& p = pn.s;
    p.z = z; p.seed = seed; p.offset = offset; p.mean_in = mean_in; p.std_in = std_in; p.kept_in = kept_in; p.kc_in = kc_in;
    p.shift = shift; p.sigma0 = sigma0; p.low = low; p.high = high; pn.noise = noise;
    p.n = n_it; p.m = m; p.h = h; p.act_dim = act_dim; p.Kk = Kk; p.add_mean = add_mean ? 1 : 0;
    p.mean_out = mean_out; p.std_out = std_out; p.a_clip = a_clip; p.seq = seq;
    return icem_sample_noise_launch<false>(ctx, "l2a_icem_sample_noise", pn, stream_v);
}

int l2a_icem_sample_noise_shard(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                                const float* std_in, const float* kept_in, const int* kc_in, const int* shift, const float* sigma0,
                                const float* noise, const float* low, const float* high, int n_it, int m, int h, int act_dim, int Kk,
                                int add_mean, int lo, int hi, float* mean_out, float* std_out, float* a_clip, float* seq_local,
                                void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    IcemNoiseParams pn;
    std::memset(&pn, 0, sizeof(pn));
    IcemSampleParams& p = pn.s;
    p.z = z; p.seed = seed; p.offset = offset; p.mean_in = mean_in; p.std_in = std_in; p.kept_in = kept_in; p.kc_in = kc_in;
    p.shift = shift; p.sigma0 = sigma0; p.low = low; p.high = high; pn.noise = noise;
    p.n = n_it; p.m = m; p.h = h; p.act_dim = act_dim; p.Kk = Kk; p.add_mean = add_mean ? 1 : 0;
    p.mean_out = mean_out; p.std_out = std_out; p.a_clip = a_clip; p.seq = seq_local;
    p.lo = lo; p.hi = hi;
    return icem_sample_noise_launch<true>(ctx, "l2a_icem_sample_noise_shard", pn, stream_v);
}

int l2a_icem_refit(l2a_ctx* ctx, const float* returns, const float* a_clip, const float* low, const float* high, int n_it, int m,
                   int h, int act_dim, int K, int Kk, float alpha, int* work, float* mean, float* std, float* kept_out, int* kc_out,
                   float* out, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    const std::string w("l2a_icem_refit");
    if (!returns || !a_clip || !low || !high || !work || !mean || !std || !kc_out || !out)
        return l2a_fail(ctx, L2A_EINVAL, w + ": null pointer");
    if (n_it < 1 || m < 1 || h < 1 || act_dim < 1 || act_dim > 16 || m > 65535)
        return l2a_fail(ctx, L2A_EINVAL, w + ": bad n_it / m / h / act_dim (1 <= act_dim <= 16, m <= 65535)");
    if (K < 1 || K > 8192) return l2a_fail(ctx, L2A_EINVAL, w + ": 1 <= K <= 8192 elites");
    if (Kk < 0 || Kk > K) return l2a_fail(ctx, L2A_EINVAL, w + ": 0 <= Kk <= K kept elites");
    if (Kk > 0 && !kept_out) return l2a_fail(ctx, L2A_EINVAL, w + ": null kept_out with Kk > 0");
    if (!(alpha >= 0.0f) || !(alpha < 1.0f)) return l2a_fail(ctx, L2A_EINVAL, w + ": alpha must lie in [0, 1)");
    const void* ins[] = {returns, a_clip, low, high};
    const void* outs[] = {work, mean, std, kept_out, kc_out, out};
    for (size_t a = 0; a < sizeof(outs) / sizeof(outs[0]); ++a) {
        if (!outs[a]) continue;
        for (const void* in : ins)
            if (in == outs[a]) return l2a_fail(ctx, L2A_EINVAL, w + ": an output aliases an input");
        for (size_t b = 0; b < a; ++b)
            if (outs[b] == outs[a]) return l2a_fail(ctx, L2A_EINVAL, w + ": two outputs alias");
    }
    if ((long long)n_it * m * h * act_dim > 0x7fffffffLL * 256) return l2a_fail(ctx, L2A_EINVAL, w + ": too many samples");
    const size_t rank_lds = (size_t)n_it * sizeof(float);
    const size_t stats_lds = (size_t)K * sizeof(int);
    if (rank_lds > (size_t)ctx->lds_per_block || stats_lds + L2A_ICEM_REFIT_STATIC_LDS > (size_t)ctx->lds_per_block)
        return l2a_fail(ctx, L2A_EINVAL, w + ": more candidates than an env's returns fit in LDS");
    l2a_device_guard guard(ctx->device);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    if (rank_lds > 48 * 1024)
        L2A_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_icem_rank_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)rank_lds));
    int blocks = (n_it + 3) / 4;                // one wave per candidate, at most 1024 waves per env
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(l2a_icem_rank_k, dim3((unsigned)blocks, (unsigned)m), dim3(256), (unsigned)rank_lds, stream, returns, n_it, K, work);
    L2A_HIP(ctx, hipGetLastError());
    IcemStatsParams p;
    std::memset(&p, 0, sizeof(p));
    p.returns = returns; p.a_clip = a_clip; p.work = work; p.low = low; p.high = high;
    p.n = n_it; p.m = m; p.D = h * act_dim; p.act_dim = act_dim; p.K = K; p.Kk = Kk; p.alpha = alpha;
    p.mean = mean; p.std = std; p.kept_out = kept_out; p.kc_out = kc_out; p.out = out;
    hipLaunchKernelGGL(l2a_icem_stats_k, dim3((unsigned)((p.D + 31) / 32), (unsigned)m), dim3(L2A_ICEM_ST), (unsigned)stats_lds, stream, p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

}  // extern "C"
