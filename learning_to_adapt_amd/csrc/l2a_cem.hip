// l2a_cem.hip - the cross-entropy-method planner's per-iteration work around the fused rollout, on the device
// (include/l2a.h: l2a_cem_sample, l2a_cem_refit, l2a_cem_shard_pack / _unpack).  gfx950 only.
//
// Reference: `MPCController.get_cem_action` (policies/mpc_controller.py:71-106).  Per iteration the reference draws
// n * m * h * act_dim standard normals on the host (:85), forms a = mean + z * std (:86), clips (:87), rolls the
// UNCLIPPED samples out reading its candidate-major rows as if they were env-major (:92-96), and refits mean / std
// to the "elites" its rank mask `(-returns).argsort() < num_elites` selects (:101-104): boolean POSITIONS p for which
// the candidate ranked p-th has an index below num_elites, pooled over the envs.  `reference` = 1 keeps those
// semantics; 0 = the fixed reading (clipped rollouts, env-major rows, true top-k per env).
//
//   l2a_cem_sample_k : one thread per sample element: z (given, or Philox4x32-10 + Box-Muller from (seed, offset)),
//                      a = mean + z * std, clip, both stored [n, m, D]; the rollout's candidate tensor
//                      [h, m * n_local, act_dim] is written in the same pass (transposed, this rank's shard only)
//   l2a_cem_rank_k   : elite rows WITHOUT a sort (one wave per rank: ballot + popcount over the env's returns in LDS).  reference: position p is an elite of env i iff p = rank_i(j) for one of
//                      the first k candidates j - k rank computations of n comparisons each; fixed: candidate c is
//                      an elite iff rank_i(c) < k - n of them.  Stable descending order (ties: lower index first), like
//                      the stable argsort it replaces
//   l2a_cem_stats_k  : mean / biased std of the elite rows per dimension (two passes, 8 row slices per dimension), pooled
//                      over the envs (reference) or per env, and the update mean = alpha * mean + (1 - alpha) * elite_mean
//
// Three launches per iteration instead of the ~20 stock tensor-library launches they replace (randn, mul, add, clamp,
// permute / contiguous, argsort, compare, transpose, masked sums, topk / gather, mean, std).

#include "l2a_host.h"
#include "l2a_philox.h"      // above every `#pragma clang fp contract(off)` of this unit: see the note at l2a_philox_normal

#include <atomic>
#include <cstring>
#include <string>

namespace {

struct CemSampleParams {
    const float* z;             // [n, m, D] or null (generate)
    unsigned long long seed, offset;
    const float* mean;          // [m, D]
    const float* std;
    const float* low;           // [act_dim]
    const float* high;
    int n, m, h, act_dim, reference, lo, hi;
    float* a_clip;              // [n, m, D]
    float* a_raw;               // [n, m, D] or null
    float* seq;                 // [h, m * (hi - lo), act_dim] or null
};

__global__ void __launch_bounds__(256) l2a_cem_sample_k(const CemSampleParams p) {
    const int D = p.h * p.act_dim;
    const long long total = (long long)p.n * p.m * D;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long g = e / D;                  // flat sample row j * m + i (the draw's [n, m, D] order, :85)
    const int d = (int)(e - g * D);
    const int i = (int)(g % p.m);
    const float z = p.z ? p.z[e] : l2a_philox_normal(p.seed, p.offset + (unsigned long long)e);
    const float a = p.mean[i * D + d] + z * p.std[i * D + d];                      // :86
    const int k = d % p.act_dim, t = d / p.act_dim;
    const float c = fminf(fmaxf(a, p.low[k]), p.high[k]);                           // :87
    p.a_clip[e] = c;
    if (p.a_raw) p.a_raw[e] = a;
    if (p.seq) {
        // plan row of this sample: the reference feeds its candidate-major rows as if they were env-major (:92-96)
        const long long prow = p.reference ? g : (long long)i * p.n + g / p.m;
        const long long cand = prow % p.n, blk = prow / p.n;
        if (cand >= p.lo && cand < p.hi) {
            const long long nsel = p.hi - p.lo;
            p.seq[((long long)t * (p.m * nsel) + blk * nsel + (cand - p.lo)) * p.act_dim + k] = p.reference ? a : c;
        }
    }
}

// Stable descending rank of candidate j among env i's returns = the number of candidates that sort before it.  One WAVE
// per j: lane l looks at candidates l, l + 64, ...; a ballot + popcount per 64 candidates (a thread-per-j loop over LDS was
// one exposed LDS round trip per candidate: 106 us for 400 ranks of 4000).
__device__ __forceinline__ int cem_rank(const float* r, int n, int j, int lane) {
    const float v = r[j];
    int rank = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int c = c0 + lane;
        const float w = (c < n) ? r[c] : -__builtin_inff();
        const bool before = (c < n) && (w > v || (w == v && c < j));
        rank += __popcll(__ballot(before));
    }
    return rank;
}

// elite_rows[i * k + q]: flat sample rows (into [n * m, D]) of env i's elites.  grid (blocks, m); the waves of an env's
// workgroups take the j's round robin (j < k in the reference's reading, j < n in the fixed one); the env's returns are
// staged in LDS.
__global__ void __launch_bounds__(256) l2a_cem_rank_k(const float* returns, int n, int m, int k, int reference,
                                                      int* elite_rows) {
    extern __shared__ float rs[];
    const int i = blockIdx.y;
    for (int c = threadIdx.x; c < n; c += 256) {
        const float x = returns[(long long)i * n + c];
        rs[c] = (x != x) ? -__builtin_inff() : x;      // NaN returns sort last (np.argsort of -returns puts them there too);
    }                                                  // with ties broken by index the ranks stay a permutation
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
    const int work = reference ? k : n;
    for (int j = wave; j < work; j += n_waves) {
        const int rank = cem_rank(rs, n, j, lane);
        if (lane != 0) continue;
        if (reference) elite_rows[i * k + j] = rank * m + i;         // position rank_i(j) of env i is an elite (:101)
        else if (rank < k) elite_rows[i * k + rank] = j * m + i;      // candidate j is among env i's top k
    }
}

// Elite statistics per dimension: group = all envs pooled (reference; the result is broadcast to every env, :103-104) or
// one env (fixed).  Workgroup = 32 dimensions x 8 row slices: the elite row ids are staged in LDS, every thread sums its
// slice of the rows (independent loads, 4 in flight), the slices meet in LDS in a fixed order; two passes (mean, then
// the squared deviations).  grid (ceil(D / 32), groups).
#define L2A_CEM_MAXROWS 8192
// mean = alpha * mean + (1 - alpha) * elite_mean with its roundings written out (no contraction left to the compiler): the pooled
// (reference) reading rounds through one fma, fma(mean, alpha, (1 - alpha) mu); the per-env (fixed) reading rounds both products
// and their sum.  l2a_cem_stats_k and l2a_cem_refit_sample_k both use it - the two stay bit-identical by construction.
__device__ __forceinline__ float cem_mean_update(float mean, float alpha, float mu, bool pooled) {
#pragma clang fp contract(off)
    const float keep = (1.0f - alpha) * mu;
    return pooled ? fmaf(mean, alpha, keep) : mean * alpha + keep;
}
__global__ void __launch_bounds__(256) l2a_cem_stats_k(const float* a_clip, const int* elite_rows, int m, int D, int k,
                                                       int reference, float alpha, float* mean, float* std) {
    __shared__ int rows[L2A_CEM_MAXROWS];
    __shared__ float part[8][33];
    const int dl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int d = blockIdx.x * 32 + dl;
    const int grp = blockIdx.y;
    const int cnt = reference ? m * k : k;
    const int* src = reference ? elite_rows : elite_rows + grp * k;
    for (int q = threadIdx.x; q < cnt; q += 256) rows[q] = src[q];
    __syncthreads();
    const bool live = d < D;
    const float* col = a_clip + (live ? d : 0);
    float mu = 0.0f, sd = 0.0f;
    for (int pass = 0; pass < 2; ++pass) {
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        int q = sl;
        for (; q + 24 < cnt; q += 32) {
            const float x0 = col[(long long)rows[q] * D], x1 = col[(long long)rows[q + 8] * D];
            const float x2 = col[(long long)rows[q + 16] * D], x3 = col[(long long)rows[q + 24] * D];
            if (pass == 0) { s0 += x0; s1 += x1; s2 += x2; s3 += x3; }
            else { s0 = fmaf(x0 - mu, x0 - mu, s0); s1 = fmaf(x1 - mu, x1 - mu, s1);
                   s2 = fmaf(x2 - mu, x2 - mu, s2); s3 = fmaf(x3 - mu, x3 - mu, s3); }
        }
        for (; q < cnt; q += 8) {
            const float x0 = col[(long long)rows[q] * D];
            if (pass == 0) s0 += x0; else s0 = fmaf(x0 - mu, x0 - mu, s0);
        }
        part[sl][dl] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        float tot = 0.0f;
#pragma unroll
        for (int w = 0; w < 8; ++w) tot += part[w][dl];
        __syncthreads();
        if (pass == 0) mu = tot / (float)cnt; else sd = sqrtf(tot / (float)cnt);
    }
    if (!live || sl != 0) return;
    if (reference) {
        for (int i = 0; i < m; ++i) {
            mean[i * D + d] = cem_mean_update(mean[i * D + d], alpha, mu, true);
            std[i * D + d] = sd;
        }
    } else {
        mean[grp * D + d] = cem_mean_update(mean[grp * D + d], alpha, mu, false);
        std[grp * D + d] = sd;
    }
}

// ---- l2a_cem_refit_sample_k: iteration i's returns -> iteration i + 1's candidates in ONE launch ---------------------------------
// Workgroup (t, s, grp): horizon step t, candidate slice s, statistics group grp (all envs pooled = 1 group in the reference's
// reading, one env per group in the fixed one).  Every workgroup ranks its group's returns itself (no inter-workgroup traffic, no
// wait), owns the act_dim dimensions of step t - their elite statistics, redundantly per slice - and writes the samples of those
// dimensions for candidates [s n / S, (s + 1) n / S) of its envs.  Bit-identical to l2a_cem_rank_k + l2a_cem_stats_k +
// l2a_cem_sample_k:
//   rank  : the same stable descending order (NaN -> -inf, ties to the lower index) without the n x k comparisons of the counting
//           rank - the returns are binned by value (a monotone map: a higher bin holds only smaller values), the rank of j is the
//           population of the bins above its own plus an exact count inside its bin (ties, however many, are compared one by one)
//   stats : the elite rows' values of step t are staged in LDS once, then summed in l2a_cem_stats_k's order exactly (8 row slices,
//           four accumulators at +8 / +16 / +24, slice totals added w = 0..7, two passes)
//   sample: l2a_cem_sample_k's arithmetic and Philox numbering on the new mean / std held in LDS
// Slices (S > 1) read the previous mean and a_clip from buffers the launch does not write (the entry point takes S = 1 when they alias).
#define L2A_CRS_THREADS 512
#define L2A_CRS_BINS 2048

struct CemRefitSampleParams {
    const float* returns;       // [m, n]
    const float* a_clip_in;     // [n, m, D]: the samples whose returns these are
    const float* mean_in;       // [m, D]: the mean they were drawn with
    const float* z;             // [n, m, D] or null (Philox)
    unsigned long long seed, offset;
    const float* low;
    const float* high;
    int n, m, h, act_dim, k, reference, lo, hi, slices;
    float alpha;
    int* elite_rows;            // [m * k] (written by the slice-0 workgroups of step 0)
    float* mean;                // [m, D]
    float* std;
    float* a_clip;              // [n, m, D]
    float* a_raw;               // [n, m, D] or null
    float* seq;                 // [h, m * (hi - lo), act_dim] or null
};

// descending bin of a value: 0 holds the largest; monotone (v1 < v2 => bin(v1) >= bin(v2)), equal values share a bin
__device__ __forceinline__ int crs_bin(float v, float vmin, float scale) {
    if (v == __builtin_inff()) return 0;
    if (v == -__builtin_inff()) return L2A_CRS_BINS - 1;
    const float t = (v - vmin) * scale;
    const int b = (t > 0.0f) ? (t < (float)(L2A_CRS_BINS - 1) ? (int)t : L2A_CRS_BINS - 1) : 0;
    return L2A_CRS_BINS - 1 - b;
}

__global__ void __launch_bounds__(L2A_CRS_THREADS) l2a_cem_refit_sample_k(const CemRefitSampleParams p) {
    extern __shared__ int crs_lds[];
    const int tid = threadIdx.x;
    const int t = blockIdx.x, s = blockIdx.y, grp = blockIdx.z;
    const int n = p.n, m = p.m, k = p.k, A = p.act_dim, D = p.h * A;
    const int gm = p.reference ? m : 1;                 // envs of this statistics group
    const int cnt = gm * k;                             // elite rows of the group
    int* rows = crs_lds;                                // [cnt]
    float* nm = reinterpret_cast<float*>(rows + cnt);   // [gm, A] the group's new mean of step t
    float* ns = nm + gm * A;                            // [A]
    float* part = ns + A;                               // [8, A]
    float* red = part + 8 * A;                          // [4 * 8] wave minima / maxima
    int* sc = reinterpret_cast<int*>(red + 32);         // [L2A_CRS_THREADS] scan
    float* vals = reinterpret_cast<float*>(sc + L2A_CRS_THREADS);   // union: [n] returns | [n] bin lists | bins | fill
    int* list = reinterpret_cast<int*>(vals + n);
    int* start = list + n;                              // [BINS]
    int* fill = start + L2A_CRS_BINS;                   // [BINS]
    float* E = vals;                                    // union: [cnt, A] elite values of step t
    const int lane = tid & 63, wv = tid >> 6;

    for (int q = tid; q < cnt; q += L2A_CRS_THREADS) rows[q] = 0;       // (every entry is written below; never a stray row id)
    for (int ii = 0; ii < gm; ++ii) {
        const int i = p.reference ? ii : grp;
        // finite minimum / maximum (the bins) and minimum / maximum of everything above -inf (one tie class?)
        float lmin = __builtin_inff(), lmax = -__builtin_inff(), umin = __builtin_inff(), umax = -__builtin_inff();
        int lninf = 0;
        for (int c = tid; c < n; c += L2A_CRS_THREADS) {
            float x = p.returns[(long long)i * n + c];
            x = (x != x) ? -__builtin_inff() : x;       // l2a_cem_rank_k: NaN sorts last
            vals[c] = x;
            if (x == -__builtin_inff()) lninf = 1;
            else {
                umin = fminf(umin, x); umax = fmaxf(umax, x);
                if (x != __builtin_inff()) { lmin = fminf(lmin, x); lmax = fmaxf(lmax, x); }
            }
        }
        for (int b = tid; b < L2A_CRS_BINS; b += L2A_CRS_THREADS) fill[b] = 0;
        for (int o = 32; o >= 1; o >>= 1) {
            lmin = fminf(lmin, __shfl_xor(lmin, o)); lmax = fmaxf(lmax, __shfl_xor(lmax, o));
            umin = fminf(umin, __shfl_xor(umin, o)); umax = fmaxf(umax, __shfl_xor(umax, o));
        }
        if (lane == 0) { red[wv] = lmin; red[8 + wv] = lmax; red[16 + wv] = umin; red[24 + wv] = umax; }
        const bool any_ninf = __syncthreads_or(lninf) != 0;
        float vmin = red[0], vmax = red[8], wmin = red[16], wmax = red[24];
        for (int w = 1; w < L2A_CRS_THREADS / 64; ++w) {
            vmin = fminf(vmin, red[w]); vmax = fmaxf(vmax, red[8 + w]); wmin = fminf(wmin, red[16 + w]); wmax = fmaxf(wmax, red[24 + w]);
        }
        // every value above -inf equal (a constant reward) - or none (every rollout diverged): no bins needed at all
        const bool uniform = !(wmin < wmax);
        // Ties of the two classes degenerate returns are made of, ranked by index order without comparisons: the -inf values
        // (diverged rollouts) sort after everything else, and in a uniform env everything above -inf is one tie.  Each thread
        // walks a contiguous index range; an exclusive scan of the ranges' class counts gives each range its first ranks.
        if (uniform || any_ninf) {
            const int per = (n + L2A_CRS_THREADS - 1) / L2A_CRS_THREADS;
            const int c0 = tid * per < n ? tid * per : n, c1 = (tid + 1) * per < n ? (tid + 1) * per : n;
            int ninf = 0;
            for (int c = c0; c < c1; ++c) ninf += (vals[c] == -__builtin_inff()) ? 1 : 0;
            const int packed = ninf | ((c1 - c0 - ninf) << 16);         // (n < 65536: n floats fit a workgroup's LDS)
            sc[tid] = packed;
            __syncthreads();
            for (int o = 1; o < L2A_CRS_THREADS; o <<= 1) {
                const int add = tid >= o ? sc[tid - o] : 0;
                __syncthreads();
                sc[tid] += add;
                __syncthreads();
            }
            const int above = sc[L2A_CRS_THREADS - 1] >> 16;           // values above -inf in the env
            int ra = above + ((sc[tid] - packed) & 0xffff), rb = (sc[tid] - packed) >> 16;
            __syncthreads();
            for (int c = c0; c < c1; ++c) {
                int rank = -1;
                if (vals[c] == -__builtin_inff()) rank = ra++;
                else if (uniform) rank = rb++;
                if (rank < 0) continue;
                if (p.reference) { if (c < k) rows[ii * k + c] = rank * m + i; }   // position rank_i(c) of env i is an elite (:101)
                else if (rank < k) rows[rank] = c * m + i;                         // candidate c is among env i's top k
            }
        }
        if (!uniform) {         // the values above -inf: value bins, and an exact count inside the bin
            const float range = vmax - vmin;            // (no finite value: -inf, scale 0 - one bin, still exact)
            const float scale = (range > 0.0f) ? (float)(L2A_CRS_BINS - 1) / range : 0.0f;
            for (int c = tid; c < n; c += L2A_CRS_THREADS)
                if (vals[c] != -__builtin_inff()) atomicAdd(&fill[crs_bin(vals[c], vmin, scale)], 1);
            __syncthreads();
            // exclusive scan of the bin populations: 4 bins per thread, Hillis-Steele over the threads
            constexpr int PER = L2A_CRS_BINS / L2A_CRS_THREADS;
            int loc[PER], run = 0;
#pragma unroll
            for (int q = 0; q < PER; ++q) { loc[q] = run; run += fill[tid * PER + q]; }
            sc[tid] = run;
            __syncthreads();
            for (int o = 1; o < L2A_CRS_THREADS; o <<= 1) {
                const int add = tid >= o ? sc[tid - o] : 0;
                __syncthreads();
                sc[tid] += add;
                __syncthreads();
            }
            const int base = sc[tid] - run;
#pragma unroll
            for (int q = 0; q < PER; ++q) { start[tid * PER + q] = base + loc[q]; fill[tid * PER + q] = base + loc[q]; }
            __syncthreads();
            for (int c = tid; c < n; c += L2A_CRS_THREADS)
                if (vals[c] != -__builtin_inff()) list[atomicAdd(&fill[crs_bin(vals[c], vmin, scale)], 1)] = c;
            __syncthreads();
            // rank of j = candidates that sort before it: every one in a higher bin, and the ones of its own bin that do
            const int work = p.reference ? k : n;
            for (int j = tid; j < work; j += L2A_CRS_THREADS) {
                const float v = vals[j];
                if (v == -__builtin_inff()) continue;   // (ranked above)
                const int b = crs_bin(v, vmin, scale);
                const int b0 = start[b], b1 = fill[b];  // (after the scatter fill[b] is the bin's end)
                int rank = b0;
                for (int q = b0; q < b1; ++q) {
                    const int c = list[q];
                    const float w = vals[c];
                    rank += (w > v || (w == v && c < j)) ? 1 : 0;
                }
                if (p.reference) rows[ii * k + j] = rank * m + i;     // position rank_i(j) of env i is an elite (:101)
                else if (rank < k) rows[rank] = j * m + i;            // candidate j is among env i's top k
            }
        }
        __syncthreads();
    }
    if (t == 0 && s == 0)
        for (int q = tid; q < cnt; q += L2A_CRS_THREADS) p.elite_rows[(p.reference ? 0 : grp * k) + q] = rows[q];
    // the elite rows' values of step t, once
    for (int e = tid; e < cnt * A; e += L2A_CRS_THREADS) {
        const int q = e / A, kk = e - q * A;
        E[e] = p.a_clip_in[(long long)rows[q] * D + t * A + kk];
    }
    __syncthreads();
    const bool st = tid < 8 * A;
    const int sl = st ? tid / A : 0, kk0 = st ? tid - sl * A : 0;
    float mu = 0.0f, sd = 0.0f;
    for (int pass = 0; pass < 2; ++pass) {
        if (st) {
            const float* col = E + kk0;
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
            int q = sl;
            for (; q + 24 < cnt; q += 32) {
                const float x0 = col[q * A], x1 = col[(q + 8) * A];
                const float x2 = col[(q + 16) * A], x3 = col[(q + 24) * A];
                if (pass == 0) { s0 += x0; s1 += x1; s2 += x2; s3 += x3; }
                else { s0 = fmaf(x0 - mu, x0 - mu, s0); s1 = fmaf(x1 - mu, x1 - mu, s1);
                       s2 = fmaf(x2 - mu, x2 - mu, s2); s3 = fmaf(x3 - mu, x3 - mu, s3); }
            }
            for (; q < cnt; q += 8) {
                const float x0 = col[q * A];
                if (pass == 0) s0 += x0; else s0 = fmaf(x0 - mu, x0 - mu, s0);
            }
            part[sl * A + kk0] = (s0 + s1) + (s2 + s3);
        }
        __syncthreads();
        if (st) {
            float tot = 0.0f;
#pragma unroll
            for (int w = 0; w < 8; ++w) tot += part[w * A + kk0];
            if (pass == 0) mu = tot / (float)cnt; else sd = sqrtf(tot / (float)cnt);
        }
        __syncthreads();
    }
    if (st && sl == 0) {
        const int d = t * A + kk0;
        for (int ii = 0; ii < gm; ++ii) {
            const int i = p.reference ? ii : grp;
            const float nmv = cem_mean_update(p.mean_in[i * D + d], p.alpha, mu, p.reference != 0);
            nm[ii * A + kk0] = nmv;
            if (s == 0) { p.mean[i * D + d] = nmv; p.std[i * D + d] = sd; }
        }
        ns[kk0] = sd;
    }
    __syncthreads();
    // the samples of step t for this slice's candidates (l2a_cem_sample_k)
    const int j0 = (int)((long long)s * n / p.slices), j1 = (int)((long long)(s + 1) * n / p.slices);
    const int total = (j1 - j0) * gm * A;
    for (int w = tid; w < total; w += L2A_CRS_THREADS) {
        const int kk = w % A, r = w / A;
        const int ii = r % gm, j = j0 + r / gm;
        const int i = p.reference ? ii : grp;
        const long long g = (long long)j * m + i;
        const int d = t * A + kk;
        const long long e = g * D + d;
        const float z = p.z ? p.z[e] : l2a_philox_normal(p.seed, p.offset + (unsigned long long)e);
        const float a = nm[ii * A + kk] + z * ns[kk];                                 // :86
        const float c = fminf(fmaxf(a, p.low[kk]), p.high[kk]);                         // :87
        p.a_clip[e] = c;
        if (p.a_raw) p.a_raw[e] = a;
        if (p.seq) {
            const long long prow = p.reference ? g : (long long)i * n + j;
            const long long cand = prow % n, blk = prow / n;
            if (cand >= p.lo && cand < p.hi) {
                const long long nsel = p.hi - p.lo;
                p.seq[((long long)t * (m * nsel) + blk * nsel + (cand - p.lo)) * A + kk] = p.reference ? a : c;
            }
        }
    }
}

// LDS bytes of one l2a_cem_refit_sample_k workgroup
size_t crs_lds_bytes(int n, int m, int k, int act_dim, int reference) {
    const size_t gm = reference ? (size_t)m : 1, cnt = gm * (size_t)k;
    const size_t fixed = cnt + gm * act_dim + act_dim + 8 * (size_t)act_dim + 32 + L2A_CRS_THREADS;
    const size_t bins = 2 * (size_t)n + 2 * L2A_CRS_BINS, elite = cnt * (size_t)act_dim;
    return 4 * (fixed + (bins > elite ? bins : elite));
}

// LDS the kernel holds besides its dynamic array: __syncthreads_or's workgroup-reduction scratch (64 ints, the object's
// group_segment_fixed_size).  Without it in the budget the shapes within 256 bytes of the limit (m = 1, h = 2, act_dim = 2,
// k = n / 10: n = 17256 .. 17286) were taken as fused and failed in hipFuncSetAttribute instead of falling back.
#define L2A_CRS_STATIC_LDS 256

// Does l2a_cem_refit_sample run this shape as one launch (else: l2a_cem_refit + l2a_cem_sample inside the call)?
bool crs_fused(const l2a_ctx* ctx, int n, int m, int h, int act_dim, int k, int reference) {
    const long long total = (long long)n * m * h * act_dim;
    return crs_lds_bytes(n, m, k, act_dim, reference) + L2A_CRS_STATIC_LDS <= (size_t)ctx->lds_per_block &&
           8 * act_dim <= L2A_CRS_THREADS && total <= 0x7fffffffLL;
}

// the dynamic-LDS limit l2a_cem_refit_sample_k has been raised to, per device
#define L2A_CRS_DEVICES 64
std::atomic<int> crs_smem_set[L2A_CRS_DEVICES];

// np.argmax's order (the reference's `np.argmax(returns, axis=1)`, mpc_controller.py:128-129): a NaN is the maximum, the first
// NaN wins; otherwise the largest value, ties to the lowest index.  A diverged rollout therefore surfaces as a NaN best return
// exactly as it does in the reference, instead of a finite-looking action.
__device__ __forceinline__ bool l2a_argmax_better(float x, int c, float best, int idx) {
    const bool xn = x != x, bn = best != best;
    if (xn != bn) return xn;
    if (xn) return c < idx;
    return x > best || (x == best && c < idx);
}

// The plan's result in ONE buffer (one read-back instead of five launches and five copies): per env the arg-max of its
// returns (np.argmax's order, NaN included), the first action of that candidate as the rollout saw it, its return; behind them
// the final mean / std.
// out: [m][act_dim + 2] floats (action | return | index as the bit pattern of an int32), then mean [m, D], std [m, D].
// act_out (nullable): the winners' first actions once more as a dense [m, act_dim] - what l2a_lstm_advance reads (the same bits).
// grid (m + ceil(2 m D / 256)): block i < m is env i.
__global__ void __launch_bounds__(256) l2a_cem_pick_k(const float* returns, const float* cand, const float* mean, const float* std,
                                                      int n, int m, int D, int act_dim, int reference, float* out, float* act_out) {
    const int W = act_dim + 2;
    if ((int)blockIdx.x >= m) {
        const long long e = (long long)(blockIdx.x - m) * 256 + threadIdx.x;
        const long long md = (long long)m * D;
        if (e < 2 * md) out[(long long)m * W + e] = (e < md) ? mean[e] : std[e - md];
        return;
    }
    const int i = blockIdx.x;
    __shared__ float bv[256];
    __shared__ int bi[256];
    float best = -__builtin_inff();
    int idx = 0x7fffffff;
    for (int c = threadIdx.x; c < n; c += 256) {
        const float x = returns[(long long)i * n + c];
        if (l2a_argmax_better(x, c, best, idx)) { best = x; idx = c; }
    }
    bv[threadIdx.x] = best; bi[threadIdx.x] = idx;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const float x = bv[threadIdx.x + s]; const int c = bi[threadIdx.x + s];
            if (l2a_argmax_better(x, c, bv[threadIdx.x], bi[threadIdx.x])) { bv[threadIdx.x] = x; bi[threadIdx.x] = c; }
        }
        __syncthreads();
    }
    int j = bi[0];
    if (j < 0 || j >= n) j = 0;                         // (all returns NaN / -inf)
    // reference: the sample memory read as [m, n, D] (:92-96), row i * n + j; fixed: candidate j of env i is sample row j * m + i
    const long long row = reference ? (long long)i * n + j : (long long)j * m + i;
    if ((int)threadIdx.x < act_dim) {
        const float a = cand[row * D + threadIdx.x];
        out[i * W + threadIdx.x] = a;
        if (act_out) act_out[i * act_dim + threadIdx.x] = a;
    }
    if (threadIdx.x == 0) { out[i * W + act_dim] = returns[(long long)i * n + j]; out[i * W + act_dim + 1] = __int_as_float(j); }
}


// ---- sharded CEM: every rank's returns of one iteration gathered by the plan's ONE collective kind, the int64 MAX all-reduce ------
// A rank contributes m * n + 3 words: word i * n + j = (1 << 32) | the RAW bits of its return of env i's candidate j when it owns
// j (lo <= j < hi), else 0 - only the owner's word is non-zero, so MAX hands it to every rank exactly (NaN payloads, -0.0, +-inf
// included; every word is below 2^33, so a signed MAX reduces them alike); behind them [launch flag | digest | MASK - digest] as
// l2a_plan_payload_k packs them.
#define L2A_CEM_WORD_PRESENT (1ull << 32)

// One launch writes ALL m * n + 3 words (zeros outside the shard: no memset in front).  returns_local [m, hi - lo].
__global__ void __launch_bounds__(256) l2a_cem_shard_pack_k(const float* __restrict__ returns_local, int m, int n, int lo, int hi,
                                                            const unsigned int* status, unsigned long long digest,
                                                            unsigned long long* __restrict__ words) {
    const long long total = (long long)m * n;
    const int n_local = hi - lo;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int i = (int)(e / n), j = (int)(e - (long long)i * n);
        unsigned long long w = 0ull;
        if (j >= lo && j < hi) w = L2A_CEM_WORD_PRESENT | (unsigned long long)__float_as_uint(returns_local[(long long)i * n_local + (j - lo)]);
        words[e] = w;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the status word lives in host-mapped memory; the rollout in front ORed into it with system scope and has completed
        const unsigned int st = __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned long long d = digest & L2A_DIGEST_MASK;
        words[total] = st ? 1ull : 0ull;
        words[total + 1] = d;
        words[total + 2] = L2A_DIGEST_MASK - d;
    }
}

// One launch decodes the reduced words into the fp32 table [m, n] the refit and the pick read, and ACCUMULATES into verdict [3]:
// [0] |= any rank's flag, [1] += zero words ("holes": a candidate nobody contributed, decoded as 0.0f), [2] |= the digest pair
// does not add up (ranks built differently, or out of step).
__global__ void __launch_bounds__(256) l2a_cem_shard_unpack_k(const unsigned long long* __restrict__ words, int m, int n,
                                                              float* __restrict__ returns_out, unsigned int* verdict) {
    const long long total = (long long)m * n;
    int holes = 0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const unsigned long long w = words[e];
        holes += (w == 0ull) ? 1 : 0;
        returns_out[e] = (w == 0ull) ? 0.0f : __uint_as_float((unsigned int)w);
    }
    for (int o = 32; o >= 1; o >>= 1) holes += __shfl_xor(holes, o);
    if ((threadIdx.x & 63) == 0 && holes > 0) atomicAdd(&verdict[1], (unsigned int)holes);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (words[total] != 0ull) atomicOr(&verdict[0], 1u);
        if (words[total + 1] + words[total + 2] != L2A_DIGEST_MASK) atomicOr(&verdict[2], 1u);
    }
}

// workgroups of the two launches above: a grid-stride loop, at most four workgroups per CU
unsigned cem_shard_blocks(const l2a_ctx* ctx, long long total) {
    const long long want = (total + 255) / 256, most = 4LL * (ctx->num_cu > 0 ? ctx->num_cu : 256);
    return (unsigned)(want < 1 ? 1 : (want < most ? want : most));
}

}  // namespace

extern "C" {

int l2a_cem_sample(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean,
                   const float* std, const float* low, const float* high, int n, int m, int h, int act_dim,
                   int reference, int lo, int hi, float* a_clip, float* a_raw, float* seq, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if (!mean || !std || !low || !high || !a_clip) return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_sample: null pointer");
    if (n < 1 || m < 1 || h < 1 || act_dim < 1 || lo < 0 || hi < lo || hi > n)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_sample: bad n / m / h / act_dim / shard");
    const long long total = (long long)n * m * h * act_dim;
    if (total > 0x7fffffffLL * 256) return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_sample: too many samples");
    l2a_device_guard guard(ctx->device);
    CemSampleParams p;
    std::memset(&p, 0, sizeof(p));
    p.z = z; p.seed = seed; p.offset = offset; p.mean = mean; p.std = std; p.low = low; p.high = high;
    p.n = n; p.m = m; p.h = h; p.act_dim = act_dim; p.reference = reference ? 1 : 0; p.lo = lo; p.hi = hi;
    p.a_clip = a_clip; p.a_raw = a_raw; p.seq = (hi > lo) ? seq : nullptr;
    hipLaunchKernelGGL(l2a_cem_sample_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream_v), p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

int l2a_cem_refit(l2a_ctx* ctx, const float* returns, const float* a_clip, int n, int m, int D, int num_elites,
                  int reference, float alpha, int* elite_rows, float* mean, float* std, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if (!returns || !a_clip || !elite_rows || !mean || !std) return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_refit: null pointer");
    if (n < 1 || m < 1 || D < 1 || num_elites < 1 || num_elites > n)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_refit: bad n / m / D / num_elites");
    if ((long long)(reference ? m : 1) * num_elites > L2A_CEM_MAXROWS)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_refit: more than 8192 elite rows per statistics group");
    if ((size_t)n * sizeof(float) > (size_t)ctx->lds_per_block)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_refit: more candidates than an env's returns fit in LDS");
    l2a_device_guard guard(ctx->device);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    const int smem = n * (int)sizeof(float);
    if (smem > 48 * 1024)
        L2A_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_cem_rank_k),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    const int work = reference ? num_elites : n;
    const int blocks = (work + 3) / 4 < 256 ? (work + 3) / 4 : 256;      // one wave per rank, at most 1024 waves per env
    hipLaunchKernelGGL(l2a_cem_rank_k, dim3((unsigned)blocks, (unsigned)m), dim3(256), smem, stream, returns,
                       n, m, num_elites, reference ? 1 : 0, elite_rows);
    hipLaunchKernelGGL(l2a_cem_stats_k, dim3((unsigned)((D + 31) / 32), (unsigned)(reference ? 1 : m)), dim3(256), 0,
                       stream, a_clip, elite_rows, m, D, num_elites, reference ? 1 : 0, alpha, mean, std);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

int l2a_cem_refit_sample(l2a_ctx* ctx, const float* returns, const float* a_clip_in, int n, int m, int h, int act_dim, int num_elites,
                         int reference, float alpha, const float* z, unsigned long long seed, unsigned long long offset, const float* low,
                         const float* high, int lo, int hi, int* elite_rows, const float* mean_in, float* mean, float* std, float* a_clip,
                         float* a_raw, float* seq, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if (!returns || !a_clip_in || !elite_rows || !mean || !std || !low || !high || !a_clip)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_refit_sample: null pointer");
    if (n < 1 || m < 1 || h < 1 || act_dim < 1 || lo < 0 || hi < lo || hi > n || num_elites < 1 || num_elites > n)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_refit_sample: bad n / m / h / act_dim / num_elites / shard");
    if ((long long)(reference ? m : 1) * num_elites > L2A_CEM_MAXROWS)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_refit_sample: more than 8192 elite rows per statistics group");
    if ((size_t)n * sizeof(float) > (size_t)ctx->lds_per_block)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_refit_sample: more candidates than an env's returns fit in LDS");
    if (!mean_in) mean_in = mean;
    l2a_device_guard guard(ctx->device);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    const size_t smem = crs_lds_bytes(n, m, num_elites, act_dim, reference);
    if (!crs_fused(ctx, n, m, h, act_dim, num_elites, reference)) {
        // shapes the fused launch does not take: the two calls it replaces (same bits)
        if (mean_in != mean)
            L2A_HIP(ctx, hipMemcpyAsync(mean, mean_in, sizeof(float) * (size_t)m * h * act_dim, hipMemcpyDeviceToDevice, stream));
        int rc = l2a_cem_refit(ctx, returns, a_clip_in, n, m, h * act_dim, num_elites, reference, alpha, elite_rows, mean, std, stream_v);
        if (rc != L2A_OK) return rc;
        return l2a_cem_sample(ctx, z, seed, offset, mean, std, low, high, n, m, h, act_dim, reference, lo, hi, a_clip, a_raw, seq,
                              stream_v);
    }
    const int groups = reference ? 1 : m;
    // candidate slices: about one workgroup per CU; in place (the previous mean or samples are overwritten) one slice
    int slices = 1;
    if (mean_in != mean && a_clip_in != a_clip) {
        const int cus = ctx->num_cu > 0 ? ctx->num_cu : 256;
        slices = l2a_ceil_div(cus, h * groups);
        const int most = n / 64 > 1 ? n / 64 : 1;
        slices = slices < most ? slices : most;
        slices = slices > 1 ? slices : 1;
    }
    if (smem > 48 * 1024 && ctx->device >= 0 && ctx->device < L2A_CRS_DEVICES && (int)smem > crs_smem_set[ctx->device].load()) {
        // raised once per device to the largest size launched so far (a race between two threads only repeats the call)
        L2A_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_cem_refit_sample_k),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        crs_smem_set[ctx->device].store((int)smem);
    } else if (smem > 48 * 1024 && (ctx->device < 0 || ctx->device >= L2A_CRS_DEVICES)) {
        L2A_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_cem_refit_sample_k),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    }
    CemRefitSampleParams p;
    std::memset(&p, 0, sizeof(p));
    p.returns = returns; p.a_clip_in = a_clip_in; p.mean_in = mean_in; p.z = z; p.seed = seed; p.offset = offset;
    p.low = low; p.high = high; p.n = n; p.m = m; p.h = h; p.act_dim = act_dim; p.k = num_elites; p.reference = reference ? 1 : 0;
    p.lo = lo; p.hi = hi; p.slices = slices; p.alpha = alpha; p.elite_rows = elite_rows; p.mean = mean; p.std = std;
    p.a_clip = a_clip; p.a_raw = a_raw; p.seq = (hi > lo) ? seq : nullptr;
    hipLaunchKernelGGL(l2a_cem_refit_sample_k, dim3((unsigned)h, (unsigned)slices, (unsigned)groups), dim3(L2A_CRS_THREADS),
                       (unsigned)smem, stream, p);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

int l2a_cem_refit_sample_fused(const l2a_ctx* ctx, int n, int m, int h, int act_dim, int num_elites, int reference) {
    if (!ctx || n < 1 || m < 1 || h < 1 || act_dim < 1 || num_elites < 1 || num_elites > n) return 0;
    return crs_fused(ctx, n, m, h, act_dim, num_elites, reference) ? 1 : 0;
}

// Both picks: `act_out` null is l2a_cem_pick.
static int cem_pick(const char* who, l2a_ctx* ctx, const float* returns, const float* cand, const float* mean, const float* std, int n,
                    int m, int D, int act_dim, int reference, float* out, float* act_out, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if (!returns || !cand || !mean || !std || !out) return l2a_fail(ctx, L2A_EINVAL, std::string(who) + ": null pointer");
    if (n < 1 || m < 1 || D < 1 || act_dim < 1 || act_dim > D || act_dim > 256)
        return l2a_fail(ctx, L2A_EINVAL, std::string(who) + ": bad n / m / D / act_dim");
    l2a_device_guard guard(ctx->device);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    const long long copy_blocks = (2LL * m * D + 255) / 256;
    hipLaunchKernelGGL(l2a_cem_pick_k, dim3((unsigned)(m + copy_blocks)), dim3(256), 0, stream, returns, cand, mean, std, n, m, D,
                       act_dim, reference ? 1 : 0, out, act_out);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

int l2a_cem_pick(l2a_ctx* ctx, const float* returns, const float* cand, const float* mean, const float* std, int n, int m, int D,
                 int act_dim, int reference, float* out, void* stream_v) {
    return cem_pick("l2a_cem_pick", ctx, returns, cand, mean, std, n, m, D, act_dim, reference, out, nullptr, stream_v);
}

int l2a_cem_pick_act(l2a_ctx* ctx, const float* returns, const float* cand, const float* mean, const float* std, int n, int m, int D,
                     int act_dim, int reference, float* out, float* act_out, void* stream_v) {
    if (ctx && !act_out) return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_pick_act: null act_out");
    return cem_pick("l2a_cem_pick_act", ctx, returns, cand, mean, std, n, m, D, act_dim, reference, out, act_out, stream_v);
}


unsigned long long l2a_cem_word_encode(float ret) {
    unsigned int bits = 0;
    std::memcpy(&bits, &ret, sizeof(bits));
    return L2A_CEM_WORD_PRESENT | (unsigned long long)bits;
}

int l2a_cem_word_decode(unsigned long long word, float* ret) {
    const unsigned int bits = word ? (unsigned int)word : 0u;      // an absent word decodes as 0.0f, like the kernel
    if (ret) std::memcpy(ret, &bits, sizeof(bits));
    return word ? 1 : 0;
}

int l2a_cem_shard_pack(l2a_ctx* ctx, const float* returns_local, int m, int n, int lo, int hi, unsigned long long digest,
                       unsigned long long* words_out, void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if (m < 1 || n < 1 || lo < 0 || hi < lo || hi > n) return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_shard_pack: bad m / n / shard");
    if (!words_out || (hi > lo && !returns_local)) return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_shard_pack: null pointer");
    if ((long long)m * n > 0x3fffffffLL) return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_shard_pack: too many candidates");
    l2a_device_guard guard(ctx->device);
    hipLaunchKernelGGL(l2a_cem_shard_pack_k, dim3(cem_shard_blocks(ctx, (long long)m * n)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream_v), returns_local, m, n, lo, hi, ctx->status_dev, digest, words_out);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

int l2a_cem_shard_unpack(l2a_ctx* ctx, const unsigned long long* words, int m, int n, float* returns_out, unsigned int* verdict,
                         void* stream_v) {
    if (!ctx) return L2A_EINVAL;
    if (m < 1 || n < 1 || (long long)m * n > 0x3fffffffLL) return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_shard_unpack: bad m / n");
    if (!words || !returns_out || !verdict) return l2a_fail(ctx, L2A_EINVAL, "l2a_cem_shard_unpack: null pointer");
    l2a_device_guard guard(ctx->device);
    hipLaunchKernelGGL(l2a_cem_shard_unpack_k, dim3(cem_shard_blocks(ctx, (long long)m * n)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream_v), words, m, n, returns_out, verdict);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

}  // extern "C"
