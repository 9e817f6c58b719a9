// l2a_step.hip - the controller step as ONE C-ABI call (include/l2a.h: l2a_controller_*).
//
// What `MPCController.get_actions` (policies/mpc_controller.py:59-69,108-129) and `RNNMPCController.get_actions`
// (policies/rnn_mpc_controller.py:57-65,112-134) are to their caller in parity mode: float64 observations in, the float64 first
// action of the best candidate out, NumPy's global generator left exactly where the reference's own draw leaves it.  Until
// round 5 the pieces of a step were glued together in Python (a Condition shared with a worker thread under the GIL for the
// candidates drawn ahead, ~10 ctypes / torch calls around the launch): ~0.1 ms per call beside a 0.18 - 1.4 ms kernel.  Here:
//   take   the block of candidates the chain of csrc/l2a_rng.c drew (and this file's callback uploaded) while the previous plan
//          ran - adopted only if the global generator's words are still the state the block started from
//   launch the fused rollout from host-mapped observations (l2a_plan_rs_sync's path; recurrent: + the state advance)
//   kick   the producer of the next block (between launch and wait)
//   wait   for the mailbox word, decode the keys, gather the winners' float64 first actions from the block's `cand_a`
// When no valid block is waiting (first call, a foreign consumer of np.random between two steps) the step draws the candidates
// itself - the reference's draw from the GLOBAL generator, on the helper's threads, into the idle slot, uploaded on the launch
// stream in front of the kernel - and re-arms the chain behind that draw (L2A_STEP_DREW); while steps keep missing it re-arms only
// every 16th step (every block drawn ahead would be thrown away).  L2A_STEP_MISS is left for a controller that cannot serve the
// call at all (a forked child: its producer thread and its HIP state did not come along).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "l2a_host.h"
#include "l2a_philox.h"
#include "l2a_rng.h"


// One allocation of a controller (`alloc`): l2a_controller_destroy walks the record.
enum mem_kind { MEM_DEVICE, MEM_PINNED, MEM_MAPPED, MEM_HEAP };
struct owned_mem { void* ptr; mem_kind kind; };

struct l2a_controller {
    // ---- the plan ----
    l2a_ctx* ctx = nullptr;
    l2a_model* mlp = nullptr;
    l2a_lstm* rnn = nullptr;
    int m = 0, n = 0, h = 0, obs_dim = 0, act_dim = 0;
    double discount = 1.0;
    l2a_reward rw;
    double low[16], high[16];
    // ---- what the controller owns: every buffer (`alloc`), the event behind a step's read-back, the producer's stream ----
    std::vector<owned_mem> mem;
    hipError_t mem_err = hipSuccess;            // the first failure of `alloc` / `upload`: every later one does nothing
    hipEvent_t done = nullptr;                  // sharded and CEM steps: the step's words have landed in page-locked memory
    // ---- the candidates ----
    size_t act_floats = 0;                      // this rank's candidate tensor [h, m * (hi - lo), act_dim]
    size_t glob_floats = 0;                     // h * m * n * act_dim: the WHOLE plan's candidate tensor (the device stream's step)
    float* dev[2] = {nullptr, nullptr};         // the tensor in HBM (what the rollout reads); device RNG: dev[0] only
    int slot = -1;                              // block of the latest successful step
    // parity mode: the candidates come from NumPy's global generator, drawn ahead by the chain of csrc/l2a_rng.c
    struct {
        void* np_addr = nullptr;
        int rng_threads = 1;
        float* pin[2] = {nullptr, nullptr};     // page-locked staging of the fp32 candidate tensor
        double* c64[2] = {nullptr, nullptr};    // float64 `cand_a` = the first horizon step's rows [m * n, act_dim]
        // sharded RECURRENT plan: the whole plan's first horizon step as fp32 [m * n, act_dim] - the cast of c64[slot] the candidate
        // tensor gets - so that the state advance behind the collective finds the GLOBAL winner's first action on the device
        float* tab_pin[2] = {nullptr, nullptr};
        float* tab_dev[2] = {nullptr, nullptr};
        hipStream_t side = nullptr;             // the producer's upload stream
        l2a_ahead* chain = nullptr;
        bool producer_bound = false;            // the producer thread has made ctx->device current
        std::string upload_err;
        int misses_in_row = 0;
        unsigned long long cooldown = 0;
    } ahead;
    // device-RNG mode (`rng="device"`, every CEM controller): no chain - a Philox kernel in front of the plan draws the candidates
    struct {
        bool on = false;
        unsigned long long seed = 0, calls = 0;
        unsigned long long offset = 0;          // the step's first stream element
        float* lowr = nullptr;                  // [2][16]: low | high - low, fp32
    } device;
    // sharded plan: this rank rolls out candidates [lo, hi) of every env (unsharded: all of them, [0, n)) and the ranks meet in the
    // int64 MAX all-reduce - RS: ONE per step, of [keys (m), launch flag, digest, MASK - digest]; CEM: one per iteration, of the returns
    struct {
        bool on = false;                        // (also with world = 1: the same code path with a one-rank collective)
        int rank = 0, world = 1, lo = 0, hi = 0;
        l2a_reduce_fn reduce = nullptr;         // null: RCCL through the context's communicator (l2a_comm_init)
        void* reduce_arg = nullptr;
        unsigned long long digest = 0;          // what every rank must agree on before the reduced words mean anything
        unsigned long long* payload_dev = nullptr;  // RS: [m + 3]
        unsigned long long* payload_host = nullptr; // page-locked [m + 3]
    } shard;
    // sharded and CEM steps launch l2a_plan_rs / l2a_lstm_plan_rs themselves: host-mapped observations, the keys on the device
    float* obs_map_host = nullptr;
    float* obs_map_dev = nullptr;
    unsigned long long* keys_dev = nullptr;     // [m]
    // ---- a step between l2a_controller_begin and l2a_controller_finish ----
    l2a_mail_pending pending;
    bool in_flight = false;
    int result = L2A_OK;                        // what the finished step reports (L2A_OK / L2A_STEP_DREW / L2A_STEP_UNSPLIT)
    float obs32[L2A_MAIL_OBS];                  // the observations as staged (a relaunch in `finish` launches from them again)
    const float *c0 = nullptr, *h0 = nullptr;   // recurrent: the caller's state pointers of the step in flight
    float *c1 = nullptr, *h1 = nullptr;
    void* stream = nullptr;
    double t_begin = 0.0, t_taken = 0.0;
    // ---- l2a_controller_stats ----
    double stage_us[8] = {0};
    unsigned long long steps = 0, relaunches = 0, sync_draws = 0;
    // CEM plan (l2a_cem_controller_create_device): K iterations of rollout -> l2a_cem_refit_sample, one read-back per step
    struct cem_state* cem = nullptr;
    // MPPI plan (l2a_mppi_controller_create_device): K iterations of l2a_mppi_sample -> rollout -> l2a_mppi_update, one read-back
    struct mppi_state* mppi = nullptr;
    // iCEM plan (l2a_icem_controller_create_device): per iteration l2a_icem_sample -> rollout of pops[it] -> l2a_icem_refit, one read-back
    struct icem_state* icem = nullptr;
    struct warm_state* warm = nullptr;          // the MPPI or the iCEM plan: what a plan that persists from step to step shares
    struct plan_state* plan = nullptr;          // whichever of the three: what every kind of plan step shares
};

enum plan_kind { PLAN_NONE, PLAN_CEM, PLAN_MPPI, PLAN_ICEM };       // (PLAN_NONE: random shooting)

// What the device-mode plan steps (CEM, MPPI, iCEM) share: the iterations' returns, the packed result behind ONE read-back and, for one
// rank of a sharded plan, the words of the per-iteration gather and the verdict accumulated over them.
struct plan_state {
    plan_kind kind = PLAN_NONE;
    const char* name = "";                      // "sharded CEM" / "sharded MPPI" / "sharded iCEM" in a sharded step's error texts
    const char* facts = "";                     // what beside seed, step count, m, n, h and iters the ranks' digests cover, in words
    int iters = 0, D = 0, row_floats = 0;       // a result row: the action | return | index bits | ... (CEM: A + 2, MPPI and iCEM: A + 4 floats)
    size_t rows_at = 0;                         // the rows `plan_finish` decodes start here in `packed` (iCEM: the last iteration's block)
    unsigned long long iter_calls = 0;          // iterations planned so far (the Philox stream's position)
    float* seq = nullptr;                       // [h, m * (hi - lo), act_dim]
    float* rets = nullptr;                      // [iters, m, n]: every iteration's returns of the latest step (iCEM: [m, pops[it]] one after another)
    float* lowhigh = nullptr;                   // [2][act_dim] fp32 bounds
    float* packed_dev = nullptr;                // m result rows (CEM: + mean [m, D], std [m, D])
    float* packed_host = nullptr;               // page-locked
    size_t packed_floats = 0;                   // (sharded: + the verdict's three words)
    float* rets_local = nullptr;                // sharded [m, hi - lo]: this rank's returns of the iteration under way
    unsigned long long* words = nullptr;        // sharded [m * n + 3]
    unsigned int* verdict_dev = nullptr;        // sharded [3] behind packed_dev's floats: flag | holes | digest mismatch, accumulated per step
};

// Device-mode CEM (`MPCController.get_cem_action_device`, policies/mpc_controller.py): the whole plan step on the launch stream -
// l2a_cem_sample for iteration 0, then per iteration the rollout and ONE l2a_cem_refit_sample (the last iteration: l2a_cem_refit),
// l2a_cem_pick, and one copy of the packed result to page-locked memory.  Philox offsets (calls + it) * n * m * D, as the Python path.
// A recurrent controller (l2a_lstm_cem_controller_create_device) rolls out with l2a_lstm_plan_rs from the caller's c0 / h0, picks with
// l2a_cem_pick_act and, with c_next / h_next, enqueues l2a_lstm_advance on the picked actions in front of the read-back.
// One rank of a sharded plan (l2a_cem_controller_create_sharded_device) rolls out candidates [lo, hi); every iteration's returns are
// gathered by the int64 MAX all-reduce of m * n + 3 words (l2a_cem_shard_pack / _unpack).
struct cem_state : plan_state {
    int k = 0, reference = 1;
    float alpha = 0.1f;
    float* mean[2] = {nullptr, nullptr};        // [m, D] ping-pong (the fused launch reads one and writes the other)
    float* std = nullptr;                       // [m, D]
    float* a_clip[2] = {nullptr, nullptr};      // [n, m, D] ping-pong
    float* a_raw = nullptr;                     // [n, m, D]
    int* rows = nullptr;                        // [m * k]
    int cur = 0;                                // the buffers of the last iteration
    float* act_dev = nullptr;                   // recurrent: the winners' first actions [m, act_dim] (l2a_cem_pick_act -> l2a_lstm_advance)
};

// What a plan that persists from step to step on the device (MPPI's mean, iCEM's mean, spread, kept rows and counts) needs: three
// copies of the state that rotate together - a step reads copy `cur` and writes the two others in turn -, the marks of the envs
// that are new or were reset with iteration 0's shift vector made from them, and the Philox position (`iter_calls`).  `cur`,
// iter_calls and the reset marks move in `finish` only: a replayed or failed step starts from the same plan.
struct warm_state : plan_state {
    float sigma32[16] = {0};                    // (the digest carries its bits)
    float* sigma = nullptr;                     // [act_dim] device
    float* a_clip = nullptr;                    // [n, m, D]
    int* shift = nullptr;                       // device [4][m]: all +1 | all 0 | all -1 | the step's own mix
    int* shift_host = nullptr;                  // page-locked [m]: the mix of the step in flight (it stays for a replay)
    const int* first = nullptr;                 // iteration 0's shift vector of the step in flight
    std::vector<unsigned char> fresh;           // [m]: the env is new or was reset - its next step starts afresh (MPPI: from zeros)
    int cur = 0, last = 0;                      // the committed copy | the copy the step in flight ends on
    float* result_host = nullptr;               // page-locked: the one copy of l2a_mppi_controller_result / l2a_icem_controller_result
};

// Device-mode MPPI (`MPCController.get_mppi_action`): per iteration l2a_mppi_sample (sharded: l2a_mppi_sample_shard over this rank's
// window), the rollout (sharded: + the gather of the returns, as CEM's), l2a_mppi_update over all n; the update's packed head is
// the step's one read-back.  Philox offsets (iter_calls + it) * n * m * D.  The plan mean is the state that persists (warm_state).
struct mppi_state : warm_state {
    float kappa = 1.0f, beta = 1.0f;
    float* mean[3] = {nullptr, nullptr, nullptr};   // [m, D] each, in one allocation in front of `rets`; result_host: [3 m D + iters m n]
};

// Device-mode iCEM (`MPCController.get_icem_action`): per iteration l2a_icem_sample (sharded: l2a_icem_sample_shard over this rank's
// window of the iteration's population pops[it]), the rollout of pops[it] candidates (sharded: + the gather), l2a_icem_refit over all
// of them into result row block `it`; the iters * m result rows are the step's one read-back.  Philox offsets (iter_calls + it) * n *
// m * D: the stride is the full n.  Mean, spread, kept rows and counts are the state that persists (warm_state).
struct icem_state : warm_state {
    int K = 0, Kk = 0, add_mean = 0;
    float alpha = 0.0f, rho = 0.0f;
    std::vector<int> pops;                      // [iters]: the caller's populations
    std::vector<size_t> ret_at;                 // [iters + 1]: iteration it's table [m, pops[it]] starts at rets + ret_at[it]
    // one allocation in front of `rets`: mean [3][m, D] | std [3][m, D] | kept [3][m, max(Kk, 1), D] | kc [3][m]
    float* mean[3] = {nullptr, nullptr, nullptr};
    float* std[3] = {nullptr, nullptr, nullptr};
    float* kept[3] = {nullptr, nullptr, nullptr};
    int* kc[3] = {nullptr, nullptr, nullptr};
    size_t head_floats = 0;                     // the floats of that allocation in front of `rets` (result_host: + m * sum(pops))
    int* work = nullptr;                        // [m, K]: the refit's scratch
    // l2a_icem_controller_set_noise: the matrix the sample reads in place of the recurrence (allocated at the first set)
    float* noise = nullptr;                     // device [h, h]
    bool noise_on = false;
    unsigned long long noise_hash = 0;          // of the matrix's bits (the digest carries it while noise_on)
};

extern "C" unsigned long long l2a_mt19937_state_digest(const void* addr);      // csrc/l2a_rng.c

// Device-RNG mode: the candidate tensor [h, m * n, act_dim] from the counter-based stream (seed, offset + element): four elements
// per thread (one Philox block), the action dimension of an element = its index modulo act_dim.
__global__ void __launch_bounds__(256) l2a_uniform_fill_k(unsigned long long seed, unsigned long long offset, long long total,
                                                          int act_dim, const float* __restrict__ lowr, float* __restrict__ out) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;      // block of four elements
    if (4 * b >= total) return;
    unsigned int c[4];
    l2a_philox4x32_10(seed, (offset >> 2) + (unsigned long long)b, L2A_PHILOX_UNIFORM, c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long e = 4 * b + i;
        if (e < total) {
            const int k = (int)(e % act_dim);
            out[e] = l2a_uniform_from_word(c[i], lowr[k], lowr[16 + k]);
        }
    }
}

// The same stream for ONE rank of a sharded plan: this rank's candidates [lo, lo + n_local) of every env, local tensor
// [h, m * n_local, act_dim]; an element takes the value of its GLOBAL position ((t m + i) n + j) act_dim + k in the stream, so the
// candidates - and with them the plan - do not depend on the number of ranks.  One element per thread (its Philox block computed
// whole: four times the rounds of the contiguous fill, on a tensor an eighth of the size).
__global__ void __launch_bounds__(256) l2a_uniform_fill_shard_k(unsigned long long seed, unsigned long long offset, long long total_local,
                                                                int n, int lo, int n_local, int act_dim, const float* __restrict__ lowr,
                                                                float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total_local) return;
    const int k = (int)(e % act_dim);
    const long long r = e / act_dim;                // local row (t m + i) n_local + jl
    const long long ti = r / n_local;
    const int jl = (int)(r - ti * n_local);
    const unsigned long long g = (unsigned long long)((ti * n + lo + jl) * act_dim + k);
    out[e] = l2a_philox_uniform(seed, offset + g, lowr[k], lowr[16 + k]);
}

namespace {

int fail(l2a_ctx* ctx, int code, const std::string& msg) { return l2a_fail(ctx, code, msg); }

const char* const SPLIT_OFF = "l2a_controller_step: the rollout was flagged invalid with the tile split disabled";

// A step enters / leaves flight: the context counts its CEM and its other steps in flight.
void set_in_flight(l2a_controller* c, bool on) {
    if (c->in_flight == on) return;
    c->in_flight = on;
    int& n = c->plan ? c->ctx->cem_steps_in_flight : c->ctx->rs_steps_in_flight;        // (an MPPI step counts as a CEM step: below)
    n += on ? 1 : -1;
}

// ---- the owner of a controller's buffers ------------------------------------------------------------------------------------------
// `count` elements of device, page-locked, host-mapped or heap memory, recorded on the controller.  After the first failure
// (c->mem_err) every call returns null and allocates nothing: a create path allocates straight through and checks once.
template <typename T>
T* alloc(l2a_controller* c, mem_kind kind, size_t count) {
    if (c->mem_err != hipSuccess) return nullptr;
    void* p = nullptr;
    const size_t bytes = sizeof(T) * count;
    if (kind == MEM_DEVICE) c->mem_err = hipMalloc(&p, bytes);
    else if (kind == MEM_HEAP) c->mem_err = (p = std::malloc(bytes)) ? hipSuccess : hipErrorOutOfMemory;
    else c->mem_err = hipHostMalloc(&p, bytes, kind == MEM_MAPPED ? hipHostMallocMapped : hipHostMallocDefault);
    if (c->mem_err != hipSuccess) return nullptr;
    c->mem.push_back({p, kind});
    return static_cast<T*>(p);
}

void upload(l2a_controller* c, void* dst, const void* src, size_t bytes) {
    if (c->mem_err == hipSuccess) c->mem_err = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
}

void release(l2a_controller* c) {
    for (const owned_mem& b : c->mem) {
        if (b.kind == MEM_DEVICE) (void)hipFree(b.ptr);
        else if (b.kind == MEM_HEAP) std::free(b.ptr);
        else (void)hipHostFree(b.ptr);
    }
    c->mem.clear();
    if (c->done) (void)hipEventDestroy(c->done);
    if (c->ahead.side) (void)hipStreamDestroy(c->ahead.side);
}

// ---- the producer of the next step's candidates (parity mode) -----------------------------------------------------------------------
// Sharded recurrent plan: the first-step table of block `slot` - float64 -> fp32 as the candidate tensor's rows are cast
// (csrc/l2a_rng.c), so for candidates in [lo, hi) it holds the planned values bit for bit - enqueued for upload on `stream`.
hipError_t upload_table(l2a_controller* c, int slot, hipStream_t stream) {
    const size_t count = (size_t)c->m * c->n * c->act_dim;
    const double* src = c->ahead.c64[slot];
    float* dst = c->ahead.tab_pin[slot];
    for (size_t i = 0; i < count; ++i) dst[i] = (float)src[i];
    return hipMemcpyAsync(c->ahead.tab_dev[slot], dst, count * sizeof(float), hipMemcpyHostToDevice, stream);
}

// Producer thread, after the block's draw: one H2D copy on the side stream, completed before the block is marked ready - the
// consumer neither waits on an event nor launches behind an unfinished copy.
int upload_block(void* arg, int slot) {
    l2a_controller* c = static_cast<l2a_controller*>(arg);
    auto& a = c->ahead;
    if (!a.producer_bound) {
        if (hipSetDevice(c->ctx->device) != hipSuccess) { a.upload_err = "hipSetDevice on the producer thread failed"; return -1; }
        a.producer_bound = true;
    }
    const bool table = a.tab_dev[slot] != nullptr;
    const bool rolls = c->shard.hi > c->shard.lo;                 // (more ranks than candidates: this rank rolls nothing out)
    if (!rolls && !table) return 0;
    hipError_t e = table ? upload_table(c, slot, a.side) : hipSuccess;
    if (e == hipSuccess && rolls) e = hipMemcpyAsync(c->dev[slot], a.pin[slot], c->act_floats * sizeof(float), hipMemcpyHostToDevice, a.side);
    if (e == hipSuccess) e = hipStreamSynchronize(a.side);
    if (e != hipSuccess) { a.upload_err = std::string("uploading a candidate block: ") + hipGetErrorString(e); return -1; }
    return 0;
}

void kick_next(void* arg) { (void)l2a_ahead_next(static_cast<l2a_controller*>(arg)->ahead.chain); }

// After a synchronous draw: the chain restarts at the generator's new state - unless steps keep missing (a consumer of np.random
// runs between the controller's steps): then only every 16th step tries again.
void kick_arm(void* arg) {
    auto& a = static_cast<l2a_controller*>(arg)->ahead;
    a.misses_in_row += 1;
    if (a.misses_in_row > 2 && (++a.cooldown % 16) != 0) return;
    (void)l2a_ahead_arm(a.chain, a.np_addr);
}

// ---- create: all 16 entry points fill a step_cfg and share everything below ----------------------------------------------------------
struct step_cfg {
    const char* who;                            // the entry point (the prefix of its error texts)
    l2a_model* mlp;
    l2a_lstm* rnn;
    int m, n, h;
    const double *low, *high;
    double discount;
    const l2a_reward* reward;
    l2a_controller** out;
    l2a_ctx* ctx = nullptr;                     // `resolve`: the model's context and dimensions
    int obs_dim = 0, act_dim = 0;
    // where the candidates come from: NumPy's global generator (its state's address, helper threads) or the Philox stream (seed)
    bool device_rng = false;
    void* np_addr = nullptr;
    int rng_threads = 1;
    unsigned long long seed = 0;
    bool sharded = false;                       // one rank of a sharded plan
    int rank = 0, world = 1;
    l2a_reduce_fn reduce = nullptr;
    void* reduce_arg = nullptr;
    plan_kind kind = PLAN_NONE;                 // a CEM, an MPPI or an iCEM plan
    int iters = 0, num_elites = 0, reference = 0;   // CEM (`iters`: every kind)
    float alpha = 0.0f;
    float kappa = 0.0f, beta = 0.0f;            // MPPI
    const double* sigma = nullptr;              // [act_dim] (iCEM: sigma0)
    const int* pops = nullptr;                  // iCEM (`alpha` as CEM's, `sigma` as MPPI's): [iters]
    int K = 0, Kk = 0, add_mean = 0;
    float rho = 0.0f;

    step_cfg& parity(void* addr, int threads) { np_addr = addr; rng_threads = threads; return *this; }
    step_cfg& device(unsigned long long s) { device_rng = true; seed = s; return *this; }
    step_cfg& shard(int r, int w, l2a_reduce_fn fn, void* arg) { sharded = true; rank = r; world = w; reduce = fn; reduce_arg = arg; return *this; }
    step_cfg& cem_plan(int it, int elites, float a, int ref, unsigned long long s) {
        kind = PLAN_CEM; iters = it; num_elites = elites; alpha = a; reference = ref ? 1 : 0;
        return device(s);
    }
    step_cfg& mppi_plan(int it, float kap, float bet, const double* sig, unsigned long long s) {
        kind = PLAN_MPPI; iters = it; kappa = kap; beta = bet; sigma = sig;
        return device(s);
    }
    step_cfg& icem_plan(int it, const int* pop, int k, int kk, float a, float r, const double* sig, int add, unsigned long long s) {
        kind = PLAN_ICEM; iters = it; pops = pop; K = k; Kk = kk; alpha = a; rho = r; sigma = sig; add_mean = add ? 1 : 0;
        return device(s);
    }
};

void resolve(step_cfg& f) {
    int units = 0;
    if (f.mlp) l2a_model_facts(f.mlp, &f.ctx, &f.obs_dim, &f.act_dim);
    else l2a_lstm_facts(f.rnn, &f.ctx, &f.obs_dim, &f.act_dim, &units);
}

// A refused create: `code`, and "<entry point>: <text>" on the context.
int refuse(const step_cfg& f, int code, const char* text) { return fail(f.ctx, code, std::string(f.who) + ": " + text); }

int check_shard(const step_cfg& f) {
    if (!f.sharded) return L2A_OK;
    if (f.world < 1 || f.rank < 0 || f.rank >= f.world) return refuse(f, L2A_EINVAL, "bad rank / world");
    if (!f.reduce && (!f.ctx->comm || f.ctx->comm_world != f.world || f.ctx->comm_rank != f.rank))
        return refuse(f, L2A_ESTATE, "no reduce function and no communicator of this rank / world (l2a_comm_init)");
    return L2A_OK;
}

int check_shape(const step_cfg& f) {
    const int m = f.m, n = f.n, h = f.h;
    const bool bad_mnh = m < 1 || m > L2A_MAIL_KEYS || (long long)m * f.obs_dim > L2A_MAIL_OBS || n < 1 || h < 1;
    const bool bad_act = f.act_dim < 1 || f.act_dim > 16;
    if (f.kind == PLAN_NONE) {
        if (bad_mnh) return refuse(f, L2A_EINVAL, "needs 1 <= m <= 64 envs (at most 4096 observation floats), n >= 1, h >= 1");
        if (bad_act) return refuse(f, L2A_EINVAL, "the host draw takes 1 <= act_dim <= 16");
        if ((long long)m * n > 0x3fffffffLL) return refuse(f, L2A_EINVAL, "too many candidates");
        if (l2a_rng_version() < 8) return refuse(f, L2A_ESTATE, "libl2a_rng.so is older than this library");
        return L2A_OK;
    }
    if (bad_mnh || bad_act)
        return refuse(f, L2A_EINVAL, "needs 1 <= m <= 64 envs (at most 4096 observation floats), n >= 1, h >= 1, 1 <= act_dim <= 16");
    const long long D = (long long)h * f.act_dim;
    if (f.kind == PLAN_CEM) {
        if (f.iters < 1 || f.num_elites < 1 || f.num_elites > n) return refuse(f, L2A_EINVAL, "needs iters >= 1 and 1 <= num_elites <= n");
        if ((long long)(f.reference ? m : 1) * f.num_elites > 8192 || (size_t)n * sizeof(float) > (size_t)f.ctx->lds_per_block)
            return refuse(f, L2A_EINVAL, "more elite rows or candidates than l2a_cem_refit takes");
        if ((long long)n * m * D > 0x7fffffffLL || (long long)f.iters * m * n > 0x7fffffffLL || (long long)m * n > 0x3fffffffLL)
            return refuse(f, L2A_EINVAL, "too many samples");
        return L2A_OK;
    }
    // MPPI, iCEM: the limits of the kind's sample and update / refit kernels on every iteration, so that no step can fail on its arguments
    if (f.iters < 1) return refuse(f, L2A_EINVAL, "needs iters >= 1");
    for (int k = 0; k < f.act_dim; ++k)
        if (!std::isfinite((float)f.sigma[k]) || !(f.sigma[k] >= 0.0))
            return refuse(f, L2A_EINVAL, f.kind == PLAN_MPPI ? "sigma must be finite and non-negative" : "sigma0 must be finite and non-negative");
    if (f.kind == PLAN_MPPI) {
        if (!(f.beta > 0.0f) || !(f.beta <= 1.0f)) return refuse(f, L2A_EINVAL, "beta must lie in (0, 1]");
        if (!(f.kappa > 0.0f) || !std::isfinite(f.kappa)) return refuse(f, L2A_EINVAL, "kappa must be positive and finite");
        if ((size_t)n * sizeof(float) + L2A_MPPI_UPDATE_STATIC_LDS > (size_t)f.ctx->lds_per_block)
            return refuse(f, L2A_EINVAL, "more candidates than an env's weights fit in LDS (l2a_mppi_update)");
    } else {
        if (f.K < 1 || f.K > 8192) return refuse(f, L2A_EINVAL, "needs 1 <= K <= 8192 elites");
        if (f.Kk < 0 || f.Kk > f.K) return refuse(f, L2A_EINVAL, "needs 0 <= Kk <= K kept elites");
        if (!(f.alpha >= 0.0f) || !(f.alpha < 1.0f)) return refuse(f, L2A_EINVAL, "alpha must lie in [0, 1)");
        if (!(f.rho >= 0.0f) || !(f.rho < 1.0f)) return refuse(f, L2A_EINVAL, "rho must lie in [0, 1)");
        if ((size_t)f.K * sizeof(int) + L2A_ICEM_REFIT_STATIC_LDS > (size_t)f.ctx->lds_per_block)
            return refuse(f, L2A_EINVAL, "more elites than the statistics' list fits in LDS (l2a_icem_refit)");
        for (int it = 0; it < f.iters; ++it) {
            if (f.pops[it] < 1 || f.pops[it] > n) return refuse(f, L2A_EINVAL, "every pops[it] must lie in 1 .. n");
            if ((size_t)f.pops[it] * sizeof(float) > (size_t)f.ctx->lds_per_block)
                return refuse(f, L2A_EINVAL, "more candidates than an env's returns fit in LDS (l2a_icem_refit)");
        }
    }
    if ((long long)n * m * D > 0x7fffffffLL * 256 || (long long)f.iters * m * n > 0x7fffffffLL || (long long)m * n > 0x3fffffffLL)
        return refuse(f, L2A_EINVAL, "too many samples");
    return L2A_OK;
}

void init_common(l2a_controller* c, const step_cfg& f) {
    c->ctx = f.ctx; c->mlp = f.mlp; c->rnn = f.rnn;
    c->m = f.m; c->n = f.n; c->h = f.h; c->obs_dim = f.obs_dim; c->act_dim = f.act_dim;
    c->discount = f.discount; c->rw = *f.reward;
    for (int k = 0; k < f.act_dim; ++k) { c->low[k] = f.low[k]; c->high[k] = f.high[k]; }
    c->ahead.np_addr = f.np_addr;
    c->ahead.rng_threads = f.rng_threads < 1 ? 1 : f.rng_threads;
    c->device.on = f.device_rng; c->device.seed = f.seed;
    c->shard.on = f.sharded; c->shard.rank = f.rank; c->shard.world = f.world; c->shard.reduce = f.reduce; c->shard.reduce_arg = f.reduce_arg;
    c->shard.lo = (int)((long long)f.rank * f.n / f.world);         // contiguous candidate ranges (MPCController._shard_range)
    c->shard.hi = (int)((long long)(f.rank + 1) * f.n / f.world);
    const int n_local = c->shard.hi - c->shard.lo;
    c->act_floats = (size_t)f.h * f.m * (n_local > 0 ? n_local : 1) * f.act_dim;
    c->glob_floats = (size_t)f.h * f.m * f.n * f.act_dim;
}

// What a step that launches l2a_plan_rs / l2a_lstm_plan_rs itself (sharded, CEM) needs beside its candidates.
void alloc_launch(l2a_controller* c) {
    c->obs_map_host = alloc<float>(c, MEM_MAPPED, L2A_MAIL_OBS);
    if (c->mem_err == hipSuccess) c->mem_err = hipHostGetDevicePointer(reinterpret_cast<void**>(&c->obs_map_dev), c->obs_map_host, 0);
    c->keys_dev = alloc<unsigned long long>(c, MEM_DEVICE, (size_t)c->m);
    if (c->mem_err == hipSuccess) c->mem_err = hipEventCreateWithFlags(&c->done, hipEventDisableTiming);
}

// Random shooting: the candidate tensor(s) of the RNG mode; sharded, the payload words of the step's one collective.
void alloc_rs(l2a_controller* c, const step_cfg& f) {
    const size_t rows = (size_t)c->m * c->n * c->act_dim;       // the whole plan's first horizon step
    auto& a = c->ahead;
    if (c->device.on) {
        // the stream's elements are addressed in blocks of four: a step's tensor starts on a block boundary
        c->dev[0] = alloc<float>(c, MEM_DEVICE, (c->act_floats + 3) / 4 * 4);
        c->device.lowr = alloc<float>(c, MEM_DEVICE, 32);
        float lr[32] = {0};
        for (int k = 0; k < c->act_dim; ++k) { lr[k] = (float)f.low[k]; lr[16 + k] = (float)f.high[k] - (float)f.low[k]; }
        upload(c, c->device.lowr, lr, sizeof(lr));
    } else {
        c->mem_err = hipStreamCreateWithFlags(&a.side, hipStreamNonBlocking);
        for (int s = 0; s < 2; ++s) {
            a.pin[s] = alloc<float>(c, MEM_PINNED, c->act_floats);
            c->dev[s] = alloc<float>(c, MEM_DEVICE, c->act_floats);
            a.c64[s] = alloc<double>(c, MEM_HEAP, rows);
            if (f.sharded && f.rnn) {
                a.tab_pin[s] = alloc<float>(c, MEM_PINNED, rows);
                a.tab_dev[s] = alloc<float>(c, MEM_DEVICE, rows);
            }
        }
        if (c->mem_err == hipSuccess) {
            // rows of the reference's draw: h * n * m (mpc_controller.py:114), row r <-> candidate r % n; the whole env-major tensor
            // goes up (one GPU: every candidate is local); the first n * m rows are kept in float64 (`cand_a`, :118)
            // (a sharded plan: every rank consumes the generator for ALL h * n * m rows and keeps candidates [lo, hi) of every env)
            a.chain = l2a_ahead_create((long long)c->h * c->n * c->m, c->act_dim, f.low, f.high, c->n, c->shard.lo, c->shard.hi,
                                       (long long)c->n * c->m, a.pin[0], a.pin[1], a.c64[0], a.c64[1], f.rng_threads, upload_block, c);
            if (!a.chain) c->mem_err = hipErrorInvalidValue;
        }
    }
    if (!f.sharded) return;
    alloc_launch(c);
    c->shard.payload_dev = alloc<unsigned long long>(c, MEM_DEVICE, (size_t)c->m + 3);
    c->shard.payload_host = alloc<unsigned long long>(c, MEM_PINNED, (size_t)c->m + 3);
}

// A device-mode plan (CEM, MPPI, iCEM): what every kind allocates, `packed` floats of result behind the one read-back.  The unsharded
// controller is rank 0 of a world of 1 without the collective's buffers.  `rets_head`: floats the caller keeps in front of the
// returns in the same allocation (MPPI: its means, iCEM: its state, so that ONE copy brings them and the returns back on request).
// `window`: the most candidates this rank rolls out in one iteration, where that is not hi - lo (iCEM: the window moves with pops[it]).
void alloc_plan(l2a_controller* c, const step_cfg& f, int row_floats, size_t packed, size_t rets_head = 0, size_t window = 0) {
    plan_state* q = c->plan;
    q->kind = f.kind;
    const int A = c->act_dim;
    q->iters = f.iters; q->D = c->h * A; q->row_floats = row_floats;
    const size_t m = (size_t)c->m, n = (size_t)c->n, md = m * q->D;
    const size_t n_local = window ? window : (size_t)(c->shard.hi - c->shard.lo), n_alloc = n_local > 0 ? n_local : 1;
    q->packed_floats = packed + (f.sharded ? 3 : 0);
    alloc_launch(c);
    q->seq = alloc<float>(c, MEM_DEVICE, n_alloc * md);
    q->rets = alloc<float>(c, MEM_DEVICE, rets_head + (size_t)f.iters * m * n);
    if (q->rets) q->rets += rets_head;
    q->lowhigh = alloc<float>(c, MEM_DEVICE, 2 * (size_t)A);
    q->packed_dev = alloc<float>(c, MEM_DEVICE, q->packed_floats);
    q->packed_host = alloc<float>(c, MEM_PINNED, q->packed_floats);
    if (f.sharded) {
        q->rets_local = alloc<float>(c, MEM_DEVICE, m * n_alloc);
        q->words = alloc<unsigned long long>(c, MEM_DEVICE, m * n + 3);
        if (q->packed_dev) q->verdict_dev = reinterpret_cast<unsigned int*>(q->packed_dev + (q->packed_floats - 3));
    }
    float lh[32] = {0};
    for (int k = 0; k < A; ++k) { lh[k] = (float)f.low[k]; lh[A + k] = (float)f.high[k]; }
    upload(c, q->lowhigh, lh, sizeof(float) * 2 * A);
}

// The state object of a plan of one kind, `name` and `facts` for its sharded step's texts (plan_verdict_sharded); null: out of memory.
template <typename State>
State* new_plan(l2a_controller* c, const char* name, const char* facts) {
    State* q = new (std::nothrow) State();
    if (!q) { c->mem_err = hipErrorOutOfMemory; return nullptr; }
    q->name = name; q->facts = facts;
    c->plan = q;
    return q;
}

void alloc_cem(l2a_controller* c, const step_cfg& f) {
    cem_state* q = c->cem = new_plan<cem_state>(c, "sharded CEM", "num_elites, mode, alpha and world");
    if (!q) return;
    const int A = c->act_dim;
    q->k = f.num_elites; q->reference = f.reference; q->alpha = f.alpha;
    const size_t m = (size_t)c->m, n = (size_t)c->n, md = m * c->h * A, nmd = n * md;
    alloc_plan(c, f, A + 2, m * (A + 2) + 2 * md);
    for (int s = 0; s < 2; ++s) {
        q->mean[s] = alloc<float>(c, MEM_DEVICE, md);
        q->a_clip[s] = alloc<float>(c, MEM_DEVICE, nmd);
    }
    q->std = alloc<float>(c, MEM_DEVICE, md);
    if (q->reference) q->a_raw = alloc<float>(c, MEM_DEVICE, nmd);
    q->rows = alloc<int>(c, MEM_DEVICE, m * f.num_elites);
    if (f.rnn) q->act_dev = alloc<float>(c, MEM_DEVICE, m * A);
}

// The reset marks: the envs of `dones` (null: every env) start their next step afresh.
void mark_fresh(l2a_controller* c, const unsigned char* dones) {
    for (int i = 0; i < c->m; ++i)
        if (!dones || dones[i]) c->warm->fresh[i] = 1;
}

// The tail of the two allocators of a plan that persists (warm_state): `result_floats` of page-locked memory for the kind's result
// call, the clipped samples, the noise scale, the four shift rows, and every env marked new.
void alloc_warm(l2a_controller* c, const step_cfg& f, size_t result_floats) {
    warm_state* q = c->warm;
    const int A = c->act_dim;
    const size_t m = (size_t)c->m;
    q->result_host = alloc<float>(c, MEM_PINNED, result_floats);
    q->a_clip = alloc<float>(c, MEM_DEVICE, (size_t)c->n * m * q->D);
    q->sigma = alloc<float>(c, MEM_DEVICE, (size_t)A);
    q->shift = alloc<int>(c, MEM_DEVICE, 4 * m);
    q->shift_host = alloc<int>(c, MEM_PINNED, m);
    q->fresh.resize(m);
    mark_fresh(c, nullptr);
    for (int k = 0; k < A; ++k) q->sigma32[k] = (float)f.sigma[k];
    upload(c, q->sigma, q->sigma32, sizeof(float) * A);
    std::vector<int> rows(4 * m, 0);
    for (size_t i = 0; i < m; ++i) { rows[i] = 1; rows[2 * m + i] = -1; }
    upload(c, q->shift, rows.data(), sizeof(int) * rows.size());
}

void alloc_mppi(l2a_controller* c, const step_cfg& f) {
    mppi_state* q = c->mppi = new_plan<mppi_state>(c, "sharded MPPI", "kappa, beta, sigma and world, and the same envs reset");
    if (!q) return;
    c->warm = q;
    const int A = c->act_dim;
    q->kappa = f.kappa; q->beta = f.beta;
    const size_t m = (size_t)c->m, n = (size_t)c->n, md = m * c->h * A;
    alloc_plan(c, f, A + 4, m * (A + 4), 3 * md);
    for (int s = 0; s < 3; ++s) q->mean[s] = q->rets ? q->rets - (3 - s) * md : nullptr;
    alloc_warm(c, f, 3 * md + (size_t)f.iters * m * n);
}

// This rank's window of a population of `n_it`: contiguous ranges in integer arithmetic, `init_common`'s rule.
void icem_window(const l2a_controller* c, int n_it, int* lo, int* hi) {
    *lo = (int)((long long)c->shard.rank * n_it / c->shard.world);
    *hi = (int)((long long)(c->shard.rank + 1) * n_it / c->shard.world);
}

void alloc_icem(l2a_controller* c, const step_cfg& f) {
    icem_state* q = c->icem = new_plan<icem_state>(c, "sharded iCEM", "populations, K, Kk, add_mean, alpha, rho, sigma0 and world, and the same "
                                                                      "envs reset");
    if (!q) return;
    c->warm = q;
    const int A = c->act_dim;
    q->K = f.K; q->Kk = f.Kk; q->add_mean = f.add_mean; q->alpha = f.alpha; q->rho = f.rho;
    q->pops.assign(f.pops, f.pops + f.iters);
    q->ret_at.assign((size_t)f.iters + 1, 0);
    const size_t m = (size_t)c->m, md = m * c->h * A, kd = m * (size_t)(f.Kk > 0 ? f.Kk : 1) * c->h * A;
    size_t window = 0;
    for (int it = 0; it < f.iters; ++it) {
        q->ret_at[it + 1] = q->ret_at[it] + m * (size_t)f.pops[it];
        int lo = 0, hi = 0;
        icem_window(c, f.pops[it], &lo, &hi);
        if ((size_t)(hi - lo) > window) window = (size_t)(hi - lo);
    }
    q->head_floats = 3 * (2 * md + kd + m);
    alloc_plan(c, f, A + 4, (size_t)f.iters * m * (A + 4), q->head_floats, window ? window : 1);
    q->rows_at = (size_t)(f.iters - 1) * m * (A + 4);
    float* head = q->rets ? q->rets - q->head_floats : nullptr;
    for (int s = 0; s < 3 && head; ++s) {
        q->mean[s] = head + s * md;
        q->std[s] = head + 3 * md + s * md;
        q->kept[s] = head + 6 * md + s * kd;
        q->kc[s] = reinterpret_cast<int*>(head + 6 * md + 3 * kd) + s * m;
    }
    if (head && c->mem_err == hipSuccess) c->mem_err = hipMemset(head, 0, sizeof(float) * q->head_floats);
    q->work = alloc<int>(c, MEM_DEVICE, m * (size_t)f.K);
    alloc_warm(c, f, q->head_floats + q->ret_at[f.iters]);
}

int create(step_cfg f) {
    if (!f.mlp && !f.rnn) return L2A_EINVAL;
    resolve(f);
    int rc = check_shard(f);
    if (rc != L2A_OK) return rc;
    if (!f.out) return refuse(f, L2A_EINVAL, "out is null");
    *f.out = nullptr;
    if (f.kind == PLAN_MPPI && !f.sigma) return refuse(f, L2A_EINVAL, "null sigma");
    if (f.kind == PLAN_ICEM && f.rnn) return refuse(f, L2A_EINVAL, "an iCEM plan takes an MLP model");
    if (f.kind == PLAN_ICEM && (!f.sigma || !f.pops)) return refuse(f, L2A_EINVAL, "null pops / sigma0");
    if (!f.low || !f.high || !f.reward || (!f.np_addr && !f.device_rng))
        return refuse(f, L2A_EINVAL, f.kind != PLAN_NONE ? "null low / high / reward" : "null low / high / reward / generator state address");
    rc = check_shape(f);
    if (rc != L2A_OK) return rc;
    l2a_controller* c = new (std::nothrow) l2a_controller();
    if (!c) return refuse(f, L2A_EHIP, "out of memory");
    init_common(c, f);
    l2a_device_guard guard(f.ctx->device);
    switch (f.kind) {                   // (a plan's allocator makes its state object first)
    case PLAN_CEM: alloc_cem(c, f); break;
    case PLAN_MPPI: alloc_mppi(c, f); break;
    case PLAN_ICEM: alloc_icem(c, f); break;
    case PLAN_NONE: alloc_rs(c, f); break;
    }
    if (c->mem_err != hipSuccess) {
        const hipError_t e = c->mem_err;
        l2a_controller_destroy(c);
        return refuse(f, L2A_EHIP, hipGetErrorString(e));
    }
    *f.out = c;
    return L2A_OK;
}

// ---- the dispatches a step repeats -------------------------------------------------------------------------------------------------
// The fused rollout of `n_local` candidates from global index `lo` on, launched from the host-mapped observations.
int rollout(l2a_controller* c, const float* actions, int n_local, int lo, float* rets) {
    return c->mlp ? l2a_plan_rs(c->mlp, c->obs_map_dev, actions, c->m, n_local, c->h, c->discount, &c->rw, lo, rets, c->keys_dev, c->stream)
                  : l2a_lstm_plan_rs(c->rnn, c->obs_map_dev, c->c0, c->h0, actions, c->m, n_local, c->h, c->discount, &c->rw, lo, rets,
                                     c->keys_dev, c->stream);
}

// The unsharded RS plan through the context's result mailbox: with `pending` it returns behind `hook`, else it waits for `keys`.
int rollout_sync(l2a_controller* c, unsigned long long* keys, l2a_after_launch_fn hook, l2a_mail_pending* pending) {
    const float* actions = c->dev[c->slot];
    return c->mlp ? l2a_plan_rs_sync_hook(c->mlp, c->obs32, actions, c->m, c->n, c->h, c->discount, &c->rw, 0, nullptr, keys, c->stream,
                                          hook, c, pending)
                  : l2a_lstm_plan_rs_sync_hook(c->rnn, c->obs32, c->c0, c->h0, actions, c->m, c->n, c->h, c->discount, &c->rw, 0, keys,
                                               c->c1, c->h1, c->stream, hook, c, pending);
}

// The sharded plans' collective: the caller's `reduce`, else RCCL (uint64 MAX over xGMI) through the context's communicator.
int reduce_words(l2a_controller* c, unsigned long long* words, int count) {
    if (!c->shard.reduce) return l2a_allreduce_best(c->ctx, words, count, c->stream);
    if (c->shard.reduce(c->shard.reduce_arg, words, count, c->stream) == L2A_OK) return L2A_OK;
    return fail(c->ctx, L2A_EHIP, "l2a_controller_step: the caller's reduce function failed");
}

// Recurrent steps that advance the state themselves (the unsharded RS step: l2a_lstm_plan_rs_sync_hook checks the same).
int check_next_state(l2a_controller* c, const float* c0, const float* h0, const float* c1, const float* h1) {
    if ((!c1) != (!h1)) return fail(c->ctx, L2A_EINVAL, "l2a_lstm_controller_begin: pass c_next and h_next together");
    if (c1 && (c1 == c0 || h1 == h0)) return fail(c->ctx, L2A_EINVAL, "l2a_lstm_controller_begin: the next state must not alias the current one");
    return L2A_OK;
}

// The step's inputs: np.float64 -> np.float32 (round to nearest even, as the host cast), also into the host-mapped word a sharded
// or CEM step's kernels read (it stays as it is for a relaunch).
void stage_obs(l2a_controller* c, const double* obs, const float* c0, const float* h0, float* c1, float* h1, void* stream) {
    const int no = c->m * c->obs_dim;
    for (int i = 0; i < no; ++i) c->obs32[i] = (float)obs[i];
    if (c->obs_map_host) std::memcpy(c->obs_map_host, c->obs32, sizeof(float) * (size_t)no);
    c->c0 = c0; c->h0 = h0; c->c1 = c1; c->h1 = h1; c->stream = stream;
}

// A finished step's counters and stage table (`t2` .. `t3`: its decode).  A CEM step neither takes a block nor kicks a producer.
void record_stages(l2a_controller* c, double t2, double t3) {
    c->steps += 1;
    c->device.calls += 1;
    const double* st = c->ctx->stamps_us;
    c->stage_us[0] = c->t_taken - c->t_begin;               // take (compare + adopt the block; waits only if the producer is late)
    c->stage_us[1] = st[1] - c->t_taken;                    // observation cast + staging (CEM: + iteration 0's sampling launch)
    c->stage_us[2] = st[2] - st[1];                         // launch call(s)
    c->stage_us[3] = c->plan ? 0.0 : st[3] - st[2];         // producer kick
    c->stage_us[4] = st[4] - st[3];                         // wait for the result (begin -> finish: whatever the host did in between is in here)
    c->stage_us[5] = t3 - t2;                               // decode + gather
    c->stage_us[6] = t3 - c->t_begin;                       // whole step
}

// The wait of the steps whose result comes back behind an event (sharded RS, CEM, sharded CEM; the unsharded RS step waits on the
// context's mailbox, `finish`).  `verdict()` reads what came back: L2A_OK, a failure it has recorded, or FLAGGED - a launch lost its
// tile-split partner: the context goes unsplit (same bits), `relaunch()` repeats the step, and a second flag ends it.
const int FLAGGED = -1000;                       // (no code of include/l2a.h)
template <typename Verdict, typename Relaunch>
int settle(l2a_controller* c, int* result, Verdict verdict, Relaunch relaunch) {
    l2a_ctx* ctx = c->ctx;
    l2a_device_guard guard(ctx->device);
    for (int attempt = 0;; ++attempt) {
        L2A_HIP(ctx, hipEventSynchronize(c->done));
        ctx->stamps_us[4] = l2a_now_us();
        int rc = verdict();
        if (rc != FLAGGED) return rc;
        if (attempt == 1)
            return fail(ctx, L2A_ESPLIT, c->shard.on ? "l2a_controller_step: some rank's rollout was flagged invalid twice" : SPLIT_OFF);
        (void)l2a_set_split(ctx, 0);
        c->relaunches += 1;
        *result = L2A_STEP_UNSPLIT;
        rc = relaunch();
        if (rc != L2A_OK) return rc;
    }
}

// ---- CEM (device mode) ---------------------------------------------------------------------------------------------------------
// The iteration-0 distribution: mean 0, std 1 (get_cem_action_device's zero_() / fill_(1.0)).
__global__ void __launch_bounds__(256) l2a_cem_init_k(int md, float* __restrict__ mean, float* __restrict__ std) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < md) { mean[e] = 0.0f; std[e] = 1.0f; }
}

// splitmix64's finaliser over the running value
unsigned long long digest_mix(unsigned long long d, unsigned long long x) {
    d = (d ^ x) + 0x9E3779B97F4A7C15ull;
    d = (d ^ (d >> 30)) * 0xBF58476D1CE4E5B9ull;
    d = (d ^ (d >> 27)) * 0x94D049BB133111EBull;
    return d ^ (d >> 31);
}

const unsigned long long DIGEST_SEED = 0x9E3779B97F4A7C15ull;

unsigned long long digest_words(unsigned long long d, std::initializer_list<unsigned long long> words) {
    for (unsigned long long x : words) d = digest_mix(d, x);
    return d;
}

unsigned long long bits(float x) {
    unsigned int b = 0;
    std::memcpy(&b, &x, sizeof(b));
    return b;
}

// What every rank of a sharded plan step must share: the controller kind, how the controller was built - the planner's constants by
// their bits - and where its Philox stream stands; for a plan that persists, the noise scale and the step's reset marks too - ranks
// that reset different envs would sample around different plans.
unsigned long long plan_digest(const l2a_controller* c) {
    const plan_state* q = c->plan;
    const auto word = [](long long x) { return (unsigned long long)x; };
    unsigned long long d = digest_words(DIGEST_SEED, {word(q->kind), c->device.seed, q->iter_calls, word(c->m), word(c->n), word(c->h),
                                                      word(q->iters), word(c->shard.world)});
    switch (q->kind) {
    case PLAN_CEM:
        d = digest_words(d, {word(c->cem->k), word(c->cem->reference), bits(c->cem->alpha), word(c->rnn ? 1 : 0)});
        break;
    case PLAN_MPPI:
        d = digest_words(d, {bits(c->mppi->kappa), bits(c->mppi->beta)});
        break;
    case PLAN_ICEM: {
        const icem_state* s = c->icem;
        for (int n_it : s->pops) d = digest_mix(d, word(n_it));
        d = digest_words(d, {word(s->K), word(s->Kk), word(s->add_mean), bits(s->alpha), bits(s->rho)});
        if (s->noise_on) d = digest_mix(d, s->noise_hash);      // (without a matrix the digest is the AR(1) step's)
        break;
    }
    case PLAN_NONE: break;
    }
    if (const warm_state* w = c->warm) {
        for (int k = 0; k < c->act_dim; ++k) d = digest_mix(d, bits(w->sigma32[k]));
        for (int i = 0; i < c->m; ++i) d = digest_mix(d, w->fresh[i] ? 1ull : 0ull);
    }
    return d;
}

// One iteration's returns of every candidate of a population of `n` into `rets` [m, n].  Unsharded: the rollout of all n.  Sharded:
// this rank's rollouts of its window [lo, hi) -> words -> the ONE collective -> every rank's returns.  (CEM and MPPI: the plan's n
// and the controller's window, every iteration; iCEM: the iteration's population and its window of it.)
int gather_returns(l2a_controller* c, float* rets, int n, int lo, int hi) {
    plan_state* q = c->plan;
    if (!c->shard.on) return rollout(c, q->seq, n, 0, rets);
    const int m = c->m;
    int rc = L2A_OK;
    if (hi > lo) rc = rollout(c, q->seq, hi - lo, lo, q->rets_local);
    if (rc == L2A_OK) rc = l2a_cem_shard_pack(c->ctx, q->rets_local, m, n, lo, hi, c->shard.digest, q->words, c->stream);
    if (rc == L2A_OK) rc = reduce_words(c, q->words, m * n + 3);
    if (rc == L2A_OK) rc = l2a_cem_shard_unpack(c->ctx, q->words, m, n, rets, q->verdict_dev, c->stream);
    return rc;
}

// The end of a plan step's launches: the packed result (sharded: with the verdict) to page-locked memory, the event behind it.
int read_back(l2a_controller* c) {
    plan_state* q = c->plan;
    hipStream_t stream = reinterpret_cast<hipStream_t>(c->stream);
    L2A_HIP(c->ctx, hipMemcpyAsync(q->packed_host, q->packed_dev, sizeof(float) * q->packed_floats, hipMemcpyDeviceToHost, stream));
    L2A_HIP(c->ctx, hipEventRecord(c->done, stream));
    c->ctx->stamps_us[2] = l2a_now_us();
    return L2A_OK;
}

// The head of a plan step's launches (the caller holds the device): a sharded step's verdict cleared, and the step's own mix of new
// and running envs - where iteration 0 shifts by one - uploaded.
int launch_prelude(l2a_controller* c) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(c->stream);
    const warm_state* w = c->warm;
    const size_t m = (size_t)c->m;
    if (w && w->first == w->shift + 3 * m)
        L2A_HIP(c->ctx, hipMemcpyAsync(w->shift + 3 * m, w->shift_host, sizeof(int) * m, hipMemcpyHostToDevice, stream));
    if (c->shard.on) L2A_HIP(c->ctx, hipMemsetAsync(c->plan->verdict_dev, 0, 3 * sizeof(unsigned int), stream));
    return L2A_OK;
}

// Iteration 0's shift vector of the step about to be launched: -1 for an env that is new or was reset, +1 for the others.
void first_shift(l2a_controller* c) {
    warm_state* q = c->warm;
    const int m = c->m;
    int fresh = 0;
    for (int i = 0; i < m; ++i) fresh += q->fresh[i] ? 1 : 0;
    if (fresh == 0) q->first = q->shift;
    else if (fresh == m) q->first = q->shift + 2 * m;
    else {
        for (int i = 0; i < m; ++i) q->shift_host[i] = q->fresh[i] ? -1 : 1;
        q->first = q->shift + 3 * m;
    }
}

// The copy of the persistent state an iteration writes: neither the one it reads (`src`) nor the committed one.
int spare_copy(const warm_state* q, int src) {
    int dst = 0;
    while (dst == src || dst == q->cur) ++dst;
    return dst;
}

// Everything of one CEM plan step, in stream order on `stream`; nothing on the host waits.
int cem_launch(l2a_controller* c) {
    l2a_ctx* ctx = c->ctx;
    cem_state* q = c->cem;
    hipStream_t stream = reinterpret_cast<hipStream_t>(c->stream);
    const int m = c->m, n = c->n, h = c->h, A = c->act_dim, D = q->D;
    const unsigned long long per_iter = (unsigned long long)n * m * D, seed = c->device.seed;
    l2a_device_guard guard(ctx->device);
    hipLaunchKernelGGL(l2a_cem_init_k, dim3((unsigned)l2a_ceil_div(m * D, 256)), dim3(256), 0, stream, m * D, q->mean[0], q->std);
    L2A_HIP(ctx, hipGetLastError());
    const float* low = q->lowhigh;
    const float* high = q->lowhigh + A;
    int cur = 0;
    // (sharded: every rank samples all n rows of the same stream and keeps the rollout tensor of its candidates [lo, hi) only)
    const int lo = c->shard.lo, hi = c->shard.hi;
    int rc = launch_prelude(c);
    if (rc == L2A_OK)
        rc = l2a_cem_sample(ctx, nullptr, seed, q->iter_calls * per_iter, q->mean[0], q->std, low, high, n, m, h, A, q->reference, lo, hi,
                            q->a_clip[0], q->reference ? q->a_raw : nullptr, q->seq, c->stream);
    if (rc != L2A_OK) return rc;
    ctx->stamps_us[1] = l2a_now_us();
    for (int it = 0; it < q->iters; ++it) {
        float* rets = q->rets + (size_t)it * m * n;
        rc = gather_returns(c, rets, n, lo, hi);
        if (rc != L2A_OK) return rc;
        if (it + 1 < q->iters) {
            rc = l2a_cem_refit_sample(ctx, rets, q->a_clip[cur], n, m, h, A, q->k, q->reference, q->alpha, nullptr, seed,
                                      (q->iter_calls + it + 1) * per_iter, low, high, lo, hi, q->rows, q->mean[cur], q->mean[cur ^ 1], q->std,
                                      q->a_clip[cur ^ 1], q->reference ? q->a_raw : nullptr, q->seq, c->stream);
            cur ^= 1;
        } else {
            rc = l2a_cem_refit(ctx, rets, q->a_clip[cur], n, m, D, q->k, q->reference, q->alpha, q->rows, q->mean[cur], q->std, c->stream);
        }
        if (rc != L2A_OK) return rc;
    }
    const float* last = q->rets + (size_t)(q->iters - 1) * m * n;
    const float* cand = q->reference ? q->a_raw : q->a_clip[cur];
    rc = c->rnn ? l2a_cem_pick_act(ctx, last, cand, q->mean[cur], q->std, n, m, D, A, q->reference, q->packed_dev, q->act_dev, c->stream)
                : l2a_cem_pick(ctx, last, cand, q->mean[cur], q->std, n, m, D, A, q->reference, q->packed_dev, c->stream);
    if (rc != L2A_OK) return rc;
    if (c->rnn && c->c1) {
        // the controller's own state moves on with the winners' first actions (rnn_mpc_controller.py:63), in stream order behind the
        // pick: sharded, every rank holds every sample row and every return, so pick and advance are local and alike on all ranks
        rc = l2a_lstm_advance(c->rnn, c->obs_map_dev, q->act_dev, c->c0, c->h0, m, c->c1, c->h1, c->stream);
        if (rc != L2A_OK) return rc;
    }
    q->cur = cur;
    return read_back(c);
}

// ---- MPPI (device mode) ---------------------------------------------------------------------------------------------------------
// Everything of one MPPI plan step, in stream order on `stream`; nothing on the host waits.  Reads the committed mean and the reset
// marks and writes neither: a replay launches the same step again.
int mppi_launch(l2a_controller* c) {
    l2a_ctx* ctx = c->ctx;
    mppi_state* q = c->mppi;
    const int m = c->m, n = c->n, h = c->h, A = c->act_dim;
    const unsigned long long per_iter = (unsigned long long)n * m * q->D, seed = c->device.seed;
    const bool sharded = c->shard.on;
    const int lo = c->shard.lo, hi = c->shard.hi;
    const float* low = q->lowhigh;
    const float* high = q->lowhigh + A;
    l2a_device_guard guard(ctx->device);
    int rc = launch_prelude(c);
    if (rc != L2A_OK) return rc;
    int src = q->cur;
    for (int it = 0; it < q->iters; ++it) {
        const int dst = spare_copy(q, src);
        const int* shift = it == 0 ? q->first : q->shift + m;
        const unsigned long long offset = (q->iter_calls + it) * per_iter;
        // (sharded: every rank samples all n rows of the same stream and keeps the rollout tensor of its candidates [lo, hi) only)
        rc = sharded ? l2a_mppi_sample_shard(ctx, nullptr, seed, offset, q->mean[src], shift, q->sigma, q->beta, low, high, n, m, h, A, lo,
                                             hi, q->mean[dst], q->a_clip, q->seq, c->stream)
                     : l2a_mppi_sample(ctx, nullptr, seed, offset, q->mean[src], shift, q->sigma, q->beta, low, high, n, m, h, A,
                                       q->mean[dst], q->a_clip, q->seq, c->stream);
        if (rc != L2A_OK) return rc;
        if (it == 0) ctx->stamps_us[1] = l2a_now_us();
        float* rets = q->rets + (size_t)it * m * n;
        rc = gather_returns(c, rets, n, lo, hi);
        if (rc == L2A_OK) rc = l2a_mppi_update(ctx, rets, q->a_clip, n, m, h, A, q->kappa, q->mean[dst], q->packed_dev, c->stream);
        if (rc != L2A_OK) return rc;
        src = dst;
    }
    q->last = src;
    return read_back(c);
}

// ---- iCEM (device mode) ---------------------------------------------------------------------------------------------------------
// Everything of one iCEM plan step, in stream order on `stream`; nothing on the host waits.  Reads the committed copy of the state and
// the reset marks and writes neither: a replay launches the same step again.
int icem_launch(l2a_controller* c) {
    l2a_ctx* ctx = c->ctx;
    icem_state* q = c->icem;
    const int m = c->m, n = c->n, h = c->h, A = c->act_dim, Kk = q->Kk;
    const unsigned long long per_iter = (unsigned long long)n * m * q->D, seed = c->device.seed;      // (the stride is the full n)
    const bool sharded = c->shard.on;
    const float* low = q->lowhigh;
    const float* high = q->lowhigh + A;
    l2a_device_guard guard(ctx->device);
    int rc = launch_prelude(c);
    if (rc != L2A_OK) return rc;
    int src = q->cur;
    for (int it = 0; it < q->iters; ++it) {
        const int dst = spare_copy(q, src);
        const int n_it = q->pops[it];
        int lo = 0, hi = n_it;
        if (sharded) icem_window(c, n_it, &lo, &hi);
        const int* shift = it == 0 ? q->first : q->shift + m;
        const unsigned long long offset = (q->iter_calls + it) * per_iter;
        const int add_mean = (q->add_mean && it == q->iters - 1) ? 1 : 0;
        const float* kept_in = Kk ? q->kept[src] : nullptr;
        const int* kc_in = Kk ? q->kc[src] : nullptr;
        // (sharded: every rank samples all n_it rows of the same stream and keeps the rollout tensor of its candidates [lo, hi) only)
        if (q->noise_on)                       // l2a_icem_controller_set_noise: nz = M z in place of the recurrence
            rc = sharded ? l2a_icem_sample_noise_shard(ctx, nullptr, seed, offset, q->mean[src], q->std[src], kept_in, kc_in, shift, q->sigma,
                                                       q->noise, low, high, n_it, m, h, A, Kk, add_mean, lo, hi, q->mean[dst], q->std[dst],
                                                       q->a_clip, q->seq, c->stream)
                         : l2a_icem_sample_noise(ctx, nullptr, seed, offset, q->mean[src], q->std[src], kept_in, kc_in, shift, q->sigma,
                                                 q->noise, low, high, n_it, m, h, A, Kk, add_mean, q->mean[dst], q->std[dst], q->a_clip,
                                                 q->seq, c->stream);
        else
            rc = sharded ? l2a_icem_sample_shard(ctx, nullptr, seed, offset, q->mean[src], q->std[src], kept_in, kc_in, shift, q->sigma, q->rho,
                                                 low, high, n_it, m, h, A, Kk, add_mean, lo, hi, q->mean[dst], q->std[dst], q->a_clip, q->seq,
                                                 c->stream)
                         : l2a_icem_sample(ctx, nullptr, seed, offset, q->mean[src], q->std[src], kept_in, kc_in, shift, q->sigma, q->rho, low,
                                           high, n_it, m, h, A, Kk, add_mean, q->mean[dst], q->std[dst], q->a_clip, q->seq, c->stream);
        if (rc != L2A_OK) return rc;
        if (it == 0) ctx->stamps_us[1] = l2a_now_us();
        float* rets = q->rets + q->ret_at[it];
        rc = gather_returns(c, rets, n_it, lo, hi);
        if (rc == L2A_OK)
            rc = l2a_icem_refit(ctx, rets, q->a_clip, low, high, n_it, m, h, A, q->K, Kk, q->alpha, q->work, q->mean[dst], q->std[dst],
                                Kk ? q->kept[dst] : nullptr, q->kc[dst], q->packed_dev + (size_t)it * m * q->row_floats, c->stream);
        if (rc != L2A_OK) return rc;
        src = dst;
    }
    q->last = src;
    return read_back(c);
}

// ---- what the CEM, the MPPI and the iCEM step share: begin, the verdicts, finish -----------------------------------------------------
int plan_launch(l2a_controller* c) {
    switch (c->plan->kind) {
    case PLAN_CEM: return cem_launch(c);
    case PLAN_MPPI: return mppi_launch(c);
    default: return icem_launch(c);
    }
}

int plan_begin(l2a_controller* c, const double* obs, const float* c0, const float* h0, float* c1, float* h1, void* stream) {
    l2a_ctx* ctx = c->ctx;
    if (!obs) return fail(ctx, L2A_EINVAL, "l2a_controller_begin: null obs");
    if (c->rnn) {                       // before anything is launched
        const int rc = check_next_state(c, c0, h0, c1, h1);
        if (rc != L2A_OK) return rc;
    }
    if (c->in_flight) return fail(ctx, L2A_ESTATE, "l2a_controller_begin: the previous step was not finished (l2a_controller_finish)");
    if (ctx->cem_steps_in_flight + ctx->rs_steps_in_flight > 0)
        return fail(ctx, L2A_ESTATE, "l2a_controller_begin: another controller's step is in flight on this context (a CEM step reads and "
                                     "clears the context's launch status word: finish the other step first)");
    c->t_begin = c->t_taken = l2a_now_us();
    stage_obs(c, obs, c0, h0, c1, h1, stream);
    c->result = L2A_OK;
    if (c->warm) first_shift(c);
    if (c->shard.on) c->shard.digest = plan_digest(c);
    const int rc = plan_launch(c);
    if (rc != L2A_OK) return rc;
    ctx->stamps_us[3] = l2a_now_us();
    set_in_flight(c, true);
    return L2A_OK;
}

// Unsharded: this context's own status word decides, and a flag with the tile split already disabled fails at once.
int plan_verdict(l2a_controller* c) {
    l2a_ctx* ctx = c->ctx;
    if (*ctx->status_host == 0) return L2A_OK;
    *ctx->status_host = 0;
    return ctx->split_policy == 0 ? fail(ctx, L2A_ESPLIT, SPLIT_OFF) : FLAGGED;
}

// Sharded: the REDUCED verdict alone decides - it is the same on every rank, so the ranks never disagree on the number of
// collectives.  This rank's own status word travelled in its words; it is consumed here and never consulted.
int plan_verdict_sharded(l2a_controller* c) {
    l2a_ctx* ctx = c->ctx;
    const plan_state* q = c->plan;
    *ctx->status_host = 0;
    unsigned int verdict[3];
    std::memcpy(verdict, q->packed_host + (q->packed_floats - 3), sizeof(verdict));
    const std::string kind = q->name;
    if (verdict[2] != 0)
        return fail(ctx, L2A_ESTATE, kind + " needs identically built controllers in step on every rank (same seed, step count, m, n, h, iters, "
                                         + q->facts + "): the ranks' digests differ");
    if (verdict[1] != 0)
        return fail(ctx, L2A_ESTATE, kind + ": " + std::to_string(verdict[1]) + " returns of this step were contributed by no rank "
                                     "(the collective did not reduce over every rank of the plan)");
    return verdict[0] == 0 ? L2A_OK : FLAGGED;
}

// Wait for the packed result; a launch flagged invalid (a tile-split partner that was not co-resident) repeats the whole step unsplit
// with the same Philox offsets - the same bits - as get_cem_action_device's and get_mppi_action's retry does (sharded: all ranks
// together).  Only a step that got this far moves the controller on: the stream position, MPPI's mean and reset marks, iCEM's state
// (mean, spread, kept rows and counts move as one index) and reset marks.
int plan_finish(l2a_controller* c, double* action_out, long long* index_out, float* return_out) {
    l2a_ctx* ctx = c->ctx;
    if (!action_out) return fail(ctx, L2A_EINVAL, "l2a_controller_finish: null action_out");
    if (!c->in_flight) return fail(ctx, L2A_ESTATE, "l2a_controller_finish: no step is in flight (l2a_controller_begin)");
    set_in_flight(c, false);
    plan_state* q = c->plan;
    int result = c->result;
    const auto relaunch = [c] { return plan_launch(c); };
    const int rc = c->shard.on ? settle(c, &result, [c] { return plan_verdict_sharded(c); }, relaunch)
                               : settle(c, &result, [c] { return plan_verdict(c); }, relaunch);
    if (rc != L2A_OK) return rc;
    const double t2 = l2a_now_us();
    const int A = c->act_dim, W = q->row_floats;
    for (int i = 0; i < c->m; ++i) {
        const float* r = q->packed_host + q->rows_at + (size_t)i * W;   // the action | the return | the index's bits | ...
        int idx = 0;
        std::memcpy(&idx, r + A + 1, sizeof(int));
        for (int k = 0; k < A; ++k) action_out[(size_t)i * A + k] = (double)r[k];
        if (index_out) index_out[i] = idx;
        if (return_out) return_out[i] = r[A];
    }
    q->iter_calls += (unsigned long long)q->iters;
    if (warm_state* w = c->warm) {
        w->cur = w->last;
        w->fresh.assign((size_t)c->m, 0);
    }
    record_stages(c, t2, l2a_now_us());
    return result;
}

// ---- random shooting ---------------------------------------------------------------------------------------------------------------
// Sharded plan: this rank's launch, the payload packed on the device behind it, the ONE collective of the step, and the copy
// of the reduced words to page-locked memory - all in stream order, nothing on the host waits (policies/mpc_controller.py
// `_combine_keys` did the same from Python with torch.distributed).
int launch_sharded(l2a_controller* c, bool first) {
    l2a_ctx* ctx = c->ctx;
    auto& S = c->shard;
    l2a_device_guard guard(ctx->device);
    hipStream_t stream = reinterpret_cast<hipStream_t>(c->stream);
    ctx->stamps_us[1] = l2a_now_us();
    int rc = L2A_OK;
    if (S.hi > S.lo) rc = rollout(c, c->dev[c->slot], S.hi - S.lo, S.lo, nullptr);
    else L2A_HIP(ctx, hipMemsetAsync(c->keys_dev, 0, sizeof(unsigned long long) * (size_t)c->m, stream));    // the neutral key
    if (rc == L2A_OK) rc = l2a_plan_payload(ctx, c->keys_dev, c->m, S.digest, S.payload_dev, c->stream);
    if (rc != L2A_OK) return rc;
    ctx->stamps_us[2] = l2a_now_us();
    if (first && !c->device.on) (c->result == L2A_STEP_DREW ? kick_arm : kick_next)(c);
    ctx->stamps_us[3] = l2a_now_us();
    rc = reduce_words(c, S.payload_dev, c->m + 3);
    if (rc != L2A_OK) return rc;
    if (c->rnn && c->c1) {
        // the controller's own state moves on with the GLOBAL winner's first action (rnn_mpc_controller.py:63), in stream order behind
        // the collective: the reduced keys index the whole plan's first step - the fp32 table of this block (parity mode) or the
        // Philox stream itself (device mode) - with the index clamped: the keys of a flagged launch, a neutral key or a placeholder
        // may hold anything, and the state written from them is overwritten by the relaunch or dropped with the failed step
        rc = l2a_lstm_advance_keys(c->rnn, c->obs_map_dev, S.payload_dev, c->device.on ? nullptr : c->ahead.tab_dev[c->slot], c->n,
                                   c->device.seed, c->device.offset, c->device.lowr, c->c0, c->h0, c->c1, c->h1, c->m, c->stream);
        if (rc != L2A_OK) return rc;
    }
    L2A_HIP(ctx, hipMemcpyAsync(S.payload_host, S.payload_dev, sizeof(unsigned long long) * (size_t)(c->m + 3), hipMemcpyDeviceToHost, stream));
    L2A_HIP(ctx, hipEventRecord(c->done, stream));
    return L2A_OK;
}

// Device-RNG mode: the candidates of this step are elements [offset, offset + h m n act_dim) of the stream (seed), drawn on the
// launch stream.
int fill_device(l2a_controller* c, hipStream_t stream) {
    auto& D = c->device;
    const auto& S = c->shard;
    D.offset = D.calls * (unsigned long long)((c->glob_floats + 3) / 4 * 4);
    l2a_device_guard guard(c->ctx->device);
    if (!S.on || S.world == 1) {
        const long long total = (long long)c->glob_floats;
        hipLaunchKernelGGL(l2a_uniform_fill_k, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, stream, D.seed, D.offset, total,
                           c->act_dim, D.lowr, c->dev[0]);
    } else if (S.hi > S.lo) {
        const long long total = (long long)c->h * c->m * (S.hi - S.lo) * c->act_dim;
        hipLaunchKernelGGL(l2a_uniform_fill_shard_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, D.seed, D.offset, total,
                           c->n, S.lo, S.hi - S.lo, c->act_dim, D.lowr, c->dev[0]);
    }
    L2A_HIP(c->ctx, hipGetLastError());
    return L2A_OK;
}

// Parity mode, no valid block waiting: the reference's own draw (mpc_controller.py:67-69,114) from the global generator, advanced
// in place, into the idle slot `*slot_out` and uploaded on the launch stream.  Returns L2A_OK, L2A_STEP_MISS or a negative code.
int draw_now(l2a_controller* c, hipStream_t stream, int* slot_out) {
    l2a_ctx* ctx = c->ctx;
    auto& a = c->ahead;
    if (!a.upload_err.empty()) { const std::string msg = a.upload_err; a.upload_err.clear(); return fail(ctx, L2A_EHIP, msg); }
    const int slot = l2a_ahead_idle_slot(a.chain);
    if (slot < 0) return L2A_STEP_MISS;                     // (a forked child, or a chain somebody else is driving)
    struct np_state { unsigned int key[624]; int pos; };
    np_state* g = static_cast<np_state*>(a.np_addr);
    if (l2a_mt19937_uniform_rows(g->key, &g->pos, (long long)c->h * c->n * c->m, c->act_dim, c->low, c->high, c->n, c->shard.lo, c->shard.hi,
                                 a.pin[slot], (long long)c->n * c->m, a.c64[slot], a.rng_threads) != 0)
        return fail(ctx, L2A_EINVAL, "l2a_controller_step: the generator state at np_state_addr is not a legacy MT19937 state");
    l2a_device_guard guard(ctx->device);
    if (c->shard.hi > c->shard.lo)
        L2A_HIP(ctx, hipMemcpyAsync(c->dev[slot], a.pin[slot], c->act_floats * sizeof(float), hipMemcpyHostToDevice, stream));
    if (a.tab_dev[slot]) L2A_HIP(ctx, upload_table(c, slot, stream));
    c->sync_draws += 1;
    *slot_out = slot;
    return L2A_OK;
}

// First half of a step: everything that touches the generator (take / draw, re-arm), the staging and the launch.  Returns
// L2A_OK (plan in flight), L2A_STEP_MISS (nothing consumed or launched) or a negative code.
int begin(l2a_controller* c, const double* obs, const float* c0, const float* h0, float* c1, float* h1, void* stream) {
    if (c->plan) return plan_begin(c, obs, c0, h0, c1, h1, stream);
    l2a_ctx* ctx = c->ctx;
    if (ctx->cem_steps_in_flight > 0)
        return fail(ctx, L2A_ESTATE, "l2a_controller_begin: a CEM step of another controller is in flight on this context (it reads and "
                                     "clears the context's launch status word: finish it first)");
    if (!obs) return fail(ctx, L2A_EINVAL, "l2a_controller_begin: null obs");
    if (c->in_flight) return fail(ctx, L2A_ESTATE, "l2a_controller_begin: the previous step was not finished (l2a_controller_finish)");
    if (c->shard.on && c->rnn) {        // before anything is consumed
        const int rc = check_next_state(c, c0, h0, c1, h1);
        if (rc != L2A_OK) return rc;
    }
    const double t0 = l2a_now_us();
    int slot = 0;
    bool drew = false;
    if (c->device.on) {
        const int rc = fill_device(c, reinterpret_cast<hipStream_t>(stream));
        if (rc != L2A_OK) return rc;
    } else if ((slot = l2a_ahead_take(c->ahead.chain, c->ahead.np_addr)) < 0) {
        const int rc = draw_now(c, reinterpret_cast<hipStream_t>(stream), &slot);
        if (rc != L2A_OK) return rc;
        drew = true;
    } else {
        c->ahead.misses_in_row = 0;
    }
    c->slot = slot;
    c->t_begin = t0;
    c->t_taken = l2a_now_us();
    stage_obs(c, obs, c0, h0, c1, h1, stream);
    c->result = drew ? L2A_STEP_DREW : L2A_OK;
    int rc;
    if (c->shard.on) {
        // what this rank's candidates were drawn from: the generator as this step's draw left it (every rank must agree)
        // (device mode: the stream's seed and position - ranks seeded differently, or out of step, would plan on different candidates)
        c->shard.digest = c->device.on ? (c->device.seed * 0x9E3779B97F4A7C15ull) ^ (c->device.calls + 1ull)
                                       : l2a_mt19937_state_digest(c->ahead.np_addr);
        ctx->stamps_us[0] = t0;
        rc = launch_sharded(c, true);
    } else {
        rc = rollout_sync(c, nullptr, c->device.on ? nullptr : (drew ? kick_arm : kick_next), &c->pending);
    }
    if (rc != L2A_OK) return rc;
    set_in_flight(c, true);
    return L2A_OK;
}

// The sharded step's reduced words: the digest pair must add up; the reduced flag is the same on every rank, so all of them switch
// to the unsplit geometry (bit-identical results) and repeat launch + collective together (also a rank that runs unsplit already: it
// must stay in step with the others' collective).  The context's split policy is not consulted.
int verdict_sharded(l2a_controller* c) {
    l2a_ctx* ctx = c->ctx;
    const unsigned long long* v = c->shard.payload_host;
    if (v[c->m + 1] + v[c->m + 2] != L2A_DIGEST_MASK)
        return fail(ctx, L2A_ESTATE, c->device.on
            ? "candidate sharding needs identical seeds and step counts on every rank (device RNG: build every rank's controller "
              "with the same seed at the same step)"
            : "candidate sharding needs identical np.random global state on every rank (seed all ranks alike and "
              "keep other consumers of the generator off the planning process; the shards themselves are disjoint)");
    if (v[c->m] == 0) return L2A_OK;
    *ctx->status_host = 0;
    return FLAGGED;
}

// Second half: wait for the keys (a launch that lost its tile-split partner is repeated unsplit - same bits; the generator is not
// touched again), decode, gather the winners' float64 first actions.
int finish(l2a_controller* c, double* action_out, long long* index_out, float* return_out) {
    if (c->plan) return plan_finish(c, action_out, index_out, return_out);
    l2a_ctx* ctx = c->ctx;
    if (!action_out) return fail(ctx, L2A_EINVAL, "l2a_controller_finish: null action_out");
    if (!c->in_flight) return fail(ctx, L2A_ESTATE, "l2a_controller_finish: no step is in flight (l2a_controller_begin)");
    set_in_flight(c, false);
    unsigned long long keys[L2A_MAIL_KEYS];
    int result = c->result;
    int rc;
    if (c->shard.on) {
        rc = settle(c, &result, [c] { return verdict_sharded(c); }, [c] { return launch_sharded(c, false); });
        if (rc == L2A_OK) std::memcpy(keys, c->shard.payload_host, sizeof(unsigned long long) * (size_t)c->m);
    } else if ((rc = l2a_plan_finish(ctx, &c->pending, keys)) == L2A_ESPLIT) {
        // a tile-split partner was not co-resident: the unsplit geometry gives the same bits (the caller is told: L2A_STEP_UNSPLIT)
        if (ctx->split_policy == 0) return fail(ctx, L2A_ESPLIT, SPLIT_OFF);
        (void)l2a_set_split(ctx, 0);
        c->relaunches += 1;
        result = L2A_STEP_UNSPLIT;
        rc = rollout_sync(c, keys, nullptr, nullptr);
        if (rc == L2A_ESPLIT) return fail(ctx, L2A_ESPLIT, SPLIT_OFF);
    }
    if (rc != L2A_OK) return rc;
    const double t2 = l2a_now_us();
    for (int i = 0; i < c->m; ++i) {
        float ret = 0.0f;
        int idx = 0;
        l2a_key_decode(keys[i], &ret, &idx);
        if (idx < 0 || idx >= c->n) return fail(ctx, L2A_EHIP, "l2a_controller_step: the arg-max key holds no candidate index");
        if (index_out) index_out[i] = idx;
        if (return_out) return_out[i] = ret;
        if (c->device.on) {
            // the winner's first action, recomputed from the counter-based stream: element (row i n + idx of step 0, dim k) -
            // the fp32 value the kernel planned on, as float64 (no gather launch, no copy back)
            for (int k = 0; k < c->act_dim; ++k) {
                const unsigned long long e = c->device.offset + ((unsigned long long)i * c->n + idx) * c->act_dim + k;
                action_out[(size_t)i * c->act_dim + k] =
                    (double)l2a_philox_uniform(c->device.seed, e, (float)c->low[k], (float)c->high[k] - (float)c->low[k]);
            }
        } else {
            std::memcpy(action_out + (size_t)i * c->act_dim, c->ahead.c64[c->slot] + ((size_t)i * c->n + idx) * c->act_dim,
                        sizeof(double) * (size_t)c->act_dim);                // cand_a[i, idx] (:118,129)
        }
    }
    record_stages(c, t2, l2a_now_us());
    return result;
}

int step(l2a_controller* c, const double* obs, const float* c0, const float* h0, float* c1, float* h1, double* action_out,
         long long* index_out, float* return_out, void* stream) {
    if (!obs || !action_out) return fail(c->ctx, L2A_EINVAL, "l2a_controller_step: null obs / action_out");
    const int rc = begin(c, obs, c0, h0, c1, h1, stream);
    if (rc != L2A_OK) return rc;
    return finish(c, action_out, index_out, return_out);
}

// ---- the plans' entry points between two steps: result, reset, reseed, set_noise ----------------------------------------------------
// `who` (the entry point) takes a controller of `kind` with no step in flight: the refusal of anything else, its text on the context.
int check_idle(l2a_controller* c, plan_kind kind, const char* who) {
    static const char* const NOUN[] = {"", "a CEM", "an MPPI", "an iCEM"};
    if (!c) return L2A_EINVAL;
    if (!c->plan || c->plan->kind != kind) return fail(c->ctx, L2A_EINVAL, std::string(who) + ": not " + NOUN[kind] + " controller");
    if (c->in_flight) return fail(c->ctx, L2A_ESTATE, std::string(who) + ": a step is in flight (l2a_controller_finish)");
    return L2A_OK;
}

// The marked envs' (null: every env's) next step starts afresh.
int warm_reset(l2a_controller* c, plan_kind kind, const char* who, const unsigned char* dones) {
    const int rc = check_idle(c, kind, who);
    if (rc == L2A_OK) mark_fresh(c, dones);
    return rc;
}

// The Philox stream restarts at 0 under `seed`; the plan is kept.
int warm_reseed(l2a_controller* c, plan_kind kind, const char* who, unsigned long long seed) {
    const int rc = check_idle(c, kind, who);
    if (rc != L2A_OK) return rc;
    c->device.seed = seed;
    c->plan->iter_calls = 0;
    return L2A_OK;
}

}  // namespace

extern "C" {

// The 16 create entry points: each names itself, its model and its options; `create` does the rest.
int l2a_controller_create(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                          const l2a_reward* reward, void* np_state_addr, int rng_threads, l2a_controller** out) {
    return create(step_cfg{"l2a_controller_create", model, nullptr, m, n, h, low, high, discount, reward, out}.parity(np_state_addr, rng_threads));
}

int l2a_controller_create_sharded(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                  const l2a_reward* reward, void* np_state_addr, int rng_threads, int rank, int world,
                                  l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out) {
    return create(step_cfg{"l2a_controller_create_sharded", model, nullptr, m, n, h, low, high, discount, reward, out}
                      .parity(np_state_addr, rng_threads).shard(rank, world, reduce, reduce_arg));
}

int l2a_controller_create_sharded_device(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                         const l2a_reward* reward, unsigned long long seed, int rank, int world,
                                         l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out) {
    return create(step_cfg{"l2a_controller_create_sharded_device", model, nullptr, m, n, h, low, high, discount, reward, out}
                      .device(seed).shard(rank, world, reduce, reduce_arg));
}

int l2a_lstm_controller_create(l2a_lstm* model, int m, int n, int h, const double* low, const double* high, double discount,
                               const l2a_reward* reward, void* np_state_addr, int rng_threads, l2a_controller** out) {
    return create(step_cfg{"l2a_lstm_controller_create", nullptr, model, m, n, h, low, high, discount, reward, out}.parity(np_state_addr, rng_threads));
}

int l2a_lstm_controller_create_sharded(l2a_lstm* model, int m, int n, int h, const double* low, const double* high, double discount,
                                       const l2a_reward* reward, void* np_state_addr, int rng_threads, int rank, int world,
                                       l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out) {
    return create(step_cfg{"l2a_lstm_controller_create_sharded", nullptr, model, m, n, h, low, high, discount, reward, out}
                      .parity(np_state_addr, rng_threads).shard(rank, world, reduce, reduce_arg));
}

int l2a_lstm_controller_create_sharded_device(l2a_lstm* model, int m, int n, int h, const double* low, const double* high,
                                              double discount, const l2a_reward* reward, unsigned long long seed, int rank, int world,
                                              l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out) {
    return create(step_cfg{"l2a_lstm_controller_create_sharded_device", nullptr, model, m, n, h, low, high, discount, reward, out}
                      .device(seed).shard(rank, world, reduce, reduce_arg));
}

int l2a_controller_create_device(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                 const l2a_reward* reward, unsigned long long seed, l2a_controller** out) {
    return create(step_cfg{"l2a_controller_create_device", model, nullptr, m, n, h, low, high, discount, reward, out}.device(seed));
}

int l2a_lstm_controller_create_device(l2a_lstm* model, int m, int n, int h, const double* low, const double* high, double discount,
                                      const l2a_reward* reward, unsigned long long seed, l2a_controller** out) {
    return create(step_cfg{"l2a_lstm_controller_create_device", nullptr, model, m, n, h, low, high, discount, reward, out}.device(seed));
}

int l2a_cem_controller_create_device(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                     const l2a_reward* reward, int iters, int num_elites, float alpha, int reference,
                                     unsigned long long seed, l2a_controller** out) {
    return create(step_cfg{"l2a_cem_controller_create_device", model, nullptr, m, n, h, low, high, discount, reward, out}
                      .cem_plan(iters, num_elites, alpha, reference, seed));
}

int l2a_cem_controller_create_sharded_device(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                             const l2a_reward* reward, int iters, int num_elites, float alpha, int reference,
                                             unsigned long long seed, int rank, int world, l2a_reduce_fn reduce, void* reduce_arg,
                                             l2a_controller** out) {
    return create(step_cfg{"l2a_cem_controller_create_sharded_device", model, nullptr, m, n, h, low, high, discount, reward, out}
                      .cem_plan(iters, num_elites, alpha, reference, seed).shard(rank, world, reduce, reduce_arg));
}

int l2a_lstm_cem_controller_create_device(l2a_lstm* model, int m, int n, int h, const double* low, const double* high, double discount,
                                          const l2a_reward* reward, int iters, int num_elites, float alpha, int reference,
                                          unsigned long long seed, l2a_controller** out) {
    return create(step_cfg{"l2a_lstm_cem_controller_create_device", nullptr, model, m, n, h, low, high, discount, reward, out}
                      .cem_plan(iters, num_elites, alpha, reference, seed));
}

int l2a_lstm_cem_controller_create_sharded_device(l2a_lstm* model, int m, int n, int h, const double* low, const double* high,
                                                  double discount, const l2a_reward* reward, int iters, int num_elites, float alpha,
                                                  int reference, unsigned long long seed, int rank, int world, l2a_reduce_fn reduce,
                                                  void* reduce_arg, l2a_controller** out) {
    return create(step_cfg{"l2a_lstm_cem_controller_create_sharded_device", nullptr, model, m, n, h, low, high, discount, reward, out}
                      .cem_plan(iters, num_elites, alpha, reference, seed).shard(rank, world, reduce, reduce_arg));
}

int l2a_cem_controller_result(l2a_controller* c, float* mean_out, float* std_out, float* returns_out) {
    const int rc = check_idle(c, PLAN_CEM, "l2a_cem_controller_result");
    if (rc != L2A_OK) return rc;
    if (c->steps == 0) return fail(c->ctx, L2A_ESTATE, "l2a_cem_controller_result: no step has finished yet");
    cem_state* q = c->cem;
    const size_t md = (size_t)c->m * q->D;
    const float* tail = q->packed_host + (size_t)c->m * (c->act_dim + 2);
    if (mean_out) std::memcpy(mean_out, tail, sizeof(float) * md);
    if (std_out) std::memcpy(std_out, tail + md, sizeof(float) * md);
    if (returns_out) {
        l2a_device_guard guard(c->ctx->device);
        L2A_HIP(c->ctx, hipMemcpy(returns_out, q->rets, sizeof(float) * (size_t)q->iters * c->m * c->n, hipMemcpyDeviceToHost));
    }
    return L2A_OK;
}

int l2a_mppi_controller_create_device(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                      const l2a_reward* reward, int iters, float kappa, float beta, const double* sigma,
                                      unsigned long long seed, l2a_controller** out) {
    return create(step_cfg{"l2a_mppi_controller_create_device", model, nullptr, m, n, h, low, high, discount, reward, out}
                      .mppi_plan(iters, kappa, beta, sigma, seed));
}

int l2a_mppi_controller_create_sharded_device(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                              const l2a_reward* reward, int iters, float kappa, float beta, const double* sigma,
                                              unsigned long long seed, int rank, int world, l2a_reduce_fn reduce, void* reduce_arg,
                                              l2a_controller** out) {
    return create(step_cfg{"l2a_mppi_controller_create_sharded_device", model, nullptr, m, n, h, low, high, discount, reward, out}
                      .mppi_plan(iters, kappa, beta, sigma, seed).shard(rank, world, reduce, reduce_arg));
}

int l2a_mppi_controller_reset(l2a_controller* c, const unsigned char* dones) {
    return warm_reset(c, PLAN_MPPI, "l2a_mppi_controller_reset", dones);
}

int l2a_mppi_controller_reseed(l2a_controller* c, unsigned long long seed) {
    return warm_reseed(c, PLAN_MPPI, "l2a_mppi_controller_reseed", seed);
}

int l2a_mppi_controller_result(l2a_controller* c, float* mean_out, float* ess_out, int* valid_out, float* returns_out) {
    const int rc = check_idle(c, PLAN_MPPI, "l2a_mppi_controller_result");
    if (rc != L2A_OK) return rc;
    if (c->steps == 0) return fail(c->ctx, L2A_ESTATE, "l2a_mppi_controller_result: no step has finished yet");
    mppi_state* q = c->mppi;
    const int A = c->act_dim;
    for (int i = 0; i < c->m; ++i) {
        const float* r = q->packed_host + (size_t)i * q->row_floats;
        if (ess_out) ess_out[i] = r[A + 2];
        if (valid_out) std::memcpy(&valid_out[i], r + A + 3, sizeof(int));
    }
    if (!mean_out && !returns_out) return L2A_OK;
    // ONE copy to page-locked memory on the step's stream - the three means and, when asked for, the returns behind them - and one wait
    const size_t md = (size_t)c->m * q->D, nr = (size_t)q->iters * c->m * c->n;
    hipStream_t stream = reinterpret_cast<hipStream_t>(c->stream);
    l2a_device_guard guard(c->ctx->device);
    L2A_HIP(c->ctx, hipMemcpyAsync(q->result_host, q->mean[0], sizeof(float) * (3 * md + (returns_out ? nr : 0)), hipMemcpyDeviceToHost, stream));
    L2A_HIP(c->ctx, hipStreamSynchronize(stream));
    if (mean_out) std::memcpy(mean_out, q->result_host + (size_t)q->cur * md, sizeof(float) * md);
    if (returns_out) std::memcpy(returns_out, q->result_host + 3 * md, sizeof(float) * nr);
    return L2A_OK;
}

int l2a_icem_controller_create_device(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                      const l2a_reward* reward, int iters, const int* pops, int K, int Kk, float alpha, float rho,
                                      const double* sigma0, int add_mean, unsigned long long seed, l2a_controller** out) {
    return create(step_cfg{"l2a_icem_controller_create_device", model, nullptr, m, n, h, low, high, discount, reward, out}
                      .icem_plan(iters, pops, K, Kk, alpha, rho, sigma0, add_mean, seed));
}

int l2a_icem_controller_create_sharded_device(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                              const l2a_reward* reward, int iters, const int* pops, int K, int Kk, float alpha, float rho,
                                              const double* sigma0, int add_mean, unsigned long long seed, int rank, int world,
                                              l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out) {
    return create(step_cfg{"l2a_icem_controller_create_sharded_device", model, nullptr, m, n, h, low, high, discount, reward, out}
                      .icem_plan(iters, pops, K, Kk, alpha, rho, sigma0, add_mean, seed).shard(rank, world, reduce, reduce_arg));
}

int l2a_icem_controller_reset(l2a_controller* c, const unsigned char* dones) {
    return warm_reset(c, PLAN_ICEM, "l2a_icem_controller_reset", dones);
}

int l2a_icem_controller_reseed(l2a_controller* c, unsigned long long seed) {
    return warm_reseed(c, PLAN_ICEM, "l2a_icem_controller_reseed", seed);
}

int l2a_icem_controller_result(l2a_controller* c, float* mean_out, float* std_out, float* kept_out, int* kc_out, float* heads_out,
                               float* returns_out) {
    const int rc = check_idle(c, PLAN_ICEM, "l2a_icem_controller_result");
    if (rc != L2A_OK) return rc;
    if (c->steps == 0) return fail(c->ctx, L2A_ESTATE, "l2a_icem_controller_result: no step has finished yet");
    icem_state* q = c->icem;
    const size_t m = (size_t)c->m, md = m * q->D, kd = m * (size_t)q->Kk * q->D;
    if (heads_out) std::memcpy(heads_out, q->packed_host, sizeof(float) * (size_t)q->iters * m * q->row_floats);
    if (!mean_out && !std_out && !kept_out && !kc_out && !returns_out) return L2A_OK;
    // ONE copy to page-locked memory on the step's stream - the state's three copies and, when asked for, the returns behind them - and
    // one wait
    const size_t nr = q->ret_at[q->iters];
    hipStream_t stream = reinterpret_cast<hipStream_t>(c->stream);
    l2a_device_guard guard(c->ctx->device);
    L2A_HIP(c->ctx, hipMemcpyAsync(q->result_host, q->mean[0], sizeof(float) * (q->head_floats + (returns_out ? nr : 0)),
                                   hipMemcpyDeviceToHost, stream));
    L2A_HIP(c->ctx, hipStreamSynchronize(stream));
    const float* host = q->result_host;
    const size_t cur = (size_t)q->cur;
    if (mean_out) std::memcpy(mean_out, host + (q->mean[cur] - q->mean[0]), sizeof(float) * md);
    if (std_out) std::memcpy(std_out, host + (q->std[cur] - q->mean[0]), sizeof(float) * md);
    if (kept_out && kd) std::memcpy(kept_out, host + (q->kept[cur] - q->mean[0]), sizeof(float) * kd);
    if (kc_out) std::memcpy(kc_out, host + (reinterpret_cast<float*>(q->kc[cur]) - q->mean[0]), sizeof(int) * m);
    if (returns_out) std::memcpy(returns_out, host + q->head_floats, sizeof(float) * nr);
    return L2A_OK;
}

int l2a_icem_controller_set_noise(l2a_controller* c, const float* M_host) {
    const int rc = check_idle(c, PLAN_ICEM, "l2a_icem_controller_set_noise");
    if (rc != L2A_OK) return rc;
    icem_state* q = c->icem;
    if (!M_host) { q->noise_on = false; return L2A_OK; }
    if (c->h > L2A_ICEM_NOISE_MAX_H) return fail(c->ctx, L2A_EINVAL, "l2a_icem_controller_set_noise: h beyond L2A_ICEM_NOISE_MAX_H");
    const size_t count = (size_t)c->h * c->h;
    l2a_device_guard guard(c->ctx->device);
    if (!q->noise) q->noise = alloc<float>(c, MEM_DEVICE, count);
    // (no step is in flight, and a finished step was waited for: nothing on the device reads the matrix now)
    upload(c, q->noise, M_host, sizeof(float) * count);
    if (c->mem_err != hipSuccess) {
        const hipError_t e = c->mem_err;
        c->mem_err = hipSuccess;
        q->noise_on = false;
        return fail(c->ctx, L2A_EHIP, std::string("l2a_icem_controller_set_noise: ") + hipGetErrorString(e));
    }
    unsigned long long d = DIGEST_SEED;
    for (size_t e = 0; e < count; ++e) d = digest_mix(d, bits(M_host[e]));
    q->noise_hash = d;
    q->noise_on = true;
    return L2A_OK;
}

void l2a_controller_destroy(l2a_controller* c) {
    if (!c) return;
    if (c->ahead.chain) l2a_ahead_destroy(c->ahead.chain);    // joins the producer: no upload is in flight afterwards
    l2a_device_guard guard(c->ctx->device);
    if (c->in_flight) (void)hipDeviceSynchronize();           // a step begun and never finished: its launch still reads these buffers
    set_in_flight(c, false);
    release(c);
    delete c->cem;
    delete c->mppi;
    delete c->icem;
    delete c;
}

int l2a_controller_step(l2a_controller* c, const double* obs, double* action_out, long long* index_out, float* return_out,
                        void* stream) {
    if (!c) return L2A_EINVAL;
    if (!c->mlp) return fail(c->ctx, L2A_EINVAL, "l2a_controller_step: this controller plans with a recurrent model (l2a_lstm_controller_step)");
    return step(c, obs, nullptr, nullptr, nullptr, nullptr, action_out, index_out, return_out, stream);
}

int l2a_lstm_controller_step(l2a_controller* c, const double* obs, const float* c0, const float* h0, float* c_next, float* h_next,
                             double* action_out, long long* index_out, float* return_out, void* stream) {
    if (!c) return L2A_EINVAL;
    if (!c->rnn) return fail(c->ctx, L2A_EINVAL, "l2a_lstm_controller_step: this controller plans with an MLP model (l2a_controller_step)");
    if (!c0 || !h0) return fail(c->ctx, L2A_EINVAL, "l2a_lstm_controller_step: null c0 / h0");
    return step(c, obs, c0, h0, c_next, h_next, action_out, index_out, return_out, stream);
}

int l2a_controller_begin(l2a_controller* c, const double* obs, void* stream) {
    if (!c) return L2A_EINVAL;
    if (!c->mlp) return fail(c->ctx, L2A_EINVAL, "l2a_controller_begin: this controller plans with a recurrent model (l2a_lstm_controller_begin)");
    return begin(c, obs, nullptr, nullptr, nullptr, nullptr, stream);
}

int l2a_lstm_controller_begin(l2a_controller* c, const double* obs, const float* c0, const float* h0, float* c_next, float* h_next,
                              void* stream) {
    if (!c) return L2A_EINVAL;
    if (!c->rnn) return fail(c->ctx, L2A_EINVAL, "l2a_lstm_controller_begin: this controller plans with an MLP model (l2a_controller_begin)");
    if (!c0 || !h0) return fail(c->ctx, L2A_EINVAL, "l2a_lstm_controller_begin: null c0 / h0");
    return begin(c, obs, c0, h0, c_next, h_next, stream);
}

int l2a_controller_finish(l2a_controller* c, double* action_out, long long* index_out, float* return_out) {
    if (!c) return L2A_EINVAL;
    return finish(c, action_out, index_out, return_out);
}

int l2a_controller_rearm(l2a_controller* c) {
    if (!c) return L2A_EINVAL;
    if (c->device.on) return L2A_OK;
    if (l2a_ahead_arm(c->ahead.chain, c->ahead.np_addr) != 0) return fail(c->ctx, L2A_ESTATE, "l2a_controller_rearm: the producer thread could not be started");
    return L2A_OK;
}

const float* l2a_controller_actions(const l2a_controller* c) {
    return (c && c->slot >= 0) ? c->dev[c->slot] : nullptr;
}

int l2a_controller_stats(l2a_controller* c, double* out, int cap) {
    if (!c || !out || cap < 1) return L2A_EINVAL;
    double v[16] = {0};
    for (int i = 0; i < 7; ++i) v[i] = c->stage_us[i];
    double ch[6] = {0, 0, 0, 0, 0, 0};
    if (c->ahead.chain) l2a_ahead_stats(c->ahead.chain, ch);
    v[7] = (double)c->steps; v[8] = (double)c->relaunches;
    for (int i = 0; i < 6; ++i) v[9 + i] = ch[i];
    v[15] = (double)c->sync_draws;
    for (int i = 0; i < cap && i < 16; ++i) out[i] = v[i];
    return L2A_OK;
}

}  // extern "C"
