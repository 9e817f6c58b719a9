// l2a_lstm_api.hip - host side of the recurrent-planner entry points of include/l2a.h
// (l2a_lstm_*): model storage (raw TF-layout weights + MFMA-packed copies + normalisation), weight
// re-packing and the launch logic of the kernels in l2a_lstm.h.  Everything is enqueued on the
// caller's stream.

#define L2A_PACK_KERNELS 1      // this unit launches the weight re-packing kernels of l2a_micro_pack.h
#include "l2a_host.h"
#include "l2a_lstm.h"
#include "l2a_lstm_valu.h"
#include "l2a_lstm_launch.h"
#include "l2a_rnn_valu.h"
#include "l2a_rnn_mfma.h"
#include "l2a_micro_pack.h"
#include "l2a_micro_launch.h"
#include "l2a_philox.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// What the launcher's decisions read of a model: dimensions, layers and which kernels have an instance for them.  Computed by
// rnn_shape for both create functions and for l2a_lstm_plan_geometry.
struct l2a_rnn_shape {
    int obs_dim = 0, act_dim = 0, in_dim = 0, units = 0;
    int KG0 = 0, OT = 0, UTW = 0;
    bool mfma_ok = false;
    bool micro_ok = false;                        // the micro-tile kernel of l2a_micro.h has an instance (256 / 512 units)
    // generic stacks (l2a_rnn_create): any cell type / several layers -> l2a_rnn_valu_k; `units` = sum(lunits)
    bool generic = false;
    int n_layers = 1, cell_type = L2A_CELL_LSTM;
    int lunits[L2A_RNN_MAX_LAYERS] = {0};
    bool gmicro_ok = false;                       // the micro-tile kernel of l2a_rnn_micro.h has one (every layer 256 or every layer 512 units wide)
    bool gmicro4_ok = false;                      // ... with workgroups of four micro tiles (plans beyond three per CU)
};

struct l2a_lstm : l2a_rnn_shape {
    l2a_ctx* ctx = nullptr;
    int cell_act = L2A_ACT_TANH, output_act = L2A_ACT_IDENTITY;
    long long pk_mg = 0, pk_mo = 0;               // the micro-tile kernel's copies of the gate matrix / output layer
    float* wblk = nullptr;
    long long total = 0;
    long long raw_wk = 0, raw_bk = 0, raw_wo = 0, raw_bo = 0, pk_wg = 0, pk_wout = 0, pk_bout = 0, nm_off = 0;
    bool weights_set = false, norm_set = false;
    std::vector<float> norm_stage;
    l2a_xbuf xb;                                  // unit-tile split exchange granules
    long long lw[L2A_RNN_MAX_LAYERS][2] = {{0}}, lb[L2A_RNN_MAX_LAYERS][2] = {{0}};     // generic stacks: the layers' kernels / biases
    long long lpk[L2A_RNN_MAX_LAYERS][2] = {{0}};  // the kernels again in MFMA fragment order (l2a_rnn_mfma.h); pk_wout alike
    long long lmk[L2A_RNN_MAX_LAYERS][2] = {{0}};  // ... and in the micro-tile kernel's (l2a_rnn_micro.h)
    float* adv_buf = nullptr;                     // l2a_lstm_plan_rs_sync: [64, act_dim] chosen actions + [64, obs_dim] next obs
    float* traj_buf = nullptr;                    // l2a_lstm_plan_rs_program / _reward_model: [returns of the carry launches (rows) | trajectory (h x rows x obs_dim)]
    long long traj_buf_floats = 0;
    float* hid_buf = nullptr;                     // the carry chain's c / h: two pairs [c | h] of [rows, state width], used in turn
    long long hid_buf_floats = 0;
};

// First action of every env's winning candidate: out[i] = actions[step 0][i * n + (index(best_key[i]) - cand_offset)]
// (key layout: l2a_key_pack; the index is clamped, a launch flagged invalid may have left anything in the key).
__global__ void l2a_gather_best_k(const unsigned long long* best_key, const float* actions, int m, int n, int cand_offset,
                                  int act_dim, float* out) {
    const int i = blockIdx.x;
    if (i >= m) return;
    const unsigned int low = (unsigned int)(best_key[i] & 0x7fffffffull);
    int idx = (int)(0x7fffffffu - low) - cand_offset;
    idx = idx < 0 ? 0 : (idx >= n ? n - 1 : idx);
    for (int d = threadIdx.x; d < act_dim; d += blockDim.x)      // any action width (the generic cells take act_dim > 64)
        out[i * act_dim + d] = actions[((long long)i * n + idx) * act_dim + d];
}

// The same gather for a plan whose candidates are the counter-based stream (device-RNG mode, sharded: the winner usually belongs to
// another rank's slice, which this rank never filled): out[i] = element ((i * n + index(best_key[i])) * act_dim + d) of the step's
// stream - l2a_philox_uniform, the function the fill kernels and the host decode use, so the bits the owning rank rolled out.
__global__ void l2a_gather_best_philox_k(const unsigned long long* best_key, int m, int n, int act_dim, unsigned long long seed,
                                         unsigned long long offset, const float* lowr, float* out) {
    const int i = blockIdx.x;
    if (i >= m) return;
    const unsigned int low = (unsigned int)(best_key[i] & 0x7fffffffull);
    int idx = (int)(0x7fffffffu - low);
    idx = idx < 0 ? 0 : (idx >= n ? n - 1 : idx);
    for (int d = threadIdx.x; d < act_dim; d += blockDim.x)
        out[i * act_dim + d] = l2a_philox_uniform(seed, offset + ((unsigned long long)i * n + idx) * act_dim + d, lowr[d], lowr[16 + d]);
}

namespace {

bool lstm_mfma_eligible(int obs_dim, int act_dim, int units) {
    if (units != 128 && units != 256 && units != 512) return false;
    if (obs_dim < 1 || obs_dim > 16 * L2A_OTMAX) return false;
    if (act_dim < 1 || act_dim > 16) return false;
    if (obs_dim + act_dim > 16 * L2A_KG0MAX) return false;
    return true;
}

void fill(const l2a_lstm* md, L2ALstmParams& p) {
    std::memset(&p, 0, sizeof(p));
    p.wblk = md->wblk;
    p.raw_wk = md->raw_wk; p.raw_bk = md->raw_bk; p.raw_wo = md->raw_wo; p.raw_bo = md->raw_bo;
    p.pk_wg = md->pk_wg; p.pk_wout = md->pk_wout; p.pk_bout = md->pk_bout; p.nm_off = md->nm_off;
    p.pk_mg = md->pk_mg; p.pk_mo = md->pk_mo;
    p.obs_dim = md->obs_dim; p.act_dim = md->act_dim; p.in_dim = md->in_dim; p.units = md->units;
    p.cell_act = md->cell_act; p.output_act = md->output_act;
    p.KG0 = md->KG0; p.OT = md->OT;
    p.n_layers = md->n_layers; p.cell_type = md->cell_type;
    for (int l = 0; l < L2A_RNN_MAX_LAYERS; ++l) {
        p.layer_units[l] = md->lunits[l];
        for (int q = 0; q < 2; ++q) {
            p.layer_w[l][q] = md->lw[l][q]; p.layer_b[l][q] = md->lb[l][q]; p.layer_pk[l][q] = md->lpk[l][q]; p.layer_mk[l][q] = md->lmk[l][q];
        }
    }
    p.disc0 = 1.0;
}

// LDS of a 16-candidate tile's rows: the generic matrix-core kernel's padded ones, and the dense ones of the two VALU kernels
long long generic_mfma_smem(const l2a_rnn_shape& s) {
    const int gates = s.cell_type == L2A_CELL_LSTM ? 4 : (s.cell_type == L2A_CELL_GRU ? 3 : 1);
    return 4 * l2a_rnn_mfma_lds_floats(s.in_dim, s.obs_dim, s.n_layers, s.lunits, gates);
}
long long valu_smem(const l2a_rnn_shape& s) { return (long long)(s.in_dim + 3 * s.units + 2 * s.obs_dim + 1) * L2A_LVT * 4; }

// The shape of a model: `n_layers` layers of `units[]` cells - or, n_layers == 0, the model of l2a_lstm_create: one LSTM layer of
// units[0] on the LSTM kernels whatever its width.  Pure; `force_generic`: the developer switch L2A_FORCE_GENERIC.
l2a_rnn_shape rnn_shape(int obs_dim, int act_dim, int n_layers, const int* units, int cell_type, int lds_per_block, bool force_generic) {
    l2a_rnn_shape s;
    s.obs_dim = obs_dim; s.act_dim = act_dim; s.in_dim = obs_dim + act_dim;
    s.KG0 = l2a_ceil_div(s.in_dim, 16);
    s.OT = l2a_ceil_div(obs_dim, 16);
    // the run_rebal.py configuration, at the widths its tuned kernel is instantiated for: the model of l2a_lstm_create;
    // one LSTM layer of any other width takes the generic matrix-core kernel like the stacks below
    // (L2A_FORCE_GENERIC: developer switch - A/B of the generic kernels against the tuned one on its own shape)
    if (n_layers == 0 || (n_layers == 1 && cell_type == L2A_CELL_LSTM && lstm_mfma_eligible(obs_dim, act_dim, units[0]) && !force_generic)) {
        s.units = s.lunits[0] = units[0];
        s.mfma_ok = lstm_mfma_eligible(obs_dim, act_dim, units[0]);
        s.UTW = s.mfma_ok ? units[0] / (16 * L2A_NW) : 0;
        s.micro_ok = s.mfma_ok && (units[0] == 256 || units[0] == 512);
        return s;
    }
    s.generic = true;
    s.n_layers = n_layers; s.cell_type = cell_type;
    for (int l = 0; l < n_layers; ++l) { s.lunits[l] = units[l]; s.units += units[l]; }
    // micro tiles (l2a_rnn_micro.h): every layer 256 (or every layer 512) units wide, the input shapes of the tuned LSTM kernel,
    // LDS for the whole stack (256 units: up to three layers; 512: one GRU or BasicRNN layer)
    s.gmicro_ok = lstm_mfma_eligible(obs_dim, act_dim, 256) && (units[0] == 256 || (units[0] == 512 && cell_type != L2A_CELL_LSTM));
    for (int l = 0; l < n_layers; ++l) s.gmicro_ok = s.gmicro_ok && units[l] == units[0];
    s.gmicro_ok = s.gmicro_ok && l2a_rnn_micro_smem(cell_type, n_layers, units[0], s.KG0, 3) <= lds_per_block;
    // (and only where a 16-candidate kernel fits too - the matrix-core one or, for three-layer stacks, the VALU one: one-step
    // launches - predict, chunk continuations - stay with those)
    s.gmicro_ok = s.gmicro_ok && (generic_mfma_smem(s) <= lds_per_block || valu_smem(s) <= lds_per_block);
    s.gmicro4_ok = s.gmicro_ok && units[0] == 256 && l2a_rnn_micro_smem(cell_type, n_layers, 256, s.KG0, 4) <= lds_per_block;
    return s;
}
bool force_generic() {
    static const bool on = std::getenv("L2A_FORCE_GENERIC") != nullptr;
    return on;
}

// ---- the launch plan of a recurrent rollout: decided once by plan_rnn_launch (pure host arithmetic: no HIP call, no environment,
//      nothing written but the plan), then executed by launch() / rollout_traj() or reported by l2a_lstm_plan_geometry and
//      l2a_lstm_traj_geometry ------------------------------------------------------------------------------------------------------

// What the decision depends on beside the model and the request: the context's policies and device facts.
struct l2a_rnn_policy { int kernel_kind, split_policy, micro_policy, num_cu, lds_per_block; };
l2a_rnn_policy rnn_policy(const l2a_ctx* ctx) {
    return {ctx->kernel_kind, ctx->split_policy, ctx->micro_policy, ctx->num_cu > 0 ? ctx->num_cu : 256, ctx->lds_per_block};
}

struct l2a_rnn_request {
    int m, n, h;
    bool per_row, state_out, results;   // per-row start states | a state is written out (state_out, c_out or h_out) | returns or keys are wanted
    bool allow_split;                   // the unit-tile split may be taken
    bool traj;                          // the trajectory rollout (rollout_traj): its single launch, or one step of its carry chain
};

enum { L2A_RNN_LSTM_VALU = 0, L2A_RNN_LSTM_MFMA16 = 1, L2A_RNN_LSTM_MICRO = 2, L2A_RNN_LSTM_MICRO_TRAJ = 3,
       L2A_RNN_GENERIC_VALU = 4, L2A_RNN_GENERIC_MFMA16 = 5, L2A_RNN_GENERIC_MICRO = 6 };   // (the numbers l2a_lstm_plan_geometry reports)

// One kernel launch: the family, its grid and LDS, and every geometry field of L2ALstmParams (fields a family does not read are 0).
struct l2a_rnn_launch {
    int family;
    int mtm;                // micro tiles the instance's workgroups hold (3; generic stacks: 3 or 4), 0: a 16-candidate kernel
    unsigned grid;
    long long smem;
    long long xbuf_bytes;   // exchange buffer of the unit-tile split; 0 = none
    int tiles_per_env, mc_w, mc_hi, mc_r, split;
};

// Does a launch on 16-candidate tiles take a matrix-core kernel?  Generic models (stacks / GRU / BasicRNN / odd LSTM widths): the
// kernel of l2a_rnn_mfma.h unless the caller asked for the VALU one, or its padded LDS rows do not fit (the VALU kernel's dense
// rows may still); one LSTM layer: the tuned kernel where the shape has an instance, or where the caller asked for it (the plan
// then fails).  Also WHETHER A BLOCKING PLAN PUBLISHES through the mailbox (l2a_lstm_plan_rs_sync_hook): only the matrix-core
// kernels have the mailbox epilogue.  That is not "the plan's family is not a VALU one": a stack whose matrix-core rows do not
// fit while gmicro_ok holds through the VALU kernel's rows (three 256-unit LSTM layers) launches micro tiles and does not publish.
bool rnn_uses_mfma(const l2a_rnn_shape& md, const l2a_rnn_policy& pol) {
    if (md.generic)
        return pol.kernel_kind != L2A_KERNEL_VALU && generic_mfma_smem(md) <= pol.lds_per_block;
    return pol.kernel_kind == L2A_KERNEL_AUTO ? md.mfma_ok : pol.kernel_kind == L2A_KERNEL_MFMA;
}

// Micro tiles for the tuned LSTM kernel (l2a_micro.h): l2a_deal_micro, at most three per workgroup - one workgroup per CU, none
// idle, no exchange.
bool lstm_micro_wanted(bool micro_ok, int micro_policy, int cus_m, int m, int n, l2a_micro_deal* g) {
    const long long tiles16 = (long long)m * l2a_ceil_div(n, 16);
    *g = l2a_deal_micro(cus_m, m, n, 3);
    const int hi = g->hi;
    // automatic (profiles/r04_ab_micro.jsonl): the plans the 16-candidate geometries cannot fill - more than CUs / 2
    // tiles (no unit-tile split) and fewer than CUs (the ReBAL default: 0.91 of the 16-candidate launch; 512 units: 0.85)
    // - and plans of at most one micro tile per CU (0.87 - 0.95 of the unit-tile split); in between the unit-tile
    // split wins (1.04 - 1.16).
    const bool unfilled = 2 * tiles16 > cus_m && tiles16 < cus_m;
    const bool wanted = micro_policy == 2 || (micro_policy == 1 && (unfilled || hi == 1));
    return micro_ok && hi <= 3 && wanted;
}

// The launch of one request, or an error code with its message.
int plan_rnn_launch(const l2a_rnn_shape& md, const l2a_rnn_policy& pol, l2a_rnn_request rq, l2a_rnn_launch* d, std::string* err) {
    auto bad = [err](int code, const std::string& msg) { *err = msg; return code; };
    *d = l2a_rnn_launch();
    const int cus = pol.num_cu;
    const bool mfma = rnn_uses_mfma(md, pol);
    auto micro_tiles = [&](int family, int mtm, const l2a_micro_deal& g, long long smem) {
        d->family = family; d->mtm = mtm;
        d->mc_w = g.W; d->mc_hi = g.hi; d->mc_r = g.mc_r;
        d->grid = (unsigned)(rq.m * g.W);
        d->smem = smem < 84 * 1024 ? 84 * 1024 : smem;      // more than half a CU's LDS: one workgroup per CU
        return L2A_OK;
    };
    d->tiles_per_env = l2a_ceil_div(rq.n, 16);              // (16 = L2A_LVT: every 16-candidate kernel's tile)
    l2a_micro_deal g = {0, 99, 0};
    const bool lstm_micro = !md.generic && mfma && md.mfma_ok && lstm_micro_wanted(md.micro_ok, pol.micro_policy, cus, rq.m, rq.n, &g);
    if (rq.traj) {
        // The trajectory rollout: the single launch where the fused plan would take micro tiles, on the matrix-core kernels, with
        // a step's slices of the trajectory and of the actions inside one buffer descriptor each (the kernel's range check) ...
        const long long rows = (long long)rq.m * rq.n;
        if (lstm_micro && rows * md.obs_dim * 4 < 0x7ffffff0LL && rows * md.act_dim * 4 < 0x7ffffff0LL)
            return micro_tiles(L2A_RNN_LSTM_MICRO_TRAJ, 3, g, l2a_lstm_micro_smem(md.units, md.KG0));
        // ... else the carry chain: this is one of its h one-step launches, each writing its state out
        rq = {rq.m, rq.n, 1, false, true, true, true, false};
    }
    // Micro tiles are for plans only (no per-row states, no state written out: those launches are one step long or chunk
    // continuations and keep the 16-candidate kernel - same bits).
    const bool plan_only = !rq.per_row && !rq.state_out && rq.results;
    if (md.generic) {
        if (pol.kernel_kind != L2A_KERNEL_VALU && md.gmicro_ok && pol.micro_policy != 0) {
            // Micro tiles (l2a_rnn_micro.h; geometry: the tuned LSTM kernel's).  These models have no unit-tile split, so every
            // plan that leaves CUs idle under 16-candidate tiles - and every plan of at most three micro tiles per CU - takes
            // them (policy 1); policy 0 keeps the 16-candidate kernel, 2 forces micro tiles where eligible.
            g = l2a_deal_micro(cus, rq.m, rq.n, 3);
            // Larger plans: workgroups of FOUR micro tiles, ceil(quads / 4) per env, as many rounds as that takes (the instances
            // with LDS rows for sixteen candidates: 256-unit layers, where the stack still fits)
            int mtm = 3;
            if (g.hi > 3 && md.gmicro4_ok) { g = l2a_deal_micro(cus, rq.m, rq.n, 4, true); mtm = 4; }
            if (plan_only && g.hi <= mtm && g.W >= 1 && g.mc_r >= 1 && g.mc_r <= g.W)
                return micro_tiles(L2A_RNN_GENERIC_MICRO, mtm, g, l2a_rnn_micro_smem(md.cell_type, md.n_layers, md.lunits[0], md.KG0, mtm));
        }
        const long long smem_m = generic_mfma_smem(md), smem_v = valu_smem(md);
        if (!mfma && pol.kernel_kind == L2A_KERNEL_MFMA)
            return bad(L2A_EINVAL, "LDS budget exceeded by the matrix-core recurrent kernel (" + std::to_string(smem_m) + " B)");
        if (!mfma && smem_v > pol.lds_per_block)
            return bad(L2A_EINVAL, "LDS budget exceeded by the generic recurrent kernel (" + std::to_string(smem_v) +
                                   " B): the layers' units may sum to about 800 at most");
        d->family = mfma ? L2A_RNN_GENERIC_MFMA16 : L2A_RNN_GENERIC_VALU;
        d->smem = mfma ? smem_m : smem_v;
        d->grid = (unsigned)(rq.m * d->tiles_per_env);
        return L2A_OK;
    }
    if (mfma && !md.mfma_ok)
        return bad(L2A_EINVAL, "LSTM shape is not eligible for the MFMA kernel "
                               "(needs a single LSTM layer, units in {128, 256, 512}, obs_dim <= 64, act_dim <= 16)");
    if (!mfma) {
        d->family = L2A_RNN_LSTM_VALU;
        d->smem = valu_smem(md);
        if (d->smem > pol.lds_per_block)
            return bad(L2A_EINVAL, "LDS budget exceeded by the VALU LSTM kernel (" + std::to_string(d->smem) + " B)");
        d->grid = (unsigned)(rq.m * d->tiles_per_env);
        return L2A_OK;
    }
    if (lstm_micro && plan_only) return micro_tiles(L2A_RNN_LSTM_MICRO, 3, g, l2a_lstm_micro_smem(md.units, md.KG0));
    d->family = L2A_RNN_LSTM_MFMA16;
    const int UT = L2A_NW * md.UTW, U = md.units;
    d->smem = 2 * UT * 64 * 16 + 2 * (L2A_NW * md.OT * 64) * 16 + (32 * md.KG0 + 48 * md.OT + 4 * U) * 4;
    if (d->smem > pol.lds_per_block) return bad(L2A_EINVAL, "LDS budget exceeded (" + std::to_string(d->smem) + " B)");
    const long long tiles = (long long)rq.m * d->tiles_per_env;
    // Unit-tile split: two workgroups per candidate tile when that still fits one workgroup per CU (both must
    // be resident: they swap their halves of h once per step).  Same bits as the unsplit launch.
    d->split = (rq.allow_split && pol.split_policy != 0 && 2 * tiles <= cus && rq.h < 4096) ? 1 : 0;
    if (d->split) d->xbuf_bytes = tiles * 4 * (long long)(UT / 2 + md.OT) * 2048;
    d->grid = (unsigned)(tiles * (d->split ? 2 : 1));
    return L2A_OK;
}

// Launches `d` for the request in `p`: copies the geometry fields and dispatches on the family.
int execute_rnn_launch(l2a_lstm* md, L2ALstmParams& p, const l2a_rnn_launch& d, hipStream_t stream) {
    l2a_ctx* ctx = md->ctx;
    if (d.xbuf_bytes) {
        const int xrc = l2a_xbuf_reserve(ctx, &md->xb, d.xbuf_bytes, stream, &p.xtag);
        if (xrc != L2A_OK) return xrc;
        p.xbuf = md->xb.buf;
        p.status = ctx->status_dev;
        p.spin_limit = ctx->spin_limit;
    }
    p.dbg = ctx->dbg;
    p.tiles_per_env = d.tiles_per_env; p.split = d.split;
    p.mc_w = d.mc_w; p.mc_hi = d.mc_hi; p.mc_r = d.mc_r;
    const int smem = (int)d.smem;
    auto micro_rc = [ctx](int rc, const char* what) {
        return l2a_fail(ctx, L2A_EHIP, std::string(what) + (rc > 0 ? hipGetErrorString((hipError_t)rc) : "no instance"));
    };
    switch (d.family) {
    case L2A_RNN_GENERIC_MICRO: {
        const int rc = l2a_launch_rnn_micro(md->lunits[0], md->cell_type, d.mtm, &p, d.grid, smem, stream);
        if (rc != 0) return micro_rc(rc, "micro-tile recurrent kernel launch: ");
        break;
    }
    case L2A_RNN_LSTM_MICRO: {
        const int rc = l2a_launch_lstm_micro(md->units, &p, d.grid, smem, stream);
        if (rc != 0) return micro_rc(rc, "micro-tile LSTM kernel launch: ");
        break;
    }
    case L2A_RNN_LSTM_MICRO_TRAJ: {
        const int rc = l2a_launch_lstm_micro_traj(md->units, &p, d.grid, smem, stream);
        if (rc != 0) return micro_rc(rc, "trajectory micro-tile LSTM kernel launch: ");
        break;
    }
    case L2A_RNN_LSTM_MFMA16: {
        const int rc = l2a_launch_lstm(md->UTW, 1, md->OT, md->KG0, &p, d.grid, smem, stream);
        if (rc == -100) return l2a_fail(ctx, L2A_EINVAL, "no MFMA LSTM kernel instance for this (obs_dim, act_dim, units)");
        if (rc != 0) return l2a_fail(ctx, L2A_EHIP, std::string("MFMA LSTM kernel launch: ") + hipGetErrorString((hipError_t)rc));
        break;
    }
    case L2A_RNN_GENERIC_MFMA16:
        L2A_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_rnn_mfma_k), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        hipLaunchKernelGGL(l2a_rnn_mfma_k, dim3(d.grid), dim3(256), (size_t)smem, stream, p);
        break;
    case L2A_RNN_GENERIC_VALU:
        L2A_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_rnn_valu_k), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        hipLaunchKernelGGL(l2a_rnn_valu_k, dim3(d.grid), dim3(256), smem, stream, p);
        break;
    default:
        L2A_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(l2a_lstm_valu_k), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        hipLaunchKernelGGL(l2a_lstm_valu_k, dim3(d.grid), dim3(256), smem, stream, p);
    }
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

// The plan of a request on a model that is ready to launch.
int plan_launch(const l2a_lstm* md, const l2a_rnn_request& rq, l2a_rnn_launch* d) {
    const l2a_ctx* ctx = md->ctx;
    if (!md->weights_set) return l2a_fail(ctx, L2A_ESTATE, "LSTM weights were never set");
    if (!md->norm_set) return l2a_fail(ctx, L2A_ESTATE, "LSTM normalisation was never set");
    std::string err;
    const int prc = plan_rnn_launch(*md, rnn_policy(ctx), rq, d, &err);
    return prc == L2A_OK ? L2A_OK : l2a_fail(ctx, prc, err);
}

// Plans the request in `p` and launches it on `stream_v`.
int launch(l2a_lstm* md, L2ALstmParams& p, void* stream_v, bool allow_split = true) {
    l2a_device_guard guard(md->ctx->device);
    l2a_rnn_launch d;
    const int prc = plan_launch(md, {p.m, p.n, p.h, p.obs_per_row != 0, p.state_out || p.c_out || p.h_out,
                                     p.returns_out || p.best_key, allow_split, false}, &d);
    if (prc != L2A_OK) return prc;
    return execute_rnn_launch(md, p, d, reinterpret_cast<hipStream_t>(stream_v));
}

// The controller's own state step on the small-rows kernel (single LSTM layer, units a multiple of 16): see l2a_lstm_advance_k.
bool advance_kernel_ok(const l2a_lstm* md) {
    return !md->generic && (md->units % 16) == 0 && md->units >= 16 && md->ctx->kernel_kind != L2A_KERNEL_VALU &&
           (md->in_dim + md->units) * L2A_ADV_ROWS * 4 + 4 * 64 * L2A_ADV_ROWS * 4 <= 64 * 1024;
}

int launch_advance(l2a_lstm* md, const float* obs, const float* act, const unsigned long long* best_key, const float* actions, int n,
                   int cand_offset, const float* c0, const float* h0, float* c1, float* h1, int m, hipStream_t stream) {
    l2a_ctx* ctx = md->ctx;
    if (!md->weights_set) return l2a_fail(ctx, L2A_ESTATE, "LSTM weights were never set");
    if (!md->norm_set) return l2a_fail(ctx, L2A_ESTATE, "LSTM normalisation was never set");
    L2ALstmAdvParams a;
    std::memset(&a, 0, sizeof(a));
    a.wblk = md->wblk; a.raw_wk = md->raw_wk; a.raw_bk = md->raw_bk; a.nm_off = md->nm_off;
    a.obs_dim = md->obs_dim; a.act_dim = md->act_dim; a.in_dim = md->in_dim; a.units = md->units; a.KG0 = md->KG0;
    a.cell_act = md->cell_act;
    a.obs = obs; a.act = act; a.best_key = best_key; a.actions = actions; a.n = n; a.cand_offset = cand_offset;
    a.c0 = c0; a.h0 = h0; a.c1 = c1; a.h1 = h1; a.m = m;
    const int smem = (md->in_dim + md->units) * L2A_ADV_ROWS * 4 + 4 * 64 * L2A_ADV_ROWS * 4;
    hipLaunchKernelGGL(l2a_lstm_advance_k, dim3((unsigned)(md->units / 16)), dim3(256), smem, stream, a);
    L2A_HIP(ctx, hipGetLastError());
    return L2A_OK;
}

// One of the model's own buffers, at least `need` floats (growing synchronises the stream: the old one may be in use).
int grow(l2a_ctx* ctx, float** buf, long long* have, long long need, hipStream_t stream) {
    if (need <= *have) return L2A_OK;
    l2a_device_guard guard(ctx->device);
    if (*buf) { L2A_HIP(ctx, hipStreamSynchronize(stream)); L2A_HIP(ctx, hipFree(*buf)); *buf = nullptr; *have = 0; }
    L2A_HIP(ctx, hipMalloc(reinterpret_cast<void**>(buf), (size_t)need * sizeof(float)));
    *have = need;
    return L2A_OK;
}

// The predicted trajectory [h, m n, obs_dim] of a plan -> traj (arguments validated by the callers).  Single launch of the
// trajectory-writing micro-tile instance where plan_rnn_launch says so, else the carry chain: h one-step launches of the
// rollout kernels - all-zero fused reward, state_out = traj[t], the trajectory slice itself being the state hand-off, c / h
// through the model's two buffer pairs in turn.  Stream-ordered; the same bits on both paths.
int rollout_traj(l2a_lstm* md, const float* obs0, const float* c0, const float* h0, const float* actions, int m, int n, int h,
                 int cand_offset, float* traj, void* stream_v) {
    l2a_ctx* ctx = md->ctx;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_rnn_launch d;
    int rc = plan_launch(md, {m, n, h, false, true, true, true, true}, &d);
    if (rc != L2A_OK) return rc;
    if (d.family == L2A_RNN_LSTM_MICRO_TRAJ) {
        l2a_device_guard guard(ctx->device);
        L2ALstmParams p;
        fill(md, p);
        p.obs0 = obs0; p.c0 = c0; p.h0 = h0; p.actions = actions;
        p.state_out = traj;                             // (this instance: the whole trajectory)
        p.m = m; p.n = n; p.h = h; p.cand_offset = cand_offset; p.discount = 1.0;
        return execute_rnn_launch(md, p, d, stream);
    }
    const long long rows = (long long)m * n;
    const long long hid = rows * md->units;             // (stacks: units = sum of the layers')
    rc = grow(ctx, &md->hid_buf, &md->hid_buf_floats, 4 * hid, stream);
    if (rc == L2A_OK) rc = grow(ctx, &md->traj_buf, &md->traj_buf_floats, rows, stream);   // (the plan entries ask for more first)
    if (rc != L2A_OK) return rc;
    float* carry_returns = md->traj_buf;                // the chunk launches' required returns_out: all zero rewards, never read
    l2a_reward zero;
    std::memset(&zero, 0, sizeof(zero));
    const long long step_state = rows * md->obs_dim, step_act = rows * md->act_dim;
    for (int t = 0; t < h; ++t) {
        const float* c_in = t == 0 ? c0 : md->hid_buf + ((t - 1) & 1) * 2 * hid;
        const float* h_in = t == 0 ? h0 : md->hid_buf + ((t - 1) & 1) * 2 * hid + hid;
        float* c_nx = md->hid_buf + (t & 1) * 2 * hid;
        rc = l2a_lstm_plan_rs_chunk(md, t == 0 ? obs0 : traj + (t - 1) * step_state, c_in, h_in, t > 0, actions + t * step_act, m, n, 1,
                                    0, 1.0, &zero, cand_offset, nullptr, carry_returns, traj + t * step_state, c_nx, c_nx + hid,
                                    nullptr, stream_v);
        if (rc != L2A_OK) return rc;
    }
    return L2A_OK;
}

// The candidate-count and reward-index checks of the plan entry points (`reward` null: a plan without a fused reward).
int check_candidates_and_reward(const l2a_lstm* md, const std::string& who, int m, int n, int cand_offset, const l2a_reward* reward) {
    const l2a_ctx* ctx = md->ctx;
    if ((long long)m * n > 0x3fffffffLL || cand_offset < 0 || (long long)cand_offset + n > 0x7fffffffLL)
        return l2a_fail(ctx, L2A_EINVAL, who + ": too many candidates");
    if (reward && reward->w_vel != 0.0f && (reward->vel_index < 0 || reward->vel_index >= md->obs_dim))
        return l2a_fail(ctx, L2A_EINVAL, "reward.vel_index out of range");
    if (reward && reward->dist_coef != 0.0f && (reward->dist_index < 0 || reward->dist_index >= md->obs_dim))
        return l2a_fail(ctx, L2A_EINVAL, "reward.dist_index out of range");
    return L2A_OK;
}

// The model's buffer of a state advance on the rollout kernels: [64, act_dim] chosen actions + [64, obs_dim] next obs.
int ensure_adv_buf(l2a_lstm* md) {
    if (!md->adv_buf)
        L2A_HIP(md->ctx, hipMalloc(reinterpret_cast<void**>(&md->adv_buf), sizeof(float) * L2A_MAIL_KEYS * (md->act_dim + md->obs_dim)));
    return L2A_OK;
}

// One step of the rollout kernel for `rows` independent rows, each with its own state (the launch of l2a_lstm_predict, and of
// the state advance of generic cells / stacks: the predicted observation then goes to the back of adv_buf and is dropped).
void one_step(const l2a_lstm* md, L2ALstmParams& q, const float* obs, const float* act, const float* c, const float* h, int rows,
              float* next_obs, float* c_out, float* h_out) {
    fill(md, q);
    q.obs0 = obs; q.c0 = c; q.h0 = h; q.actions = act;
    q.state_out = next_obs ? next_obs : md->adv_buf + (size_t)L2A_MAIL_KEYS * md->act_dim;
    q.c_out = c_out; q.h_out = h_out;
    q.obs_per_row = 1; q.hid_per_row = 1;
    q.m = 1; q.n = rows; q.h = 1; q.discount = 1.0;
}

// argument checks shared by the three entries; *traj: traj_out, or the model's own buffer behind the carry returns
int traj_args(l2a_lstm* md, const char* who, const float* obs0, const float* c0, const float* h0, const float* actions, int m, int n,
              int h, int cand_offset, bool need_out, bool have_out) {
    l2a_ctx* ctx = md->ctx;
    const std::string w(who);
    if (!obs0 || !c0 || !h0 || !actions) return l2a_fail(ctx, L2A_EINVAL, w + ": null obs0/c0/h0/actions");
    if (need_out && !have_out) return l2a_fail(ctx, L2A_EINVAL, w + ": nothing to write");
    if (m < 1 || n < 1 || h < 1) return l2a_fail(ctx, L2A_EINVAL, w + ": m, n and h must be >= 1");
    return check_candidates_and_reward(md, w, m, n, cand_offset, nullptr);
}

// the rollout of a plan entry -> *traj (traj_out, or the model's own buffer)
int plan_traj(l2a_lstm* md, const float* obs0, const float* c0, const float* h0, const float* actions, int m, int n, int h,
              int cand_offset, float* traj_out, void* stream_v, float** traj) {
    const long long rows = (long long)m * n;
    if (!traj_out) {
        const int rc = grow(md->ctx, &md->traj_buf, &md->traj_buf_floats, rows + (long long)h * rows * md->obs_dim,
                            reinterpret_cast<hipStream_t>(stream_v));
        if (rc != L2A_OK) return rc;
    }
    *traj = traj_out ? traj_out : md->traj_buf + rows;
    return rollout_traj(md, obs0, c0, h0, actions, m, n, h, cand_offset, *traj, stream_v);
}

}  // namespace

extern "C" {

int l2a_lstm_traj_geometry(int obs_dim, int act_dim, int units, int m, int n, int h, int micro_policy, int num_cu, int* out) {
    if (!out || obs_dim < 1 || act_dim < 1 || units < 1 || units > 1024 || m < 1 || n < 1 || h < 1 || micro_policy < 0 || micro_policy > 2)
        return L2A_EINVAL;
    if ((long long)m * n > 0x3fffffffLL) return L2A_EINVAL;
    const int cus = num_cu > 0 ? num_cu : 256, lds = 160 * 1024;
    l2a_rnn_launch d;
    std::string err;
    const int rc = plan_rnn_launch(rnn_shape(obs_dim, act_dim, 0, &units, L2A_CELL_LSTM, lds, false),
                                   {L2A_KERNEL_AUTO, 1, micro_policy, cus, lds}, {m, n, h, false, true, true, true, true}, &d, &err);
    const bool single = rc == L2A_OK && d.family == L2A_RNN_LSTM_MICRO_TRAJ;    // (a chain whose launches would fail is a chain here)
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = single ? 1 : 0;
    out[1] = single ? 1 : h;
    out[2] = single ? (int)d.grid : m * l2a_ceil_div(n, 16);    // (chain: before any unit-tile split of the one-step launches)
    out[3] = single ? d.mc_w : 0;
    out[4] = single ? d.mc_hi : l2a_deal_micro(cus, m, n, 3).hi;
    out[5] = single ? d.mc_r : 0;
    return L2A_OK;
}

int l2a_lstm_plan_geometry(int obs_dim, int act_dim, int n_layers, const int* units, int cell_type, int m, int n, int h, int request,
                           const int* policy, int* out) {
    if (!units || !out || obs_dim < 1 || act_dim < 1 || n_layers < 0 || n_layers > L2A_RNN_MAX_LAYERS || m < 1 || n < 1 || h < 1 ||
        request < 0 || request > 31 || (long long)m * n > 0x3fffffffLL)
        return L2A_EINVAL;
    if (cell_type != L2A_CELL_LSTM && cell_type != L2A_CELL_GRU && cell_type != L2A_CELL_RNN) return L2A_EINVAL;
    for (int l = 0; l < (n_layers ? n_layers : 1); ++l)
        if (units[l] < 1 || units[l] > 1024) return L2A_EINVAL;
    if (policy && policy[0] > L2A_KERNEL_VALU) return L2A_EINVAL;
    l2a_rnn_policy pol = {L2A_KERNEL_AUTO, 1, 1, 256, 160 * 1024};
    if (policy) {
        if (policy[0] > 0) pol.kernel_kind = policy[0];
        if (policy[1] >= 0) pol.split_policy = policy[1];
        if (policy[2] >= 0) pol.micro_policy = policy[2];
        if (policy[3] > 0) pol.num_cu = policy[3];
        if (policy[4] > 0) pol.lds_per_block = policy[4];
    }
    const l2a_rnn_shape md = rnn_shape(obs_dim, act_dim, n_layers, units, cell_type, pol.lds_per_block, force_generic());
    l2a_rnn_launch d;
    std::string err;
    const int rc = plan_rnn_launch(md, pol, {m, n, h, (request & 1) != 0, (request & 2) != 0, (request & 4) == 0, (request & 8) == 0,
                                             (request & 16) != 0}, &d, &err);
    if (rc != L2A_OK) return rc;
    const int g[12] = {d.family, d.mtm, d.split, (int)d.grid, (int)d.smem, d.tiles_per_env, d.mc_w, d.mc_hi, d.mc_r, (int)d.xbuf_bytes,
                       rnn_uses_mfma(md, pol) ? 1 : 0, 0};
    std::memcpy(out, g, sizeof(g));
    return L2A_OK;
}

int l2a_lstm_rollout_traj(l2a_lstm* md, const float* obs0, const float* c0, const float* h0, const float* actions, int m, int n,
                          int h, int cand_offset, float* traj_out, void* stream_v) {
    if (!md) return L2A_EINVAL;
    const int rc = traj_args(md, "l2a_lstm_rollout_traj", obs0, c0, h0, actions, m, n, h, cand_offset, true, traj_out != nullptr);
    if (rc != L2A_OK) return rc;
    return rollout_traj(md, obs0, c0, h0, actions, m, n, h, cand_offset, traj_out, stream_v);
}

// The recurrent plan step of an env with a reward program: the rollout and one scoring launch (l2a_score.hip).
int l2a_lstm_plan_rs_program(l2a_lstm* md, const float* obs0, const float* c0, const float* h0, const float* actions, int m, int n,
                             int h, double discount, const l2a_reward_program* program, int cand_offset, float* returns_out,
                             unsigned long long* best_key, float* traj_out, void* stream_v) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    int rc = l2a_reward_program_check(program, md->obs_dim, md->act_dim);
    if (rc != L2A_OK) return l2a_fail(ctx, rc, l2a_last_error(nullptr));
    rc = traj_args(md, "l2a_lstm_plan_rs_program", obs0, c0, h0, actions, m, n, h, cand_offset, true, best_key || returns_out);
    if (rc != L2A_OK) return rc;
    float* traj = nullptr;
    rc = plan_traj(md, obs0, c0, h0, actions, m, n, h, cand_offset, traj_out, stream_v, &traj);
    if (rc != L2A_OK) return rc;
    return l2a_score_trajectory(ctx, obs0, traj, actions, m, n, h, md->obs_dim, md->act_dim, discount, program, cand_offset,
                                returns_out, best_key, stream_v);
}

// ... with a learned reward model: the rollout and the matrix-core scoring launch (l2a_score_mlp.hip).
int l2a_lstm_plan_rs_reward_model(l2a_lstm* md, l2a_reward_model* rm, const float* obs0, const float* c0, const float* h0,
                                  const float* actions, int m, int n, int h, double discount, int cand_offset, float* returns_out,
                                  unsigned long long* best_key, float* traj_out, void* stream_v) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    if (!rm) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_reward_model: null reward model");
    l2a_ctx* rm_ctx = nullptr;
    int rm_obs = 0, rm_act = 0;
    l2a_reward_model_facts(rm, &rm_ctx, &rm_obs, &rm_act);
    if (rm_ctx != ctx) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_reward_model: the reward model lives on another context");
    if (rm_obs != md->obs_dim || rm_act != md->act_dim)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_reward_model: the reward model is for obs_dim " + std::to_string(rm_obs) +
                                         " / act_dim " + std::to_string(rm_act) + ", the dynamics model for " +
                                         std::to_string(md->obs_dim) + " / " + std::to_string(md->act_dim));
    int rc = traj_args(md, "l2a_lstm_plan_rs_reward_model", obs0, c0, h0, actions, m, n, h, cand_offset, true, best_key || returns_out);
    if (rc != L2A_OK) return rc;
    float* traj = nullptr;
    rc = plan_traj(md, obs0, c0, h0, actions, m, n, h, cand_offset, traj_out, stream_v, &traj);
    if (rc != L2A_OK) return rc;
    return l2a_score_trajectory_model(rm, obs0, traj, actions, m, n, h, discount, cand_offset, returns_out, best_key, stream_v);
}

int l2a_lstm_mfma_eligible(int obs_dim, int act_dim, int units) {
    return lstm_mfma_eligible(obs_dim, act_dim, units) ? 1 : 0;
}

// A new model of `shape`, and the tail of both create functions: the weight block of md->total floats, zeroed.
static l2a_lstm* new_model(l2a_ctx* ctx, const l2a_rnn_shape& shape, int cell_act, int output_act) {
    l2a_lstm* md = new l2a_lstm();
    static_cast<l2a_rnn_shape&>(*md) = shape;
    md->ctx = ctx;
    md->cell_act = cell_act; md->output_act = output_act;
    return md;
}
static int alloc_model(l2a_ctx* ctx, l2a_lstm* md, const char* what, l2a_lstm** out) {
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&md->wblk), (size_t)md->total * sizeof(float));
    if (e == hipSuccess) e = hipMemset(md->wblk, 0, (size_t)md->total * sizeof(float));
    if (e != hipSuccess) {
        std::string msg = std::string("allocating ") + what + " model storage: " + hipGetErrorString(e);
        delete md;
        return l2a_fail(ctx, L2A_EHIP, msg);
    }
    *out = md;
    return L2A_OK;
}

int l2a_lstm_create(l2a_ctx* ctx, int obs_dim, int act_dim, int units, int cell_act, int output_act,
                    l2a_lstm** out) {
    if (!ctx) return L2A_EINVAL;
    if (!out) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_create: out is null");
    *out = nullptr;
    if (obs_dim < 1 || act_dim < 1) return l2a_fail(ctx, L2A_EINVAL, "obs_dim and act_dim must be >= 1");
    if (units < 1 || units > 1024) return l2a_fail(ctx, L2A_EINVAL, "units must be in [1, 1024]");
    if (cell_act < 0 || cell_act > L2A_ACT_SWISH || output_act < 0 || output_act > L2A_ACT_SWISH)
        return l2a_fail(ctx, L2A_EINVAL, "unsupported nonlinearity");
    l2a_lstm* md = new_model(ctx, rnn_shape(obs_dim, act_dim, 0, &units, L2A_CELL_LSTM, ctx->lds_per_block, false), cell_act, output_act);
    long long off = 0;
    auto take = [&off](long long n) { long long o = off; off += (n + 15) / 16 * 16; return o; };
    md->raw_wk = take((long long)(md->in_dim + units) * 4 * units);
    md->raw_bk = take(4LL * units);
    md->raw_wo = take((long long)units * obs_dim);
    md->raw_bo = take(obs_dim);
    if (md->mfma_ok) {
        const int UT = units / 16;
        md->pk_wg = take(4LL * UT * (md->KG0 + UT) * 256);
        md->pk_wout = take((long long)md->OT * UT * 256);
        if (md->micro_ok) {
            md->pk_mg = take(l2a_lstm_micro_gate_floats(units, md->KG0));
            md->pk_mo = take((long long)(units / 4) * 256);
        }
    }
    md->pk_bout = take(16 * md->OT);
    md->nm_off = take(32 * md->KG0 + 32 * md->OT);
    md->total = off;
    return alloc_model(ctx, md, "LSTM", out);
}

int l2a_rnn_create(l2a_ctx* ctx, int obs_dim, int act_dim, int n_layers, const int* units, int cell_type,
                   int cell_act, int output_act, l2a_lstm** out) {
    if (!ctx) return L2A_EINVAL;
    if (!out || !units) return l2a_fail(ctx, L2A_EINVAL, "l2a_rnn_create: null argument");
    *out = nullptr;
    if (n_layers < 1 || n_layers > L2A_RNN_MAX_LAYERS)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_rnn_create: 1 to " + std::to_string(L2A_RNN_MAX_LAYERS) + " layers");
    if (cell_type != L2A_CELL_LSTM && cell_type != L2A_CELL_GRU && cell_type != L2A_CELL_RNN)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_rnn_create: unknown cell type");
    if (obs_dim < 1 || act_dim < 1) return l2a_fail(ctx, L2A_EINVAL, "obs_dim and act_dim must be >= 1");
    if (cell_act < 0 || cell_act > L2A_ACT_SWISH || output_act < 0 || output_act > L2A_ACT_SWISH)
        return l2a_fail(ctx, L2A_EINVAL, "unsupported nonlinearity");
    for (int l = 0; l < n_layers; ++l)
        if (units[l] < 1 || units[l] > 1024) return l2a_fail(ctx, L2A_EINVAL, "units must be in [1, 1024]");
    const l2a_rnn_shape shape = rnn_shape(obs_dim, act_dim, n_layers, units, cell_type, ctx->lds_per_block, force_generic());
    if (!shape.generic) return l2a_lstm_create(ctx, obs_dim, act_dim, units[0], cell_act, output_act, out);
    l2a_lstm* md = new_model(ctx, shape, cell_act, output_act);
    long long off = 0;
    auto take = [&off](long long n) { long long o = off; off += (n + 15) / 16 * 16; return o; };
    int kin = md->in_dim;
    for (int l = 0; l < n_layers; ++l) {
        const int U = units[l];
        const int cols0 = (cell_type == L2A_CELL_LSTM) ? 4 * U : (cell_type == L2A_CELL_GRU ? 2 * U : U);
        md->lw[l][0] = take((long long)(kin + U) * cols0);
        md->lb[l][0] = take(cols0);
        md->lpk[l][0] = take(l2a_rnn_pack_floats(kin, U, cols0 / U, true));
        if (cell_type == L2A_CELL_GRU) {
            md->lw[l][1] = take((long long)(kin + U) * U);
            md->lb[l][1] = take(U);
            md->lpk[l][1] = take(l2a_rnn_pack_floats(kin, U, 1, true));
        }
        if (md->gmicro_ok) {
            md->lmk[l][0] = take(l2a_rnn_micro_floats(kin, U, cols0 / U));
            if (cell_type == L2A_CELL_GRU) md->lmk[l][1] = take(l2a_rnn_micro_floats(kin, U, 1));
        }
        kin = U;
    }
    md->raw_wo = take((long long)kin * obs_dim);
    md->raw_bo = take(obs_dim);
    md->pk_wout = take(l2a_rnn_pack_floats(kin, obs_dim, 1, false));
    if (md->gmicro_ok) md->pk_mo = take((long long)(kin / 4) * 256);
    md->pk_bout = take(16 * md->OT);
    md->nm_off = take(32 * md->KG0 + 32 * md->OT);
    md->total = off;
    return alloc_model(ctx, md, "recurrent", out);
}

void l2a_lstm_destroy(l2a_lstm* md) {
    if (!md) return;
    if (md->wblk) {
        (void)hipDeviceSynchronize();
        (void)hipFree(md->wblk);
    }
    if (md->xb.buf) (void)hipFree(md->xb.buf);
    if (md->adv_buf) (void)hipFree(md->adv_buf);
    if (md->traj_buf) (void)hipFree(md->traj_buf);
    if (md->hid_buf) (void)hipFree(md->hid_buf);
    delete md;
}

int l2a_lstm_set_weights(l2a_lstm* md, const void* const* device_ptrs, void* stream_v) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    if (!device_ptrs) return l2a_fail(ctx, L2A_EINVAL, "device_ptrs is null");
    for (int i = 0; i < 4 && !md->generic; ++i)
        if (!device_ptrs[i]) return l2a_fail(ctx, L2A_EINVAL, "null LSTM parameter pointer " + std::to_string(i));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    if (md->generic) {
        // per layer: lstm (kernel, bias) | gru (gates/kernel, gates/bias, candidate/kernel, candidate/bias) |
        // rnn (kernel, bias); then output/kernel, output/bias
        int pi = 0, kin = md->in_dim;
        auto copy = [&](long long off, size_t count) -> int {
            const void* src = device_ptrs[pi++];
            if (!src) return l2a_fail(ctx, L2A_EINVAL, "null recurrent parameter pointer " + std::to_string(pi - 1));
            L2A_HIP(ctx, hipMemcpyAsync(md->wblk + off, src, sizeof(float) * count, hipMemcpyDeviceToDevice, stream));
            return L2A_OK;
        };
        for (int l = 0; l < md->n_layers; ++l) {
            const int Ul = md->lunits[l];
            const int cols0 = (md->cell_type == L2A_CELL_LSTM) ? 4 * Ul : (md->cell_type == L2A_CELL_GRU ? 2 * Ul : Ul);
            // (the fragment-order copies are made from the block's own raw copies, in stream order behind them)
            auto pack = [&](long long raw, long long dst, int rows_in, int Uc, int G, int recurrent) {
                const long long total = l2a_rnn_pack_floats(rows_in, Uc, G, recurrent != 0);
                hipLaunchKernelGGL(l2a_rnn_pack_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                                   md->wblk + raw, rows_in, Uc, G, recurrent, total, md->wblk + dst);
            };
            auto pack_micro = [&](long long raw, long long dst, int rows_in, int Uc, int G) {
                if (!md->gmicro_ok) return;
                const long long total = l2a_rnn_micro_floats(rows_in, Uc, G);
                hipLaunchKernelGGL(l2a_rnn_micro_pack_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                                   md->wblk + raw, rows_in, Uc, G, total, md->wblk + dst);
            };
            int rc = copy(md->lw[l][0], (size_t)(kin + Ul) * cols0);
            if (rc == L2A_OK) { pack(md->lw[l][0], md->lpk[l][0], kin, Ul, cols0 / Ul, 1); pack_micro(md->lw[l][0], md->lmk[l][0], kin, Ul, cols0 / Ul); }
            if (rc == L2A_OK) rc = copy(md->lb[l][0], (size_t)cols0);
            if (rc == L2A_OK && md->cell_type == L2A_CELL_GRU) {
                rc = copy(md->lw[l][1], (size_t)(kin + Ul) * Ul);
                if (rc == L2A_OK) { pack(md->lw[l][1], md->lpk[l][1], kin, Ul, 1, 1); pack_micro(md->lw[l][1], md->lmk[l][1], kin, Ul, 1); }
                if (rc == L2A_OK) rc = copy(md->lb[l][1], (size_t)Ul);
            }
            if (rc != L2A_OK) return rc;
            kin = Ul;
        }
        int rc = copy(md->raw_wo, (size_t)kin * md->obs_dim);
        if (rc == L2A_OK) {
            const long long total = l2a_rnn_pack_floats(kin, md->obs_dim, 1, false);
            hipLaunchKernelGGL(l2a_rnn_pack_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                               md->wblk + md->raw_wo, kin, md->obs_dim, 1, 0, total, md->wblk + md->pk_wout);
            if (md->gmicro_ok) {
                const long long total_m = (long long)(kin / 4) * 256;
                hipLaunchKernelGGL(l2a_lstm_micro_pack_out_k, dim3((unsigned)((total_m + 255) / 256)), dim3(256), 0, stream,
                                   md->wblk + md->raw_wo, kin, md->obs_dim, total_m, md->wblk + md->pk_mo);
            }
        }
        if (rc == L2A_OK) rc = copy(md->raw_bo, (size_t)md->obs_dim);
        if (rc != L2A_OK) return rc;
        L2A_HIP(ctx, hipGetLastError());
        md->weights_set = true;
        return L2A_OK;
    }
    const int U = md->units;
    const float* wk = static_cast<const float*>(device_ptrs[0]);
    const float* wo = static_cast<const float*>(device_ptrs[2]);
    L2A_HIP(ctx, hipMemcpyAsync(md->wblk + md->raw_wk, wk, sizeof(float) * (size_t)(md->in_dim + U) * 4 * U,
                                hipMemcpyDeviceToDevice, stream));
    L2A_HIP(ctx, hipMemcpyAsync(md->wblk + md->raw_bk, device_ptrs[1], sizeof(float) * 4 * (size_t)U,
                                hipMemcpyDeviceToDevice, stream));
    L2A_HIP(ctx, hipMemcpyAsync(md->wblk + md->raw_wo, wo, sizeof(float) * (size_t)U * md->obs_dim,
                                hipMemcpyDeviceToDevice, stream));
    L2A_HIP(ctx, hipMemcpyAsync(md->wblk + md->raw_bo, device_ptrs[3], sizeof(float) * (size_t)md->obs_dim,
                                hipMemcpyDeviceToDevice, stream));
    L2A_HIP(ctx, hipMemcpyAsync(md->wblk + md->pk_bout, device_ptrs[3], sizeof(float) * (size_t)md->obs_dim,
                                hipMemcpyDeviceToDevice, stream));
    if (md->mfma_ok) {
        const int UT = U / 16;
        long long total = 4LL * UT * (md->KG0 + UT) * 256;
        hipLaunchKernelGGL(l2a_lstm_pack_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, wk,
                           md->KG0, UT, md->in_dim, total, md->wblk + md->pk_wg);
        L2A_HIP(ctx, hipGetLastError());
        total = (long long)md->OT * UT * 256;
        hipLaunchKernelGGL(l2a_lstm_pack_out_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, wo, U,
                           md->obs_dim, UT, total, md->wblk + md->pk_wout);
        L2A_HIP(ctx, hipGetLastError());
        if (md->micro_ok) {
            total = l2a_lstm_micro_gate_floats(U, md->KG0);
            hipLaunchKernelGGL(l2a_lstm_micro_pack_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, wk,
                               md->in_dim, U, md->KG0, total, md->wblk + md->pk_mg);
            total = (long long)(U / 4) * 256;
            hipLaunchKernelGGL(l2a_lstm_micro_pack_out_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, wo, U,
                               md->obs_dim, total, md->wblk + md->pk_mo);
            L2A_HIP(ctx, hipGetLastError());
        }
    }
    md->weights_set = true;
    return L2A_OK;
}

int l2a_lstm_set_norm(l2a_lstm* md, const double* mean_obs, const double* std_obs, const double* mean_act,
                      const double* std_act, const double* mean_delta, const double* std_delta, void* stream_v) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    const int n_null = !mean_obs + !std_obs + !mean_act + !std_act + !mean_delta + !std_delta;
    if (n_null != 0 && n_null != 6)
        return l2a_fail(ctx, L2A_EINVAL, "pass all six normalisation vectors, or none for identity");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    const int KG0 = md->KG0, OT = md->OT;
    std::vector<float>& st = md->norm_stage;
    if (!st.empty()) L2A_HIP(ctx, hipStreamSynchronize(stream));
    st.assign((size_t)(32 * KG0 + 32 * OT), 0.0f);
    float* in_mu = st.data();
    float* in_iv = in_mu + 16 * KG0;
    float* out_mu = in_iv + 16 * KG0;
    float* out_sd = out_mu + 16 * OT;
    const double eps = 1e-10;   // rnn_dynamics.py:329-334
    for (int k = 0; k < md->in_dim; ++k) {
        if (n_null) { in_mu[k] = 0.0f; in_iv[k] = 1.0f; continue; }
        const double mu = (k < md->obs_dim) ? mean_obs[k] : mean_act[k - md->obs_dim];
        const double sd = (k < md->obs_dim) ? std_obs[k] : std_act[k - md->obs_dim];
        in_mu[k] = (float)mu;
        in_iv[k] = (float)(1.0 / (sd + eps));
    }
    for (int d = 0; d < md->obs_dim; ++d) {
        out_mu[d] = n_null ? 0.0f : (float)mean_delta[d];
        out_sd[d] = n_null ? 1.0f : (float)(std_delta[d] + eps);
    }
    L2A_HIP(ctx, hipMemcpyAsync(md->wblk + md->nm_off, st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    md->norm_set = true;
    return L2A_OK;
}

int l2a_lstm_plan_rs(l2a_lstm* md, const float* obs0, const float* c0, const float* h0, const float* actions,
                     int m, int n, int h, double discount, const l2a_reward* reward, int cand_offset,
                     float* returns_out, unsigned long long* best_key, void* stream_v) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    if (!obs0 || !c0 || !h0 || !actions || !reward)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs: null obs0/c0/h0/actions/reward");
    if (!best_key && !returns_out) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs: nothing to write");
    if (m < 1 || n < 1 || h < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs: m, n and h must be >= 1");
    const int arc = check_candidates_and_reward(md, "l2a_lstm_plan_rs", m, n, cand_offset, reward);
    if (arc != L2A_OK) return arc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    if (best_key) L2A_HIP(ctx, hipMemsetAsync(best_key, 0, sizeof(unsigned long long) * (size_t)m, stream));
    L2ALstmParams p;
    fill(md, p);
    p.obs0 = obs0; p.c0 = c0; p.h0 = h0; p.actions = actions;
    p.returns_out = returns_out; p.best_key = best_key;
    p.m = m; p.n = n; p.h = h; p.cand_offset = cand_offset; p.discount = discount; p.rw = *reward;
    return launch(md, p, stream_v);
}

int l2a_lstm_plan_rs_sync(l2a_lstm* md, const float* obs_host, const float* c0, const float* h0, const float* actions,
                          int m, int n, int h, double discount, const l2a_reward* reward, int cand_offset,
                          unsigned long long* keys_host_out, float* c_next, float* h_next, void* stream_v) {
    return l2a_lstm_plan_rs_sync_hook(md, obs_host, c0, h0, actions, m, n, h, discount, reward, cand_offset, keys_host_out, c_next,
                                      h_next, stream_v, nullptr, nullptr);
}

void l2a_lstm_facts(const l2a_lstm* md, l2a_ctx** ctx, int* obs_dim, int* act_dim, int* units) {
    *ctx = md->ctx; *obs_dim = md->obs_dim; *act_dim = md->act_dim; *units = md->units;
}

int l2a_lstm_plan_rs_sync_hook(l2a_lstm* md, const float* obs_host, const float* c0, const float* h0, const float* actions,
                               int m, int n, int h, double discount, const l2a_reward* reward, int cand_offset,
                               unsigned long long* keys_host_out, float* c_next, float* h_next, void* stream_v,
                               l2a_after_launch_fn hook, void* hook_arg, l2a_mail_pending* pending) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    ctx->stamps_us[0] = l2a_now_us();
    if (!obs_host || !c0 || !h0 || !actions || !reward || (!keys_host_out && !pending))
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_sync: null obs / c0 / h0 / actions / reward / keys_host_out");
    if ((!c_next) != (!h_next)) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_sync: pass c_next and h_next together");
    if (c_next && (c_next == c0 || h_next == h0))
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_sync: the next state must not alias the current one");
    if (m < 1 || n < 1 || h < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_sync: m, n and h must be >= 1");
    int rc = check_candidates_and_reward(md, "l2a_lstm_plan_rs_sync", m, n, cand_offset, reward);
    if (rc != L2A_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    const bool publish = rnn_uses_mfma(*md, rnn_policy(ctx));       // only the matrix-core kernels have the mailbox epilogue
    if (c_next && (rc = ensure_adv_buf(md)) != L2A_OK) return rc;
    l2a_mail_ticket tk;
    rc = l2a_mail_begin(ctx, m, obs_host, (long long)m * md->obs_dim, stream, &tk);
    if (rc != L2A_OK) return rc;
    tk.shape = (unsigned long long)(size_t)md ^ ((unsigned long long)m << 48) ^ ((unsigned long long)n << 24) ^ (unsigned long long)h;
    L2ALstmParams p;
    fill(md, p);
    p.obs0 = tk.obs_dev; p.c0 = c0; p.h0 = h0; p.actions = actions;
    p.best_key = tk.keys_dev;
    p.m = m; p.n = n; p.h = h; p.cand_offset = cand_offset; p.discount = discount; p.rw = *reward;
    if (publish) {
        p.done_ctr = ctx->done_ctr;
        p.mail_keys = ctx->mail_dev->keys;
        p.mail_seq_ptr = &ctx->mail_dev->seq;
        p.mail_seq = tk.seq;
        p.next_keys = tk.next_keys;
    }
    ctx->stamps_us[1] = l2a_now_us();
    rc = launch(md, p, stream_v);
    if (rc == L2A_OK && c_next && advance_kernel_ok(md)) {
        // the controller's own state moves on with the chosen action (rnn_mpc_controller.py:63) - in stream order behind the
        // plan, without waiting for the host to learn the arg-max: ONE small launch that gathers the winners' first actions
        // through the keys and spreads the gate matrix over units / 16 workgroups (l2a_lstm_advance_k)
        rc = launch_advance(md, tk.obs_dev, nullptr, tk.keys_dev, actions, n, cand_offset, c0, h0, c_next, h_next, m, stream);
    } else if (rc == L2A_OK && c_next) {
        // generic cells / stacks: a gather launch and a one-step launch of the rollout kernel
        hipLaunchKernelGGL(l2a_gather_best_k, dim3((unsigned)m), dim3(64), 0, stream, tk.keys_dev, actions, m, n, cand_offset,
                           md->act_dim, md->adv_buf);
        L2ALstmParams q;
        one_step(md, q, tk.obs_dev, md->adv_buf, c0, h0, m, nullptr, c_next, h_next);
        // NEVER tile-split: l2a_mail_end reads the status word as soon as the PLAN has published, while this launch may
        // still run - an exchange timeout in it would be noticed one call late and the state it wrote adopted
        rc = launch(md, q, stream_v, false);
    }
    ctx->stamps_us[2] = l2a_now_us();
    if (rc == L2A_OK && hook) hook(hook_arg);
    ctx->stamps_us[3] = l2a_now_us();
    if (pending && rc == L2A_OK) {
        pending->tk = tk; pending->publish = publish; pending->m = m; pending->stream = stream;
        pending->who = "l2a_lstm_plan_rs_sync"; pending->live = true;
        return L2A_OK;
    }
    rc = l2a_mail_end(ctx, tk, m, publish, rc, stream, keys_host_out, "l2a_lstm_plan_rs_sync");
    ctx->stamps_us[4] = l2a_now_us();
    return rc;
}

int l2a_lstm_advance_keys(l2a_lstm* md, const float* obs, const unsigned long long* keys, const float* table, int n,
                          unsigned long long seed, unsigned long long offset, const float* lowr, const float* c0, const float* h0,
                          float* c_next, float* h_next, int m, void* stream_v) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    if (!obs || !keys || (!table && !lowr) || !c0 || !h0 || !c_next || !h_next)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_advance_keys: null pointer");
    if (m < 1 || m > L2A_MAIL_KEYS || n < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_advance_keys: needs 1 <= m <= 64, n >= 1");
    if (!table && md->act_dim > 16) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_advance_keys: the stream's bounds hold 16 action dimensions");
    if (c_next == c0 || h_next == h0) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_advance_keys: the next state must not alias the current one");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    // one LSTM layer, actions in a table: the advance kernel gathers through the keys itself (as behind the unsharded plan)
    if (table && advance_kernel_ok(md)) return launch_advance(md, obs, nullptr, keys, table, n, 0, c0, h0, c_next, h_next, m, stream);
    const int brc = ensure_adv_buf(md);
    if (brc != L2A_OK) return brc;
    float* act_sel = md->adv_buf;
    if (table)
        hipLaunchKernelGGL(l2a_gather_best_k, dim3((unsigned)m), dim3(64), 0, stream, keys, table, m, n, 0, md->act_dim, act_sel);
    else
        hipLaunchKernelGGL(l2a_gather_best_philox_k, dim3((unsigned)m), dim3(64), 0, stream, keys, m, n, md->act_dim, seed, offset, lowr,
                           act_sel);
    L2A_HIP(ctx, hipGetLastError());
    if (advance_kernel_ok(md)) return launch_advance(md, obs, act_sel, nullptr, nullptr, 0, 0, c0, h0, c_next, h_next, m, stream);
    // generic cells / stacks: one step of the rollout kernel on the gathered actions - never tile-split (see the comment in
    // l2a_lstm_plan_rs_sync_hook: a flag raised here would be noticed one step late)
    L2ALstmParams q;
    one_step(md, q, obs, act_sel, c0, h0, m, nullptr, c_next, h_next);
    return launch(md, q, stream_v, false);
}

int l2a_lstm_plan_rs_chunk(l2a_lstm* md, const float* state, const float* c, const float* h, int per_row,
                           const float* actions, int m, int n, int h_chunk, int t0, double discount,
                           const l2a_reward* reward, int cand_offset, const float* returns_in, float* returns_out,
                           float* state_out, float* c_out, float* h_out, unsigned long long* best_key, void* stream_v) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    if (!state || !c || !h || !actions || !reward)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_chunk: null state/c/h/actions/reward");
    if (!returns_out) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_chunk: returns_out is required");
    if (m < 1 || n < 1 || h_chunk < 1 || t0 < 0)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_chunk: bad m / n / h_chunk / t0");
    if (t0 > 0 && (!returns_in || !per_row))
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_chunk: a continuation needs returns_in and per-row states");
    if ((!state_out) != (!c_out) || (!state_out) != (!h_out))
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_plan_rs_chunk: pass state_out, c_out and h_out together");
    const int arc = check_candidates_and_reward(md, "l2a_lstm_plan_rs_chunk", m, n, cand_offset, reward);
    if (arc != L2A_OK) return arc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    if (best_key) L2A_HIP(ctx, hipMemsetAsync(best_key, 0, sizeof(unsigned long long) * (size_t)m, stream));
    L2ALstmParams p;
    fill(md, p);
    p.obs0 = state; p.c0 = c; p.h0 = h; p.actions = actions;
    p.obs_per_row = per_row ? 1 : 0; p.hid_per_row = per_row ? 1 : 0;
    p.returns_out = returns_out; p.best_key = best_key;
    p.state_out = state_out; p.c_out = c_out; p.h_out = h_out;
    p.ret_in = (t0 > 0) ? returns_in : nullptr;
    double d0 = 1.0;
    for (int t = 0; t < t0; ++t) d0 *= discount;
    p.disc0 = d0;
    p.m = m; p.n = n; p.h = h_chunk; p.cand_offset = cand_offset; p.discount = discount; p.rw = *reward;
    return launch(md, p, stream_v);
}

int l2a_lstm_advance(l2a_lstm* md, const float* obs, const float* act, const float* c, const float* h, int rows,
                     float* c_out, float* h_out, void* stream_v) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    if (!obs || !act || !c || !h || !c_out || !h_out) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_advance: null pointer");
    if (rows < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_advance: rows must be >= 1");
    if (c_out == c || h_out == h) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_advance: the next state must not alias the current one");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    l2a_device_guard guard(ctx->device);
    if (advance_kernel_ok(md)) return launch_advance(md, obs, act, nullptr, nullptr, 0, 0, c, h, c_out, h_out, rows, stream);
    // generic cells / stacks (and the VALU kernel when asked for): one step of the rollout kernel, the predicted observation dropped
    if ((long long)rows > L2A_MAIL_KEYS) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_advance: at most 64 rows (use l2a_lstm_predict)");
    const int brc = ensure_adv_buf(md);
    if (brc != L2A_OK) return brc;
    L2ALstmParams p;
    one_step(md, p, obs, act, c, h, rows, nullptr, c_out, h_out);
    return launch(md, p, stream_v, false);
}

int l2a_lstm_predict(l2a_lstm* md, const float* obs, const float* act, const float* c, const float* h, int rows,
                     float* next_obs_out, float* c_out, float* h_out, void* stream_v) {
    if (!md) return L2A_EINVAL;
    l2a_ctx* ctx = md->ctx;
    if (!obs || !act || !c || !h || !next_obs_out || !c_out || !h_out)
        return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_predict: null pointer");
    if (rows < 1) return l2a_fail(ctx, L2A_EINVAL, "l2a_lstm_predict: rows must be >= 1");
    L2ALstmParams p;
    one_step(md, p, obs, act, c, h, rows, next_obs_out, c_out, h_out);
    return launch(md, p, stream_v);
}

}  // extern "C"
