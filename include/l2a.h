/*
 * l2a.h - C ABI of libl2a_hip.so: the MI355X (gfx950) MPC random-shooting rollout.
 *
 * The reference (iclavera/learning_to_adapt) has no FFI: its planner is Python that calls
 * `dynamics_model.predict` (-> TensorFlow `sess.run`) once per horizon step.  This header is
 * the boundary a maintainer would bind instead; every entry point names the reference code
 * it replaces.  All pointers marked "device" are HIP device pointers (in practice
 * `tensor.data_ptr()` of PyTorch-ROCm tensors - torch only stores the bytes); everything else
 * is host memory.  No torch types, no C++ types and no exceptions cross this boundary.
 *
 * Error model: functions return 0 on success and a negative L2A_E* code on failure;
 * `l2a_last_error` returns a human-readable message for the last failure on that context.
 * Threading: one context per (process, device); calls on one context are not re-entrant.
 * All device work is enqueued on the caller's stream; the library never synchronises except
 * inside l2a_init / l2a_model_create / l2a_model_destroy / l2a_destroy.
 */
#ifndef L2A_H_
#define L2A_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct l2a_ctx l2a_ctx;
typedef struct l2a_model l2a_model;
typedef struct l2a_lstm l2a_lstm;
typedef struct l2a_reward_model l2a_reward_model;
typedef struct l2a_value_model l2a_value_model;
typedef struct l2a_policy_model l2a_policy_model;
typedef struct l2a_controller l2a_controller;

/* ---- error codes --------------------------------------------------------------------- */
#define L2A_OK 0
#define L2A_EINVAL (-1)      /* bad argument / unsupported shape                           */
#define L2A_EHIP (-2)        /* a HIP runtime call failed (message has hipGetErrorString)  */
#define L2A_ENODEV (-3)      /* no usable gfx950 device                                    */
#define L2A_ESTATE (-4)      /* call order violated (e.g. plan before weights were set)    */
#define L2A_ESPLIT (-5)      /* l2a_plan_rs_sync only: a tile-split exchange timed out, the result is
                                invalid; call l2a_set_split(ctx, 0) and repeat the call              */

/* ---- enums ---------------------------------------------------------------------------- */
/* hidden / output nonlinearity: dynamics/mlp_dynamics.py:16-23 (`_activations`).           */
#define L2A_ACT_IDENTITY 0
#define L2A_ACT_RELU 1
#define L2A_ACT_TANH 2
#define L2A_ACT_SIGMOID 3
#define L2A_ACT_SWISH 4

/* how the E weight sets of a model are used                                                 */
#define L2A_MODE_SINGLE 0     /* E == 1: MLPDynamicsModel.predict (mlp_dynamics.py:204-222)   */
#define L2A_MODE_PER_BLOCK 1  /* row block i (env i) <-> set i: MetaMLPDynamicsModel._predict
                                 with adapted weights (meta_mlp_dynamics.py:296-306,143-163)  */
#define L2A_MODE_MEAN 2       /* delta = mean_e denorm_e(MLP_e(norm_e(.))) - build-defined
                                 ensemble of BASELINE.json (not in the reference)            */

/* which rollout kernel l2a_plan_rs / l2a_predict dispatch to                                */
#define L2A_KERNEL_AUTO 0     /* MFMA kernel when the shape allows it, else the VALU kernel  */
#define L2A_KERNEL_MFMA 1     /* fail with L2A_EINVAL when the shape is not MFMA-eligible    */
#define L2A_KERNEL_VALU 2     /* generic fp32 VALU kernel (any layer sizes)                  */

/*
 * Closed-form reward, evaluated in-kernel once per (candidate, horizon step).  Replaces the
 * host call `self.unwrapped_env.reward(observation, a[t], next_observation)`
 * (policies/mpc_controller.py:125) for the reference's env rewards:
 *   envs/half_cheetah_env.py:58-65, envs/ant_env.py:56-66, envs/arm_7dof_env.py:91-99.
 *
 *   r = w_vel * (next[vel_index] - obs[vel_index]) * inv_dt + alive
 *       - ctrl_coef * sum_k act[k]^2 - dist_coef * || next[dist_index .. dist_index+2] ||
 */
typedef struct l2a_reward {
    float w_vel;
    float inv_dt;
    float alive;
    float ctrl_coef;
    float dist_coef;
    int vel_index;
    int dist_index;
    int reserved;
} l2a_reward;

/*
 * Reward program: any closed-form env reward as a short list of terms, scored by a kernel of its own behind the
 * rollout (l2a_score_trajectory, l2a_plan_rs_program) - for envs whose `reward(obs, act, next_obs)` is not the
 * formula above.
 *
 *   r = bias + sum over terms, in program order, of  coef * v(term)
 *
 * A term reads the contiguous range [index, index + len) of one source vector x: the observation (OBS), the
 * action (ACT), the next observation (NEXT) or DELTA = next - obs.
 *   LINEAR  (len 1)  v = x[index]
 *   SQSUM            v = sum_k (x[index + k] - target_k)^2
 *   NORM             v = sqrt of the same sum
 *   INRANGE (len 1)  v = 1 when lo <= x[index] <= hi, else 0 (a NaN gives 0, as NumPy's comparison does)
 * `target` is an offset into `consts` (goal positions, set points: target_k = consts[target + k]) or -1 for zeros.
 *
 * Arithmetic (fixed, so that a host can restate it bit for bit - envs/reward_spec.py: RewardProgram.evaluate_f32):
 * fp32, round to nearest, nothing contracted.  d = x - t; s = s + d * d as a separate multiply and add, k ascending
 * from s = 0; r = r + coef * v as a separate multiply and add, starting from r = bias; the return R = R + disc_t * r
 * as a separate multiply and add from R = 0, disc_t = discount ** t carried in float64 by repeated multiplication
 * and rounded to fp32 once per step (as l2a_plan_rs does).
 *
 * Plain C, passed by value, no pointers inside: sizeof(l2a_reward_term) == 32, sizeof(l2a_reward_program) ==
 * 16 + 16 * 32 + 64 * 4 == 784.
 */
#define L2A_PROGRAM_MAX_TERMS 16
#define L2A_PROGRAM_MAX_CONSTS 64
#define L2A_SRC_OBS 0
#define L2A_SRC_ACT 1
#define L2A_SRC_NEXT 2
#define L2A_SRC_DELTA 3
#define L2A_TERM_LINEAR 0
#define L2A_TERM_SQSUM 1
#define L2A_TERM_NORM 2
#define L2A_TERM_INRANGE 3
typedef struct l2a_reward_term {
    int kind;
    int source;
    int index;
    int len;
    int target;
    float coef;
    float lo;
    float hi;
} l2a_reward_term;
typedef struct l2a_reward_program {
    int n_terms;
    int n_consts;
    float bias;
    int reserved;
    l2a_reward_term terms[L2A_PROGRAM_MAX_TERMS];
    float consts[L2A_PROGRAM_MAX_CONSTS];
} l2a_reward_program;

/* ---- context -------------------------------------------------------------------------- */
/* Create a context on HIP device `device`.  Lazy by design: the reference forks its env
 * workers (samplers/sampler.py:37) before it creates the TF session
 * (trainers/mb_trainer.py:46-48); callers must likewise call this after forking.            */
int l2a_init(int device, l2a_ctx** out);
void l2a_destroy(l2a_ctx* ctx);
/* Message of the last failed call on `ctx` (or of a failed l2a_init when ctx == NULL).      */
const char* l2a_last_error(const l2a_ctx* ctx);
/* Library / device facts: writes up to `cap` bytes of a JSON object (arch, CU count, ...).  */
int l2a_device_info(const l2a_ctx* ctx, char* buf, int cap);
/* Select the kernel (L2A_KERNEL_*) used by subsequent launches on this context.             */
int l2a_set_kernel(l2a_ctx* ctx, int kind);
/* Tile-split policy of the MFMA kernel.  When a plan has at most (CUs / 2) candidate tiles, two
 * workgroups can share each tile and exchange partial sums once per horizon step through global
 * memory: 0 = never; 2 = split the ensemble into two groups of whole sets (needs >= 2 sets);
 * 1 (default) = as 2, and additionally the middle set of an odd ensemble - or the only set of a
 * single / per-block model - is shared, each workgroup computing the last hidden layer and the
 * output layer for one half of the hidden units (needs >= 2 hidden layers).  Results are
 * bit-identical under all three policies: the summation order is fixed (sets: group A + group B;
 * output layer: eight chunks of hidden units in a balanced tree, ((c0+c1)+(c2+c3)) + ((c4+c5)+(c6+c7))).  */
int l2a_set_split(l2a_ctx* ctx, int policy);
/* Set batching of the MFMA kernel (models with two hidden layers).  A workgroup that runs several weight sets per
 * horizon step (an ensemble member group) can run layer 0 of `sets` sets back to back, then their hidden GEMMs and
 * output layers, then their reduces - two workgroup barriers per batch instead of two per set, the activations of a
 * batch held in LDS side by side.  0 (default) = as many as fit the CU's LDS (at most 4), 1 = one set at a time.
 * Arithmetic and summation order do not depend on it: results are bit-identical for every value.       */
int l2a_set_batch(l2a_ctx* ctx, int sets);
/* Placement of a uniformly split launch (two workgroups per candidate tile).  1 (default): the grid is padded to a
 * multiple of eight workgroups so that the workgroups of ensemble group A land on XCDs 0-3 and those of group B on XCDs
 * 4-7 exactly (hardware workgroup id % 8 = XCD); the up to six spare workgroups return at once.  Without it a tile count
 * that is not a multiple of four leaves one workgroup alone with its weight sets in a foreign L2, and its tile ends the
 * launch late (config 2, 125 tiles: 1.431 -> 1.417 ms).  0: the contiguous remap of 2 x tiles workgroups.  Placement
 * only: results are bit-identical.                                                                          */
int l2a_set_xcd_align(l2a_ctx* ctx, int on);
/* Member fan of the MFMA kernel (mean ensembles of 3 .. 8 sets).  A small plan - E x candidate tiles <= CUs, e.g. one
 * rank's 500-candidate shard of BASELINE config 5: 32 tiles - runs ONE workgroup per (candidate tile, ensemble member):
 * every workgroup streams one weight set, and once per horizon step the E workgroups of a tile swap their members' terms
 * (the tagged granules of the tile split, E - 1 partners instead of one) and add them in the unsplit launch's order.  The
 * tile split runs such a plan on 2 x tiles workgroups of 2.5 sets each; the fan on E x tiles of one set each.  1 (default)
 * = wherever it fits (and l2a_set_split is not 0: a flagged launch degrades to the unsplit geometry as before), 0 = never.
 * Geometry only: results are bit-identical.                                                                     */
int l2a_set_fan(l2a_ctx* ctx, int on);
/* Double rounds of the MFMA kernel (hidden width 512, up to 48 observation dims).  A plan of at least two rounds of
 * 16-candidate tiles (2 x CUs tiles: BASELINE config 3's 625, config 4 on one GPU, run_mb_mpc.py's default 1250) runs its
 * first 2 x CUs x D tiles as D rounds of DOUBLE tiles - two candidate tiles per workgroup on kernel instances that carry
 * neither exchange nor half-member code (and so keep their registers at this width): every weight fragment feeds both tiles
 * and a step's fixed costs are paid once for 32 candidates, ~0.945 of a single round's cost per tile.  The rest of every
 * env's candidates follows in a second launch on the same stream with the ordinary geometry (whole round, tail split); a rest
 * of more than a round and a half joins the double tiles.  The same instances also run WHOLE single tiles of plans with one
 * weight set per candidate (single model, per-block sets), 3 - 4 % faster per round than the general instances.
 * 1 (default) = wherever they apply, 0 = never (general instances only).  Geometry only: results are bit-identical.   */
int l2a_set_double_rounds(l2a_ctx* ctx, int on);
/* Static three-set step of the tile split (hidden width 512, two hidden layers, up to 32 inputs, relu / identity).  Under the
 * shared-set tile split a mean ensemble of FIVE sets gives every workgroup the same sequence per horizon step - two full
 * sets, then its half of the shared one, in one batch (BASELINE config 2).  Kernel instances that know this sequence at compile
 * time run the step as straight-line code; every other plan keeps the general instances.  1 (default) = wherever the plan is
 * exactly that sequence, 0 = never (environment default: L2A_SEQ3).  Schedule only: results are bit-identical.           */
int l2a_set_seq3(l2a_ctx* ctx, int on);
/* Micro tiles (csrc/l2a_micro.h).  A plan whose 16-candidate tiles would leave CUs idle - e.g. the reference's own default
 * plans, run_grbal.py:84-85 / run_rebal.py:77-78: 5 x 500 candidates = 160 tiles on 256 CUs - can run in candidate tiles of
 * FOUR on v_mfma_f32_4x4x1_16b_f32 instead: workgroups of 4, 8 or 12 candidates, every CU busy, no exchange between
 * workgroups.  0 = never; 1 (default) = where it shortens the launch; 2 = whenever the plan is eligible (testing).  The
 * arithmetic is ordered like the 16-candidate MATRIX-CORE kernels': results are bit-identical under all three policies wherever
 * policy 0 runs such a kernel.  The one exception: a generic recurrent stack whose 16-candidate matrix-core kernel does not fit
 * the LDS runs the VALU kernel under policy 0 (and for one-step / predict launches) - a different rounding, so there the
 * policies, and ranks of a sharded plan whose shard widths select different kernels, agree to the fp32 tolerance only.   */
int l2a_set_micro(l2a_ctx* ctx, int policy);
/* Status word of the launches issued since the last call (caller must have synchronised the
 * stream): 0 = fine, bit 0 = a member-split exchange timed out (results are invalid; relaunch
 * with l2a_set_split(ctx, 0)).  Reading clears it.                                            */
int l2a_launch_status(l2a_ctx* ctx, int* status_out);
/* How many polls a split workgroup may spend waiting for its partner, per launch, before it gives up and sets
 * status bit 0 (0 = default 2^18, about half a second).  Tests use a tiny value to force the condition. */
int l2a_set_spin_limit(l2a_ctx* ctx, unsigned int polls);
/* Test hook (host only): OR `bits` into the status word, as if a launch had reported them. */
int l2a_inject_status(l2a_ctx* ctx, int bits);
/* Developer aid (tools/timeline.py): when `device_ptr` is non-NULL the MFMA kernel's first
 * candidate tile stamps the shader clock at its phase boundaries into it as u64
 * [group 2][step h][set 8][slot 8].  NULL (default) disables it.                               */
int l2a_set_debug_buffer(l2a_ctx* ctx, void* device_ptr);

/* ---- model ----------------------------------------------------------------------------- */
/* Describe the MLP dynamics model: replaces the graph construction of
 * MLPDynamicsModel.__init__ (dynamics/mlp_dynamics.py:61-89) / the post-update graph of
 * MetaMLPDynamicsModel (meta_mlp_dynamics.py:143-163) and dynamics/core/utils.py:111-142.
 * `hidden` has `n_hidden` entries; `n_sets` weight sets are allocated (E).                  */
int l2a_model_create(l2a_ctx* ctx, int obs_dim, int act_dim, int n_hidden, const int* hidden,
                     int hidden_act, int output_act, int n_sets, int mode, l2a_model** out);
void l2a_model_destroy(l2a_model* model);

/* Load weight set `e` from fp32 DEVICE arrays in the reference's parameter order
 * (dynamics/core/layers.py:160-163; forward_mlp, dynamics/core/utils.py:250,273-274):
 *   ptrs = { hidden_0/kernel [in,h0], hidden_0/bias [h0], ..., output/kernel [hL,obs],
 *            output/bias [obs] },  kernels row-major [in, out].
 * Replaces feeding `network_params_feed_dict` on every sess.run (meta_mlp_dynamics.py:429-432).
 * The library re-packs into its own HBM layout (MFMA fragment order) on `stream`; the caller
 * keeps ownership of the source arrays and may free them once `stream` has passed this call. */
int l2a_model_set_weights(l2a_model* model, int e, const void* const* device_ptrs,
                          void* stream);

/* Normalisation statistics of set `e` (float64 HOST vectors, as `compute_normalization`
 * stores them, mlp_dynamics.py:253-262).  The +1e-10 of normalize/denormalize
 * (mlp_dynamics.py:265-270) is applied inside.  Passing NULL for all six = identity
 * (normalize_input=False).                                                                  */
int l2a_model_set_norm(l2a_model* model, int e, const double* mean_obs, const double* std_obs,
                       const double* mean_act, const double* std_act,
                       const double* mean_delta, const double* std_delta, void* stream);

/* ---- the hot path ------------------------------------------------------------------------ */
/* One random-shooting plan step: replaces the whole horizon loop of
 * MPCController.get_rs_action (policies/mpc_controller.py:116-129) and of one CEM iteration
 * (:92-100) - normalise, MLP (all sets), denormalise, state update, reward, discounted
 * return, arg-max - in one kernel launch.
 *
 *   obs0      device fp32 [m, obs_dim]        current observation of each env
 *   actions   device fp32 [h, m*n, act_dim]   candidate action sequences, row r = i*n + j
 *                                             (env i, candidate j) - the layout of
 *                                             `a.reshape(h, n*m, -1)` (mpc_controller.py:114)
 *   returns_out  device fp32 [m, n] or NULL   discounted return of every candidate
 *   best_key  device u64 [m]                  packed arg-max, see l2a_key_decode.  The library
 *                                             zeroes it on `stream` before the launch.
 *   cand_offset                               global index of local candidate 0 (multi-GPU
 *                                             sharding: indices in best_key are global)
 * Rows whose env index is i use weight set i in L2A_MODE_PER_BLOCK (needs n_sets >= m).
 * `discount` is float64 like the reference's `self.discount ** t` (:126); the kernel carries the power in
 * float64 by repeated multiplication and rounds it to fp32 once per step, where it meets the fp32 reward. */
int l2a_plan_rs(l2a_model* model, const float* obs0, const float* actions, int m, int n, int h,
                double discount, const l2a_reward* reward, int cand_offset, float* returns_out,
                unsigned long long* best_key, void* stream);

/* The blocking form of l2a_plan_rs - what `get_rs_action` (policies/mpc_controller.py:108-129) is to its caller:
 * observations in (HOST fp32 [m, obs_dim], m <= 64), arg-max keys out (HOST u64 [m]), nothing else to do.  The
 * library stages the observations in host-mapped memory that the kernel reads directly, keeps its own key slot
 * (zeroed by the previous launch) and lets the last candidate tile of the launch publish the keys and a sequence
 * number to a host-mapped mailbox which this call polls: no H2D copy, no memset, no D2H copy and no
 * hipStreamSynchronize on the path.  `actions` (device) must already be ordered before `stream`.  Single GPU only
 * (sharded plans need the keys on the device for the all-reduce: l2a_plan_rs).  Returns L2A_ESPLIT when the launch
 * was flagged (see l2a_launch_status); the status word is consumed.                                          */
int l2a_plan_rs_sync(l2a_model* model, const float* obs_host, const float* actions, int m, int n, int h,
                     double discount, const l2a_reward* reward, int cand_offset, float* returns_out,
                     unsigned long long* keys_host_out, void* stream);

/* A plan step cut along the horizon: launch k covers horizon steps t0 .. t0 + h_chunk - 1 of
 * get_rs_action's loop (policies/mpc_controller.py:116-127) and hands the per-candidate state and the
 * accumulated returns to launch k + 1.  Lets the host draw / upload the NEXT chunk of candidate actions (the
 * reference's `get_random_action`, :67-69,114, consumes its RNG stream horizon-major) while the GPU rolls out the
 * current one; the chain is bit-identical to one l2a_plan_rs over the whole horizon.
 *   state:       t0 == 0: obs0 [m, obs_dim] (state_per_row = 0) ; t0 > 0: state_out of the previous chunk
 *                [m * n, obs_dim] (state_per_row = 1)
 *   actions:     [h_chunk, m * n, act_dim] - the rows of this chunk only
 *   returns_in:  returns_out of the previous chunk (ignored when t0 == 0); returns_out [m, n] is required
 *   state_out:   [m * n, obs_dim] or NULL (last chunk); best_key: [m] or NULL (give it on the last chunk)   */
int l2a_plan_rs_chunk(l2a_model* model, const float* state, int state_per_row, const float* actions, int m, int n,
                      int h_chunk, int t0, double discount, const l2a_reward* reward, int cand_offset,
                      const float* returns_in, float* returns_out, float* state_out, unsigned long long* best_key,
                      void* stream);

/* ---- plans with a reward program ------------------------------------------------------------
 * l2a_reward_program_check: host only, needs no GPU.  L2A_EINVAL - with a message through l2a_last_error(NULL) - for an
 * unknown kind or source, a range outside its vector (OBS / NEXT / DELTA: obs_dim, ACT: act_dim), len != 1 on LINEAR /
 * INRANGE, a target range outside the constant table, counts above the capacities.  Both entries below call it first.
 *
 * l2a_score_trajectory: the scoring kernel alone (csrc/l2a_score.hip) - every candidate's discounted return and the
 * per-env arg-max of trajectories that are already in HBM.
 *   obs0     device fp32 [m, obs_dim]            observation of each env in front of step 0
 *   traj     device fp32 [h, m*n, obs_dim]       traj[t] = the state after horizon step t; row r belongs to env r / n
 *   actions  device fp32 [h, m*n, act_dim]
 * `obs` of step 0 is obs0[env], of step t > 0 traj[t - 1][r].  returns_out [m, n] or NULL, best_key [m] or NULL (zeroed
 * on `stream` in front of the launch; keys as l2a_plan_rs packs them: lowest index wins ties, NaN sorts highest,
 * indices are cand_offset + r % n).  A workgroup's 64 rows of a step must fit the LDS:
 * 256 * (2 * (obs_dim | 1) + (act_dim | 1)) bytes <= 63 KiB, e.g. obs_dim <= 117 at act_dim 16.
 *
 * l2a_plan_rs_program: the plan step for an env with a reward program - the rollout of l2a_rollout_traj (below: ONE launch
 * of the trajectory-writing micro-tile kernel for the plans that fit one, the same bits) or else `h` one-step launches of the rollout kernels
 * with the state carried from launch to launch (l2a_plan_rs_chunk's hand-off: traj[t] is launch t's state_out and launch
 * t + 1's state), then ONE scoring launch; all on `stream`, no host synchronisation inside.  The price of generality is
 * h launches per plan instead of one and a trajectory that passes through HBM; the rollout kernels themselves are
 * untouched.  traj_out: device fp32 [h, m*n, obs_dim], or NULL: the library keeps a buffer of its own (grown on demand,
 * which synchronises `stream`; freed with the model).  The launch status word keeps its meaning: a flagged tile-split
 * launch anywhere in the chain flags the call (l2a_launch_status) and the caller repeats it unsplit.                */
int l2a_reward_program_check(const l2a_reward_program* program, int obs_dim, int act_dim);
int l2a_score_trajectory(l2a_ctx* ctx, const float* obs0, const float* traj, const float* actions, int m, int n, int h,
                         int obs_dim, int act_dim, double discount, const l2a_reward_program* program, int cand_offset,
                         float* returns_out, unsigned long long* best_key, void* stream);
int l2a_plan_rs_program(l2a_model* model, const float* obs0, const float* actions, int m, int n, int h, double discount,
                        const l2a_reward_program* program, int cand_offset, float* returns_out,
                        unsigned long long* best_key, float* traj_out, void* stream);

/* ---- plans with a learned reward model --------------------------------------------------------
 * For envs with no closed-form reward at all (`use_reward_model=True`, reference policies/mpc_controller.py:121-123): the
 * reward of a transition is an MLP of (obs, act, next_obs), evaluated on the matrix cores (csrc/l2a_score_mlp.hip).  Per
 * row, all in fp32:
 *   x = [ (obs - mean_obs) * inv_obs | (act - mean_act) * inv_act | ((next_obs - obs) - mean_delta) * inv_delta ],
 *       inv = fp32(1 / (std + 1e-10)); obs_dim + act_dim + obs_dim features
 *   z = MLP(x): n_hidden = 1 .. 3 hidden layers with `hidden_act` (L2A_ACT_*), a linear scalar output layer
 *   r = z * fp32(std_r + 1e-10) + fp32(mean_r); r = NaN when any of the row's obs / act / next_obs values is not finite
 * and over a trajectory R = R + fp32(disc) * r with disc = discount ** t carried in float64, as l2a_score_trajectory.
 * A row's reward bits depend on that row's inputs only - not on m, n, cand_offset, the shard or the launch geometry.
 *
 * l2a_reward_model_check: host only, needs no GPU.  L2A_EINVAL - with a message through l2a_last_error(NULL) - unless
 * 1 <= obs_dim <= 64, 1 <= act_dim <= 16, 1 <= n_hidden <= 3, every hidden width a multiple of 64 up to 512 and
 * hidden_act one of L2A_ACT_*.  l2a_reward_model_create calls it first; a new model has identity statistics.
 * l2a_reward_model_set_weights: fp32 DEVICE arrays { hidden_0/kernel [2 obs_dim + act_dim, h0], hidden_0/bias [h0], ...,
 * output/kernel [hL, 1], output/bias [1] }, kernels row-major [in, out] as l2a_model_set_weights; re-packed on `stream`.
 * l2a_reward_model_set_norm: float64 HOST vectors (mean_r / std_r: one value each); all eight NULL = identity.
 * l2a_reward_model_predict: obs [rows, obs_dim], act [rows, act_dim], next_obs [rows, obs_dim] -> rewards_out [rows]
 * (device fp32) - the same kernel as a one-step trajectory with per-row observations.
 * l2a_score_trajectory_model: arguments and outputs as l2a_score_trajectory (keys, ties, NaN, best_key zeroed on `stream`).
 * l2a_plan_rs_reward_model: the rollout of l2a_plan_rs_program - the single launch of l2a_rollout_traj, or h one-step launches of
 * the rollout kernels through traj_out (or the model's own buffer) - followed by l2a_score_trajectory_model.  `rm` and `model` must live on the same
 * context and agree on obs_dim and act_dim (L2A_EINVAL).  A flagged tile-split launch anywhere in the chain flags the
 * call (l2a_launch_status), as for l2a_plan_rs_program.
 * l2a_reward_model_geometry: host only, needs no GPU - the scorer's launcher decision (its own function, on plain integers)
 * for `rows` = m * n candidates over `h` steps on a device of `num_cu` CUs (<= 0: 256) and `lds_per_block` bytes of LDS per
 * workgroup.  out[8] = { RT row tiles per pass, CT candidate tiles per workgroup, S steps per pass (CT * S = RT),
 * workgroups = ceil(rows / (16 CT)), passes = ceil(h / S), dynamic LDS bytes, 0, 0 }.  L2A_EINVAL for a NULL out, rows < 1,
 * h < 1, a model l2a_reward_model_check refuses, or an LDS size that no geometry fits.  Any geometry gives the same bits. */
int l2a_reward_model_check(int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act);
int l2a_reward_model_geometry(int obs_dim, int act_dim, int n_hidden, const int* hidden, long long rows, int h, int num_cu,
                              int lds_per_block, int* out);
int l2a_reward_model_create(l2a_ctx* ctx, int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act,
                            l2a_reward_model** out);
void l2a_reward_model_destroy(l2a_reward_model* rm);
int l2a_reward_model_set_weights(l2a_reward_model* rm, const void* const* device_ptrs, void* stream);
int l2a_reward_model_set_norm(l2a_reward_model* rm, const double* mean_obs, const double* std_obs, const double* mean_act,
                              const double* std_act, const double* mean_delta, const double* std_delta, const double* mean_r,
                              const double* std_r, void* stream);
int l2a_reward_model_predict(l2a_reward_model* rm, const float* obs, const float* act, const float* next_obs, int rows,
                             float* rewards_out, void* stream);
int l2a_score_trajectory_model(l2a_reward_model* rm, const float* obs0, const float* traj, const float* actions, int m, int n,
                               int h, double discount, int cand_offset, float* returns_out, unsigned long long* best_key,
                               void* stream);
int l2a_plan_rs_reward_model(l2a_model* model, l2a_reward_model* rm, const float* obs0, const float* actions, int m, int n,
                             int h, double discount, int cand_offset, float* returns_out, unsigned long long* best_key,
                             float* traj_out, void* stream);

/* ---- plans with a learned terminal value --------------------------------------------------------
 * A planner stops counting reward at the last horizon step; a learned value of the last predicted state added to the return
 * is the usual remedy for a short horizon (POLO, Lowrey et al. 2019; TD-MPC, Hansen et al. 2022).  Not in the reference: the
 * semantics are build-defined.  The value is an MLP of the observation, evaluated on the matrix cores (csrc/l2a_value.hip).
 * Per row (one candidate's state after the last horizon step), all in fp32, round to nearest, nothing contracted outside the
 * MFMAs:
 *   x  = (s_h - mean_obs) * inv_obs, inv_obs = fp32(1 / (std_obs + 1e-10)); obs_dim features
 *   z  = MLP(x): n_hidden = 1 .. 3 hidden layers with `hidden_act` (L2A_ACT_*), a linear scalar output layer
 *   v  = z * fp32(std_v + 1e-10) + fp32(mean_v); v = NaN when any value of the row's state is not finite
 *   w  = fp32(value_coef * d_h), d_h = discount ** h carried in float64 by h repeated multiplications from 1.0 (the rollout's
 *        own recurrence), multiplied by the float64 value_coef and rounded to fp32 ONCE
 *   R' = R + w * v, a separate multiply and add; w == 0 leaves R' = R bit for bit (v is not looked at)
 * Keys over R' are packed as l2a_plan_rs packs them (index cand_offset + j, the lowest index wins ties, NaN sorts highest);
 * best_key is zeroed on `stream` before the launch and every workgroup makes one integer atomicMax per env it touches - no
 * float atomics.  A row's value bits depend on that row's state only - not on m, n, cand_offset, the shard, the row's place in
 * a tile or the launch geometry.  Non-finite values follow IEEE through the formula; the planners' rules then apply unchanged.
 *
 * l2a_value_model_check: host only, needs no GPU.  L2A_EINVAL - with a message through l2a_last_error(NULL) - unless
 * 1 <= obs_dim <= 64, 1 <= n_hidden <= 3, every hidden width a multiple of 64 up to 512 and hidden_act one of L2A_ACT_*.
 * l2a_value_model_create calls it first; a new model has identity statistics.
 * l2a_value_model_geometry: host only, needs no GPU - the launcher's decision (its own function, on plain integers) for `rows`
 * states on a device of `num_cu` CUs (<= 0: 256) and `lds_per_block` bytes of LDS per workgroup: the smallest RT in 1 | 2 | 4 | 8
 * row tiles of 16 rows per workgroup that leaves at most `num_cu` workgroups, capped by the accumulators (RT * widest / 64
 * <= 32) and the LDS image (RT * max(ceil(obs_dim / 16), widest / 16) KiB + 4 KiB).  out[8] = { RT, workgroups =
 * ceil(rows / (16 RT)), dynamic LDS bytes, 0 .. }.  L2A_EINVAL for a NULL out, rows < 1, a model l2a_value_model_check
 * refuses, or an LDS size that no RT fits.  Any RT gives the same bits.
 * l2a_value_model_set_weights: fp32 DEVICE arrays { hidden_0/kernel [obs_dim, h0], hidden_0/bias [h0], ..., output/kernel
 * [hL, 1], output/bias [1] }, kernels row-major [in, out]; re-packed on `stream`.
 * l2a_value_model_set_norm: float64 HOST vectors mean_obs / std_obs [obs_dim], mean_v / std_v (one value each); all four
 * NULL = identity.
 * l2a_value_model_predict: states [rows, obs_dim] -> values_out [rows] (device fp32), the same kernel without the fold.
 * l2a_value_terminal: the kernel alone.  final_state [m*n, obs_dim], returns_in [m, n] -> returns_out [m, n] (or NULL;
 * returns_out == returns_in is allowed: the work is row-local) and best_key [m] (or NULL).  L2A_EINVAL, nothing launched and
 * no output touched: a NULL final_state / returns_in, both outputs NULL, m, n or h < 1, a non-finite value_coef or discount,
 * m * n > 2^30 - 1, cand_offset < 0 or cand_offset + n > 2^31 - 1.
 *
 * The plan steps - all stream-ordered, no host synchronisation unless a model-owned buffer grows (freed with the model); `vm`
 * and `model` must live on the same context and agree on obs_dim (L2A_EINVAL); a flagged tile-split launch flags the call
 * (l2a_launch_status); arguments otherwise as the entry each one extends:
 * l2a_plan_rs_value: ONE rollout launch as l2a_plan_rs_chunk makes it (t0 = 0, h_chunk = h, state_out into the model's own
 * buffer, no keys), then l2a_value_terminal.  The rollout kernels and their launch decisions are untouched: a state-writing
 * request takes the geometry it takes today (micro tiles decline it).
 * l2a_plan_rs_program_value / l2a_plan_rs_reward_model_value: l2a_plan_rs_program / l2a_plan_rs_reward_model with the keys
 * not requested, then l2a_value_terminal on traj[h - 1].                                                                  */
int l2a_value_model_check(int obs_dim, int n_hidden, const int* hidden, int hidden_act);
int l2a_value_model_geometry(int obs_dim, int n_hidden, const int* hidden, long long rows, int num_cu, int lds_per_block,
                             int* out);
int l2a_value_model_create(l2a_ctx* ctx, int obs_dim, int n_hidden, const int* hidden, int hidden_act, l2a_value_model** out);
void l2a_value_model_destroy(l2a_value_model* vm);
int l2a_value_model_set_weights(l2a_value_model* vm, const void* const* device_ptrs, void* stream);
int l2a_value_model_set_norm(l2a_value_model* vm, const double* mean_obs, const double* std_obs, const double* mean_v,
                             const double* std_v, void* stream);
int l2a_value_model_predict(l2a_value_model* vm, const float* states, int rows, float* values_out, void* stream);
int l2a_value_terminal(l2a_value_model* vm, const float* final_state, const float* returns_in, int m, int n, int h,
                       double discount, double value_coef, int cand_offset, float* returns_out, unsigned long long* best_key,
                       void* stream);
int l2a_plan_rs_value(l2a_model* model, l2a_value_model* vm, const float* obs0, const float* actions, int m, int n, int h,
                      double discount, const l2a_reward* reward, double value_coef, int cand_offset, float* returns_out,
                      unsigned long long* best_key, void* stream);
int l2a_plan_rs_program_value(l2a_model* model, l2a_value_model* vm, const float* obs0, const float* actions, int m, int n,
                              int h, double discount, const l2a_reward_program* program, double value_coef, int cand_offset,
                              float* returns_out, unsigned long long* best_key, float* traj_out, void* stream);
int l2a_plan_rs_reward_model_value(l2a_model* model, l2a_reward_model* rm, l2a_value_model* vm, const float* obs0,
                                   const float* actions, int m, int n, int h, double discount, double value_coef,
                                   int cand_offset, float* returns_out, unsigned long long* best_key, float* traj_out,
                                   void* stream);

/* ---- policy priors: candidates proposed by a learned policy ------------------------------------------
 * TD-MPC, LOOP and POPLIN seed a share of every population from a learned policy rolled in closed loop through the dynamics
 * model, a_t = pi(s_t) + sigma * eps, s_{t+1} = f(s_t, a_t).  l2a_policy_model is that policy: the value model's MLP with an
 * act_dim-wide linear output.  Per row, fp32, nothing contracted:
 *   x = (s - mu_obs) * inv_obs, inv = fp32(1 / (sd + 1e-10));   y = MLP(x), one accumulator chain per output element, k ascending,
 *   K zero-padded;   a_k = y_k * fp32(sd_a,k + 1e-10) + fp32(mu_a,k);   where sigma_k != 0: a_k = a_k + sigma_k * z_k (a multiply
 *   and an add; where sigma_k == 0 no z is read or drawn);   a_k = min(max(a_k, low_k), high_k), NaN propagating;   a row with a
 *   non-finite state value gets NaN in every action.
 * z is given, or the Philox4x32-10 + Box-Muller normal of l2a_cem_sample / l2a_mppi_sample at the counters stated below.
 *
 * l2a_policy_model_check: host only.  The limits of l2a_value_model_check and 1 <= act_dim <= 16 (one output tile); refuses with
 * a message through l2a_last_error(NULL).
 * l2a_policy_model_geometry: host only - l2a_value_model_geometry's contract and rule for this kernel's launcher.
 * l2a_policy_model_set_weights: fp32 DEVICE arrays { hidden_l/kernel, hidden_l/bias, ..., output/kernel [hL, act_dim],
 * output/bias [act_dim] }, kernels row-major [in, out].
 * l2a_policy_model_set_norm: float64 HOST vectors mean_obs / std_obs [obs_dim], mean_act / std_act [act_dim]; all four NULL =
 * identity.
 * l2a_policy_act: the kernel alone.  states [rows, obs_dim] -> actions_out [rows, act_dim]; z [rows, act_dim] or NULL: the
 * normal at counter offset + row * act_dim + k.  sigma / low / high: DEVICE fp32 [act_dim].  L2A_EINVAL for a NULL pointer or
 * rows outside 1 .. 2^30 - 1.
 * l2a_policy_propose: overwrites candidate j of env i, for every GLOBAL index gj = cand_offset + j < n_pi, in seq [h, m * n,
 * act_dim] (row i * n + j) and, when given, in mirror [n_total, m, h * act_dim] (row gj * m + i: the a_clip layout of
 * l2a_cem_refit / l2a_mppi_update / l2a_icem_refit) with the policy rolled in closed loop from obs0 [m, obs_dim]: per step one
 * launch of the policy kernel over the shard's proposal rows and, for t < h - 1, one one-step launch of the unchanged rollout
 * kernels (l2a_plan_rs_chunk's form: h_chunk = 1, an all-zero reward, state_out) - 2 h - 1 launches.  The normal of element
 * (t, i, gj, k) sits at counter offset + ((t * m + i) * n_pi + gj) * act_dim + k - positional in the global index, so shards
 * agree; an injected z [h, m, n_pi, act_dim] is indexed the same way.  Rows with gj >= n_pi are not touched; a shard without a
 * proposal row returns L2A_OK and launches nothing.  Stream-ordered; no host synchronisation unless the model-owned buffer
 * grows.  L2A_EINVAL before the first launch and before the buffer grows: a NULL pointer; m, n, h or n_pi < 1; n_pi > n_total;
 * cand_offset < 0 or cand_offset + n > n_total; `pm` and `model` on different contexts or disagreeing on obs_dim / act_dim;
 * per-block mode with m > n_sets; m * n > 2^30 - 1.  A flagged tile-split launch in the chain flags the call
 * (l2a_launch_status).                                                                                                    */
int l2a_policy_model_check(int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act);
int l2a_policy_model_geometry(int obs_dim, int act_dim, int n_hidden, const int* hidden, long long rows, int num_cu,
                              int lds_per_block, int* out);
int l2a_policy_model_create(l2a_ctx* ctx, int obs_dim, int act_dim, int n_hidden, const int* hidden, int hidden_act,
                            l2a_policy_model** out);
void l2a_policy_model_destroy(l2a_policy_model* pm);
int l2a_policy_model_set_weights(l2a_policy_model* pm, const void* const* device_ptrs, void* stream);
int l2a_policy_model_set_norm(l2a_policy_model* pm, const double* mean_obs, const double* std_obs, const double* mean_act,
                              const double* std_act, void* stream);
int l2a_policy_act(l2a_policy_model* pm, const float* states, int rows, const float* z, unsigned long long seed,
                   unsigned long long offset, const float* sigma, const float* low, const float* high, float* actions_out,
                   void* stream);
int l2a_policy_propose(l2a_model* model, l2a_policy_model* pm, const float* obs0, int m, int n, int n_pi, int h, int cand_offset,
                       const float* z, unsigned long long seed, unsigned long long offset, const float* sigma, const float* low,
                       const float* high, float* seq, float* mirror, int n_total, void* stream);

/* ---- plans on envs that terminate: termination programs ---------------------------------------------
 * Hopper, Walker2d, gym's Ant and Humanoid end an episode when the state leaves a healthy range; PETS and MBPO carry a per-env
 * termination function for that reason.  Not in the reference (its five envs never set `done`): the semantics are build-defined.
 * A termination program is 1 .. 8 guards over the NEXT observation of a step.  Guard g = { index, len, lo, hi } holds iff every
 * x in next_obs[index : index + len] satisfies lo <= x <= hi (a NaN is outside, as L2A_TERM_INRANGE has it; lo = -inf and
 * hi = +inf are allowed).  A transition is terminal iff any guard fails.  Per candidate row, in fp32, round to nearest, nothing
 * contracted, disc = discount ** t carried in float64 and rounded once per step exactly as l2a_score_trajectory does:
 *   alive = true; R = 0; steps_alive = h
 *   for t in 0 .. h-1, while alive:
 *       R = R + fp32(disc) * r_t                        r_t: the reward program on (obs, act, next), or step_rewards[t][row]
 *       if any guard fails on next_obs:
 *           if terminal_reward != 0: R = R + fp32(disc) * terminal_reward         a separate multiply and add; skipped at 0
 *           alive = false; steps_alive = t + 1
 *   if alive and terminal_values given and w != 0: R = R + w * terminal_values[row]       w as l2a_value_terminal defines it
 * The terminating transition's reward counts, as in gym; nothing after it is looked at - a selection, not a multiplication by
 * zero: a NaN that appears in the trajectory (or in step_rewards) after a row's terminal step does not reach R.  Non-finite
 * values otherwise follow IEEE.  Keys are packed as everywhere: lowest index wins ties, NaN sorts highest, the index is
 * cand_offset + j; one integer atomicMax per (workgroup, env touched), no float atomics.  For a row whose guards never fire, R
 * is bit-equal to l2a_score_trajectory's; with step rewards taken from a reward model as l2a_plan_rs_term takes them, to
 * l2a_score_trajectory_model's; with terminal values, to l2a_plan_rs_program_value's / _reward_model_value's.
 *
 * l2a_termination_check: host only, needs no GPU.  L2A_EINVAL - with a message through l2a_last_error(NULL) - for a NULL program,
 * n_guards outside 1 .. 8, a non-finite terminal_reward, a guard with len < 1 or a range outside obs_dim, a NaN bound, lo > hi.
 *
 * l2a_score_trajectory_term: the kernel alone (l2a_score_term_k, csrc/l2a_score.hip), on trajectories that are already in HBM.
 * Exactly one of `program` / `step_rewards` (device fp32 [h, m*n]) is given; with step_rewards, obs0 and actions are not read
 * and may be NULL.  obs0 / traj / actions as l2a_score_trajectory.  terminal_values: device fp32 [m*n], or NULL.  returns_out
 * [m, n] or NULL, steps_alive_out int32 [m, n] or NULL, best_key [m] or NULL (zeroed on `stream` in front of the launch).
 * Every refusal (L2A_EINVAL) is made before the memset and the launch: both or neither of program / step_rewards, a program or
 * a termination its check refuses, a NULL traj (or obs0 / actions with a program), all three outputs NULL, m, n or h < 1, a
 * non-finite discount or value_coef, m * n > 2^30 - 1, cand_offset < 0 or cand_offset + n > 2^31 - 1, and the LDS bound:
 * l2a_score_trajectory's with a program, 256 * (obs_dim | 1) bytes <= 63 KiB with step_rewards.
 *
 * l2a_plan_rs_term: the plan step - stream-ordered, no host synchronisation unless a model-owned buffer grows (freed with the
 * model).  Exactly one of `rm` / `program` is given; `vm` may be NULL (value_coef is then not looked at beyond its finiteness).
 *   1. the rollout of l2a_rollout_traj (single launch or carry chain; the launch status word keeps its meaning);
 *   2. with a reward model, the per-step rewards from the scorer kernel of l2a_score_trajectory_model, unchanged: step 0 is one
 *      l2a_score_trajectory_model call with h = 1 and discount 1 into rewards[0]; steps 1 .. h - 1 are ONE
 *      l2a_reward_model_predict over the (h - 1) * m * n contiguous rows obs = traj[0 .. h-2], act = actions[1 ..], next =
 *      traj[1 ..] (refused when (h - 1) * m * n > 2^30 - 1);
 *   3. with a value model, one l2a_value_model_predict on traj[h - 1];
 *   4. one launch of l2a_score_term_k.
 * Launches: rollout + 1 for a program, rollout + 3 for a reward model (+ 2 at h = 1), + 1 with a value model.  `rm`, `vm` and
 * `model` must live on the same context and agree on obs_dim / act_dim (L2A_EINVAL).  A fused l2a_reward reaches this entry as
 * a program (RewardProgram.from_spec on the Python side).  traj_out as l2a_plan_rs_program.                               */
#define L2A_TERMINATION_MAX_GUARDS 8
typedef struct l2a_guard {
    int index;                   /* next_obs[index : index + len]                                       */
    int len;
    float lo;                    /* the guard holds iff lo <= x <= hi for every element                 */
    float hi;
} l2a_guard;
typedef struct l2a_termination {
    int n_guards;                /* 1 .. L2A_TERMINATION_MAX_GUARDS                                     */
    int reserved;
    float terminal_reward;       /* added, discounted, at the terminating step; 0: nothing is added     */
    float reserved2;
    l2a_guard guards[L2A_TERMINATION_MAX_GUARDS];
} l2a_termination;
int l2a_termination_check(const l2a_termination* termination, int obs_dim);
int l2a_score_trajectory_term(l2a_ctx* ctx, const float* obs0, const float* traj, const float* actions, const float* step_rewards,
                              int m, int n, int h, int obs_dim, int act_dim, double discount, const l2a_reward_program* program,
                              const l2a_termination* termination, const float* terminal_values, double value_coef,
                              int cand_offset, float* returns_out, int* steps_alive_out, unsigned long long* best_key,
                              void* stream);
int l2a_plan_rs_term(l2a_model* model, l2a_reward_model* rm, l2a_value_model* vm, const float* obs0, const float* actions, int m,
                     int n, int h, double discount, const l2a_reward_program* program, const l2a_termination* termination,
                     double value_coef, int cand_offset, float* returns_out, int* steps_alive_out, unsigned long long* best_key,
                     float* traj_out, void* stream);

/* ---- the MLP planner's trajectory rollout -------------------------------------------------------
 * What l2a_plan_rs_program and l2a_plan_rs_reward_model put in front of their scoring launch, and the MLP counterpart of
 * l2a_lstm_rollout_traj.  Stream-ordered; no host synchronisation unless the model's own buffer grows.
 *
 * l2a_rollout_traj: the model's rollout alone.  obs0 [m, obs_dim] (one row per env, as l2a_plan_rs), actions
 * [h, m*n, act_dim] -> traj_out device fp32 [h, m*n, obs_dim], traj_out[t] = the predicted observation after horizon step t;
 * traj_out NULL: the model's own buffer (grown on demand; freed with the model).  No rewards.  Two paths, the same bits on both:
 *   single launch  hidden width 256 / 512 on the matrix-core kernels, when the whole plan is one micro-tile launch (at most
 *                  three micro tiles per CU), its LDS fits, the streamed weight sets span < 2^31 bytes and a step's slice of the
 *                  trajectory and of the actions is < 2^31 - 16 bytes - and wanted under l2a_set_micro (0 never, 2 whenever
 *                  eligible, 1 the measured classes: DESIGN 4.8): the trajectory-writing instance of the micro-tile kernel,
 *                  the state never leaves the CU between steps.
 *   carry chain    everything else: h one-step l2a_plan_rs_chunk launches with an all-zero reward, state_out = traj_out[t].
 * cand_offset is validated as everywhere and changes nothing in the trajectory.  The launch status word keeps its meaning: a
 * flagged tile-split launch anywhere in the chain flags the call (l2a_launch_status); the single launch has no exchange.
 *
 * l2a_mlp_traj_geometry: host only, needs no GPU - which path l2a_rollout_traj takes for `n_hidden` layers of `hidden` units,
 * `n_sets` weight sets in `mode` (L2A_MODE_*), under micro policy `micro_policy` (0 | 1 | 2) on `num_cu` CUs (<= 0: 256) with
 * the automatic kernel choice and 160 KiB of LDS; the decision function is the launcher's own.  out[8]: { 0 single launch (1) or
 * chain (0), 1 launches of the rollout, 2 workgroups of a launch, 3 workgroups per env (single launch), 4 micro tiles of the
 * largest workgroup (99: no workgroup geometry), 5 workgroups of that size per env, 6 .. 7 zero }.  L2A_EINVAL for a NULL out,
 * sizes < 1, an unknown mode or policy, more than 2^30 - 1 candidates, per-block mode with m > n_sets.                     */
int l2a_rollout_traj(l2a_model* model, const float* obs0, const float* actions, int m, int n, int h, int cand_offset,
                     float* traj_out, void* stream);
int l2a_mlp_traj_geometry(int obs_dim, int act_dim, int n_hidden, int hidden, int mode, int n_sets, int m, int n, int h,
                          int micro_policy, int num_cu, int* out);

/* ---- particle plans: trajectory sampling over the members of a mean ensemble -----------------------
 * PETS-style TS-infinity and TS1 (Chua et al. 2018); not in the reference, the semantics are build-defined.  TS-infinity first
 * (a particle stays on one member for the whole horizon; TS1, which deals the particles anew at every step, follows).  Every member of an
 * L2A_MODE_MEAN model of E = n_sets >= 2 weight sets rolls every candidate out as a trajectory of its own, and a candidate is
 * scored by the mean of its E returns, less `lambda` times their standard deviation (lambda > 0 prefers plans the members
 * agree on, lambda < 0 seeks disagreement, 0 is the plain mean).
 *
 * l2a_particle_score: the reduction alone (csrc/l2a_particles.hip).
 *   member_returns  device fp32 [m, E, n]     R_e of candidate j of env i at (i * E + e) * n + j;  E >= 1
 *   score_out       device fp32 [m, n] or NULL
 *   spread_out      device fp32 [m, n] or NULL  the standard deviation `std` below
 *   best_key        device u64 [m] or NULL    zeroed on `stream` in front of the launch; keys as l2a_plan_rs packs them over the
 *                                             SCORE: index cand_offset + j, lowest index wins ties, NaN sorts highest
 * Arithmetic (fixed, so that a host can restate it bit for bit - tests/particle_reference.py): fp32, round to nearest, nothing
 * contracted, e ascending.  s = R_0, s = s + R_e; mean = s / (float)E; v = 0, d = R_e - mean, v = v + d * d as a separate
 * multiply and add; std = sqrtf(v / (float)E); score = mean - lambda * std as a separate multiply and subtract - and with
 * lambda == 0 the score is `mean` itself (a +inf mean stays +inf where 0 * NaN would not).  Non-finite member returns follow IEEE
 * through this formula: one NaN member makes the candidate's score NaN; +inf and -inf members together likewise; a lone +inf
 * gives mean +inf and std NaN.  The planners' rules then apply unchanged: a NaN score is the arg-max (l2a_cem_pick, the keys),
 * l2a_mppi_update weighs NaN and -inf with 0.  No float atomics: the same inputs give the same bits on every run and grid.
 * L2A_EINVAL (nothing launched): a NULL member_returns, all three outputs NULL, m / E / n < 1, a non-finite lambda,
 * m * E * n > 2^30 - 1, a bad cand_offset.
 *
 * l2a_plan_rs_particles: the plan step.  obs0, actions, m, n, h, discount, reward, cand_offset as l2a_plan_rs.  An expansion
 * launch copies the inputs into the model's own buffer (grown on demand, which synchronises `stream`; freed with the model) as
 * m per-block requests of E blocks - particle row (i * E + e) * n + j - then every env's request runs as its own launch of
 * the rollout kernels on the model's E weight sets (block e <-> set e, returns only), then l2a_particle_score: m + 2 launches
 * on `stream` where every request is one launch (a request the launcher cuts in two - double rounds and their rest - is two),
 * no host synchronisation.  score_out [m, n], spread_out [m, n], best_key [m] as above (score_out or best_key is
 * required); member_returns_out [m, E, n] or NULL (the model's buffer then).  The member returns are bit-equal to l2a_plan_rs
 * on a per-block model of the same E sets fed the expanded inputs.  The launch status word keeps its meaning: a flagged
 * tile-split launch anywhere flags the call (l2a_launch_status).
 * l2a_plan_rs_particles_program / _reward_model: the same with every request's trajectory rollout and scoring launch of
 * l2a_plan_rs_program / l2a_plan_rs_reward_model in place of the fused rollout: 2 m + 2 launches where the trajectory rollout is
 * its single launch, m (h + 1) + 2 on the carry chain.
 * L2A_EINVAL (nothing launched, no output touched): a model that is not L2A_MODE_MEAN with n_sets >= 2, a non-finite lambda,
 * m / n / h < 1, m * E * n > 2^30 - 1, a bad cand_offset, a NULL pointer, what the stem entry refuses of its reward, an action
 * tensor beyond one expansion launch (2^32 - 257 words of 16 bytes, or of 4 where n * act_dim is no multiple of four).  A refused
 * call does not grow the model's buffer either.          */
int l2a_particle_score(l2a_ctx* ctx, const float* member_returns, int m, int E, int n, float lambda, int cand_offset,
                       float* score_out, float* spread_out, unsigned long long* best_key, void* stream);
int l2a_plan_rs_particles(l2a_model* model, const float* obs0, const float* actions, int m, int n, int h, double discount,
                          const l2a_reward* reward, float lambda, int cand_offset, float* score_out, float* spread_out,
                          float* member_returns_out, unsigned long long* best_key, void* stream);
int l2a_plan_rs_particles_program(l2a_model* model, const float* obs0, const float* actions, int m, int n, int h, double discount,
                                  const l2a_reward_program* program, float lambda, int cand_offset, float* score_out,
                                  float* spread_out, float* member_returns_out, unsigned long long* best_key, void* stream);
int l2a_plan_rs_particles_reward_model(l2a_model* model, l2a_reward_model* rm, const float* obs0, const float* actions, int m, int n,
                                       int h, double discount, float lambda, int cand_offset, float* score_out, float* spread_out,
                                       float* member_returns_out, unsigned long long* best_key, void* stream);

/* ---- particle plans, TS1: the particles are dealt anew over the members at every horizon step ------------
 * Between horizon steps t and t + 1 ("boundary t", t = 0 .. h - 2) every candidate's E particles - state and accumulated return -
 * move among the E blocks by a random permutation; block e <-> weight set e stays what the rollout kernels know.  A permutation
 * keeps every member at exactly one particle per candidate (PETS' own implementation shuffles the same way).
 *
 * The permutation pi = pi(seed, offset, t, i, gj), gj = cand_offset + j: pi(e) is the block that the particle of block e CAME FROM.
 * Fisher-Yates from the identity, k = E - 1 down to 1: r = (word * (k + 1)) >> 32 (64-bit product), entries k and r change
 * places.  Draw d = E - 1 - k is word d & 3 of Philox4x32-10 with key `seed`, counter words
 * { lo, hi, 0x7065726d ('perm') + (d >> 2), 0 } of ctr = ((offset + t * m + i) << 31) | gj.  The domain word differs from the
 * uniform stream's ('unif') and from CEM's.  A 32-bit word gives r a bias of at most k / 2^32 against the uniform draw - below
 * 4e-9 at E = 16.  `offset` counts (step, env) slots: every slot offset + t * m + i must stay below 2^33 - a whole plan needs
 * offset + h * m <= 2^33 - and E <= 16.  pi is positional: it depends on those five values and on nothing else - not on n, the
 * grid, the shard or the run.
 *
 * l2a_particle_perm: host only, needs no GPU; the same code the kernel runs.  out_host uint8 [i_count, cand_count, E]: row
 * (i * cand_count + j) * E + e = pi(e) of env i_first + i, candidate cand_first + j at boundary t.  L2A_EINVAL, out_host untouched:
 * E < 1, E > 16, a NULL out_host, t < 0, m < 1, a negative range, i_first + i_count > m, cand_first + cand_count > 2^31 - 1,
 * a slot offset + t * m + i at or beyond 2^33.
 *
 * l2a_particle_shuffle: the kernel alone (csrc/l2a_particles.hip), ONE launch for all m envs, out of place:
 *   state_out[i][e][j][:] = state_in[i][pi(e)][j][:]     states device fp32 [m][E * n][obs_dim]
 *   ret_out[i][e][j]      = ret_in[i][pi(e)][j]          returns device fp32 [m][E][n]
 * A pure copy of 32-bit words: NaN payloads, infinities and -0 pass bit for bit.  perm: NULL (Philox, above), or device uint8
 * [m, n, E], row (i * n + j) * E + e = pi(e), which replaces the draw.  Injected entries are not validated on the device: an entry
 * >= E is clamped to E - 1 (never a read out of bounds), and a row that is no permutation duplicates and drops particles.
 * L2A_EINVAL, nothing launched, no output touched: a NULL buffer, state_out overlapping state_in or ret_out overlapping ret_in,
 * m / E / n / obs_dim < 1, t < 0, E > 16, m * E * n > 2^30 - 1, a bad cand_offset (l2a_particle_score's limits), a slot at or beyond 2^33.
 *
 * l2a_plan_rs_particles_ts1: the plan step.  l2a_plan_rs_particles' checks and expansion, then for t = 0 .. h - 1 every env's
 * request as ONE-step launches of the rollout kernels (l2a_plan_rs_chunk's hand-off, per-block mode, E blocks) and between t and
 * t + 1 ONE shuffle launch over all envs, then l2a_particle_score: m * h + h + 1 launches where every request is one launch, on
 * `stream`, no host synchronisation.  States and returns ping-pong in the model's own buffer (grown on demand before the first
 * launch, which synchronises `stream`).  perm: NULL, or device uint8 [h - 1, m, n, E] (boundary t at t * m * n * E).  With identity
 * permutations, and at h = 1 (no shuffle is launched), every output is bit-equal to l2a_plan_rs_particles.  score_out, spread_out,
 * best_key as there; particle_returns_out [m, E, n] or NULL: the returns of the particles that END in block e - row e is no
 * longer member e's: every step of such a return was predicted by the member its particle sat on at that step.  This entry takes
 * the fused l2a_reward formula; reward programs and reward models - whose scorers read a step's two states from one trajectory row,
 * which a shuffle breaks - plan through the two entries below, which take each step's reward at the boundary.
 * The launch status word keeps its meaning: a flagged tile-split launch anywhere flags the call (l2a_launch_status); the caller
 * repeats it unsplit with the same seed / offset, which replays the same permutations.
 * L2A_EINVAL (nothing launched, no output touched, the buffer not grown): what l2a_plan_rs_particles refuses, n_sets > 16,
 * a NULL reward, offset + h * m > 2^33.
 *
 * TS1 with a reward program or a reward model.  At the boundary behind horizon step t the step's pre-state, action and post-state
 * of every particle lie in device memory, so the step's reward is taken in the launch that moves the particles:
 * l2a_particle_step: the kernel alone (csrc/l2a_particle_step.hip), ONE launch for all m envs, out of place.  For every particle
 * (env i, block e, candidate j), BEFORE anything moves:
 *   r  = program(pre, action, post)    l2a_score_trajectory's arithmetic, operation for operation (RewardProgram.evaluate_f32
 *                                      restates it bit for bit), or rewards[i][e][j] - exactly one of `program` / `rewards` is given
 *   R' = R + (float)disc_t * r         a separate multiply and add; R = ret_in[i][e][j], or the literal 0.0f when ret_in is NULL
 *                                      (the addition is still made: a -0 reward gives +0, as in the trajectory scorer)
 * then   ret_out[i][e][j] = R'[i][pi(e)][j],   state_out[i][e][j][:] = post[i][pi(e)][j][:]   (32-bit words, as the shuffle's)
 * with pi of boundary t as l2a_particle_shuffle takes it (perm NULL: Philox of seed / offset / t; else device uint8 [m, n, E],
 * entries >= E clamped to E - 1).  state_out NULL is the last step: nothing is dealt, perm is neither read nor checked, ret_out[e] = R'[e].
 *   pre      device fp32 [m][E][obs_dim] (pre_per_row 0: one row per member block, the expansion's obs_x) or [m][E * n][obs_dim]
 *   post     device fp32 [m][E * n][obs_dim]
 *   actions  device fp32, env i's [E * n][act_dim] at actions + i * act_env_stride floats (act_env_stride >= E * n * act_dim)
 *   rewards, ret_in, ret_out   device fp32 [m][E][n];  disc_t: discount ** t as the host's repeated product d *= discount
 * L2A_EINVAL, nothing launched, no output touched: what l2a_particle_shuffle refuses (a NULL pre / post / actions / ret_out,
 * act_dim < 1 likewise), both or neither of rewards / program, a program l2a_reward_program_check refuses, dimensions of which 64
 * staged rows (each 2 (obs_dim | 1) + (act_dim | 1) words) do not fit 61 KiB of LDS (program mode), a bad act_env_stride, an output overlapping an input
 * or the other output.
 *
 * l2a_plan_rs_particles_ts1_program / _reward_model: l2a_plan_rs_particles_ts1 with the program, or the reward model, in place of
 * the l2a_reward.  The expansion once; per step and env ONE one-step launch of the rollout kernels with an all-zero fused reward
 * that writes the step's post-states (the carry chain's form); the reward-model entry then scores every env's step with a one-step
 * launch of the reward model's kernel at discount 1 into a rewards buffer; per step ONE l2a_particle_step over all envs; then
 * l2a_particle_score: m * h + h + 2 launches (program), 2 * m * h + h + 2 (reward model).  Three state buffers (pre / post / dealt)
 * and two return buffers rotate in the model's own buffer.  With identity permutations, and at h = 1, every output is bit-equal to
 * l2a_plan_rs_particles_program / _reward_model.  Outputs, perm, seed, offset, cand_offset and the refusals as
 * l2a_plan_rs_particles_ts1 (the reward's own checks as l2a_plan_rs_particles_program / _reward_model make them), and a
 * particle_returns_out that overlaps perm.  The last step reads no table: perm's h - 1 boundaries are all that is touched. */
int l2a_particle_perm(unsigned long long seed, unsigned long long offset, int t, int m, int i_first, int i_count, int cand_first,
                      int cand_count, int E, unsigned char* out_host);
int l2a_particle_shuffle(l2a_ctx* ctx, const float* state_in, const float* ret_in, float* state_out, float* ret_out,
                         const unsigned char* perm, unsigned long long seed, unsigned long long offset, int t, int m, int E, int n,
                         int obs_dim, int cand_offset, void* stream);
int l2a_plan_rs_particles_ts1(l2a_model* model, const float* obs0, const float* actions, int m, int n, int h, double discount,
                              const l2a_reward* reward, float lambda, unsigned long long seed, unsigned long long offset,
                              const unsigned char* perm, int cand_offset, float* score_out, float* spread_out,
                              float* particle_returns_out, unsigned long long* best_key, void* stream);
int l2a_particle_step(l2a_ctx* ctx, const float* pre, int pre_per_row, const float* post, const float* actions,
                      long long act_env_stride, const float* rewards, const l2a_reward_program* program, double disc_t,
                      const float* ret_in, float* state_out, float* ret_out, const unsigned char* perm, unsigned long long seed,
                      unsigned long long offset, int t, int m, int E, int n, int obs_dim, int act_dim, int cand_offset,
                      void* stream);
int l2a_plan_rs_particles_ts1_program(l2a_model* model, const float* obs0, const float* actions, int m, int n, int h, double discount,
                                      const l2a_reward_program* program, float lambda, unsigned long long seed,
                                      unsigned long long offset, const unsigned char* perm, int cand_offset, float* score_out,
                                      float* spread_out, float* particle_returns_out, unsigned long long* best_key, void* stream);
int l2a_plan_rs_particles_ts1_reward_model(l2a_model* model, l2a_reward_model* rm, const float* obs0, const float* actions, int m,
                                           int n, int h, double discount, float lambda, unsigned long long seed,
                                           unsigned long long offset, const unsigned char* perm, int cand_offset, float* score_out,
                                           float* spread_out, float* particle_returns_out, unsigned long long* best_key,
                                           void* stream);

/* One-step batched prediction: MLPDynamicsModel.predict / MetaMLPDynamicsModel.predict
 * (mlp_dynamics.py:204-222, meta_mlp_dynamics.py:276-294).
 *   obs device fp32 [R, obs_dim], act device fp32 [R, act_dim] -> next_obs device fp32 [R, obs_dim]
 * In L2A_MODE_PER_BLOCK the rows are split into `n_blocks` equal blocks (block i <-> set i);
 * pass n_blocks = 1 otherwise.                                                               */
int l2a_predict(l2a_model* model, const float* obs, const float* act, int rows, int n_blocks,
                float* next_obs_out, void* stream);

/* best_key packing (host helpers, pure functions):
 *   key = (orderable_u32(return) << 31) | (0x7fffffff - global_index), top bit always 0, so
 *   unsigned max == signed max == "largest return, ties -> lowest index" = np.argmax
 *   (mpc_controller.py:129).  A max all-reduce of the keys over ranks (RCCL, int64 MAX) is the
 *   only collective of a plan step.                                                          */
unsigned long long l2a_key_encode(float ret, int index);
void l2a_key_decode(unsigned long long key, float* ret, int* index);

/* Batched form of l2a_model_set_weights for `count` consecutive weight sets first_set .. first_set+count-1
 * whose parameters are stacked along a leading axis: device_ptrs[i] points at parameter i of set first_set
 * and set_strides[i] (in floats) is the distance to the same parameter of the next set.  This is the shape
 * GrBAL's inner adaptation produces (`_adapted_param_values`, meta_mlp_dynamics.py:344,429-432: one dict of
 * arrays per task) when all tasks are adapted in one batched step; 2 * (n_hidden + 1) strided copies and
 * n_hidden + 1 pack launches in total instead of per set.                                              */
int l2a_model_set_weights_strided(l2a_model* model, int first_set, int count, const void* const* device_ptrs,
                                  const long long* set_strides, void* stream);

/* GrBAL's inner adaptation on the device: for every task i < m one SGD step
 *   theta_i = theta - lr * grad mean((f_theta(x_i) - y_i)^2)
 * (MetaMLPDynamicsModel.adapt / _adapt_sym, dynamics/meta_mlp_dynamics.py:321-345,409-421; loss :118), written
 * straight into weight sets 0 .. m-1 of `model` (L2A_MODE_PER_BLOCK) in both the reference layout and the
 * kernel's packed layout - replaces the sess.run + host round trip of the adapted parameters (:344) and their
 * re-feed on every later predict (:429-432).  base_ptrs: the pre-update parameters theta in the order of
 * l2a_model_set_weights (device fp32).  x [m, rows, obs_dim + act_dim] and y [m, rows, obs_dim] (device fp32):
 * the NORMALISED inputs and target deltas of each task's adaptation batch (:324-326; rows <= 16 =
 * adapt_batch_size of run_scripts/run_grbal.py).  Requires an identity output layer and a relu / tanh /
 * sigmoid / identity hidden nonlinearity.                                                             */
int l2a_model_adapt_sgd(l2a_model* model, const void* const* base_ptrs, const float* x, const float* y, int m,
                        int rows, float lr, void* stream);

/* The same step with the adaptation batches handed over as HOST arrays - which is how the reference's caller holds
 * them (samplers/sampler.py:81-90 passes lists of NumPy arrays to dynamics_model.adapt).  x_host / y_host are copied
 * into host-mapped staging that the kernels read directly (no H2D copy on the stream; two slots, so the call only
 * waits when the launch two steps back is still running).  The arrays may be reused as soon as the call returns.
 * Results are bit-identical to l2a_model_adapt_sgd.                                                       */
int l2a_model_adapt_sgd_host(l2a_model* model, const void* const* base_ptrs, const float* x_host, const float* y_host,
                             int m, int rows, float lr, void* stream);

/* The same step from the UN-normalised transitions, as `dynamics_model.adapt(obs, act, next_obs)` receives them
 * (meta_mlp_dynamics.py:321-326): float64 host arrays obs / next_obs [m, rows, obs_dim], act [m, rows, act_dim] and the six
 * float64 normalisation vectors (`self.normalization`).  The first forward launch normalises inputs and target deltas
 * itself - (v - mean) / (std + 1e-10) in float64, then the cast to fp32, i.e. the host's arithmetic bit for bit
 * (mlp_dynamics.py:265-266) - so the host keeps nothing but the copy into staging.  Input layers of at most 128 features. */
int l2a_model_adapt_sgd_raw(l2a_model* model, const void* const* base_ptrs, const double* obs_host,
                            const double* act_host, const double* next_obs_host, const double* mean_obs,
                            const double* std_obs, const double* mean_act, const double* std_act,
                            const double* mean_delta, const double* std_delta, int m, int rows, float lr, void* stream);

/* Copy weight set `e` out of the model in the reference's parameter order and layout (device fp32 buffers of
 * the sizes l2a_model_set_weights takes) - e.g. to read back adapted sets (`_adapted_param_values`).    */
int l2a_model_get_weights(l2a_model* model, int e, void* const* device_ptrs_out, void* stream);

/* ---- cross-entropy-method planner: the per-iteration work around the rollout, on the device -----------------------
 * `MPCController.get_cem_action` (policies/mpc_controller.py:71-106).  reference = 1 keeps the reference's semantics
 * (rollouts on the UNCLIPPED samples with its candidate-major rows read as env-major, :92-96; "elites" = the boolean
 * rank mask of :101 pooled over the envs), 0 = clipped rollouts, env-major rows, true top-k per env.
 *
 * l2a_cem_sample: a = mean + z * std (:86), clip (:87) for all n * m sample rows of one iteration.  z [n, m, D]
 * (device fp32, D = h * act_dim) or NULL: standard normals from Philox4x32-10 + Box-Muller, element e of the iteration
 * drawing counter (offset + e) under `seed` - every rank of a sharded plan generates the same numbers.  mean / std
 * [m, D], low / high [act_dim] (device).  Outputs: a_clip [n, m, D], a_raw [n, m, D] (optional, the unclipped samples)
 * and seq [h, m * (hi - lo), act_dim], the candidate tensor l2a_plan_rs reads for candidates lo <= j < hi (this
 * rank's shard; optional).
 *
 * l2a_cem_refit: elites of `returns` [m, n] and the update mean = alpha * mean + (1 - alpha) * mean(elites),
 * std = std(elites) (:101-104; biased) on mean / std [m, D] in place; elite_rows [m * num_elites] is scratch.  No sort:
 * the mask of :101 only needs the ranks of the first num_elites candidates.                                     */
int l2a_cem_sample(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset,
                   const float* mean, const float* std, const float* low, const float* high, int n, int m, int h,
                   int act_dim, int reference, int lo, int hi, float* a_clip, float* a_raw, float* seq, void* stream);
int l2a_cem_refit(l2a_ctx* ctx, const float* returns, const float* a_clip, int n, int m, int D, int num_elites,
                  int reference, float alpha, int* elite_rows, float* mean, float* std, void* stream);
/* l2a_cem_pick: what the plan returns (:106), in one buffer for one read-back: per env the arg-max of the LAST iteration's
 * `returns` [m, n] (first maximum), the first action of that candidate in `cand` - the unclipped samples read as [m, n, D]
 * (reference = 1, :92-96) or the clipped samples [n, m, D] (0) - and its return; behind them the final mean / std.
 * out: m x (act_dim + 2) floats (action | return | index as the bits of an int32), then mean [m, D], std [m, D].  NaN
 * returns are ordered as np.argmax orders them (a NaN is the maximum, the first one wins): a diverged plan reports NaN.  */
int l2a_cem_pick(l2a_ctx* ctx, const float* returns, const float* cand, const float* mean, const float* std, int n, int m,
                 int D, int act_dim, int reference, float* out, void* stream);
/* l2a_cem_pick_act: l2a_cem_pick - the same launch, the same `out` bit for bit - that also writes the winners' first actions as a
 * dense `act_out` [m, act_dim] (device fp32): act_out[i] holds the bits of out[i * (act_dim + 2) ..], the unclipped first action of
 * row i * n + j (reference = 1) or the clipped one of row j * m + i (0), j = 0 when every return of env i is NaN or -inf.  It is what
 * l2a_lstm_advance reads behind a recurrent CEM plan: pick, advance, one read-back - no gather launch, no host wait in between.     */
int l2a_cem_pick_act(l2a_ctx* ctx, const float* returns, const float* cand, const float* mean, const float* std, int n, int m,
                     int D, int act_dim, int reference, float* out, float* act_out, void* stream);
/* l2a_cem_refit_sample: l2a_cem_refit followed by l2a_cem_sample in ONE launch - iteration i's `returns` [m, n] and samples
 * `a_clip_in` [n, m, D] in, iteration i + 1's samples out - bit-identical to the two calls (mean, std, elite_rows, a_clip, a_raw,
 * seq; injected z or Philox z under (seed, offset); both readings).  mean_in [m, D]: the mean iteration i sampled with, read only;
 * NULL (or == mean) updates `mean` in place.  The launch is one workgroup per (horizon step, candidate slice, statistics group):
 * each ranks its group's returns itself, refits the act_dim dimensions of its step and samples them - no wait between
 * workgroups.  Several slices per step only when neither mean_in nor a_clip_in is also an output (pass distinct buffers, e.g.
 * ping-pong pairs, for the fast path); a_raw and seq must not alias a_clip_in.  Shapes beyond the launch's LDS budget (the
 * pooled elite rows' values or 2 n + 4096 words) run the two calls instead, inside this call; the same argument checks as they
 * have (n * 4 bytes within the LDS of a workgroup, at most 8192 elite rows per statistics group). */
int l2a_cem_refit_sample(l2a_ctx* ctx, const float* returns, const float* a_clip_in, int n, int m, int h, int act_dim,
                         int num_elites, int reference, float alpha, const float* z, unsigned long long seed,
                         unsigned long long offset, const float* low, const float* high, int lo, int hi, int* elite_rows,
                         const float* mean_in, float* mean, float* std, float* a_clip, float* a_raw, float* seq, void* stream);
/* 1 when l2a_cem_refit_sample runs this shape as its one launch, 0 when it runs the two calls instead (or the shape is invalid). */
int l2a_cem_refit_sample_fused(const l2a_ctx* ctx, int n, int m, int h, int act_dim, int num_elites, int reference);

/* ---- reward-weighted (MPPI) planner: the per-iteration work around the rollout, on the device ---------------------
 * PDDM's "filtered and reward-weighted refinement" (Nagabandi et al. 2019); the reference has no such planner, the
 * semantics are build-defined.  Per env i a persistent fp32 plan mean mu[i] of shape [h, A], A = act_dim, D = h * A, kept on
 * the device between controller steps.  One iteration = l2a_mppi_sample, the rollout (returns [m, n]), l2a_mppi_update.
 *
 * l2a_mppi_sample
 *   shift  [m] device int32: < 0 the mean starts from zeros (first step, or after a reset of env i); > 0 the plan moves on one
 *          step, mu'_t = mu_min(t + 1, h - 1); 0 the mean is kept (iterations after the first within one controller step)
 *   noise  z[j, i, t, k] is a standard normal for element e = (j * m + i) * D + t * A + k of the [n, m, D] draw: `z` (device
 *          fp32) or, z = NULL, l2a_cem_sample's Philox4x32-10 + Box-Muller stream at counter offset + e under `seed`.
 *          u = z * sigma[k]; n_t = beta * u_t + (1 - beta) * n_(t-1), n_(-1) = 0 - each operation rounded to fp32 on its own,
 *          1 - beta formed once in fp32
 *   out    a = clip(mu'[i, t, k] + n_t, low[k], high[k]) into a_clip [n, m, D] and, unless NULL, into seq [h, m * n, A], the
 *          candidate tensor l2a_plan_rs reads: plan row i * n + j is sample row j * m + i (l2a_cem_sample's reference = 0);
 *          mean_out [m, D] receives mu' (it must not be mean_in: L2A_EINVAL)
 *   sigma / low / high [act_dim] device fp32; sigma finite and >= 0 is the caller's business (the arrays live on the device).
 *   L2A_EINVAL (nothing written): act_dim outside 1..16, n / m / h < 1, beta outside (0, 1], aliasing means, a null pointer.
 *
 * l2a_mppi_update
 *   returns [m, n] device fp32, a_clip the samples they belong to, mean = the sample call's mean_out, updated in place.
 *   A candidate is valid when its return is neither NaN nor -inf; invalid candidates weigh 0 - a diverged rollout is not a
 *   plan to imitate (unlike the arg-max of l2a_cem_pick, where a NaN is the maximum).  Rmax = the largest valid return.
 *   Rmax = +inf: w = 1 for the +inf returns, else 0; otherwise w_j = expf(kappa * (R_j - Rmax)) with the difference and the
 *   product in fp32 (a difference that overflows to -inf gives 0).  mu[i, d] = sum_j w_j a[j, i, d] / sum_j w_j over the
 *   clipped samples; an env without a valid candidate keeps mu' untouched.  No atomics, one fixed summation order.
 *   out    [m][act_dim + 4] floats: new mu[i, 0, :] | Rmax (NaN without a valid candidate) | index of the first maximum as
 *          the bits of an int32 (-1) | effective sample size (sum w)^2 / sum w^2 (0) | number of valid candidates, int32 bits
 *   L2A_EINVAL (nothing written): act_dim outside 1..16, n / m / h < 1, m > 65535, kappa not positive and finite, or n * 4 bytes
 *   plus the kernel's own L2A_MPPI_UPDATE_STATIC_LDS bytes beyond a workgroup's LDS (l2a_device_info: lds_per_block).       */
#define L2A_MPPI_UPDATE_STATIC_LDS 4480
int l2a_mppi_sample(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                    const int* shift, const float* sigma, float beta, const float* low, const float* high,
                    int n, int m, int h, int act_dim, float* mean_out, float* a_clip, float* seq, void* stream);
int l2a_mppi_update(l2a_ctx* ctx, const float* returns, const float* a_clip, int n, int m, int h, int act_dim, float kappa,
                    float* mean, float* out, void* stream);
/* l2a_mppi_sample for ONE rank of a sharded plan (as l2a_cem_sample's lo / hi): the rank draws, filters and clips ALL n candidates
 * of the same stream - a_clip [n, m, D] and mean_out are l2a_mppi_sample's bit for bit, the update runs on them unchanged - and
 * keeps the rollout tensor of its window only: seq_local [h, m * (hi - lo), A], plan row i * (hi - lo) + (j - lo) for lo <= j < hi
 * (the values of l2a_mppi_sample's seq rows i * n + j).  lo == hi writes no seq_local (it may be NULL then).  L2A_EINVAL (nothing
 * written): l2a_mppi_sample's, lo < 0, hi > n, lo > hi, or a NULL seq_local with lo < hi.  The same kernel body, one more instance. */
int l2a_mppi_sample_shard(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                          const int* shift, const float* sigma, float beta, const float* low, const float* high,
                          int n, int m, int h, int act_dim, int lo, int hi, float* mean_out, float* a_clip, float* seq_local,
                          void* stream);

/* ---- improved cross-entropy-method (iCEM) planner: the per-iteration work around the rollout, on the device --------
 * iCEM (Pinneri et al. 2020): CEM with a plan that is shifted and reused at the next step, a fraction of the elites carried into
 * the next iteration and step, time-correlated noise, a shrinking population and the best candidate's action executed.  The
 * reference has no such planner, the semantics are build-defined.  A = act_dim, D = h * A.  Sample rows are candidate-major
 * ([n_it, m, D]: row j * m + i), plan rows env-major (i * n_it + j): l2a_cem_sample's reference = 0.  Per env i, on the device:
 * the plan mean mu[i] [h, A], the spread sd[i] [h, A], the kept elites kept[i] [Kk, D] and their count kc[i] <= Kk.  Sizes (the
 * caller's, computed on the host in double precision): K = max(int(n * percent_elites), 1) elites, Kk = int(icem_keep * K) kept
 * ones (0 is allowed), the population of iteration `it` n_it = min(n, max(int(n / icem_decay ** it), 2 K)).
 * One iteration = l2a_icem_sample, the rollout (returns [m, n_it]), l2a_icem_refit.
 *
 * l2a_icem_sample (one launch: l2a_icem_sample_k)
 *   shift  [m] device int32.  < 0 (a new or reset env): mu' = 0, sd' = sigma0[k], kc' = 0.  > 0 (first iteration of a later step):
 *          mu'_t = mu_min(t + 1, h - 1), sd' = sigma0[k] (the spread is re-opened), the kept rows are shifted the same way (the last
 *          step repeated), kc' = kc.  0 (later iterations): mu' = mu, sd' = sd, kept rows as they are, kc' = kc.  A stored count
 *          outside 0 .. Kk is held to that range.
 *   rows   row j < kc'_i is kept row j as stored (it was clipped when it was drawn).  With add_mean != 0 row n_it - 1 is
 *          clip(mu') - and it wins where both rules name the same row (n_it <= kc').  Every other row: z[j, i, t, k] is a standard
 *          normal for element e = (j * m + i) * D + t * A + k of the [n_it, m, D] draw - `z` (device fp32) or, z = NULL,
 *          l2a_cem_sample's Philox4x32-10 + Box-Muller stream at counter offset + e under `seed` (the numbering is positional: a
 *          kept row's normals are not used, the stream does not depend on kc) -, nz_0 = z_0, nz_t = rho * nz_(t-1) + c * z_t with
 *          c = sqrtf(1 - rho * rho) formed once in fp32 (unit variance for every t), a = clip(mu' + nz_t * sd', low[k], high[k]);
 *          each operation rounded to fp32 on its own.  rho = 0 is l2a_cem_sample's white noise.
 *   out    a_clip [n_it, m, D] and, unless NULL, seq [h, m * n_it, A], the candidate tensor l2a_plan_rs reads; mean_out and
 *          std_out [m, D] receive mu' and sd'.
 *   sigma0 / low / high [act_dim] device fp32; kept_in [m, Kk, D], kc_in [m] (both may be NULL when Kk == 0).
 *   L2A_EINVAL (nothing written, nothing launched): act_dim outside 1..16, n_it / m / h < 1, Kk outside 0..8192, rho outside [0, 1),
 *   a NULL pointer (z and seq may be NULL; kept_in / kc_in with Kk == 0), an output that is an input or another output.
 *
 * l2a_icem_refit (two launches: l2a_icem_rank_k over candidates, l2a_icem_stats_k over dimensions)
 *   returns [m, n_it] device fp32, a_clip the samples they belong to, mean / std = the sample call's mean_out / std_out, updated
 *   in place.  A candidate is valid when its return is neither NaN nor -inf (l2a_mppi_update's rule: a diverged rollout is never
 *   an elite).  The elites are the top Ke = min(K, valid) valid candidates in the stable descending order (ties: the lower index
 *   first).  Per dimension em and the biased es of the elite rows of a_clip in one fixed summation order (csrc/l2a_icem.hip), then
 *   mu = alpha * mu' + (1 - alpha) * em, sd = alpha * sd' + (1 - alpha) * es; Ke = 0 leaves both untouched.  No atomics: the same
 *   inputs give the same bits on every run.
 *   work      device int32 [m, K], scratch (the elites' candidate indices in rank order; entries >= Ke are not written)
 *   kept_out  [m, Kk, D]: the first min(Kk, Ke) elite rows in rank order (NULL allowed when Kk == 0); kc_out [m]: that number
 *   out       [m][act_dim + 4] floats: the first action of the best valid candidate (the first maximum) | its return | its index as
 *             the bits of an int32 | Ke, int32 bits | the valid count, int32 bits.  Without a valid candidate: mu'[i, 0, :] clipped
 *             to low / high | NaN | -1 | 0 | 0.
 *   L2A_EINVAL (nothing written, nothing launched): act_dim outside 1..16, n_it / m / h < 1, m > 65535, K outside 1..8192, Kk outside
 *   0..K, alpha outside [0, 1), a NULL pointer, an output that is an input or another output, or LDS: n_it * 4 bytes (the ranking's
 *   returns) or K * 4 + L2A_ICEM_REFIT_STATIC_LDS bytes (the statistics' elite list and its static part) beyond a workgroup's
 *   LDS (l2a_device_info: lds_per_block).
 * The controller step as one call, unsharded and sharded over ranks: l2a_icem_controller_create_device below.
 * Noise with a power-law spectrum (the paper's coloured noise, PSD ~ f^-beta): l2a_icem_noise_matrix / l2a_icem_sample_noise below.
 * Not built: a recurrent model, reward programs and reward models through the C step, NumPy normals, power-law noise on horizons
 * above L2A_ICEM_NOISE_MAX_H, a beta per action dimension.                                                                        */
#define L2A_ICEM_REFIT_STATIC_LDS 4288
int l2a_icem_sample(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                    const float* std_in, const float* kept_in, const int* kc_in, const int* shift, const float* sigma0, float rho,
                    const float* low, const float* high, int n_it, int m, int h, int act_dim, int Kk, int add_mean,
                    float* mean_out, float* std_out, float* a_clip, float* seq, void* stream);
int l2a_icem_refit(l2a_ctx* ctx, const float* returns, const float* a_clip, const float* low, const float* high, int n_it, int m,
                   int h, int act_dim, int K, int Kk, float alpha, int* work, float* mean, float* std, float* kept_out,
                   int* kc_out, float* out, void* stream);
/* l2a_icem_sample for ONE rank of a sharded plan (as l2a_mppi_sample_shard): the rank fetches, draws, runs the recurrence and clips
 * ALL n_it rows of the same stream - a_clip [n_it, m, D], mean_out and std_out are l2a_icem_sample's bit for bit, the refit runs on
 * them unchanged - and keeps the rollout tensor of its window only: seq_local [h, m * (hi - lo), A], plan row i * (hi - lo) + (j - lo)
 * for lo <= j < hi (the values of l2a_icem_sample's seq rows i * n_it + j).  A kept row (j < kc') or the mean row (j == n_it - 1 with
 * add_mean) inside the window is written like any other row.  lo == hi writes no seq_local (it may be NULL then).  L2A_EINVAL
 * (nothing written, nothing launched): l2a_icem_sample's, lo < 0, hi > n_it, lo > hi, or a NULL seq_local with lo < hi.  The same
 * kernel body, one more instance.                                                                                                  */
int l2a_icem_sample_shard(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                          const float* std_in, const float* kept_in, const int* kc_in, const int* shift, const float* sigma0,
                          float rho, const float* low, const float* high, int n_it, int m, int h, int act_dim, int Kk, int add_mean,
                          int lo, int hi, float* mean_out, float* std_out, float* a_clip, float* seq_local, void* stream);

/* ---- iCEM: the noise as a matrix, and the power-law matrix ---------------------------------------------------------
 * The noise sequence of one (candidate, action dimension) is nz = M z: z the h standard normals l2a_icem_sample draws for it (the
 * Philox numbering stays positional: element e = (j * m + i) * D + t * A + k), M [h, h] row-major fp32.  One fixed order, every
 * operation rounded to fp32 on its own:
 *     acc = M[t, 0] * z_0;  for s = 1 .. h - 1: acc = acc + (M[t, s] * z_s);  nz_t = acc;  a = clip(mu'_t + nz_t * sd'_t, low, high)
 * The bits of an element depend on its row of M and its normals alone - not on the launch geometry, the rows per workgroup or a
 * shard's window.  Shift, the re-opened spread, kept rows, the mean row and its precedence, mean_out / std_out and the layouts of
 * a_clip and seq are l2a_icem_sample's; a kept row's and the mean row's normals are not used.  M = I is l2a_icem_sample at rho = 0
 * (as values: the sum adds signed zeros).
 *
 * l2a_icem_noise_matrix (host only, no context, no GPU): the power-law matrix for PSD ~ f^-beta, built in double precision and
 * rounded once to fp32.  s_k = max(k, 1)^(-beta / 2) * h^(beta / 2) for k = 0 .. floor(h / 2) (the DC term gets the lowest
 * frequency's amplitude), "mid" = 1 <= k <= floor((h - 1) / 2), N = sqrt(s_0^2 + 2 sum_mid s_k^2 + [h even, h > 1] s_(h/2)^2);
 *     M[t, 0] = s_0 / N;  M[t, 2k - 1] = sqrt(2) s_k cos(2 pi k t / h) / N,  M[t, 2k] = -sqrt(2) s_k sin(2 pi k t / h) / N  (mid k);
 *     even h > 1: M[t, h - 1] = s_(h/2) (-1)^t / N.
 *   Every row has norm 1 (unit variance for every t, as the AR(1) noise), M M^T is circulant (a stationary process), beta = 0 gives
 *   an orthogonal M (white noise), h = 2 is white for every beta.  L2A_EINVAL, nothing written: h outside 1 .. L2A_ICEM_NOISE_MAX_H,
 *   beta not finite or outside [0, 8], a NULL pointer.
 * l2a_icem_sample_noise / l2a_icem_sample_noise_shard (one launch: l2a_icem_sample_noise_k, the whole horizon of a row in LDS, M
 *   read from global memory): l2a_icem_sample's / l2a_icem_sample_shard's arguments with `float rho` replaced by `noise`, device
 *   fp32 [h, h] - ANY matrix, not only the power-law one.  L2A_EINVAL (nothing written, nothing launched): every refusal of
 *   l2a_icem_sample / l2a_icem_sample_shard except rho's, h > L2A_ICEM_NOISE_MAX_H, a NULL noise, noise being one of the outputs.
 * l2a_icem_controller_set_noise: further down, with the iCEM controller step.                                                        */
#define L2A_ICEM_NOISE_MAX_H 128
int l2a_icem_noise_matrix(int h, double beta, float* M_host);
int l2a_icem_sample_noise(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset, const float* mean_in,
                          const float* std_in, const float* kept_in, const int* kc_in, const int* shift, const float* sigma0,
                          const float* noise, const float* low, const float* high, int n_it, int m, int h, int act_dim, int Kk,
                          int add_mean, float* mean_out, float* std_out, float* a_clip, float* seq, void* stream);
int l2a_icem_sample_noise_shard(l2a_ctx* ctx, const float* z, unsigned long long seed, unsigned long long offset,
                                const float* mean_in, const float* std_in, const float* kept_in, const int* kc_in, const int* shift,
                                const float* sigma0, const float* noise, const float* low, const float* high, int n_it, int m, int h,
                                int act_dim, int Kk, int add_mean, int lo, int hi, float* mean_out, float* std_out, float* a_clip,
                                float* seq_local, void* stream);

/* ---- sharded plans: the one collective ------------------------------------------------------
 * Candidates are independent, so G GPUs (one process and one context each) plan disjoint shards of one candidate
 * tensor (l2a_plan_rs with cand_offset = first global index of the shard) and combine the per-shard keys with ONE
 * in-place MAX all-reduce of m u64 words over RCCL / xGMI - the reference has no collective (single process);
 * the semantics preserved are np.argmax's "first maximum" over the whole candidate set
 * (policies/mpc_controller.py:128-129), which the key packing encodes (see l2a_key_encode).
 *   l2a_comm_unique_id : rank 0 fills a 128-byte id (ncclGetUniqueId) and hands it to the other ranks by any means
 *                        (file, pipe, MPI, torch.distributed store)
 *   l2a_comm_init      : every rank, same id; binds the communicator to the context's device (ncclCommInitRank)
 *   l2a_allreduce_best : best_key device u64 [m], in place, enqueued on `stream` after the plan
 * RCCL is loaded at run time on the first of these calls; without it they fail with L2A_ENODEV and single-GPU
 * planning is unaffected.  (The Python drop-in uses torch.distributed - the same RCCL - for this step.)          */
int l2a_comm_unique_id(char id_out[128]);
int l2a_comm_init(l2a_ctx* ctx, int rank, int world, const char id[128]);
int l2a_comm_destroy(l2a_ctx* ctx);
int l2a_allreduce_best(l2a_ctx* ctx, unsigned long long* best_key, int m, void* stream);
/* What the ranks of a sharded plan all-reduce, packed on the device behind the plan launch (no host synchronisation
 * between the launch and the collective): payload [m + 3] u64 =
 *   [0, m)   the shard's arg-max keys (copied from best_key)
 *   [m]      1 when this context's launch status word is set (a tile-split exchange timed out: the keys are invalid)
 *   [m + 1]  digest & L2A_DIGEST_MASK, [m + 2]  L2A_DIGEST_MASK - (digest & L2A_DIGEST_MASK)
 * After an in-place MAX all-reduce of the m + 3 words (l2a_allreduce_best with m + 3, or torch.distributed) every rank
 * holds the global keys, knows whether ANY rank has to repeat its launch unsplit ([m] != 0: all ranks do, together),
 * and whether every rank planned on the same candidate tensor ([m + 1] + [m + 2] == L2A_DIGEST_MASK iff all digests
 * were equal; the digest is the caller's fingerprint of its RNG position).  One device-to-host copy of m + 3 words
 * ends the step.  Every word is below 2^63, so signed 64-bit MAX (torch.int64) reduces them correctly.            */
#define L2A_DIGEST_MASK 0x7fffffffffffull
int l2a_plan_payload(l2a_ctx* ctx, const unsigned long long* best_key, int m, unsigned long long digest,
                     unsigned long long* payload, void* stream);
/* Sharded CEM: the ranks' returns of one iteration travel through the SAME collective - no second collective kind, no second
 * callback type.  A rank contributes m * n + 3 u64 words per iteration:
 *   [i * n + j]  (1ull << 32) | the RAW bits of its fp32 return of env i's global candidate j when lo <= j < hi, else 0.  Only the
 *                owner contributes a non-zero word, so MAX returns it exactly: NaN payloads, -0.0 and +-inf survive bit for bit
 *   [m * n]      1 when this context's launch status word is set (read on the device, as l2a_plan_payload does)
 *   [m * n + 1]  digest & L2A_DIGEST_MASK, [m * n + 2]  L2A_DIGEST_MASK - (digest & L2A_DIGEST_MASK)
 * Every word is below 2^33: signed 64-bit MAX (torch.int64) reduces them correctly.  After the in-place MAX all-reduce every
 * rank holds every candidate's return, the any-rank flag and the digest check.
 *   l2a_cem_shard_pack   : ONE launch writes ALL m * n + 3 words (zeros outside the shard - no memset in front); returns_local
 *                          [m, hi - lo] (may be NULL when hi == lo: more ranks than candidates - zeros and the three tail words)
 *   l2a_cem_shard_unpack : ONE launch decodes the reduced words into the fp32 table returns_out [m, n] that l2a_cem_refit_sample
 *                          and l2a_cem_pick read, and ACCUMULATES into verdict (device u32 [3], NOT reset by the call - the caller
 *                          zeroes it once per plan step): [0] |= the flag word, [1] += the number of zero words ("holes": a
 *                          candidate nobody contributed, decoded as 0.0f), [2] |= 1 when words[m * n + 1] + words[m * n + 2] !=
 *                          L2A_DIGEST_MASK
 *   l2a_cem_word_encode / _decode : the word of a return on the host; _decode returns 0 for an absent (zero) word, else 1.   */
int l2a_cem_shard_pack(l2a_ctx* ctx, const float* returns_local, int m, int n, int lo, int hi, unsigned long long digest,
                       unsigned long long* words_out, void* stream);
int l2a_cem_shard_unpack(l2a_ctx* ctx, const unsigned long long* words, int m, int n, float* returns_out,
                         unsigned int* verdict, void* stream);
unsigned long long l2a_cem_word_encode(float ret);
int l2a_cem_word_decode(unsigned long long word, float* ret);

/* ---- recurrent planner (ReBAL) --------------------------------------------------------------
 * Single-layer LSTM dynamics model: `RNNDynamicsModel` (dynamics/rnn_dynamics.py:11-100) built by
 * `create_rnn` (dynamics/core/utils.py:192-236) with cell_type='lstm' - the configuration of
 * run_scripts/run_rebal.py:98-99.  `cell_act` is the cell's `activation` (hidden_nonlinearity,
 * default tanh, rnn_dynamics.py:20), `output_act` the output layer's nonlinearity.
 * Fused MFMA kernel for units in {128, 256, 512}, obs_dim <= 64, act_dim <= 16; generic VALU
 * kernel otherwise (l2a_set_kernel applies).                                                    */
int l2a_lstm_create(l2a_ctx* ctx, int obs_dim, int act_dim, int units, int cell_act, int output_act,
                    l2a_lstm** out);
void l2a_lstm_destroy(l2a_lstm* model);

/* The other recurrent models `create_rnn` (dynamics/core/utils.py:192-236) can build: `cell_type` 'lstm' / 'gru' /
 * 'rnn' and several stacked layers (`len(hidden_sizes) > 1` -> tf.nn.rnn_cell.MultiRNNCell).  One LSTM layer is
 * the model of l2a_lstm_create (its own MFMA kernel); everything else runs on the generic matrix-core kernel of
 * l2a_rnn_mfma.h (l2a_set_kernel VALU: the fp32 VALU kernel of l2a_rnn_valu.h; the layers' units may sum to about 800 -
 * one candidate tile's states live in a CU's LDS).  Cell arithmetic: tensorflow==1.13.1 LSTMCell / GRUCell; 'rnn' = BasicRNNCell
 * (h = act([x | h] K + b)) - the reference passes the abstract `tf.nn.rnn_cell.RNNCell` there (:209), which cannot
 * be instantiated, so this is the evident intent, not a measured behaviour.
 * Parameters (l2a_lstm_set_weights), in `get_params()` order, kernels row-major [in_l + U_l, .] with the layer's
 * input first (in_0 = obs_dim + act_dim, in_l = U_(l-1)):
 *   lstm layer: kernel [., 4 U] (gates i j f o), bias [4 U]
 *   gru layer:  gates/kernel [., 2 U] (r | u), gates/bias [2 U], candidate/kernel [., U], candidate/bias [U]
 *   rnn layer:  kernel [., U], bias [U]
 * then output/kernel [U_top, obs_dim], output/bias [obs_dim].
 * State: wherever the l2a_lstm_* entry points take c / h [rows, units], a stack takes the layers' states
 * concatenated, [rows, sum(U_l)]; c is read and written for LSTM stacks only (pass any valid buffer otherwise). */
#define L2A_CELL_LSTM 0
#define L2A_CELL_GRU 1
#define L2A_CELL_RNN 2
int l2a_rnn_create(l2a_ctx* ctx, int obs_dim, int act_dim, int n_layers, const int* units, int cell_type,
                   int cell_act, int output_act, l2a_lstm** out);

/* Upload the four trainable variables in the reference's order (rnn.get_params(),
 * dynamics/core/layers.py:219-221): rnn/lstm_cell/kernel [obs_dim + act_dim + units, 4 * units]
 * (TF gate order i, j, f, o), rnn/lstm_cell/bias [4 * units], output/kernel [units, obs_dim],
 * output/bias [obs_dim]; fp32 device pointers, row-major.  Replaces `Layer.set_params`
 * (core/layers.py:81-94).                                                                        */
int l2a_lstm_set_weights(l2a_lstm* model, const void* const* device_ptrs, void* stream);

/* `self.normalization` of RNNDynamicsModel (rnn_dynamics.py:295-307; host float64 vectors, eps 1e-10
 * applied inside as in :329-334); all NULL = identity.                                           */
int l2a_lstm_set_norm(l2a_lstm* model, const double* mean_obs, const double* std_obs,
                      const double* mean_act, const double* std_act, const double* mean_delta,
                      const double* std_delta, void* stream);

/* One recurrent plan step = the loop of RNNMPCController.get_rs_action
 * (policies/rnn_mpc_controller.py:112-134; also the rollout of one CEM iteration, :92-104):
 * `repeat_hidden` (:165-187) of the per-env LSTM state (c0, h0: device fp32 [m, units]) to the n
 * candidates of each env, h x `dynamics_model.predict(obs, a[t], hidden)` + `env.reward` + return
 * accumulation + arg-max.  Other arguments as l2a_plan_rs.                                       */
int l2a_lstm_plan_rs(l2a_lstm* model, const float* obs0, const float* c0, const float* h0,
                     const float* actions, int m, int n, int h, double discount, const l2a_reward* reward,
                     int cand_offset, float* returns_out, unsigned long long* best_key, void* stream);

/* Blocking form of l2a_lstm_plan_rs for one GPU (see l2a_plan_rs_sync): `obs_host` [m, obs_dim] is a HOST array,
 * the arg-max keys arrive in `keys_host_out` [m] through the host-mapped mailbox (MFMA kernel; the generic kernels copy
 * and synchronise).  With c_next / h_next (device, [m, state width], not aliasing c0 / h0) the controller's own state
 * is moved on as well: state' = cell(obs, first action of the winning candidate, state) - what
 * `RNNMPCController.get_actions` does after planning (rnn_mpc_controller.py:57-65) - enqueued behind the plan without a
 * host round trip (the action is gathered from `actions` on the device; its fp32 value is the one a host would pass).
 * Returns L2A_ESPLIT like l2a_plan_rs_sync; c_next / h_next are then invalid too and the repeated call rewrites them. */
int l2a_lstm_plan_rs_sync(l2a_lstm* model, const float* obs_host, const float* c0, const float* h0,
                          const float* actions, int m, int n, int h, double discount, const l2a_reward* reward,
                          int cand_offset, unsigned long long* keys_host_out, float* c_next, float* h_next,
                          void* stream);

/* l2a_lstm_plan_rs cut along the horizon (see l2a_plan_rs_chunk): launch k covers steps t0 .. t0 + h_chunk - 1
 * and hands per-candidate observation, LSTM state and accumulated returns to launch k + 1; the chain is
 * bit-identical to one launch.  t0 == 0: state [m, obs_dim], c / h [m, units] (per_row = 0); t0 > 0: the
 * state_out / c_out / h_out of the previous chunk, [m * n, ...] (per_row = 1).  state_out, c_out, h_out: all
 * three or none (last chunk); best_key on the last chunk.                                               */
int l2a_lstm_plan_rs_chunk(l2a_lstm* model, const float* state, const float* c, const float* h, int per_row,
                           const float* actions, int m, int n, int h_chunk, int t0, double discount,
                           const l2a_reward* reward, int cand_offset, const float* returns_in, float* returns_out,
                           float* state_out, float* c_out, float* h_out, unsigned long long* best_key, void* stream);

/* RNNDynamicsModel.predict (rnn_dynamics.py:233-252): one step for `rows` independent rows, each
 * with its own LSTM state.  obs [rows, obs_dim], act [rows, act_dim], c / h [rows, units] ->
 * next_obs_out [rows, obs_dim], c_out / h_out [rows, units] (all device fp32).  Used by
 * RNNMPCController.get_actions (:63) to advance the controller's hidden state with the chosen action. */
int l2a_lstm_predict(l2a_lstm* model, const float* obs, const float* act, const float* c, const float* h,
                     int rows, float* next_obs_out, float* c_out, float* h_out, void* stream);

/* The controller's OWN state step - `_, self._hidden_state = self.dynamics_model.predict(observations, actions,
 * self._hidden_state)` (rnn_mpc_controller.py:63), whose predicted observation the caller discards: c_out / h_out [rows, state
 * width] from obs [rows, obs_dim], act [rows, act_dim] (the chosen actions), c / h (all device fp32; the outputs must not alias
 * the inputs).  For one LSTM layer a dedicated small-rows kernel (the gate matrix cut over units / 16 workgroups, no output
 * layer) - the launch l2a_lstm_plan_rs_sync enqueues behind its plan; other cells take one step of their rollout kernel
 * (rows <= 64).  Agrees with l2a_lstm_predict's states to fp32 rounding (another summation order), not bit for bit.           */
int l2a_lstm_advance(l2a_lstm* model, const float* obs, const float* act, const float* c, const float* h, int rows,
                     float* c_out, float* h_out, void* stream);

/* 1 when (obs_dim, act_dim, units) is eligible for the MFMA LSTM kernel, else 0.                 */
int l2a_lstm_mfma_eligible(int obs_dim, int act_dim, int units);

/* ---- recurrent plans with a reward program or a learned reward model ---------------------------
 * The recurrent counterpart of l2a_plan_rs_program / l2a_plan_rs_reward_model: the model's predicted trajectory goes
 * to HBM and the scorers of csrc/l2a_score.hip / l2a_score_mlp.hip - unchanged - run behind it.  All stream-ordered; no
 * host synchronisation unless a buffer of the model's own grows.
 *
 * l2a_lstm_rollout_traj: the model's rollout alone.  obs0 [m, obs_dim], c0 / h0 [m, state width] (one row per env, as
 * l2a_lstm_plan_rs), actions [h, m*n, act_dim] -> traj_out device fp32 [h, m*n, obs_dim], traj_out[t] = the predicted
 * observation after horizon step t.  No rewards.  Two paths, the same bits on both:
 *   single launch  one LSTM layer of 256 / 512 units, for the plans l2a_lstm_plan_rs rolls on micro tiles (at most three
 *                  micro tiles per CU, and wanted under l2a_set_micro: 0 never, 2 whenever eligible): the trajectory-writing
 *                  instance of the micro-tile kernel, c / h never leave the CU.
 *   carry chain    everything else (128 units, GRU / BasicRNN / stacks, the VALU kernels, larger plans): h one-step
 *                  l2a_lstm_plan_rs_chunk launches with an all-zero reward, state_out = traj_out[t]; c / h ping-pong between
 *                  two buffer pairs of the model's own ([m*n, state width] each, grown on demand, which synchronises `stream`).
 * cand_offset is validated as everywhere and changes nothing in the trajectory.  The launch status word keeps its meaning: a
 * flagged unit-tile-split launch anywhere in the chain flags the call (l2a_launch_status).
 *
 * l2a_lstm_plan_rs_program: the rollout above, then l2a_score_trajectory.  l2a_lstm_plan_rs_reward_model: the rollout, then
 * l2a_score_trajectory_model; `rm` and `model` must live on the same context and agree on obs_dim / act_dim (L2A_EINVAL).
 * returns_out [m, n] or NULL, best_key [m] or NULL (not both), keys as l2a_lstm_plan_rs packs them.  traj_out: device fp32
 * [h, m*n, obs_dim], or NULL: the model keeps a buffer of its own (grown on demand; freed with the model).
 *
 * l2a_lstm_traj_geometry: host only, needs no GPU - which path l2a_lstm_rollout_traj takes for one LSTM layer of `units`
 * under micro policy `micro_policy` (0 | 1 | 2) on `num_cu` CUs (<= 0: 256) with the automatic kernel choice; the decision
 * function is the launcher's own.  out[8]: { 0 single launch (1) or chain (0), 1 launches of the rollout, 2 workgroups of a
 * launch, 3 workgroups per env (single launch), 4 micro tiles of the largest workgroup (99: no workgroup geometry),
 * 5 workgroups of that size per env, 6 .. 7 zero }.                                                                   */
int l2a_lstm_rollout_traj(l2a_lstm* model, const float* obs0, const float* c0, const float* h0, const float* actions,
                          int m, int n, int h, int cand_offset, float* traj_out, void* stream);
int l2a_lstm_plan_rs_program(l2a_lstm* model, const float* obs0, const float* c0, const float* h0, const float* actions,
                             int m, int n, int h, double discount, const l2a_reward_program* program, int cand_offset,
                             float* returns_out, unsigned long long* best_key, float* traj_out, void* stream);
int l2a_lstm_plan_rs_reward_model(l2a_lstm* model, l2a_reward_model* rm, const float* obs0, const float* c0, const float* h0,
                                  const float* actions, int m, int n, int h, double discount, int cand_offset,
                                  float* returns_out, unsigned long long* best_key, float* traj_out, void* stream);
int l2a_lstm_traj_geometry(int obs_dim, int act_dim, int units, int m, int n, int h, int micro_policy, int num_cu, int* out);

/* ---- the controller step as one call ----------------------------------------------------------
 * `MPCController.get_actions(observations)` in random-shooting mode (policies/mpc_controller.py:59-69,108-129) and
 * `RNNMPCController.get_actions` (policies/rnn_mpc_controller.py:57-65,112-134), as their caller sees them: float64
 * observations in, the float64 first action of every env's best candidate out, NumPy's legacy global generator left
 * exactly where the reference's `np.random.uniform(low, high, (h*n*m, act_dim))` (:67-69,114) leaves it.  One GPU.
 *
 * A controller owns two page-locked / HBM buffer pairs for the candidate tensor [h, m*n, act_dim] and a producer
 * thread (csrc/l2a_rng.c, `l2a_ahead_*`) that draws the NEXT step's candidates from a private copy of the generator
 * state and uploads them while the GPU runs the current plan.
 *   np_state_addr  address of the global generator's `mt19937_state` { uint32 key[624]; int pos; } - in Python
 *                  `np.random.mtrand._rand._bit_generator.ctypes.state_address` (who may touch it when: the threading
 *                  contract at l2a_controller_begin below)
 *   low / high     the action bounds (`env.action_space.low / high`, float64 [act_dim], act_dim <= 16)
 *   rng_threads    threads of one draw (the stream is cut into disjoint slices, same numbers for every count)
 * l2a_controller_step:
 *   obs          HOST float64 [m, obs_dim]        (cast to fp32 like the host would, staged in host-mapped memory)
 *   action_out   HOST float64 [m, act_dim]        cand_a[i, argmax_i] (:118,129) - the float64 values NumPy drew
 *   index_out    HOST int64 [m] or NULL           the winning candidate of each env
 *   return_out   HOST fp32 [m] or NULL            its (fp32) return
 *   returns      L2A_OK; L2A_STEP_DREW (= OK: no valid block was waiting - first call, somebody else drew from np.random
 *                since the last step - so the step drew the candidates itself, the reference's own draw from the global
 *                generator on the helper's threads, and re-armed the chain behind it); L2A_STEP_UNSPLIT (= OK, but a
 *                tile-split launch lost its partner and the plan was repeated unsplit - same bits - with the context
 *                switched to l2a_set_split(ctx, 0)); L2A_STEP_MISS when this controller cannot serve the call (a forked
 *                child): NOTHING was consumed or launched, the caller plans the ordinary way (l2a_plan_rs_sync) and may
 *                call l2a_controller_rearm afterwards; a negative L2A_E* on failure.
 * l2a_lstm_controller_step additionally takes the controller's recurrent state c0 / h0 (device fp32 [m, state width])
 * and, with c_next / h_next, advances it with the winning first actions behind the plan (l2a_lstm_plan_rs_sync).
 * l2a_controller_rearm: restart the chain at the CURRENT global generator state (after a synchronous draw).
 * l2a_controller_actions: the device tensor [h, m*n, act_dim] the latest successful step planned on (diagnostics).
 * l2a_controller_stats: out[0..6] host microseconds of the latest step - take | stage obs | launch | kick | wait |
 * decode + gather | whole call; [7] steps, [8] unsplit relaunches; [9..14] chain: hits, misses, blocks produced,
 * producer us per block, consumer wait us per take, armed; [15] steps that drew synchronously.                  */
#define L2A_STEP_MISS 1
#define L2A_STEP_UNSPLIT 2
#define L2A_STEP_DREW 3
int l2a_controller_create(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                          const l2a_reward* reward, void* np_state_addr, int rng_threads, l2a_controller** out);
int l2a_lstm_controller_create(l2a_lstm* model, int m, int n, int h, const double* low, const double* high,
                               double discount, const l2a_reward* reward, void* np_state_addr, int rng_threads,
                               l2a_controller** out);
/* The SHARDED step (`MPCController._shard_range / _combine_keys`): rank r of `world` rolls out candidates
 * [r n / world, (r + 1) n / world) of every env - every rank consumes the generator for ALL h*n*m rows, so the shards are
 * slices of the one candidate tensor the reference draws (policies/mpc_controller.py:114) - and the step's ONE collective, an
 * int64 MAX all-reduce of [keys (m) | launch flag | digest | L2A_DIGEST_MASK - digest] packed on the device behind the
 * launch (l2a_plan_payload), runs in stream order; one page-locked copy of m + 3 words brings the result back.  MAX on the
 * packed keys = max return, ties -> lowest GLOBAL index = np.argmax over all candidates (:128-129); a set flag makes every
 * rank repeat launch + collective unsplit together (L2A_STEP_UNSPLIT); digests that differ (ranks seeded differently, a
 * foreign consumer of the generator on one rank) fail the step on every rank (L2A_ESTATE).
 *   reduce       NULL: RCCL over xGMI through the context's communicator (l2a_comm_init; this is l2a_allreduce_best on
 *                m + 3 words).  Otherwise the caller's collective: all-reduce `words` uint64 at `payload_dev` in place with
 *                MAX, ordered on `stream`; return 0 on success (torch.distributed behind a ctypes callback; tests).
 * Steps through l2a_controller_step / _begin / _finish like an unsharded controller; action_out = the float64 first action
 * of the GLOBAL winner (every rank holds every candidate's float64 first step).  MLP models.                          */
typedef int (*l2a_reduce_fn)(void* arg, unsigned long long* payload_dev, int words, void* stream);
int l2a_controller_create_sharded(l2a_model* model, int m, int n, int h, const double* low, const double* high,
                                  double discount, const l2a_reward* reward, void* np_state_addr, int rng_threads, int rank,
                                  int world, l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out);
/* The sharded step with the candidates drawn ON THE DEVICE (`MPCController(rng="device")` at N > 1): every rank fills its slice of
 * the SAME counter-based Philox stream (an element's value is that of its position in the whole plan's tensor [h, m*n, act_dim]),
 * so the candidates - and the chosen action - do not depend on the number of ranks, and every rank recomputes the winner's first
 * action from the stream on the host: one collective per step, no gather.  Ranks must be built with the same seed at the same
 * step (the digest pair of the collective carries seed and step count: L2A_ESTATE otherwise).                              */
int l2a_controller_create_sharded_device(l2a_model* model, int m, int n, int h, const double* low, const double* high,
                                         double discount, const l2a_reward* reward, unsigned long long seed, int rank, int world,
                                         l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out);
/* The sharded step of the RECURRENT planner (`RNNMPCController` at N > 1; run_scripts/run_rebal.py's plan over several GPUs): shard,
 * collective and failure protocol are those of l2a_controller_create_sharded / _sharded_device above, unchanged - rank r rolls out
 * candidates [r n / world, (r + 1) n / world) of every env with l2a_lstm_plan_rs (cand_offset = lo); parity mode: every rank consumes
 * the generator for ALL h*n*m rows; device mode: every rank fills its slice of the SAME Philox stream, so the plan does not depend on
 * the number of ranks; ONE MAX all-reduce of the m + 3 words of l2a_plan_payload per launch, one page-locked read-back; a digest
 * mismatch fails the step with L2A_ESTATE on every rank, a reduced flag makes every rank repeat the step unsplit once
 * (L2A_STEP_UNSPLIT; flagged again: L2A_ESPLIT); a rank with an empty shard (world > n) contributes the neutral key and still joins.
 * Steps through l2a_lstm_controller_step / l2a_lstm_controller_begin / l2a_controller_finish / _stats / _destroy; action_out = the
 * float64 first action of the GLOBAL winner (parity: the value NumPy drew; device: the fp32 stream value as float64).
 * With c_next / h_next the controller's own state is advanced as well, in stream order BEHIND the collective:
 *   state' = cell(obs, fp32 first action of the GLOBAL winner of each env, state)
 * - the winner usually belongs to another rank, so the action is looked up through the REDUCED keys on the device, without a host
 * round trip and without a second collective: parity mode in an fp32 table of the whole plan's first horizon step [m * n, act_dim]
 * (the cast the candidate tensor gets, uploaded with every block), device mode in the stream itself (l2a_philox_uniform - the bits
 * the owning rank rolled out).  One LSTM layer: l2a_lstm_advance's kernel; other cells: a gather and one step of the rollout kernel
 * (never tile-split).  The index decoded from a key is clamped to [0, n): a flagged launch or a neutral key may hold anything, and
 * the state written from it is overwritten by the relaunch (launch, payload, collective, advance, read-back - in that order again)
 * or discarded with the failed step.  c_next / h_next are valid after L2A_OK / L2A_STEP_DREW / L2A_STEP_UNSPLIT and invalid after a
 * negative return; with the same inputs they equal the unsharded controller's (l2a_lstm_controller_create[_device]) bit for bit.
 * No mailbox; the in-flight exclusion rules of the CEM controllers below apply as for every RS / recurrent step.                   */
int l2a_lstm_controller_create_sharded(l2a_lstm* model, int m, int n, int h, const double* low, const double* high,
                                       double discount, const l2a_reward* reward, void* np_state_addr, int rng_threads, int rank,
                                       int world, l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out);
int l2a_lstm_controller_create_sharded_device(l2a_lstm* model, int m, int n, int h, const double* low, const double* high,
                                              double discount, const l2a_reward* reward, unsigned long long seed, int rank, int world,
                                              l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out);
/* The same step with the candidates drawn ON THE DEVICE (`MPCController(rng="device")`: statistically equivalent to the reference's
 * draw, not its numbers; NumPy's generator is not touched): every step a Philox4x32-10 kernel fills the candidate tensor from the
 * counter-based stream (seed, steps so far) in front of the plan, and the winners' first actions are recomputed on the host from
 * the same stream (csrc/l2a_philox.h: identical integer rounds and fp32 map on both sides) - no upload, no gather, no copy back.
 * Steps through l2a_controller_step / l2a_lstm_controller_step as above (they never return L2A_STEP_DREW / _MISS here). */
int l2a_controller_create_device(l2a_model* model, int m, int n, int h, const double* low, const double* high, double discount,
                                 const l2a_reward* reward, unsigned long long seed, l2a_controller** out);
int l2a_lstm_controller_create_device(l2a_lstm* model, int m, int n, int h, const double* low, const double* high,
                                      double discount, const l2a_reward* reward, unsigned long long seed, l2a_controller** out);
/* ---- the CEM controller step as one call (device mode) -------------------------------------------------------------------
 * `MPCController.get_cem_action_device` (policies/mpc_controller.py; the reference's `get_cem_action`, :71-106, with the normals
 * drawn on the device): the whole plan step on the launch stream - l2a_cem_sample for iteration 0, then per iteration the fused
 * rollout and ONE l2a_cem_refit_sample (the last iteration: l2a_cem_refit), l2a_cem_pick, and ONE read-back of the packed result.
 * The normals of iteration `it` of the controller's s-th step are the Philox stream (seed) at offset (s * iters + it) * n * m * D,
 * D = h * act_dim - with the same seed a step equals get_cem_action_device bit for bit (action, index, return, final mean / std).
 *   iters       CEM iterations per step (`num_cem_iters`)
 *   num_elites  max(int(n * percent_elites), 1), computed by the caller as the reference does
 *   reference   1 = the reference's reading (unclipped rollouts, candidate-major rows, the pooled rank mask of :101); 0 = fixed
 * Steps through l2a_controller_step / _begin / _finish / _stats / _destroy (action_out = the first action of each env's best
 * candidate of the last iteration, as float64; L2A_STEP_UNSPLIT when a tile-split launch lost its partner and the step was repeated
 * unsplit with the same offsets - same bits).  MLP models (recurrent: l2a_lstm_cem_controller_create_device below); one GPU
 * (sharded: l2a_cem_controller_create_sharded_device below).
 * The launch status word is per context, and a CEM step reads
 * and clears it: a CEM step never shares the context with another controller's step in flight.  l2a_controller_begin of a CEM
 * controller returns L2A_ESTATE while any other controller on the context is between _begin and _finish, and that of an RS or
 * recurrent controller returns L2A_ESTATE while a CEM step is - nothing is launched or consumed then, and the step in flight
 * finishes with its solo result.
 * l2a_cem_controller_result: after a finished step, the final mean / std (host fp32 [m, D] each, or NULL) and every iteration's
 * returns of that step (host fp32 [iters, m, n], or NULL; one synchronous copy).                                                */
int l2a_cem_controller_create_device(l2a_model* model, int m, int n, int h, const double* low, const double* high,
                                     double discount, const l2a_reward* reward, int iters, int num_elites, float alpha,
                                     int reference, unsigned long long seed, l2a_controller** out);
/* The same step for ONE rank of a plan sharded over `world` GPUs (config 5: 8 x 500 of 4000 candidates): every rank samples ALL
 * n rows of the same Philox stream (the stream does not depend on `world`), rolls out candidates [lo, hi) = [rank n / world,
 * (rank + 1) n / world) and, per iteration, packs its returns (l2a_cem_shard_pack), runs the collective - `reduce`, or
 * l2a_allreduce_best on m * n + 3 words over the context's communicator when `reduce` is NULL - unpacks the gathered table
 * (l2a_cem_shard_unpack) and refits on it: `iters` collectives per step, all in stream order, no host wait between iterations,
 * ONE read-back of the packed result and the verdict.  The digest fingerprints seed, stream position, m, n, h, iters, num_elites,
 * reference, alpha and world.  _finish decides from the REDUCED verdict only (identical on every rank, so the ranks never disagree
 * on the number of collectives): a digest mismatch or a hole fails the step with L2A_ESTATE on every rank and the stream position
 * does not advance; a flag makes every rank switch to l2a_set_split(ctx, 0) and repeat the whole step once with the same offsets
 * (L2A_STEP_UNSPLIT, one relaunch; flagged again: L2A_ESPLIT).  With the same seed every rank's step equals the unsharded
 * controller's bit for bit, and l2a_cem_controller_result returns the GATHERED [iters, m, n] tables.  The in-flight exclusion
 * rules above apply unchanged.                                                                                                   */
int l2a_cem_controller_create_sharded_device(l2a_model* model, int m, int n, int h, const double* low, const double* high,
                                             double discount, const l2a_reward* reward, int iters, int num_elites, float alpha,
                                             int reference, unsigned long long seed, int rank, int world, l2a_reduce_fn reduce,
                                             void* reduce_arg, l2a_controller** out);
/* The CEM step of the RECURRENT planner (`RNNMPCController(use_cem=True, rng="device")`; run_scripts/run_rebal.py's plan with
 * use_cem): the sequence, the Philox offsets (s * iters + it) * n * m * D, the failure protocol and the argument limits (m <= 64,
 * act_dim <= 16, the LDS checks of refit and sample) are those of l2a_cem_controller_create_device / _sharded_device above, for any
 * model l2a_lstm_create or l2a_rnn_create builds (LSTM, GRU, BasicRNN, stacks).  Every iteration's rollout is l2a_lstm_plan_rs from
 * the caller's state c0 / h0 (device fp32 [m, state width]; cand_offset 0 over n, sharded: lo over this rank's hi - lo), the pick is
 * l2a_cem_pick_act, and with c_next / h_next the controller's own state is advanced behind it, in front of the read-back:
 *   state' = cell(obs, fp32 first action of each env's best candidate, state)               (l2a_lstm_advance)
 * Sharded, every rank holds every sample row and - after each iteration's collective - every return, so the pick and the advance
 * are local and identical on all ranks: no further collective, no key lookup; a rank with an empty shard (world > n) skips the
 * rollout and still packs, reduces, refits, picks and advances.
 * Steps through l2a_lstm_controller_step / l2a_lstm_controller_begin (c0, h0, c_next, h_next) / l2a_controller_finish / _stats /
 * _destroy and l2a_cem_controller_result.  l2a_controller_step / _begin on a recurrent CEM controller, and the l2a_lstm_* step
 * functions on an MLP CEM controller, return L2A_EINVAL: nothing is launched, nothing consumed.  c_next / h_next: both NULL = plan
 * only; one of them NULL, or an output aliasing c0 / h0, is L2A_EINVAL.  c0 / h0 are read by every iteration's rollout and by the
 * advance: they stay valid and unwritten until _finish.  A flagged step repeats the WHOLE sequence unsplit, the advance included -
 * from the same c0 / h0 with the same offsets, so c_next / h_next are simply rewritten; they are invalid after a negative return and
 * after L2A_OK / L2A_STEP_UNSPLIT equal what l2a_lstm_advance gives for the returned action, bit for bit.  With the same seed every
 * rank's step equals the unsharded controller's bit for bit, the state included - as long as every shard width selects the same
 * rollout kernel: ranks whose widths select a VALU kernel against a matrix-core kernel agree to fp32 tolerance only (l2a_set_micro).
 * The in-flight exclusion rules above apply unchanged; the digest also carries the controller kind.                               */
int l2a_lstm_cem_controller_create_device(l2a_lstm* model, int m, int n, int h, const double* low, const double* high,
                                          double discount, const l2a_reward* reward, int iters, int num_elites, float alpha,
                                          int reference, unsigned long long seed, l2a_controller** out);
int l2a_lstm_cem_controller_create_sharded_device(l2a_lstm* model, int m, int n, int h, const double* low, const double* high,
                                                  double discount, const l2a_reward* reward, int iters, int num_elites, float alpha,
                                                  int reference, unsigned long long seed, int rank, int world, l2a_reduce_fn reduce,
                                                  void* reduce_arg, l2a_controller** out);
int l2a_cem_controller_result(l2a_controller* controller, float* mean_out, float* std_out, float* returns_out);
/* ---- the MPPI controller step as one call (device mode) ------------------------------------------------------------------
 * `MPCController.get_mppi_action` (policies/mpc_controller.py; the planner of l2a_mppi_sample / l2a_mppi_update above): the whole
 * plan step on the launch stream - per iteration l2a_mppi_sample, the fused rollout, l2a_mppi_update - and ONE read-back of the
 * update's packed head, m * (act_dim + 4) floats.  The plan mean [m, D] lives in the controller (three device buffers rotate: the
 * committed mean is never written by the step that reads it) and stays on the device, as every iteration's returns do, until
 * l2a_mppi_controller_result asks.  Iteration 0 samples with the per-env shift vector - -1 for an env that is new or was reset
 * (l2a_mppi_controller_reset), +1 otherwise -, later iterations with shift 0.  The normals of iteration `it` are the Philox stream
 * (seed) at offset (iter_calls + it) * n * m * D, iter_calls = iterations finished so far since create / reseed: with the same seed
 * a step equals get_mppi_action bit for bit (action, index, Rmax, mean, ESS, valid count, returns).
 *   iters  refinements per step (`mppi_iters`);  kappa, beta, sigma [act_dim]: `mppi_kappa`, `mppi_beta`, the noise scale per action
 *          dimension (host float64, rounded to fp32 as `_mppi_sigma_vector` does)
 * Refused at create (L2A_EINVAL, nothing allocated): the argument limits of l2a_mppi_sample and l2a_mppi_update - the LDS check
 * n * 4 + L2A_MPPI_UPDATE_STATIC_LDS <= lds_per_block among them -, m > 64 or more than 4096 observation floats, a sigma that is
 * negative or not finite, beta outside (0, 1], kappa not positive and finite, iters < 1; sharded: l2a_cem_controller_create_sharded_device's
 * rank / world / collective rules.
 * Steps through l2a_controller_step / _begin / _finish / _stats / _destroy: action_out = the new mean's first step as float64,
 * index_out / return_out = the packed row's best valid index (-1 without a valid candidate) and Rmax (NaN then).  The l2a_lstm_*
 * step functions return L2A_EINVAL.  The step's mean, iter_calls and the cleared reset marks are committed in _finish behind the
 * verdict only: a launch flagged invalid (a tile-split partner was lost) repeats the WHOLE step unsplit from the same mean with the
 * same offsets (L2A_STEP_UNSPLIT, same bits; flagged again: L2A_ESPLIT), and a failed step leaves the controller where it was.
 * The in-flight exclusion rules of the CEM step apply (the step reads and clears the context's status word).
 * Sharded (one rank of `world`): l2a_mppi_sample_shard over the window [lo, hi) = [rank n / world, (rank + 1) n / world), the
 * rollout of that window, and per iteration the gather of the returns exactly as sharded CEM's - l2a_cem_shard_pack, the int64 MAX
 * all-reduce of m * n + 3 words (`reduce`, or the context's communicator), l2a_cem_shard_unpack - in front of the UNCHANGED update
 * over all n: every rank's step equals the unsharded one bit for bit.  The read-back gains the three verdict words.  The digest
 * carries the controller kind, seed, iter_calls, m, n, h, iters, world, the bits of kappa, beta and sigma, and the step's shift
 * vector (ranks that reset different envs would sample from different plans): a mismatch, or a hole, is L2A_ESTATE on every rank
 * and nothing is consumed; a flag on any rank makes all of them repeat the step unsplit, together.
 *   l2a_mppi_controller_reset  : dones [m] (non-zero: env i's next step starts from a zero mean), NULL = every env
 *   l2a_mppi_controller_reseed : the stream restarts at 0 under `seed`; the mean is kept (what get_mppi_action does when
 *                                torch.initial_seed() changes)
 *   l2a_mppi_controller_result : of the latest finished step - the mean (host fp32 [m, D]), ESS [m], valid counts [m], every
 *                                iteration's returns [iters, m, n] (sharded: the GATHERED tables); any pointer may be NULL; mean and
 *                                returns come back in ONE copy on the latest step's stream, waited for
 * _reset / _reseed / _result return L2A_ESTATE while a step is in flight, _result also before the first step has finished.
 * Not built: a recurrent model, reward programs and reward models (l2a_reward only), NumPy normals.                              */
int l2a_mppi_controller_create_device(l2a_model* model, int m, int n, int h, const double* low, const double* high,
                                      double discount, const l2a_reward* reward, int iters, float kappa, float beta,
                                      const double* sigma, unsigned long long seed, l2a_controller** out);
int l2a_mppi_controller_create_sharded_device(l2a_model* model, int m, int n, int h, const double* low, const double* high,
                                              double discount, const l2a_reward* reward, int iters, float kappa, float beta,
                                              const double* sigma, unsigned long long seed, int rank, int world,
                                              l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out);
int l2a_mppi_controller_reset(l2a_controller* controller, const unsigned char* dones);
int l2a_mppi_controller_reseed(l2a_controller* controller, unsigned long long seed);
int l2a_mppi_controller_result(l2a_controller* controller, float* mean_out, float* ess_out, int* valid_out, float* returns_out);
/* ---- the iCEM controller step as one call (device mode) ------------------------------------------------------------------
 * `MPCController.get_icem_action` (policies/mpc_controller.py; the planner of l2a_icem_sample / l2a_icem_refit above): the whole
 * plan step on the launch stream - per iteration `it` l2a_icem_sample with n_it = pops[it], the fused rollout of those n_it
 * candidates, l2a_icem_refit into result row block `it` - and ONE read-back of the iters * m * (act_dim + 4) floats of result rows.
 * Mean, spread [m, D], kept rows [m, Kk, D] and counts [m] live in the controller (three device copies of each rotate together: the
 * committed copy is never written by the step that reads it) and stay on the device, as every iteration's returns do, until
 * l2a_icem_controller_result asks.  Iteration 0 samples with the per-env shift vector - -1 for an env that is new or was reset
 * (l2a_icem_controller_reset), +1 otherwise -, later iterations with shift 0; add_mean applies to the last iteration only.  The
 * normals of iteration `it` are the Philox stream (seed) at offset (iter_calls + it) * n * m * D - the stride is the full n,
 * whatever pops[it] is -, iter_calls = iterations finished so far since create / reseed: with the same seed a step equals
 * get_icem_action bit for bit (action, index, best return, mean, spread, kept rows, counts, every iteration's result row and returns).
 *   iters  iterations per step (`icem_iters`);  pops [iters] host int32, K, Kk: the populations, the elites and the kept elites - the
 *          caller's (`MPCController._icem_sizes`), computed on the host in double precision and never recomputed here;  alpha, rho:
 *          `alpha`, `icem_rho`;  sigma0 [act_dim]: the initial spread (host float64, rounded to fp32 as `_icem_sigma_vector` does);
 *          add_mean: `icem_add_mean`.  Kk == 0: no kept rows (the kept arguments of sample and refit are NULL).
 * Refused at create (L2A_EINVAL, nothing allocated): the argument limits of l2a_icem_sample and l2a_icem_refit on every iteration -
 * the LDS checks pops[it] * 4 <= lds_per_block and K * 4 + L2A_ICEM_REFIT_STATIC_LDS <= lds_per_block among them, so that no step
 * can fail on its arguments -, iters < 1, a pops[it] outside 1 .. n, NULL pops / sigma0 / low / high / reward, a sigma0 that is
 * negative or not finite, alpha or rho outside [0, 1), m > 64 or more than 4096 observation floats; sharded:
 * l2a_cem_controller_create_sharded_device's rank / world / collective rules.
 * Steps through l2a_controller_step / _begin / _finish / _stats / _destroy: action_out / index_out / return_out come from the LAST
 * iteration's result rows - the best valid candidate's first action as float64, its index and return; without a valid candidate the
 * clipped mu'[i, 0, :], -1 and NaN, as l2a_icem_refit packs them.  The l2a_lstm_* step functions return L2A_EINVAL.  The committed
 * copy's index, iter_calls and the cleared reset marks move in _finish behind the verdict only: a launch flagged invalid (a tile-split
 * partner was lost) repeats the WHOLE step unsplit from the same state with the same offsets (L2A_STEP_UNSPLIT, same bits; flagged
 * again: L2A_ESPLIT), and a failed step leaves the controller where it was.  The in-flight exclusion rules of the CEM step apply
 * (the step reads and clears the context's status word).
 * Sharded (one rank of `world`): in iteration `it` l2a_icem_sample_shard over the window [rank n_it / world, (rank + 1) n_it / world)
 * - it moves with the population; an empty window rolls nothing out -, and the gather of the returns exactly as sharded CEM's with
 * n_it in place of n - l2a_cem_shard_pack, the int64 MAX all-reduce of m * n_it + 3 words (`reduce`, or the context's communicator),
 * l2a_cem_shard_unpack - in front of the UNCHANGED refit over all n_it: every rank's step equals the unsharded one bit for bit.  The
 * read-back gains the three verdict words.  The digest carries the controller kind, seed, iter_calls, m, n, h, iters, world, every
 * pops[it], K, Kk, add_mean, the bits of alpha, rho and sigma0, and the step's fresh marks: a mismatch, or a hole, is L2A_ESTATE on
 * every rank and nothing is consumed; a flag on any rank makes all of them repeat the step unsplit, together.
 *   l2a_icem_controller_reset  : dones [m] (non-zero: env i's next step starts afresh - shift -1), NULL = every env
 *   l2a_icem_controller_reseed : the stream restarts at 0 under `seed`; mean, spread, kept rows and counts are kept (what
 *                                get_icem_action does when torch.initial_seed() changes)
 *   l2a_icem_controller_result : of the latest finished step - mean and spread (host fp32 [m, D]), the kept rows [m, Kk, D] as
 *                                stored (env i's first kc[i] rows are this step's, what lies behind them is not), the counts [m],
 *                                every iteration's result rows [iters, m, act_dim + 4] and every iteration's returns, the tables
 *                                [m, pops[it]] one after another (sharded: the GATHERED tables); any pointer may be NULL; the rows
 *                                are the step's own read-back, everything else comes back in ONE copy on the latest step's stream,
 *                                waited for
 *   l2a_icem_controller_set_noise : M_host [h, h] (host fp32, the controller's h; any matrix - l2a_icem_noise_matrix's for power-law
 *                                noise) is copied to the device, and from the next step on every iteration samples with
 *                                l2a_icem_sample_noise (sharded: l2a_icem_sample_noise_shard) in place of the AR(1) entries; NULL
 *                                returns the controller to its rho.  Stream offsets, commit / replay, result rows, reset and
 *                                reseed are unchanged; a sharded step's digest additionally carries a hash of the matrix's bits
 *                                (every rank must have set the same one).  L2A_EINVAL with h > L2A_ICEM_NOISE_MAX_H.
 * _reset / _reseed / _result / _set_noise return L2A_ESTATE while a step is in flight, _result also before the first step has
 * finished, and L2A_EINVAL on a controller of another kind (as l2a_mppi_controller_* and l2a_cem_controller_result do on an iCEM
 * controller).
 * Not built: a recurrent model, reward programs and reward models (l2a_reward only), particle plans, NumPy normals.               */
int l2a_icem_controller_create_device(l2a_model* model, int m, int n, int h, const double* low, const double* high,
                                      double discount, const l2a_reward* reward, int iters, const int* pops, int K, int Kk,
                                      float alpha, float rho, const double* sigma0, int add_mean, unsigned long long seed,
                                      l2a_controller** out);
int l2a_icem_controller_create_sharded_device(l2a_model* model, int m, int n, int h, const double* low, const double* high,
                                              double discount, const l2a_reward* reward, int iters, const int* pops, int K, int Kk,
                                              float alpha, float rho, const double* sigma0, int add_mean, unsigned long long seed,
                                              int rank, int world, l2a_reduce_fn reduce, void* reduce_arg, l2a_controller** out);
int l2a_icem_controller_reset(l2a_controller* controller, const unsigned char* dones);
int l2a_icem_controller_reseed(l2a_controller* controller, unsigned long long seed);
int l2a_icem_controller_result(l2a_controller* controller, float* mean_out, float* std_out, float* kept_out, int* kc_out,
                               float* heads_out, float* returns_out);
int l2a_icem_controller_set_noise(l2a_controller* controller, const float* M_host);
void l2a_controller_destroy(l2a_controller* controller);
int l2a_controller_step(l2a_controller* controller, const double* obs, double* action_out, long long* index_out,
                        float* return_out, void* stream);
int l2a_lstm_controller_step(l2a_controller* controller, const double* obs, const float* c0, const float* h0,
                             float* c_next, float* h_next, double* action_out, long long* index_out, float* return_out,
                             void* stream);
/* The step in two halves.  l2a_controller_begin / l2a_lstm_controller_begin: take (or draw) the candidates, stage the
 * observations, launch, kick the producer - and return while the GPU plans (L2A_OK; L2A_STEP_MISS / negative codes as above,
 * nothing in flight then).  l2a_controller_finish: wait for the keys, decode, gather - returns what l2a_controller_step
 * returns (L2A_OK / L2A_STEP_DREW / L2A_STEP_UNSPLIT); between the two the host is free (the next env step's bookkeeping).
 * One step in flight per controller; the recurrent state pointers must stay valid until the step is finished.
 * THREADING CONTRACT of `np_state_addr`: the generator's words are read and written ONLY inside l2a_controller_begin (and
 * therefore the first half of l2a_controller_step) and l2a_controller_rearm, on the calling thread; the producer thread
 * works on a private copy of the state and never touches the caller's; l2a_controller_finish / _stats / _actions / _destroy
 * do not access it.  A caller whose OTHER threads may draw from the same generator holds that generator's lock (NumPy:
 * `_bit_generator.lock`) around _begin / _rearm - not around the wait for the GPU; a single-threaded caller (the
 * reference's run scripts) needs no lock.                                                                            */
int l2a_controller_begin(l2a_controller* controller, const double* obs, void* stream);
int l2a_lstm_controller_begin(l2a_controller* controller, const double* obs, const float* c0, const float* h0,
                              float* c_next, float* h_next, void* stream);
int l2a_controller_finish(l2a_controller* controller, double* action_out, long long* index_out, float* return_out);
int l2a_controller_rearm(l2a_controller* controller);
const float* l2a_controller_actions(const l2a_controller* controller);
int l2a_controller_stats(l2a_controller* controller, double* out, int cap);

/* ---- introspection used by tests (no GPU needed) ------------------------------------------ */
/* Which launch geometry the library picks for a plan of m envs x n candidates x h steps of an MLP model of this shape (relu /
 * identity, `n_sets` weight sets in `mode`) on a 256-CU device - the launcher's own decision code, stopped before its first HIP
 * call.  policy: NULL or {split, fan, micro, compute units, double rounds} (negative / 0 = the default: 1, 1, 1, 256, 1).  out[12] =
 * {kernel (0 generic fp32, 1 matrix core on 16-candidate tiles, 2 micro tiles), candidate tiles per workgroup, split mode
 * (0 none, 1 whole sets, 2 + shared half member, 3 member fan), first shared tile of a tail split or -1, member fan (0 / 1),
 * workgroups launched (incl. the placement's spare ones), LDS bytes per workgroup, sets per batch, micro tiles of the largest
 * workgroup, XCD placement units, double-tile workgroups of the launch IN FRONT of the described one (l2a_set_double_rounds:
 * the described launch then covers the rest of every env's candidates; 0 = the plan is one launch), 1 when the described launch
 * runs on a whole-tiles-only kernel instance (double tiles; whole single tiles of one set per candidate)}.  Results do not depend
 * on the geometry (bit-identical); this is how tests/test_host_logic.py pins the routing table without a GPU.          */
int l2a_plan_geometry(int obs_dim, int act_dim, int n_hidden, const int* hidden, int n_sets, int mode, int m, int n, int h,
                      const int* policy, int* out);
/* The same with counted arrays: policy[n_policy <= 7] = the five above, then {sets per batch (l2a_set_batch; negative = the
 * default 0), static three-set step (l2a_set_seq3; negative = the default 1)}; out[n_out = 12 | 13] = the twelve above, then 1
 * when the described launch runs on a static three-set-step instance (the other twelve do not depend on that switch).     */
int l2a_plan_geometry_ex(int obs_dim, int act_dim, int n_hidden, const int* hidden, int n_sets, int mode, int m, int n, int h,
                         const int* policy, int n_policy, int* out, int n_out);
/* The same for the recurrent launcher: which launch the library picks for a request of m envs x n candidates x h steps on the
 * model l2a_rnn_create builds from (obs_dim, act_dim, n_layers, units[], cell_type) - n_layers == 0: the model of
 * l2a_lstm_create with units[0] units - as the launcher's own plan function decides it, without a HIP call.
 * request: bit 0 per-row start states, bit 1 a state is written out (state_out / c_out / h_out), bit 2 NO results wanted
 * (neither returns nor keys), bit 3 the unit-tile split is NOT allowed (the state advance behind a blocking plan), bit 4 the
 * trajectory rollout (l2a_lstm_rollout_traj: its single launch, or one of the h one-step launches of its carry chain; the other
 * bits are then ignored).  0 = a plan as l2a_lstm_plan_rs launches it.
 * policy: NULL or {kernel kind (L2A_KERNEL_*), split, micro, compute units, LDS bytes per workgroup} (negative / 0 = the default:
 * auto, 1, 1, 256, 160 KiB).
 * out[12] = {kernel family (0 LSTM VALU, 1 LSTM matrix core on 16-candidate tiles, 2 LSTM micro tiles, 3 LSTM micro tiles writing
 * the trajectory, 4 generic VALU, 5 generic matrix core, 6 generic micro tiles), micro tiles a workgroup of the instance holds (3
 * or 4; 0: a 16-candidate kernel), unit-tile split (0 / 1), workgroups, LDS bytes per workgroup, 16-candidate tiles per env,
 * micro tiles: workgroups per env, micro tiles of the largest one, workgroups of that size per env (0 elsewhere), bytes of the
 * split's exchange buffer, 1 when a blocking plan on this shape and policy publishes its keys through the mailbox (else: copy and
 * synchronise), 0}.  Returns the launch's own error code (L2A_EINVAL: a kernel asked for that the shape is not eligible for, LDS
 * budget exceeded) with out untouched.  Results do not depend on the geometry (bit-identical).                          */
int l2a_lstm_plan_geometry(int obs_dim, int act_dim, int n_layers, const int* units, int cell_type, int m, int n, int h, int request,
                           const int* policy, int* out);
/* 1 when (obs_dim, act_dim, hidden[]) is eligible for the MFMA kernel, else 0.
 * Eligible shapes whose kernel instance keeps part of its working set in scratch memory (spilled VGPRs; correct, slower per
 * MFMA than their neighbours - tools/isa_notes.sh, profiles/r05_scratch_table.txt; none is a BASELINE.json shape):
 *   - hidden width 512 with 33 .. 64 observation dims, other than 49 inputs with relu / identity (the Ant instance is clean):
 *     6 - 8 VGPRs at 33 .. 48 observation dims, 40 - 132 at 49 .. 64.  The spill comes from the half-member paths of the tile
 *     split; the member-fan instances of the same shapes (l2a_set_fan) have none.  Alternative: the generic VALU kernel
 *     (l2a_set_kernel(ctx, L2A_KERNEL_VALU)), ~35 x slower.
 *   - l2a_lstm_mfma_eligible shapes with 512 units: 10 - 134 VGPRs (the 512-unit micro-tile instance: 14); 256 and 128 units are
 *     clean.  Alternative: the VALU kernel, ~40 x slower.
 * They stay selectable because every alternative is an order of magnitude slower.                                  */
int l2a_mfma_eligible(int obs_dim, int act_dim, int n_hidden, const int* hidden);
/* Host implementation of the weight re-packing used by the device pack kernel (same index
 * function).  Packs kernel W [k_in, n_out] (row-major) into `out`, which must hold
 * l2a_packed_layer_floats(k_in, n_out) floats.                                               */
long long l2a_packed_layer_floats(int k_in, int n_out);
int l2a_pack_layer_host(const float* w, int k_in, int n_out, float* out);
/* The micro-tile kernels' copy of a weight set (csrc/l2a_micro_pack.h: wave-stream order), on the host - what tests/
 * micro_emulator.py consumes.  l2a_micro_layout_floats: floats per set for an MLP obs_dim + act_dim -> n_hidden x hidden ->
 * obs_dim (0: no micro-tile instance for the shape).  l2a_micro_pack_layer_host: scatter layer `layer`'s row-major
 * [k_in, n_out] kernel (layer == n_hidden: the output layer) into `out`, which the caller zero-initialised.     */
long long l2a_micro_layout_floats(int obs_dim, int act_dim, int n_hidden, int hidden);
int l2a_micro_pack_layer_host(const float* w, int obs_dim, int act_dim, int n_hidden, int hidden, int layer, float* out);

#ifdef __cplusplus
}
#endif
#endif /* L2A_H_ */
