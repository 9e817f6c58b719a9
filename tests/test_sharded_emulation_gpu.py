"""The multi-GPU configs in the launch geometry an 8-GPU run uses, on ONE GPU: the ranks run one after another through the
sequential loopback world (tests/loopback_world.py), so a rank launches what it launches when it owns its GPU - config 4's shard
(n = 2000) the tile split with the exchange between workgroup pairs, config 5's shard (n = 500, h = 30) the member fan.
`tests/test_distributed_gpu.py` runs real processes and a real collective, but has to switch the split (and with it the fan) off.

Only the collectives are replaced.  The draw, the slice, the launch, `l2a_plan_payload`, the digest and flag checks, the relaunch
protocol, `_cem_iteration` and `get_cem_action_device` are the product's.  Every test first asserts - `_lib.plan_geometry`, the
launcher's own decision code - that its shard takes the geometry it claims to test.

Not covered here: RCCL with more than one rank, and timing."""

import numpy as np
import pytest
import torch

import cases
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.policies.mpc_controller import MPCController
from learning_to_adapt_amd.policies.native_step import NativeStep
from loopback_world import LoopbackWorld

pytestmark = pytest.mark.gpu

RTOL = 1e-4                 # the project's return tolerance (tests/test_gpu_parity.py)
DIGEST_MASK = 0x7FFFFFFFFFFF


def _shard(n, rank, world):
    return MPCController._shard_range(n, rank, world)


def _restore_context(ctx):
    """What a rank that owns its process would find: the context's default policies, no degradation, a clear status word.  (All
    ranks share `_lib.Context.get(0)` here, and a relaunch on one of them switches the split off for all.)"""
    torch.cuda.synchronize()
    ctx.set_split(1)
    ctx.set_fan(1)
    ctx.set_micro(1)
    ctx.set_double_rounds(1)
    ctx.split_degraded = False
    assert ctx.launch_status_value() == 0, "a launch of the previous rank left the status word set"


@pytest.fixture
def ctx():
    c = _lib.Context.get(0)
    torch.cuda.synchronize()
    c.launch_status_value()         # (whatever an earlier test file left behind)
    _restore_context(c)
    yield c
    torch.cuda.synchronize()
    c.launch_status_value()
    _restore_context(c)


def _geometry(ctx, case, env, n_local):
    return _lib.plan_geometry(env.observation_space.shape[0], env.action_space.shape[0], case["hidden"], case["E"], case["mode"],
                              case["m"], n_local, case["h"], cus=ctx.info()["compute_units"])


def _assert_tile_split(ctx, case, env, world):
    for r in range(world):
        lo, hi = _shard(case["n"], r, world)
        g = _geometry(ctx, case, env, hi - lo)
        assert hi - lo == 2000 and (g["split"], g["fan"], g["workgroups"]) == (2, False, 256), g


def _assert_member_fan(ctx, case, env, world):
    for r in range(world):
        lo, hi = _shard(case["n"], r, world)
        g = _geometry(ctx, case, env, hi - lo)
        assert hi - lo == 500 and case["h"] == 30 and (g["split"], g["fan"], g["nt"]) == (3, True, 1), g


def _assert_micro(ctx, case, env, world):
    for r in range(world):
        lo, hi = _shard(case["n"], r, world)
        assert _geometry(ctx, case, env, hi - lo)["kernel"] == "micro"


def _rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


# ---- the sharded C step (`l2a_controller_create_sharded`) as `world` ranks ------------------------------------------------------
def _run_sharded_c_step(ctx, cid, world_size, inject_on=None):
    """One step of `world_size` sharded C controllers, one fresh controller per (pass, rank): its first step draws synchronously
    from the restored global generator, so the draw-ahead chain of an earlier pass never meets a rewound state."""
    case, seed = cases.split_id(cid)
    gold = cases.load_golden(cid)
    env, model = cases.product_model(case)
    native = model.planner_model()
    assert native.ctx is ctx
    stream = torch.cuda.current_stream(native.device).cuda_stream
    np.random.seed(seed)
    state0 = np.random.get_state()

    def reset(rank):
        np.random.set_state(state0)
        _restore_context(ctx)

    def program(rank, comm):
        st = NativeStep(native, False, case["m"], case["n"], case["h"], env.action_space.low, env.action_space.high,
                        case.get("discount", 1.0), env.reward_spec, shard=(rank, world_size, comm.reduce))
        try:
            if rank == inject_on:
                # what a lost tile-split partner reports, set on the host (tests/test_distributed_gpu.py does the same)
                ctx.check(ctx.lib.l2a_inject_status(ctx.handle, 1), "l2a_inject_status")
            assert st.step(gold["obs0"], stream)
            return dict(idx=st.idx.copy(), act=st.act.copy(), ret=st.ret.copy(), rng_next=np.random.uniform(), stats=st.stats(),
                        degraded=bool(ctx.split_degraded), reduces=comm.calls)
        finally:
            st.close()

    world = LoopbackWorld(world_size, reset=reset)
    outs = world.run(program)
    return case, gold, env, world, outs


def _assert_golden_step(case, gold, outs):
    want_ret = gold["returns"][np.arange(case["m"]), gold["best"]]
    for rank, out in enumerate(outs):
        assert np.array_equal(out["idx"], gold["best"]), rank
        assert out["act"].dtype == np.float64 and out["act"].tobytes() == np.ascontiguousarray(gold["chosen"], dtype=np.float64).tobytes(), rank
        assert out["rng_next"] == float(gold["rng_next"]), rank
        assert _rel_err(out["ret"], want_ret) < RTOL, rank


def _assert_payloads(case, gold, world, k, world_size):
    """Collective `k` of the run: m + 3 words per rank, equal digest pairs, no flag; the winning key of every env appears in exactly
    the payload of the rank whose [lo, hi) holds the golden winner."""
    m = case["m"]
    words = np.stack(world.collectives[k]["parts"])
    assert world.collectives[k]["kind"] == "reduce" and words.shape == (world_size, m + 3) and words.dtype == np.int64
    assert np.all(words[:, m + 1] == words[0, m + 1]) and np.all(words[:, m + 2] == words[0, m + 2])
    assert int(words[0, m + 1]) + int(words[0, m + 2]) == DIGEST_MASK
    assert np.all(words[:, m] == 0)
    for i in range(m):
        best = int(gold["best"][i])
        win = words[:, i].max()
        assert _lib.key_decode(win)[1] == best
        owners = [r for r in range(world_size) if words[r, i] == win]
        assert owners == [r for r in range(world_size) if _shard(case["n"], r, world_size)[0] <= best < _shard(case["n"], r, world_size)[1]]
    return words


@pytest.mark.parametrize("cid", ["c4_hc_rs_n16000_h30_e5_s0", "c4_hc_rs_n16000_h30_e5_s1"])
def test_config4_as_eight_ranks_of_the_sharded_c_step(cid, ctx):
    """Tile split -> payload packed on the device -> collective -> decode, eight times 2000 candidates: every rank returns the
    reference planner's golden index, its float64 action bit for bit and its return, and leaves np.random where the reference
    leaves it; nobody relaunches."""
    case, _ = cases.split_id(cid)
    env, _, _ = cases.recipe(case)
    _assert_tile_split(ctx, case, env, 8)
    case, gold, env, world, outs = _run_sharded_c_step(ctx, cid, 8)
    assert world.passes == 2 and world.calls == [1] * 8
    _assert_golden_step(case, gold, outs)
    _assert_payloads(case, gold, world, 0, 8)
    for out in outs:
        assert out["stats"]["relaunches"] == 0 and not out["degraded"] and out["reduces"] == 1
        assert out["stats"]["steps"] == 1 and out["stats"]["sync_draws"] == 1


def test_a_flagged_rank_makes_all_eight_relaunch_unsplit_in_config4s_geometry(ctx):
    """The relaunch protocol where it matters: ONE middle rank's launch reports a lost tile-split partner (status word set on the
    host).  The reduced flag makes ALL EIGHT ranks repeat launch and collective unsplit - two reduce calls each, one relaunch,
    the step reports L2A_STEP_UNSPLIT - and every rank still returns the golden plan (the unsplit geometry gives the same bits)."""
    cid = "c4_hc_rs_n16000_h30_e5_s0"
    case, _ = cases.split_id(cid)
    env, _, _ = cases.recipe(case)
    _assert_tile_split(ctx, case, env, 8)
    assert _geometry(ctx, case, env, 2000)["split"] == 2
    case, gold, env, world, outs = _run_sharded_c_step(ctx, cid, 8, inject_on=3)
    assert world.passes == 3 and world.calls == [2] * 8
    _assert_golden_step(case, gold, outs)
    m = case["m"]
    first = np.stack(world.collectives[0]["parts"])
    assert first[:, m].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]               # only the flagged rank raised the flag ...
    assert int(world.result(0)[m]) == 1                                     # ... and everybody saw it
    second = _assert_payloads(case, gold, world, 1, 8)
    assert np.array_equal(first[:, :m], second[:, :m])                      # the split and the unsplit launch: the same keys
    for out in outs:
        assert out["stats"]["relaunches"] == 1 and out["degraded"] and out["reduces"] == 2


def test_uneven_shards_of_the_micro_tile_plan_through_the_sharded_c_step(ctx):
    """`c3b_ant_rs_n500_h10_pb5_3x512_s0` at world = 3: micro-tile kernels, per-block sets, five envs (a payload of 5 + 3 words),
    shards of 166 / 167 / 167 candidates."""
    cid = "c3b_ant_rs_n500_h10_pb5_3x512_s0"
    case, _ = cases.split_id(cid)
    env, _, _ = cases.recipe(case)
    _assert_micro(ctx, case, env, 3)
    assert [_shard(case["n"], r, 3)[1] - _shard(case["n"], r, 3)[0] for r in range(3)] == [166, 167, 167] and case["m"] == 5
    case, gold, env, world, outs = _run_sharded_c_step(ctx, cid, 3)
    assert world.passes == 2 and world.calls == [1] * 3
    _assert_golden_step(case, gold, outs)
    _assert_payloads(case, gold, world, 0, 3)
    assert all(out["stats"]["relaunches"] == 0 for out in outs)


def test_config4_through_get_actions_on_eight_loopback_ranks(ctx):
    """The same composition entered where the product enters it: `MPCController.get_actions` with `_dist` and `_reduce_payload`
    replaced builds the sharded C controller itself (its dry run of the collective is one more reduce, of zeros) and steps it."""
    cid = "c4_hc_rs_n16000_h30_e5_s0"
    case, seed = cases.split_id(cid)
    gold = cases.load_golden(cid)
    env, model = cases.product_model(case)
    _assert_tile_split(ctx, case, env, 8)
    np.random.seed(seed)
    state0 = np.random.get_state()

    def reset(rank):
        np.random.set_state(state0)
        _restore_context(ctx)

    def program(rank, comm):
        ctrl = comm.install(cases.product_controller(case, model=model, env=env))
        try:
            actions, _ = ctrl.get_actions(gold["obs0"])
            assert ctrl._cstep is not None and ctrl._cstep.stats()["relaunches"] == 0
            return dict(idx=np.array(ctrl.last_plan["best_index"]), act=actions.copy(), ret=np.array(ctrl.last_plan["best_return"]),
                        rng_next=np.random.uniform(), shard=ctrl.last_plan["shard"])
        finally:
            if ctrl._cstep is not None:
                ctrl._cstep.close()
                ctrl._cstep = None

    world = LoopbackWorld(8, reset=reset)
    outs = world.run(program)
    assert world.passes == 3 and world.calls == [2] * 8
    assert not np.stack(world.collectives[0]["parts"]).any()               # the dry run
    _assert_golden_step(case, gold, outs)
    _assert_payloads(case, gold, world, 1, 8)
    assert [tuple(out["shard"]) for out in outs] == [_shard(case["n"], r, 8) for r in range(8)]


# ---- CEM in parity mode: `_cem_iteration` per rank, iteration after iteration ----------------------------------------------------
def _world1_cem(case, seed, gold, model, env, **kw):
    """The same seed planned by a plain world-1 controller; the generator state it left after every iteration is recorded."""
    ref = cases.product_controller(case, model=model, env=env, **kw)
    stock = ref._cem_iteration
    states = []

    def recording(*a, **k):
        out = stock(*a, **k)
        states.append(np.random.get_state())
        return out

    ref._cem_iteration = recording
    np.random.seed(seed)
    state0 = np.random.get_state()
    actions, _ = ref.get_actions(gold["obs0"])
    rng_next = np.random.uniform()
    if ref._ahead is not None:
        ref._ahead.stop()
    return dict(actions=actions.copy(), best=np.array(ref.last_plan["best_index"]), trace=ref.last_plan["cem_trace"],
                states=[state0] + states, rng_next=rng_next)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _run_sharded_cem(ctx, cid, world_size):
    """`ctrl._cem_iteration(obs0, mean, std, k, clip_low, clip_high, lo_r, hi_r, world)` for every rank through the loopback world,
    iteration after iteration, against the world-1 run's trace: gathered returns, refitted mean / std and the generator position
    bit-identical on every rank; at the end the arg-max index and the action."""
    case, seed = cases.split_id(cid)
    gold = cases.load_golden(cid)
    env, model = cases.product_model(case)
    want = _world1_cem(case, seed, gold, model, env)
    ctrl = cases.product_controller(case, model=model, env=env)
    n, m, h = case["n"], case["m"], case["h"]
    act_dim = env.action_space.shape[0]
    iters = case["num_cem_iters"]
    assert len(want["trace"]) == iters and ctrl.num_cem_iters == iters
    num_elites = max(int(n * ctrl.percent_elites), 1)
    mean, std = np.zeros((m, h * act_dim)), np.ones((m, h * act_dim))
    clip_low = np.concatenate([env.action_space.low] * h)
    clip_high = np.concatenate([env.action_space.high] * h)
    outs = None
    for it in range(iters):
        start = want["states"][it]

        def reset(rank):
            np.random.set_state(start)
            _restore_context(ctx)

        def program(rank, comm, mean=mean, std=std):
            comm.install(ctrl)
            lo, hi = _shard(n, rank, world_size)
            new_mean, new_std, returns, cand_a = ctrl._cem_iteration(gold["obs0"], mean, std, num_elites, clip_low, clip_high,
                                                                     lo, hi, world_size)
            return dict(mean=np.array(new_mean), std=np.array(new_std), returns=np.array(returns), cand_a=np.array(cand_a),
                        state=np.random.get_state(), degraded=bool(ctx.split_degraded))

        world = LoopbackWorld(world_size, reset=reset)
        outs = world.run(program)
        assert world.passes == 3 and [c["kind"] for c in world.collectives] == ["reduce", "gather"]
        assert not np.stack(world.collectives[0]["parts"])[:, 0].any()     # no launch was flagged
        tr = want["trace"][it]
        for rank, out in enumerate(outs):
            where = "iteration %d, rank %d" % (it, rank)
            assert out["returns"].dtype == np.float64 and out["returns"].shape == (m, n), where
            diff = np.flatnonzero(out["returns"].reshape(-1) != np.asarray(tr["returns"]).reshape(-1))
            assert out["returns"].tobytes() == np.ascontiguousarray(tr["returns"]).tobytes(), \
                "%s: %d gathered returns differ from the world-1 run's, first at candidate %s" % (where, diff.size, diff[:1])
            assert out["mean"].tobytes() == np.ascontiguousarray(tr["mean"]).tobytes(), where
            assert out["std"].tobytes() == np.ascontiguousarray(tr["std"]).tobytes(), where
            assert _same_state(out["state"], want["states"][it + 1]), where
            assert not out["degraded"], where
        mean, std = outs[0]["mean"], outs[0]["std"]
    if ctrl._ahead is not None:
        ctrl._ahead.stop()
    np.random.set_state(want["states"][iters])
    rng_next = np.random.uniform()
    assert rng_next == want["rng_next"]
    final = []
    for out in outs:
        idx = np.argmax(out["returns"], axis=1)
        final.append((idx, out["cand_a"][range(m), idx]))
        assert np.array_equal(idx, want["best"])
        assert final[-1][1].tobytes() == want["actions"].tobytes()
    return case, gold, final, rng_next


@pytest.mark.parametrize("cid", ["c5_hc_cem_n4000_h30_e5_s0", "c5_hc_cem_n4000_h30_e5_s1", "c5_hc_cem_n4000_h30_e5_s2"])
def test_config5_as_eight_ranks_through_cem_iteration(cid, ctx):
    """Fan rollout -> gather -> refit, five times over, then pick: 8 x 500 candidates at h = 30 on the member fan against ONE
    process planning all 4000 (the horizon-pipelined rollout on whole tiles) - three launch paths, one set of bits
    (include/l2a.h: "Geometry only: results are bit-identical").  s0 must be the reference planner's golden plan too; s1 and s2
    leave the reference at witnessed elite-mask rank ties (tests/test_gpu_parity.py) and are held to the world-1 run only."""
    case, _ = cases.split_id(cid)
    env, _, _ = cases.recipe(case)
    _assert_member_fan(ctx, case, env, 8)
    case, gold, final, rng_next = _run_sharded_cem(ctx, cid, 8)
    if cid.endswith("_s0"):
        for idx, act in final:
            assert np.array_equal(idx, gold["best"])
            np.testing.assert_array_equal(act, gold["chosen"])
        assert rng_next == float(gold["rng_next"])


def test_uneven_shards_of_a_cem_plan_through_cem_iteration(ctx):
    """`hc_cem_n400_h10_s0` at world = 3: shards of 133 / 133 / 134 candidates on micro tiles, so the gather is padded and cut
    back - against the world-1 run bit for bit and against the reference planner's golden plan."""
    cid = "hc_cem_n400_h10_s0"
    case, _ = cases.split_id(cid)
    env, _, _ = cases.recipe(case)
    _assert_micro(ctx, case, env, 3)
    assert [_shard(case["n"], r, 3)[1] - _shard(case["n"], r, 3)[0] for r in range(3)] == [133, 133, 134]
    case, gold, final, rng_next = _run_sharded_cem(ctx, cid, 3)
    for idx, act in final:
        assert np.array_equal(idx, gold["best"])
        np.testing.assert_array_equal(act, gold["chosen"])
    assert rng_next == float(gold["rng_next"])


# ---- CEM with the device RNG: `get_cem_action_device` per rank --------------------------------------------------------------------
@pytest.mark.parametrize("cem_mode", ["reference", "fixed"])
@pytest.mark.parametrize("cid", ["c5_hc_cem_n4000_h30_e5_s0", "c5_hc_cem_n4000_h30_e5_s1"])
def test_config5_device_rng_as_eight_ranks_does_not_depend_on_the_world_size(cid, cem_mode, ctx):
    """Every rank samples its slice of the SAME Philox stream (`l2a_cem_sample` with lo, hi), rolls 500 candidates out on the member
    fan and refits on the gathered returns (five gathers, one agreement): index, action, final mean and std must be those of ONE
    process planning all 4000 under the same seed, bit for bit, on every rank."""
    case, seed = cases.split_id(cid)
    gold = cases.load_golden(cid)
    env, model = cases.product_model(case)
    _assert_member_fan(ctx, case, env, 8)
    torch_seed = 4242 + seed

    ref = cases.product_controller(case, model=model, env=env, rng="device", cem_mode=cem_mode)
    torch.manual_seed(torch_seed)
    want_act, _ = ref.get_actions(gold["obs0"])
    want = dict(ref.last_plan)

    ctrl = cases.product_controller(case, model=model, env=env, rng="device", cem_mode=cem_mode)

    def reset(rank):
        torch.manual_seed(torch_seed)
        ctrl._bufs.pop("cem_seed", None)            # (the stream's counters: back to the first plan step under this seed)
        ctrl._bufs.pop("cem_calls", None)
        _restore_context(ctx)

    def program(rank, comm):
        comm.install(ctrl)
        act, _ = ctrl.get_actions(gold["obs0"])
        plan = ctrl.last_plan
        return dict(act=act.copy(), best=np.array(plan["best_index"]), ret=np.array(plan["best_return"]),
                    mean=np.array(plan["cem_mean"]), std=np.array(plan["cem_std"]), calls=ctrl._bufs["cem_calls"],
                    degraded=bool(ctx.split_degraded))

    world = LoopbackWorld(8, reset=reset)
    outs = world.run(program)
    iters = case["num_cem_iters"]
    assert world.passes == iters + 2 and [c["kind"] for c in world.collectives] == ["gather"] * iters + ["reduce"]
    agreed = np.stack(world.collectives[iters]["parts"])
    assert not agreed[:, 0].any() and np.all(agreed == agreed[0])
    for rank, out in enumerate(outs):
        assert np.array_equal(out["best"], want["best_index"]), rank
        assert out["act"].tobytes() == want_act.tobytes(), rank
        assert out["ret"].tobytes() == np.asarray(want["best_return"]).tobytes(), rank
        assert out["mean"].tobytes() == want["cem_mean"].tobytes(), rank
        assert out["std"].tobytes() == want["cem_std"].tobytes(), rank
        assert out["calls"] == iters and not out["degraded"], rank
    # every iteration's gathered table is the same on every rank by construction; its parts are the ranks' own rollouts
    for k in range(iters):
        assert all(p.shape == (case["m"], 500) and p.dtype == np.float32 for p in world.collectives[k]["parts"])
