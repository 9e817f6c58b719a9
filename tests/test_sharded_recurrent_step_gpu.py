"""The sharded RECURRENT controller step as one C call (`l2a_lstm_controller_create_sharded[_device]`): plan, the one collective
and - behind it, in stream order - the hidden-state advance with the GLOBAL winner's first action, which usually belongs to
another rank.

Built on the sequential loopback world (tests/loopback_world.py) exactly as tests/test_sharded_emulation_gpu.py: one process, the
ranks one after another, a fresh `NativeStep` / controller per (pass, rank), `reset(rank)` restores what a separate process would
own; only the collectives are replaced.  A program runs all K controller steps of a golden replay: K collectives, K + 1 passes
(through `get_actions`: one more of each, the dry run of the collective).  The last test runs real processes (two gloo ranks
sharing the GPU) to pin the routing.

The states are compared BIT FOR BIT with the unsharded C controller's (`l2a_lstm_controller_create[_device]`) on the same inputs:
the advance is the same kernel on the same fp32 action - only where the action is found differs."""

import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cases
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.policies.mpc_controller import MPCController
from learning_to_adapt_amd.policies.native_step import NativeStep
from loopback_world import LoopbackWorld

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

RTOL = 1e-4                 # the project's return tolerance (tests/test_gpu_parity.py)
DIGEST_MASK = 0x7FFFFFFFFFFF


def _shard(n, rank, world):
    return MPCController._shard_range(n, rank, world)


def _restore_context(ctx):
    """What a rank that owns its process would find (tests/test_sharded_emulation_gpu.py)."""
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
    c.launch_status_value()
    _restore_context(c)
    yield c
    torch.cuda.synchronize()
    c.launch_status_value()
    _restore_context(c)


def _rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


_MODELS = {}


def _model(case):
    """(env, model) of a recurrent case, built once per test session and never changed."""
    if case["name"] not in _MODELS:
        _MODELS[case["name"]] = cases.product_rnn_model(case)
    return _MODELS[case["name"]]


def _resets(case):
    return {int(k): np.array(v, dtype=bool) for k, v in case.get("reset_after", {}).items()}


def _bits(t):
    return t.detach().cpu().numpy().copy()


def _replay_native(case, gold, native, env, steps, shard=None, before_step=None):
    """All `steps` controller steps through ONE NativeStep from zero hidden state (rows zeroed where the case resets an env):
    per step index, float64 action, return and the advanced state's bits."""
    m, U = case["m"], native.units
    stream = torch.cuda.current_stream(native.device).cuda_stream
    st = NativeStep(native, True, m, case["n"], case["h"], env.action_space.low, env.action_space.high, case.get("discount", 1.0),
                    env.reward_spec, shard=shard)
    resets = _resets(case)
    try:
        c = torch.zeros((m, U), dtype=torch.float32, device=native.device)
        h = torch.zeros((m, U), dtype=torch.float32, device=native.device)
        out = []
        for k in range(steps):
            if before_step is not None:
                before_step(k)
            c1, h1 = torch.empty_like(c), torch.empty_like(h)
            assert st.step(gold["obs"][k % len(gold["obs"])], stream, (c.data_ptr(), h.data_ptr(), c1.data_ptr(), h1.data_ptr()))
            torch.cuda.synchronize()
            out.append(dict(idx=st.idx.copy(), act=st.act.copy(), ret=st.ret.copy(), c=_bits(c1), h=_bits(h1)))
            c, h = c1, h1
            if k in resets:
                c, h = c.clone(), h.clone()
                c[torch.from_numpy(resets[k]).to(c.device)] = 0.0
                h[torch.from_numpy(resets[k]).to(h.device)] = 0.0
        return dict(steps=out, stats=st.stats())
    finally:
        st.close()


_UNSHARDED = {}


def _unsharded(ctx, cid, case=None):
    """The UNSHARDED C controller (`l2a_lstm_controller_create`) on the case's inputs: the reference of the state bits.  Computed
    once and shared."""
    key = (cid, None if case is None else case["n"])
    if key not in _UNSHARDED:
        base, seed = cases.split_id(cid)
        case = case or base
        gold = cases.load_golden(cid)
        env, model = _model(base)
        _restore_context(ctx)
        np.random.seed(seed)
        _UNSHARDED[key] = _replay_native(case, gold, model.planner_model(), env, base["steps"])["steps"]
    return _UNSHARDED[key]


def _run_native(ctx, cid, world_size, case=None, inject_on=None, steps=None, may_fail_tainted=False):
    base, seed = cases.split_id(cid)
    case = case or base
    gold = cases.load_golden(cid)
    env, model = _model(base)
    native = model.planner_model()
    assert native.ctx is ctx
    steps = steps or base["steps"]
    np.random.seed(seed)
    state0 = np.random.get_state()

    def reset(rank):
        np.random.set_state(state0)
        _restore_context(ctx)

    def program(rank, comm):
        def before_step(k):
            if rank == inject_on and k == 0:
                # what a lost tile-split partner reports, set on the host (tests/test_sharded_emulation_gpu.py does the same)
                ctx.check(ctx.lib.l2a_inject_status(ctx.handle, 1), "l2a_inject_status")
        try:
            out = _replay_native(case, gold, native, env, steps, shard=(rank, world_size, comm.reduce), before_step=before_step)
        except _lib.L2AError:
            # (a rank with an EMPTY shard that is handed its own words back - the placeholder of a pass in which the collective
            #  is not known yet - decodes the neutral key: that pass's result is discarded anyway)
            if may_fail_tainted and comm.tainted:
                return None
            raise
        out.update(rng_next=np.random.uniform(), degraded=bool(ctx.split_degraded), reduces=comm.calls)
        return out

    world = LoopbackWorld(world_size, reset=reset)
    outs = world.run(program)
    return case, gold, world, outs


def _owners(words, i, m):
    win = words[:, i].max()
    return [r for r in range(words.shape[0]) if words[r, i] == win]


def _assert_payloads(case, best, world, k, world_size):
    """Collective `k`: m + 3 words per rank, equal digest pairs, no flag; the winning key of every env appears in exactly the payload of
    the rank whose [lo, hi) holds the winner (tests/test_sharded_emulation_gpu.py).  Returns the owner rank of every env."""
    m = case["m"]
    words = np.stack(world.collectives[k]["parts"])
    assert world.collectives[k]["kind"] == "reduce" and words.shape == (world_size, m + 3) and words.dtype == np.int64
    assert np.all(words[:, m + 1] == words[0, m + 1]) and np.all(words[:, m + 2] == words[0, m + 2])
    assert int(words[0, m + 1]) + int(words[0, m + 2]) == DIGEST_MASK
    assert np.all(words[:, m] == 0)
    owner = []
    for i in range(m):
        b = int(best[i])
        assert _lib.key_decode(words[:, i].max())[1] == b
        own = _owners(words, i, m)
        assert own == [r for r in range(world_size) if _shard(case["n"], r, world_size)[0] <= b < _shard(case["n"], r, world_size)[1]]
        owner.append(own[0])
    return owner


def _assert_golden_replay(case, gold, outs, want, steps):
    m = case["m"]
    for rank, out in enumerate(outs):
        for k in range(steps):
            s, w, where = out["steps"][k], want[k], "rank %d, step %d" % (rank, k)
            assert np.array_equal(s["idx"], gold["best_%d" % k]), where
            assert s["act"].dtype == np.float64 and s["act"].tobytes() == np.ascontiguousarray(gold["chosen_%d" % k], dtype=np.float64).tobytes(), where
            ret = gold["returns_%d" % k].reshape(m, -1)[np.arange(m), gold["best_%d" % k]]
            assert _rel_err(s["ret"], ret) < RTOL, where
            # the unsharded C controller on the same inputs: the same state, bit for bit
            assert np.array_equal(w["idx"], s["idx"]) and w["act"].tobytes() == s["act"].tobytes(), where
            assert s["c"].tobytes() == w["c"].tobytes() and s["h"].tobytes() == w["h"].tobytes(), where
            assert np.isfinite(s["h"]).all() and np.abs(s["h"]).max() > 0.0, where
        assert out["rng_next"] == float(gold["rng_next"]), rank


# ---- 1 + 2: golden replays through the sharded C step, parity mode; the winner is foreign ------------------------------------------
@pytest.mark.parametrize("cid,world_size,shards", [
    ("hc_rnn_rs_u128_n40_h3_s0", 3, [13, 13, 14]),                  # one LSTM layer: the advance kernel gathers through the reduced keys
    ("hc_rnn_rs_gru2_n48_h4_s0", 3, [16, 16, 16]),                  # a generic stack: gather + one step of the rollout kernel
    ("c6_hc_rnn_rs_n500_h10_m5_s0", 8, [62, 63, 62, 63, 62, 63, 62, 63]),       # run_rebal.py's default plan
])
def test_golden_replay_through_the_sharded_recurrent_c_step(cid, world_size, shards, ctx):
    """Every golden controller step on every rank: the reference's index and float64 action bit for bit, its return, np.random left
    where the reference leaves it - and after every step c_next / h_next bit-identical to the unsharded C controller's, although for
    most ranks the winner was rolled out by ANOTHER rank (asserted from the recorded payloads)."""
    base, _ = cases.split_id(cid)
    assert [_shard(base["n"], r, world_size)[1] - _shard(base["n"], r, world_size)[0] for r in range(world_size)] == shards
    want = _unsharded(ctx, cid)
    case, gold, world, outs = _run_native(ctx, cid, world_size)
    K = case["steps"]
    assert world.passes == K + 1 and world.calls == [K] * world_size
    _assert_golden_replay(case, gold, outs, want, K)
    for k in range(K):
        # every env's winning key sits in exactly ONE rank's payload (asserted inside); the states of ALL ranks were compared above, so
        # every rank but that owner advanced env i with an action it never rolled out - the gather behind the collective
        owner = _assert_payloads(case, gold["best_%d" % k], world, k, world_size)
        for i in range(case["m"]):
            foreign = [r for r in range(world_size) if r != owner[i]]
            assert len(foreign) == world_size - 1 >= 1 and all(outs[r]["steps"][k]["c"].tobytes() == want[k]["c"].tobytes() for r in foreign)
    for out in outs:
        assert out["stats"]["steps"] == K and out["stats"]["relaunches"] == 0 and not out["degraded"] and out["reduces"] == K
        # the first step drew itself (and uploaded the first-step table on the launch stream); the later ones took the blocks the
        # producer thread drew ahead (table uploaded on the side stream)
        assert out["stats"]["sync_draws"] == 1 and out["stats"]["hits"] == K - 1


def _replay_controller(ctrl, case, gold, steps, before_step=None):
    resets = _resets(case)
    ctrl.reset(dones=[True] * case["m"])
    out = []
    for k in range(steps):
        if before_step is not None:
            before_step(k)
        actions, _ = ctrl.get_actions(gold["obs"][k % len(gold["obs"])])
        torch.cuda.synchronize()
        assert ctrl._hid_stale == "host"              # the device copy is the current one: adopted from the C step
        c, h = ctrl._hid_dev
        out.append(dict(idx=np.array(ctrl.last_plan["best_index"]), act=actions.copy(), ret=np.array(ctrl.last_plan["best_return"]),
                        c=_bits(c), h=_bits(h), shard=tuple(ctrl.last_plan["shard"])))
        if k in resets:
            ctrl.reset(dones=resets[k])
    return out


def _close(ctrl):
    if ctrl._cstep is not None:
        ctrl._cstep.close()
        ctrl._cstep = None
    if getattr(ctrl, "_ahead", None) is not None:
        ctrl._ahead.stop()


def test_golden_replay_with_a_reset_through_get_actions_on_two_loopback_ranks(ctx):
    """`hc_rnn_rs_m2_n64_h4_reset_s0` entered where the product enters it: `RNNMPCController.get_actions` with the collectives
    replaced builds the sharded recurrent C controller itself (the dry run of its collective is one more reduce, of zeros), adopts
    c_next / h_next through `_native_step_state` / `_native_step_done` and zeroes a finished env's rows between two steps."""
    cid, world_size = "hc_rnn_rs_m2_n64_h4_reset_s0", 2
    case, seed = cases.split_id(cid)
    gold = cases.load_golden(cid)
    env, model = _model(case)
    K = case["steps"]
    assert _resets(case)
    want = _unsharded(ctx, cid)
    np.random.seed(seed)
    state0 = np.random.get_state()

    def reset(rank):
        np.random.set_state(state0)
        _restore_context(ctx)

    def program(rank, comm):
        ctrl = comm.install(cases.product_rnn_controller(case, model=model, env=env))
        try:
            steps = _replay_controller(ctrl, case, gold, K)
            assert ctrl._cstep is not None and ctrl._cstep.recurrent
            stats = ctrl._cstep.stats()
            return dict(steps=steps, stats=stats, rng_next=np.random.uniform(), degraded=bool(ctx.split_degraded), reduces=comm.calls)
        finally:
            _close(ctrl)

    world = LoopbackWorld(world_size, reset=reset)
    outs = world.run(program)
    assert world.passes == K + 2 and world.calls == [K + 1] * world_size
    assert not np.stack(world.collectives[0]["parts"]).any()               # the dry run
    _assert_golden_replay(case, gold, outs, want, K)
    for k in range(K):
        _assert_payloads(case, gold["best_%d" % k], world, k + 1, world_size)
    for rank, out in enumerate(outs):
        assert out["stats"]["steps"] == K and out["stats"]["relaunches"] == 0 and not out["degraded"]
        assert all(s["shard"] == _shard(case["n"], rank, world_size) for s in out["steps"])


# ---- 3: device RNG ---------------------------------------------------------------------------------------------------------------
class _DevFloats(object):
    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


def _device_run(ctx, cid, world_size, torch_seed, steps):
    case, _ = cases.split_id(cid)
    gold = cases.load_golden(cid)
    env, model = _model(case)
    native = model.planner_model()
    m, n, h, A = case["m"], case["n"], case["h"], env.action_space.shape[0]

    def reset(rank):
        torch.manual_seed(torch_seed)
        _restore_context(ctx)

    def program(rank, comm):
        ctrl = cases.product_rnn_controller(case, model=model, env=env, rng="device")
        if comm is not None:
            comm.install(ctrl)
        lo, hi = _shard(n, rank, world_size)

        def check_owned(k):
            # the float64 action is float64(the fp32 value the owning rank planned on), read from its candidate tensor
            st = ctrl._cstep
            assert st is not None and st.device_rng and st.recurrent
            ptr = st.actions_ptr()
            local = torch.as_tensor(_DevFloats(ptr, h * m * (hi - lo) * A), device=native.device).cpu().numpy().reshape(h, m, hi - lo, A)
            owned = 0
            for i in range(m):
                j = int(st.idx[i])
                if lo <= j < hi:
                    assert st.act[i].tobytes() == local[0, i, j - lo].astype(np.float64).tobytes(), (rank, k, i)
                    owned += 1
            return owned

        try:
            ctrl.reset(dones=[True] * m)
            out, owned = [], 0
            for k in range(steps):
                actions, _ = ctrl.get_actions(gold["obs"][k % len(gold["obs"])])
                torch.cuda.synchronize()
                owned += check_owned(k)
                c, hh = ctrl._hid_dev
                out.append(dict(idx=np.array(ctrl.last_plan["best_index"]), act=actions.copy(), c=_bits(c), h=_bits(hh)))
            return dict(steps=out, owned=owned, stats=ctrl._cstep.stats())
        finally:
            _close(ctrl)

    if world_size == 1:
        reset(0)
        return [program(0, None)]
    world = LoopbackWorld(world_size, reset=reset)
    outs = world.run(program)
    assert world.passes == steps + 2 and world.calls == [steps + 1] * world_size
    return outs


@pytest.mark.parametrize("cid", ["hc_rnn_rs_u128_n40_h3_s0", "hc_rnn_rs_gru2_n48_h4_s0"])
def test_device_rng_recurrent_plan_does_not_depend_on_the_world_size(cid, ctx):
    """`RNNMPCController(rng="device")` on 1, 2 and 3 ranks with the same seed, three consecutive steps: every rank fills its slice of
    the SAME Philox stream, so indices, float64 actions and hidden-state bits are identical across ranks and world sizes - the
    advance recomputes the global winner's action from the stream on the device."""
    case, _ = cases.split_id(cid)
    steps = 3
    runs = {w: _device_run(ctx, cid, w, 9001, steps) for w in (1, 2, 3)}
    want = runs[1][0]["steps"]
    assert runs[1][0]["owned"] == steps * case["m"]
    for w in (2, 3):
        assert sum(out["owned"] for out in runs[w]) == steps * case["m"]          # every winner has exactly one owner
        assert any(out["owned"] < steps * case["m"] for out in runs[w])           # ... and somebody advanced with a foreign one
        for rank, out in enumerate(runs[w]):
            assert out["stats"]["steps"] == steps and out["stats"]["relaunches"] == 0
            for k in range(steps):
                s, where = out["steps"][k], "world %d, rank %d, step %d" % (w, rank, k)
                assert np.array_equal(s["idx"], want[k]["idx"]), where
                assert s["act"].dtype == np.float64 and s["act"].tobytes() == want[k]["act"].tobytes(), where
                assert s["c"].tobytes() == want[k]["c"].tobytes() and s["h"].tobytes() == want[k]["h"].tobytes(), where
    # another seed plans on other candidates (the stream is the seed's)
    other = _device_run(ctx, cid, 2, 9002, 1)
    assert other[0]["steps"][0]["act"].tobytes() != want[0]["act"].tobytes()


# ---- 4: flagged relaunch ------------------------------------------------------------------------------------------------------------
def test_a_flagged_middle_rank_makes_all_four_relaunch_and_advance_again(ctx):
    """`l2a_inject_status(ctx, 1)` on rank 2 of 4: the reduced flag makes every rank repeat launch, payload, collective AND advance
    unsplit (one relaunch, two collectives, L2A_STEP_UNSPLIT -> the context is marked degraded); actions and c_next / h_next are the
    unflagged run's bits - the state written behind the FIRST collective is overwritten."""
    cid = "hc_rnn_rs_u128_n40_h3_s0"
    _, _, world0, plain = _run_native(ctx, cid, 4, steps=1)
    case, gold, world, outs = _run_native(ctx, cid, 4, inject_on=2, steps=1)
    assert world0.passes == 2 and world.passes == 3 and world.calls == [2] * 4
    m = case["m"]
    first = np.stack(world.collectives[0]["parts"])
    assert first[:, m].tolist() == [0, 0, 1, 0] and int(world.result(0)[m]) == 1
    second = np.stack(world.collectives[1]["parts"])
    assert np.all(second[:, m] == 0) and np.array_equal(first[:, :m], second[:, :m])
    for rank, (out, ref) in enumerate(zip(outs, plain)):
        assert out["stats"]["relaunches"] == 1 and out["degraded"] and out["reduces"] == 2 and out["stats"]["steps"] == 1
        assert ref["stats"]["relaunches"] == 0 and not ref["degraded"]
        s, w = out["steps"][0], ref["steps"][0]
        assert np.array_equal(s["idx"], gold["best_0"]) and np.array_equal(s["idx"], w["idx"]), rank
        assert s["act"].tobytes() == w["act"].tobytes() and s["ret"].tobytes() == w["ret"].tobytes(), rank
        assert s["c"].tobytes() == w["c"].tobytes() and s["h"].tobytes() == w["h"].tobytes(), rank


# ---- 5: more ranks than candidates -----------------------------------------------------------------------------------------------
def test_more_ranks_than_candidates_leaves_one_rank_with_an_empty_shard(ctx):
    """n = 2 on three ranks: rank 0's shard is empty - it contributes the neutral key, still joins the collective and still advances
    its state with the global winner's action (from the first-step table every rank holds).  Every rank returns the world-1 result
    and state."""
    cid = "hc_rnn_rs_u128_n40_h3_s0"
    base, _ = cases.split_id(cid)
    case = dict(base, n=2)
    assert [_shard(2, r, 3) for r in range(3)] == [(0, 0), (0, 1), (1, 2)]
    want = _unsharded(ctx, cid, case=case)
    _, _, world, outs = _run_native(ctx, cid, 3, case=case, may_fail_tainted=True)
    K = base["steps"]
    assert world.passes == K + 1 and world.calls == [K] * 3
    for k in range(K):
        words = np.stack(world.collectives[k]["parts"])
        assert not words[0, :case["m"]].any() and words[1:, :case["m"]].all()       # the neutral key of the empty shard
    for rank, out in enumerate(outs):
        assert out["stats"]["steps"] == K and out["stats"]["relaunches"] == 0
        for k in range(K):
            s, w = out["steps"][k], want[k]
            assert np.array_equal(s["idx"], w["idx"]) and s["act"].tobytes() == w["act"].tobytes(), (rank, k)
            assert _rel_err(s["ret"], w["ret"]) < RTOL, (rank, k)
            assert s["c"].tobytes() == w["c"].tobytes() and s["h"].tobytes() == w["h"].tobytes(), (rank, k)


# ---- 6: digest mismatch ------------------------------------------------------------------------------------------------------------
def test_a_rank_seeded_differently_fails_the_step_on_every_rank_and_nothing_is_adopted(ctx):
    """Two ranks step once in agreement; then rank 1 is seeded differently: the second step fails with L2A_ESTATE on BOTH ranks (the
    digest pair of the collective), and `_hidden_state` is what the first step left - the c_next / h_next written behind the
    collective of the failed step are not adopted."""
    cid, world_size = "hc_rnn_rs_m2_n64_h4_reset_s0", 2
    case, seed = cases.split_id(cid)
    gold = cases.load_golden(cid)
    env, model = _model(case)
    np.random.seed(seed)
    state0 = np.random.get_state()

    def reset(rank):
        np.random.set_state(state0)
        _restore_context(ctx)

    def program(rank, comm):
        ctrl = comm.install(cases.product_rnn_controller(case, model=model, env=env))
        try:
            ctrl.reset(dones=[True] * case["m"])
            actions, _ = ctrl.get_actions(gold["obs"][0])
            assert np.array_equal(actions, gold["chosen_0"]) or comm.tainted
            torch.cuda.synchronize()
            before_dev = tuple(_bits(t) for t in ctrl._hid_dev)
            before = tuple(np.array(p) for p in ctrl._pack(ctrl._hidden_state))
            assert np.abs(before[1]).max() > 0.0 and before[1].astype(np.float32).tobytes() == before_dev[1].tobytes()
            if rank == 1:
                np.random.seed(seed + 1)
            error = None
            try:
                ctrl.get_actions(gold["obs"][1])
            except _lib.L2AError as exc:
                error = str(exc)
            torch.cuda.synchronize()
            after = tuple(np.array(p) for p in ctrl._pack(ctrl._hidden_state))
            after_dev = tuple(_bits(t) for t in ctrl._device_hidden(model.planner_model().device))
            same = all(a.tobytes() == b.tobytes() for a, b in zip(before + before_dev, after + after_dev))
            return dict(error=error, same=same, next=ctrl._hid_next)
        finally:
            _close(ctrl)

    world = LoopbackWorld(world_size, reset=reset)
    outs = world.run(program)
    assert world.passes == 4 and world.calls == [3] * world_size               # dry run, step 0, the failed step
    words = np.stack(world.collectives[2]["parts"])
    m = case["m"]
    assert words[0, m + 1] != words[1, m + 1]
    for rank, out in enumerate(outs):
        assert out["error"] is not None and "(%d)" % _lib.L2A_ESTATE in out["error"], rank
        assert "identical np.random global state" in out["error"], rank
        assert out["same"] and out["next"] is None, rank


# ---- 7: routing, with real processes -----------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker_routing(rank, world, port, cid, out_dir):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["L2A_SPLIT"] = "0"           # ranks sharing one GPU: a tile's two workgroups may not be co-resident
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    try:
        case, seed = cases.split_id(cid)
        gold = cases.load_golden(cid)
        ctrl = cases.product_rnn_controller(case)
        ctrl.reset(dones=[True] * case["m"])
        np.random.seed(seed)
        out = {}
        K = int(gold["obs"].shape[0])
        for k in range(K):
            actions, _ = ctrl.get_actions(gold["obs"][k])
            out["actions_%d" % k] = actions
            out["best_%d" % k] = np.asarray(ctrl.last_plan["best_index"])
        out["native"] = np.asarray(0 if ctrl._cstep is None else 1)
        out["steps"] = np.asarray(-1 if ctrl._cstep is None else ctrl._cstep.stats()["steps"])
        out["recurrent"] = np.asarray(0 if ctrl._cstep is None else int(ctrl._cstep.recurrent))
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        _close(ctrl)
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_route_the_recurrent_plan_through_the_sharded_c_step(tmp_path):
    """`c6_hc_rnn_rs_n500_h10_m5_s0` through `RNNMPCController.get_actions` on two real processes: every step of both ranks ran
    inside the C controller (`ctrl._cstep`, its step counter), with the golden indices and actions."""
    cid, world = "c6_hc_rnn_rs_n500_h10_m5_s0", 2
    mp.spawn(_worker_routing, args=(world, _free_port(), cid, str(tmp_path)), nprocs=world, join=True)
    gold = cases.load_golden(cid)
    K = int(gold["obs"].shape[0])
    for r in range(world):
        o = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert int(o["native"]) == 1 and int(o["recurrent"]) == 1 and int(o["steps"]) == K, r
        for k in range(K):
            assert np.array_equal(o["best_%d" % k], gold["best_%d" % k]), (r, k)
            np.testing.assert_array_equal(o["actions_%d" % k], gold["chosen_%d" % k])
