"""The sharded recurrent (ReBAL) device-mode CEM plan step as ONE C call (``l2a_lstm_cem_controller_create_sharded_device``): every
rank rolls out its slice of the candidates from the controller's hidden state, every iteration's returns are gathered by the int64
MAX all-reduce of ``m * n + 3`` words, and - every rank then holding every sample row and every return - the pick and the state
advance are local and identical on all ranks.

The ranks run one after another on ONE GPU through the sequential loopback world (tests/loopback_world.py), a fresh controller per
(pass, rank), as in tests/test_sharded_cem_step_gpu.py.  A *tainted* pass - a rank whose collective is not fully known yet gets its
own words back - sees holes and fails with ``L2AError``; the programs tolerate that only while ``comm.tainted``.  Everything is
compared bit for bit against the unsharded recurrent ``NativeCemStep`` (or the one-process controller) under the same seed.

``ant_rnn_cem_gru2x256_n200_h4_m2`` is left out on purpose: its shard widths may cross the kernel boundary that ``l2a_set_micro``
documents as tolerance-only.  Not covered here: RCCL with more than one rank, and timing."""

import numpy as np
import pytest
import torch

import cases
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.policies.mpc_controller import MPCController
from learning_to_adapt_amd.policies.native_cem_step import NativeCemStep
from loopback_world import LoopbackWorld

DIGEST_MASK = 0x7FFFFFFFFFFF

pytestmark = pytest.mark.gpu


def _shard(n, rank, world):
    return MPCController._shard_range(n, rank, world)


def _restore_context(ctx):
    """What a rank that owns its process would find: the context's default policies, no degradation, a clear status word."""
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


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


class _Setup(object):
    """A recurrent CEM golden case as direct ``NativeCemStep`` plans.  The state a step starts from is fixed up front and is the
    same for every rank and for the unsharded run: random rows for step 0, the unsharded run's advanced state after that."""

    def __init__(self, name, cem_mode, n=None, iters=None, num_elites=None):
        self.case = dict(cases.CASES[name])
        gold = cases.load_golden(name + "_s0")
        self.env, self.model = cases.product_rnn_model(self.case)
        self.native = self.model.planner_model()
        ctrl = cases.product_rnn_controller(self.case, model=self.model, env=self.env, rng="device", cem_mode=cem_mode)
        self.n = self.case["n"] if n is None else n
        self.m, self.h = self.case["m"], self.case["h"]
        self.iters = self.case["num_cem_iters"] if iters is None else iters
        self.num_elites = max(int(self.n * ctrl.percent_elites), 1) if num_elites is None else num_elites
        self.alpha, self.reward, self.discount = ctrl.alpha, ctrl._reward_spec, self.case.get("discount", 1.0)
        self.reference = cem_mode == "reference"
        self.dev = self.native.device
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.obs = [gold["obs"][0], gold["obs"][1]]
        rs = np.random.RandomState(12)
        U = self.native.units
        self.c0 = torch.from_numpy((0.1 * rs.randn(self.m, U)).astype(np.float32)).to(self.dev)
        self.h0 = torch.from_numpy(np.tanh(0.1 * rs.randn(self.m, U)).astype(np.float32)).to(self.dev)
        self.states = None          # per step: (c, h) the step starts from - set by `unsharded`

    def controller(self, seed, shard=None):
        return NativeCemStep(self.native, self.m, self.n, self.h, self.env.action_space.low, self.env.action_space.high, self.discount,
                             self.reward, self.iters, self.num_elites, self.alpha, self.reference, seed, shard=shard)

    def step(self, st, k, c_in=None, h_in=None):
        """Step `k` from its fixed start state into fresh output buffers; returns the snapshot."""
        c_in, h_in = self.states[k] if c_in is None else (c_in, h_in)
        c1, h1 = torch.full_like(c_in, 3.0), torch.full_like(h_in, 3.0)
        rc = st.step(self.obs[k], self.stream, (c_in.data_ptr(), h_in.data_ptr(), c1.data_ptr(), h1.data_ptr()))
        mean, std, rets = st.result()
        torch.cuda.synchronize()
        return dict(rc=rc, act=st.act.copy(), idx=st.idx.copy(), ret=st.ret.copy(), mean=mean, std=std, rets=rets,
                    c=c1.cpu().numpy(), h=h1.cpu().numpy(), c_dev=c1, h_dev=h1)

    def unsharded(self, seed, steps):
        st = self.controller(seed)
        try:
            outs, c, h = [], self.c0, self.h0
            self.states = []
            for k in range(steps):
                self.states.append((c, h))
                outs.append(self.step(st, k, c, h))
                c, h = outs[-1]["c_dev"], outs[-1]["h_dev"]
            return outs
        finally:
            st.close()


def _same_step(got, want, where):
    assert got["act"].dtype == np.float64 and _bits(got["act"]) == _bits(want["act"]), where
    assert np.array_equal(got["idx"], want["idx"]), where
    assert _bits(got["ret"]) == _bits(want["ret"]), where
    assert _bits(got["mean"]) == _bits(want["mean"]) and _bits(got["std"]) == _bits(want["std"]), where
    assert got["rets"].shape == want["rets"].shape
    for it in range(want["rets"].shape[0]):                              # EVERY iteration's gathered [m, n] table
        assert _bits(got["rets"][it]) == _bits(want["rets"][it]), "%s, iteration %d" % (where, it)
    assert _bits(got["c"]) == _bits(want["c"]) and _bits(got["h"]) == _bits(want["h"]), where      # the advanced state
    assert np.isfinite(got["c"]).all() and not (got["c"] == 3.0).all(), where


def _run_world(ctx, setup, world_size, seed, steps=1, inject_on=None, seeds=None):
    """`steps` consecutive steps of `world_size` sharded controllers, one fresh controller per (pass, rank).  `seeds`: per rank,
    the seed of the FIRST controller of that rank (a rank whose seed differs is rebuilt with `seed` after its first step failed)."""
    def reset(rank):
        _restore_context(ctx)

    def program(rank, comm):
        st = setup.controller(seed if seeds is None else seeds[rank], shard=(rank, world_size, comm.reduce))
        outs = []
        try:
            for k in range(steps):
                if rank == inject_on and k == 0:
                    ctx.check(ctx.lib.l2a_inject_status(ctx.handle, 1), "l2a_inject_status")
                try:
                    out = setup.step(st, sum(1 for o in outs if "rc" in o))      # (a refused step is repeated)
                except _lib.L2AError as exc:
                    if comm.tainted:
                        return None                                      # holes: the rank got its own words back
                    if seeds is None or k > 0:
                        raise
                    outs.append(dict(error=str(exc)))
                    if seeds[rank] != seed:                              # the odd rank: rebuilt like the others
                        st.close()
                        st = setup.controller(seed, shard=(rank, world_size, comm.reduce))
                    continue
                out.update(stats=st.stats(), degraded=bool(ctx.split_degraded), status=ctx.launch_status_value(),
                           collectives=comm.calls)
                outs.append(out)
            return outs
        finally:
            st.close()

    world = LoopbackWorld(world_size, reset=reset, max_collectives=64)
    return world, world.run(program)


@pytest.mark.parametrize("name,world_size", [("hc_rnn_cem_n200_h5_m2", 2), ("hc_rnn_cem_n200_h5_m2", 3), ("hc_rnn_cem_n200_h5_m2", 8),
                                             ("ant_rnn_cem_gru2_n60_h3", 2), ("ant_rnn_cem_gru2_n60_h3", 8)])
def test_sharded_recurrent_cem_step_equals_the_unsharded_one(name, world_size, ctx):
    """Two consecutive steps on every rank (3 ranks: uneven shards): action, index, return, final mean / std, the gathered
    [iters, m, n] returns and c_next / h_next are the unsharded C controller's; `iters` collectives of m * n + 3 words per step."""
    setup = _Setup(name, "reference")
    wants = setup.unsharded(4242, 2)
    assert _bits(wants[0]["rets"]) != _bits(wants[1]["rets"])
    world, outs = _run_world(ctx, setup, world_size, 4242, steps=2)
    iters, mn = setup.iters, setup.m * setup.n
    assert world.passes == 2 * iters + 1 and world.calls == [2 * iters] * world_size
    assert [c["kind"] for c in world.collectives] == ["reduce"] * (2 * iters)
    for col in world.collectives:
        assert all(p.dtype == np.int64 and p.shape == (mn + 3,) for p in col["parts"])
        assert all(int(p[mn]) == 0 and int(p[mn + 1]) + int(p[mn + 2]) == DIGEST_MASK for p in col["parts"])
    for rank, out in enumerate(outs):
        for k in range(2):
            assert out[k]["rc"] == _lib.L2A_OK, (rank, k)
            _same_step(out[k], wants[k], "rank %d, step %d" % (rank, k))
            assert out[k]["collectives"] == (k + 1) * iters
        assert out[1]["stats"]["steps"] == 2 and out[1]["stats"]["relaunches"] == 0 and not out[1]["degraded"]


def test_a_rank_with_an_empty_shard_still_plans_and_advances(ctx):
    """n = 5 candidates over 8 ranks: the three ranks with lo == hi skip the rollout, still pack, reduce, refit, pick and advance -
    and return the unsharded result and state like every other rank."""
    setup = _Setup("ant_rnn_cem_gru2_n60_h3", "fixed", n=5, iters=2, num_elites=1)
    widths = [_shard(5, r, 8)[1] - _shard(5, r, 8)[0] for r in range(8)]
    assert sorted(widths) == [0, 0, 0, 1, 1, 1, 1, 1]
    want = setup.unsharded(9, 1)[0]
    world, outs = _run_world(ctx, setup, 8, 9)
    assert world.calls == [2] * 8 and world.passes == 3
    for rank, out in enumerate(outs):
        assert out[0]["rc"] == _lib.L2A_OK, rank
        _same_step(out[0], want, "rank %d (%d candidates)" % (rank, widths[rank]))


def test_one_flagged_rank_of_four_makes_every_rank_repeat_the_step_unsplit(ctx):
    """ONE rank's status word is set: the reduced flag makes all ranks repeat the whole step unsplit, the advance included - 2 x iters
    collectives, L2A_STEP_UNSPLIT, one relaunch, the unflagged result and state."""
    setup = _Setup("hc_rnn_cem_n200_h5_m2", "reference")
    world_size, flagged = 4, 2
    want = setup.unsharded(77, 1)[0]
    world, outs = _run_world(ctx, setup, world_size, 77, inject_on=flagged)
    iters, mn = setup.iters, setup.m * setup.n
    assert world.calls == [2 * iters] * world_size and world.passes == 2 * iters + 1
    for k in range(iters):                                               # the first attempt: only the flagged rank raised the flag ...
        assert [int(p[mn]) for p in world.collectives[k]["parts"]] == [1 if r == flagged else 0 for r in range(world_size)]
        assert int(world.result(k)[mn]) == 1                             # ... and every rank saw it
    for k in range(iters, 2 * iters):
        assert not any(int(p[mn]) for p in world.collectives[k]["parts"])
        assert all(np.array_equal(a[:mn], b[:mn]) for a, b in zip(world.collectives[k]["parts"], world.collectives[k - iters]["parts"]))
    for rank, out in enumerate(outs):
        assert out[0]["rc"] == _lib.L2A_STEP_UNSPLIT, rank
        assert out[0]["stats"]["relaunches"] == 1 and out[0]["stats"]["steps"] == 1, rank
        assert out[0]["degraded"] and out[0]["status"] == 0, rank
        _same_step(out[0], want, "rank %d" % rank)
    _restore_context(ctx)


def test_a_rank_built_with_another_seed_fails_every_rank_and_consumes_nothing(ctx):
    """Digests that differ fail the step with L2A_ESTATE on EVERY rank; the stream position does not advance: the following step -
    the odd rank rebuilt with the right seed - reproduces step 1 of the unsharded run."""
    setup = _Setup("ant_rnn_cem_gru2_n60_h3", "fixed")
    world_size, odd = 3, 1
    want = setup.unsharded(55, 1)[0]
    seeds = [56 if r == odd else 55 for r in range(world_size)]
    world, outs = _run_world(ctx, setup, world_size, 55, steps=2, seeds=seeds)
    assert world.calls == [2 * setup.iters] * world_size
    mn = setup.m * setup.n
    first = world.collectives[0]["parts"]
    assert len(set(int(p[mn + 1]) for p in first)) == 2                  # two different digests met ...
    assert int(world.result(0)[mn + 1]) + int(world.result(0)[mn + 2]) != DIGEST_MASK
    for rank, out in enumerate(outs):
        assert "(-4)" in out[0]["error"] and "digests differ" in out[0]["error"], (rank, out[0])     # L2A_ESTATE, on every rank
        assert out[1]["rc"] == _lib.L2A_OK
        _same_step(out[1], want, "rank %d" % rank)
        assert out[1]["stats"]["steps"] == 1


def _flat(hidden):
    if isinstance(hidden, (list, tuple)):
        return [a for part in hidden for a in _flat(part)]
    return [np.asarray(hidden)]


def test_rnn_mpc_controller_builds_and_steps_the_sharded_cem_controller(ctx):
    """`RNNMPCController(use_cem=True, rng="device", native_cem_step=True)` on four loopback ranks: `_cemstep` serves the call (its
    dry run of the collective is one more reduce, of zeros), `last_plan["shard"]` is the rank's range, and actions and hidden state
    equal the one-process controller's."""
    name = "hc_rnn_cem_n200_h5_m2"
    case = dict(cases.CASES[name])
    obs = cases.load_golden(name + "_s0")["obs"][0]
    env, model = cases.product_rnn_model(case)
    torch_seed, world_size = 4242, 4
    ref = cases.product_rnn_controller(case, model=model, env=env, rng="device")
    torch.manual_seed(torch_seed)
    want_act, _ = ref.get_actions(obs)
    want = dict(ref.last_plan)
    want_hidden = [a.copy() for a in _flat(ref._hidden_state)]
    assert ref._cemstep is None

    def reset(rank):
        torch.manual_seed(torch_seed)
        _restore_context(ctx)

    def program(rank, comm):
        ctrl = comm.install(cases.product_rnn_controller(case, model=model, env=env, rng="device", native_cem_step=True))
        try:
            try:
                act, _ = ctrl.get_actions(obs)
            except _lib.L2AError:
                if comm.tainted:
                    return None
                raise
            st = ctrl._cemstep
            assert st is not None and st.steps == 1 and st.shard == (rank, world_size)
            plan = ctrl.last_plan
            return dict(act=act.copy(), idx=np.array(plan["best_index"]), ret=np.array(plan["best_return"]), mean=plan["cem_mean"],
                        std=plan["cem_std"], trace=len(plan["cem_trace"]), shard=tuple(plan["shard"]), calls=ctrl._bufs["cem_calls"],
                        hidden=[a.copy() for a in _flat(ctrl._hidden_state)])
        finally:
            if ctrl._cemstep is not None:
                ctrl._cemstep.close()
                ctrl._cemstep = None

    world = LoopbackWorld(world_size, reset=reset)
    outs = world.run(program)
    iters, mn = case["num_cem_iters"], case["m"] * case["n"]
    assert world.passes == iters + 2 and world.calls == [iters + 1] * world_size
    assert all(c["kind"] == "reduce" and all(p.shape == (mn + 3,) for p in c["parts"]) for c in world.collectives)
    assert not np.stack(world.collectives[0]["parts"]).any()             # the dry run
    for rank, out in enumerate(outs):
        assert _bits(out["act"]) == _bits(want_act), rank
        assert np.array_equal(out["idx"], want["best_index"]), rank
        assert _bits(np.asarray(out["ret"], dtype=np.float32)) == _bits(np.asarray(want["best_return"], dtype=np.float32)), rank
        assert _bits(out["mean"]) == _bits(want["cem_mean"]) and _bits(out["std"]) == _bits(want["cem_std"]), rank
        assert out["trace"] == iters and out["shard"] == _shard(case["n"], rank, world_size) and out["calls"] == iters, rank
        assert len(out["hidden"]) == len(want_hidden)
        assert all(_bits(g) == _bits(w) for g, w in zip(out["hidden"], want_hidden)), rank
