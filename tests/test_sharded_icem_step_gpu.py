"""The sharded iCEM plan step as ONE C call (``l2a_icem_controller_create_sharded_device``): every rank samples all candidates of
the same stream (``l2a_icem_sample_shard``), rolls out its window of the iteration's population, and every iteration's returns are
gathered by the plan's one collective kind - the int64 MAX all-reduce of ``m * pops[it] + 3`` words (``l2a_cem_shard_pack`` /
``_unpack``) - in front of the unchanged refit over all ``pops[it]``.  The window moves with the population.

As in ``tests/test_sharded_mppi_step_gpu.py`` the ranks run one after another on ONE GPU through the sequential loopback world
(``tests/loopback_world.py``), a fresh controller per (pass, rank); a *tainted* pass - a rank whose collective is not fully known
yet gets its own words back - sees holes and fails with ``L2AError``, which the programs tolerate only while ``comm.tainted``.
Two consecutive steps of ``iters`` iterations each: ``2 * iters + 1`` passes.  Everything is compared bit for bit with the
unsharded ``NativeIcemStep`` under the same seed (which ``tests/test_icem_step_gpu.py`` holds to the Python loop).

Not covered here: RCCL with more than one rank, and timing."""

import os
import socket
import sys

import numpy as np
import pytest
import torch

from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.policies.mpc_controller import MPCController
from loopback_world import LoopbackWorld
from icem_step_cases import Setup, bits, restore_context, same_snapshot

HERE = os.path.dirname(os.path.abspath(__file__))
DIGEST_MASK = 0x7FFFFFFFFFFF
PRESENT = 1 << 32

pytestmark = pytest.mark.gpu


def _shard(n, rank, world):
    return MPCController._shard_range(n, rank, world)


@pytest.fixture
def ctx():
    c = _lib.Context.get(0)
    torch.cuda.synchronize()
    c.launch_status_value()         # (whatever an earlier test file left behind)
    restore_context(c)
    yield c
    torch.cuda.synchronize()
    c.launch_status_value()
    restore_context(c)


def _unsharded(setup, seed, steps, resets=None, **over):
    st = setup.controller(seed, **over)
    try:
        outs = []
        for k in range(steps):
            if resets and k in resets:
                st.reset(resets[k])
            outs.append(setup.snapshot(st, st.step(setup.obs[k], setup.stream)))
        return outs
    finally:
        st.close()


def _run_world(ctx, setup, world_size, seed, steps=2, inject_on=None, first=None, resets=None, reduce_of=None, **over):
    """`steps` consecutive steps of `world_size` sharded controllers, one fresh controller per (pass, rank).  `first(rank)`: create
    arguments of the FIRST controller of that rank that differ from the others' (`seed=` among them) - a rank whose first step was
    refused is rebuilt like the others.  `resets[k](rank)`: the `dones` a rank applies in front of step `k`.  `reduce_of(comm)`: the
    odd controller's reduce function (default: `comm.reduce`).  A refused step is recorded (`error`) and repeated."""
    def reset(rank):
        restore_context(ctx)

    def build(rank, comm, odd):
        args = dict(over)
        if odd:
            args.update(first(rank))
        reduce = reduce_of(comm) if odd and reduce_of is not None else comm.reduce
        return setup.controller(args.pop("seed", seed), shard=(rank, world_size, reduce), **args)

    def program(rank, comm):
        odd = first is not None and bool(first(rank))
        st = build(rank, comm, odd)
        outs = []
        try:
            for attempt in range(steps + 1):
                k = sum(1 for o in outs if "rc" in o)
                if k == steps:
                    break
                if resets and k in resets and not any("error" in o for o in outs):
                    st.reset(resets[k](rank))
                if rank == inject_on and attempt == 0:
                    ctx.check(ctx.lib.l2a_inject_status(ctx.handle, 1), "l2a_inject_status")
                try:
                    rc = st.step(setup.obs[k], setup.stream)
                except _lib.L2AError as exc:
                    if comm.tainted:
                        return None                                      # holes: the rank got its own words back
                    if any("error" in o for o in outs):
                        raise
                    outs.append(dict(error=str(exc), stats=st.stats()))
                    if odd:                                              # the odd rank: rebuilt like the others
                        st.close()
                        st = build(rank, comm, False)
                    elif resets:
                        return outs                                      # (ranks that disagree on their resets stay refused)
                    continue
                out = setup.snapshot(st, rc)
                torch.cuda.synchronize()
                out.update(stats=st.stats(), degraded=bool(ctx.split_degraded), status=ctx.launch_status_value(), collectives=comm.calls)
                outs.append(out)
            return outs
        finally:
            st.close()

    world = LoopbackWorld(world_size, reset=reset, max_collectives=24)
    return world, world.run(program)


def _assert_collectives(world, m, pops, world_size, wants):
    """Collective `step * iters + it` is a reduce of m * pops[it] + 3 int64 words; rank r's contribution holds exactly the words of
    its window of that iteration's population in the unsharded run's table, a clear flag and the shared digest pair."""
    iters = len(pops)
    assert [c["kind"] for c in world.collectives] == ["reduce"] * (len(wants) * iters)
    for k, col in enumerate(world.collectives):
        step, it = divmod(k, iters)
        n = pops[it]
        table = wants[step]["rets"][it]
        want = (np.ascontiguousarray(table, dtype=np.float32).view(np.uint32).astype(np.int64) | PRESENT).reshape(m, n)
        parts = col["parts"]
        for rank, part in enumerate(parts):
            assert part.dtype == np.int64 and part.shape == (m * n + 3,), (k, rank)
            lo, hi = _shard(n, rank, world_size)
            mine = np.zeros((m, n), dtype=np.int64)
            mine[:, lo:hi] = want[:, lo:hi]
            assert np.array_equal(part[:m * n].reshape(m, n), mine), (k, rank)
            assert int(part[m * n]) == 0 and int(part[m * n + 1]) + int(part[m * n + 2]) == DIGEST_MASK, (k, rank)
            assert np.array_equal(part[m * n + 1:], parts[0][m * n + 1:]), (k, rank)


@pytest.mark.parametrize("world_size,n", [(2, None), (3, None), (8, 7)], ids=["world2", "world3_uneven", "world8_of_7_empty_windows"])
def test_every_rank_equals_the_unsharded_step_over_two_steps(world_size, n, ctx):
    setup = Setup("mlp") if n is None else Setup("mlp", n=n, icem_keep=1.0, icem_iters=2)
    K, Kk, pops = setup.sizes()
    widths = [[_shard(p, r, world_size)[1] - _shard(p, r, world_size)[0] for r in range(world_size)] for p in pops]
    if world_size == 3:
        assert pops == [64, 51, 40] and widths == [[21, 21, 22], [17, 17, 17], [13, 13, 14]]
    if world_size == 8:
        assert (pops, K, Kk) == ([7, 5], 1, 1) and widths[0].count(0) == 1 and widths[1].count(0) == 3
    wants = _unsharded(setup, 31, 2)
    assert bits(wants[0]["mean"]) != bits(wants[1]["mean"]) and bits(wants[0]["kept"]) != bits(wants[1]["kept"])
    world, outs = _run_world(ctx, setup, world_size, 31)
    iters = len(pops)
    assert world.passes == 2 * iters + 1 and world.calls == [2 * iters] * world_size
    _assert_collectives(world, setup.m, pops, world_size, wants)
    for rank, out in enumerate(outs):
        for k in range(2):
            assert out[k]["rc"] == _lib.L2A_OK, (rank, k)
            same_snapshot(out[k], wants[k], "rank %d, step %d" % (rank, k))
        assert out[1]["stats"]["steps"] == 2 and out[1]["stats"]["relaunches"] == 0 and not out[1]["degraded"]


def test_one_flagged_rank_makes_every_rank_repeat_the_step_unsplit(ctx):
    setup = Setup("mlp")
    pops = setup.sizes()[2]
    iters = len(pops)
    world_size, flagged = 3, 1
    wants = _unsharded(setup, 77, 2)
    world, outs = _run_world(ctx, setup, world_size, 77, inject_on=flagged)
    assert world.calls == [3 * iters] * world_size and world.passes == 3 * iters + 1      # step 0 twice, step 1 once
    mn = setup.m * pops[0]
    assert [int(p[mn]) for p in world.collectives[0]["parts"]] == [1 if r == flagged else 0 for r in range(world_size)]
    assert int(world.result(0)[mn]) == 1                                # every rank saw the flag
    for it in range(iters):                                             # the replay: no flag, the same returns
        w = setup.m * pops[it]
        assert not any(int(p[w]) for p in world.collectives[iters + it]["parts"])
        assert all(np.array_equal(a[:w], b[:w]) for a, b in zip(world.collectives[it]["parts"], world.collectives[iters + it]["parts"]))
    for rank, out in enumerate(outs):
        assert [o["rc"] for o in out] == [_lib.L2A_STEP_UNSPLIT, _lib.L2A_OK], rank
        assert out[0]["stats"]["relaunches"] == 1 and out[0]["stats"]["steps"] == 1 and out[1]["stats"]["steps"] == 2, rank
        assert out[0]["degraded"] and out[0]["status"] == 0, rank
        for k in range(2):                                              # the replay started from the same state, the stream moved once
            same_snapshot(out[k], wants[k], "rank %d, step %d" % (rank, k))


def _resized_reduce(comm, m, mine, theirs):
    """The odd rank of the `pops` case plans the last iteration on `mine` candidates where the others plan on `theirs`: its
    collective would have another length, which no backend (and not the loopback world) reduces.  So that the DIGEST can be seen to
    refuse the step, this reduce presents the odd rank's words in the others' length - the returns zero-padded or cut, the flag and
    the digest pair at the end - and hands the reduced ones back the same way."""
    def reduce(payload):
        if payload.numel() != m * mine + 3:
            return comm.reduce(payload)
        body = min(mine, theirs) * m
        wide = torch.zeros((m * theirs + 3,), dtype=torch.int64, device=payload.device)
        wide[:body] = payload[:body]
        wide[-3:] = payload[-3:]
        comm.reduce(wide)
        payload[:body] = wide[:body]
        payload[-3:] = wide[-3:]
    return reduce


@pytest.mark.parametrize("what", ["seed", "rho", "pops"])
def test_a_rank_built_differently_fails_every_rank_and_consumes_nothing(what, ctx):
    """Digests that differ fail the step with L2A_ESTATE on EVERY rank; neither the stream position nor the state nor the reset
    marks move: the following step - the odd rank rebuilt like the others - reproduces step 0 of the unsharded run."""
    setup = Setup("mlp")
    pops = setup.sizes()[2]
    iters = len(pops)
    world_size, odd = 3, 1
    wants = _unsharded(setup, 55, 1)
    other = dict(seed=dict(seed=56), rho=dict(rho=0.25), pops=dict(pops=pops[:-1] + [pops[-1] - 1]))[what]
    reduce_of = (lambda comm: _resized_reduce(comm, setup.m, pops[-1] - 1, pops[-1])) if what == "pops" else None
    world, outs = _run_world(ctx, setup, world_size, 55, steps=1, first=lambda rank: other if rank == odd else {}, reduce_of=reduce_of)
    assert world.calls == [2 * iters] * world_size
    mn = setup.m * pops[0]
    assert len(set(int(p[mn + 1]) for p in world.collectives[0]["parts"])) == 2          # two different digests met ...
    assert int(world.result(0)[mn + 1]) + int(world.result(0)[mn + 2]) != DIGEST_MASK
    for rank, out in enumerate(outs):
        assert "(-4)" in out[0]["error"] and "digests differ" in out[0]["error"], (rank, out[0])     # L2A_ESTATE, on every rank
        assert out[0]["stats"]["steps"] == 0
        assert out[1]["rc"] == _lib.L2A_OK and out[1]["stats"]["steps"] == 1
        same_snapshot(out[1], wants[0], "rank %d" % rank)


def test_a_rank_that_reset_another_env_fails_every_rank(ctx):
    """After a common first step rank 1 resets env 1 and the others env 0: they would sample around different plans."""
    setup = Setup("mlp")
    iters = len(setup.sizes()[2])
    world_size, odd = 3, 1
    wants = _unsharded(setup, 55, 1)
    dones = lambda rank: [rank != odd, rank == odd, False]              # noqa: E731
    world, outs = _run_world(ctx, setup, world_size, 55, resets={1: dones})
    assert world.calls == [2 * iters] * world_size and world.passes == 2 * iters + 1
    for rank, out in enumerate(outs):
        assert len(out) == 2 and out[0]["rc"] == _lib.L2A_OK
        same_snapshot(out[0], wants[0], "rank %d" % rank)
        assert "(-4)" in out[1]["error"] and "digests differ" in out[1]["error"], (rank, out[1])
        assert out[1]["stats"]["steps"] == 1
    # the same reset on every rank is fine, and equals the unsharded controller's
    same = lambda rank: [True, False, False]                            # noqa: E731
    wants = _unsharded(setup, 55, 2, resets={1: same(0)})
    world, outs = _run_world(ctx, setup, 2, 55, resets={1: same})
    for rank, out in enumerate(outs):
        for k in range(2):
            same_snapshot(out[k], wants[k], "rank %d, step %d" % (rank, k))


def test_sharded_icem_controller_without_a_collective_is_refused(ctx):
    setup = Setup("mlp")
    with pytest.raises(_lib.L2AError, match="no reduce function and no communicator"):
        setup.controller(13, shard=(0, 2, None))
    with pytest.raises(_lib.L2AError, match="bad rank / world"):
        setup.controller(13, shard=(2, 2, lambda payload: None))


def _plan_arrays(plan):
    """`last_plan` as a flat dict of arrays (the trace's entries by iteration)."""
    flat = {k: np.asarray(v) for k, v in plan.items() if k not in ("icem_trace", "shard")}
    for it, step in enumerate(plan["icem_trace"]):
        for key, v in step.items():
            flat["trace%d_%s" % (it, key)] = np.asarray(v)
    return flat


def test_mpc_controller_builds_and_steps_the_sharded_controller(ctx):
    """`MPCController(use_icem=True, native_icem_step=True)` on three loopback ranks: `_icemstep` serves the calls (its dry run of
    the collective is one more reduce, of zeros) and two steps equal ONE process's Python loop; with the keyword on and a C
    controller that does not apply, or with the keyword off, the "shard" error is raised."""
    setup = Setup("mlp")
    pops = setup.sizes()[2]
    iters = len(pops)
    want = setup.python_steps(4242, 2)
    world_size = 3

    def reset(rank):
        torch.manual_seed(4242)
        restore_context(ctx)

    def program(rank, comm):
        ctrl = comm.install(setup.python(native_icem_step=True))
        outs = []
        try:
            for k in range(2):
                try:
                    act, _ = ctrl.get_actions(setup.obs[k])
                except _lib.L2AError:
                    if comm.tainted:
                        return None
                    raise
                st = ctrl._icemstep
                assert st is not None and st.steps == k + 1 and st.shard == (rank, world_size)
                outs.append(dict(act=act.copy(), plan=dict(ctrl.last_plan)))
            return outs
        finally:
            if ctrl._icemstep is not None:
                ctrl._icemstep.close()
                ctrl._icemstep = None

    world = LoopbackWorld(world_size, reset=reset)
    outs = world.run(program)
    assert world.passes == 2 * iters + 2 and world.calls == [2 * iters + 1] * world_size
    sizes = [setup.m * setup.n + 3] + [setup.m * p + 3 for p in pops] * 2
    assert [c["kind"] for c in world.collectives] == ["reduce"] * len(sizes)
    assert all(p.shape == (w,) for c, w in zip(world.collectives, sizes) for p in c["parts"])
    assert not np.stack(world.collectives[0]["parts"]).any()             # the dry run
    for rank, out in enumerate(outs):
        for k in range(2):
            assert bits(out[k]["act"]) == bits(want[k]["act"]), (rank, k)
            plan = out[k]["plan"]
            assert [tuple(w) for w in plan["shard"]] == [_shard(p, rank, world_size) for p in pops]
            got, ref = _plan_arrays(plan), _plan_arrays(want[k]["plan"])
            assert set(got) == set(ref)
            for key, v in ref.items():
                assert got[key].dtype == v.dtype and bits(got[key]) == bits(v), (rank, k, key)
    # the keyword on, world > 1, a C controller that does not apply (a replaced normal hook): the "shard" error
    ctrl = setup.python(native_icem_step=True)
    ctrl._dist = lambda: (0, 2)
    ctrl._icem_normal_device = lambda shape, device: None
    with pytest.raises(_lib.L2AError, match="shard"):
        ctrl.get_actions(setup.obs[0])
    assert ctrl._icemstep is None
    ctrl = setup.python()
    ctrl._dist = lambda: (0, 2)
    with pytest.raises(_lib.L2AError, match="native_icem_step=True"):
        ctrl.get_actions(setup.obs[0])


# ---- two real gloo ranks on one GPU ------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker_gloo(rank, world, port, out_dir):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["L2A_SPLIT"] = "0"           # ranks sharing one GPU: a tile's two workgroups may not be co-resident
    import datetime
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    try:
        import icem_step_cases as isc
        setup = isc.Setup("mlp")
        torch.manual_seed(99)
        ctrl = setup.python(native_icem_step=True)
        out = {}
        for k in range(2):
            act, _ = ctrl.get_actions(setup.obs[k])
            assert ctrl._icemstep is not None and ctrl._icemstep.steps == k + 1 and ctrl._icemstep.shard == (rank, world)
            out["act_%d" % k] = act
            for key, v in _plan_arrays(ctrl.last_plan).items():
                out["%s_%d" % (key, k)] = v
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_on_one_gpu_reproduce_the_unsharded_step(tmp_path):
    """Real processes and a real collective (gloo behind `_reduce_payload`; tile split off, as processes that share a GPU need):
    both ranks reproduce ONE process's unsharded C step, two steps running."""
    import torch.multiprocessing as mp
    world = 2
    ctx_mp = mp.spawn(_worker_gloo, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=False)
    deadline = 240.0
    import time
    t0 = time.time()
    while not ctx_mp.join(timeout=5.0):
        if time.time() - t0 > deadline:
            for p in ctx_mp.processes:
                p.terminate()
            pytest.fail("the gloo ranks did not finish within %d s" % deadline)
    setup = Setup("mlp")
    torch.manual_seed(99)
    ref = setup.python(native_icem_step=True)
    outs = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    try:
        for k in range(2):
            want_act, _ = ref.get_actions(setup.obs[k])
            assert ref._icemstep is not None and ref._icemstep.shard is None
            want = _plan_arrays(ref.last_plan)
            for rank, o in enumerate(outs):
                assert bits(o["act_%d" % k]) == bits(want_act), (rank, k)
                for key, v in want.items():
                    got = o["%s_%d" % (key, k)]
                    assert got.dtype == v.dtype and got.shape == v.shape and bits(got) == bits(v), (rank, k, key)
    finally:
        ref._icemstep.close()
        ref._icemstep = None
