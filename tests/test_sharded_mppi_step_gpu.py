"""The sharded MPPI plan step as ONE C call (``l2a_mppi_controller_create_sharded_device``): every rank samples all candidates of
the same stream (``l2a_mppi_sample_shard``), rolls out its window, and every iteration's returns are gathered by the plan's one
collective kind - the int64 MAX all-reduce of ``m * n + 3`` words (``l2a_cem_shard_pack`` / ``_unpack``) - in front of the unchanged
update over all ``n``.

As in ``tests/test_sharded_cem_step_gpu.py`` the ranks run one after another on ONE GPU through the sequential loopback world
(``tests/loopback_world.py``), a fresh controller per (pass, rank); a *tainted* pass - a rank whose collective is not fully known
yet gets its own words back - sees holes and fails with ``L2AError``, which the programs tolerate only while ``comm.tainted``.
Two consecutive steps of one iteration each: three passes.  Everything is compared bit for bit with the unsharded
``NativeMppiStep`` under the same seed (which ``tests/test_mppi_step_gpu.py`` holds to the Python loop).

Not covered here: RCCL with more than one rank, and timing."""

import os
import socket
import sys

import numpy as np
import pytest
import torch

import cases
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.policies.mpc_controller import MPCController
from loopback_world import LoopbackWorld
from mppi_step_cases import Setup, bits, restore_context, same_snapshot, same_step

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


def _run_world(ctx, setup, world_size, seed, steps=2, inject_on=None, first=None, resets=None, **over):
    """`steps` consecutive steps of `world_size` sharded controllers, one fresh controller per (pass, rank).  `first(rank)`: create
    arguments of the FIRST controller of that rank that differ from the others' (`seed=` among them) - a rank whose first step was
    refused is rebuilt like the others.  `resets[k](rank)`: the `dones` a rank applies in front of step `k`.  A refused step is
    recorded (`error`) and repeated."""
    def reset(rank):
        restore_context(ctx)

    def build(rank, comm, odd):
        args = dict(over)
        if odd:
            args.update(first(rank))
        return setup.controller(args.pop("seed", seed), shard=(rank, world_size, comm.reduce), **args)

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

    world = LoopbackWorld(world_size, reset=reset, max_collectives=16)
    return world, world.run(program)


def _assert_collectives(world, m, n, world_size, tables):
    """Every collective is a reduce of m * n + 3 int64 words; rank r's contribution holds exactly the words of its window of the
    unsharded run's table, a clear flag and the shared digest pair."""
    assert [c["kind"] for c in world.collectives] == ["reduce"] * len(tables)
    for k, table in enumerate(tables):
        want = (np.ascontiguousarray(table, dtype=np.float32).view(np.uint32).astype(np.int64) | PRESENT).reshape(m, n)
        parts = world.collectives[k]["parts"]
        for rank, part in enumerate(parts):
            assert part.dtype == np.int64 and part.shape == (m * n + 3,), (k, rank)
            lo, hi = _shard(n, rank, world_size)
            mine = np.zeros((m, n), dtype=np.int64)
            mine[:, lo:hi] = want[:, lo:hi]
            assert np.array_equal(part[:m * n].reshape(m, n), mine), (k, rank)
            assert int(part[m * n]) == 0 and int(part[m * n + 1]) + int(part[m * n + 2]) == DIGEST_MASK, (k, rank)
            assert np.array_equal(part[m * n + 1:], parts[0][m * n + 1:]), (k, rank)


@pytest.mark.parametrize("world_size,n", [(2, None), (3, None), (8, 7)], ids=["world2", "world3_uneven", "world8_of_7_empty_shard"])
def test_every_rank_equals_the_unsharded_step_over_two_steps(world_size, n, ctx):
    setup = Setup("mlp")
    over = {} if n is None else dict(n=n)
    n = setup.n if n is None else n
    widths = [_shard(n, r, world_size)[1] - _shard(n, r, world_size)[0] for r in range(world_size)]
    if world_size == 3:
        assert widths == [21, 21, 22]
    if world_size == 8:
        assert widths.count(0) == 1 and sum(widths) == 7
    wants = _unsharded(setup, 31, 2, **over)
    assert bits(wants[0]["rets"]) != bits(wants[1]["rets"]) and bits(wants[0]["mean"]) != bits(wants[1]["mean"])
    world, outs = _run_world(ctx, setup, world_size, 31, **over)
    assert world.passes == 3 and world.calls == [2] * world_size
    _assert_collectives(world, setup.m, n, world_size, [w["rets"][0] for w in wants])
    for rank, out in enumerate(outs):
        for k in range(2):
            assert out[k]["rc"] == _lib.L2A_OK, (rank, k)
            same_snapshot(out[k], wants[k], "rank %d, step %d" % (rank, k))
        assert out[1]["stats"]["steps"] == 2 and out[1]["stats"]["relaunches"] == 0 and not out[1]["degraded"]


def test_two_ranks_over_several_passes_equal_the_python_loop_over_two_steps(ctx):
    """h = 90 at A = 6: the SHARD instance of ``l2a_mppi_sample_k`` stores ``seq_local`` of its window in two passes (85 + 5
    steps, the second at step ``t0 + tt`` with the window's row index), and step 1 samples around a mean shifted across the pass
    boundary.  Both loopback ranks against ONE process's Python loop under the same seed, bit for bit."""
    setup = Setup("long", mppi_kappa=0.5)
    assert setup.h == 90 and setup.h > 512 // 6
    want = setup.python_steps(31, 2)
    assert bits(want[0]["plan"]["mppi_mean"]) != bits(want[1]["plan"]["mppi_mean"])
    world, outs = _run_world(ctx, setup, 2, 31)
    assert world.passes == 3 and world.calls == [2, 2]
    _assert_collectives(world, setup.m, setup.n, 2, [w["plan"]["returns"] for w in want])
    for rank, out in enumerate(outs):
        for k in range(2):
            assert out[k]["rc"] == _lib.L2A_OK, (rank, k)
            same_step(out[k], want[k], "long, rank %d, step %d" % (rank, k))
        assert out[1]["stats"]["steps"] == 2 and out[1]["stats"]["relaunches"] == 0 and not out[1]["degraded"]


def test_one_flagged_rank_makes_every_rank_repeat_the_step_unsplit(ctx):
    setup = Setup("mlp")
    world_size, flagged = 3, 1
    wants = _unsharded(setup, 77, 2)
    world, outs = _run_world(ctx, setup, world_size, 77, inject_on=flagged)
    mn = setup.m * setup.n
    assert world.calls == [3] * world_size and world.passes == 4        # step 0 twice, step 1 once
    assert [int(p[mn]) for p in world.collectives[0]["parts"]] == [1 if r == flagged else 0 for r in range(world_size)]
    assert int(world.result(0)[mn]) == 1                                # every rank saw the flag
    assert not any(int(p[mn]) for p in world.collectives[1]["parts"])
    assert all(np.array_equal(a[:mn], b[:mn]) for a, b in zip(world.collectives[0]["parts"], world.collectives[1]["parts"]))
    for rank, out in enumerate(outs):
        assert [o["rc"] for o in out] == [_lib.L2A_STEP_UNSPLIT, _lib.L2A_OK], rank
        assert out[0]["stats"]["relaunches"] == 1 and out[0]["stats"]["steps"] == 1 and out[1]["stats"]["steps"] == 2, rank
        assert out[0]["degraded"] and out[0]["status"] == 0, rank
        for k in range(2):                                              # the replay started from the same mean, the stream moved once
            same_snapshot(out[k], wants[k], "rank %d, step %d" % (rank, k))


@pytest.mark.parametrize("what", ["seed", "kappa"])
def test_a_rank_built_differently_fails_every_rank_and_consumes_nothing(what, ctx):
    """Digests that differ fail the step with L2A_ESTATE on EVERY rank; neither the stream position nor the mean nor the reset marks
    move: the following step - the odd rank rebuilt like the others - reproduces step 0 of the unsharded run."""
    setup = Setup("mlp")
    world_size, odd = 3, 1
    wants = _unsharded(setup, 55, 1)
    other = dict(seed=56) if what == "seed" else dict(kappa=2.0)
    world, outs = _run_world(ctx, setup, world_size, 55, steps=1, first=lambda rank: other if rank == odd else {})
    assert world.calls == [2] * world_size
    mn = setup.m * setup.n
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
    world_size, odd = 3, 1
    wants = _unsharded(setup, 55, 1)
    dones = lambda rank: [rank != odd, rank == odd, False]              # noqa: E731
    world, outs = _run_world(ctx, setup, world_size, 55, resets={1: dones})
    assert world.calls == [2] * world_size and world.passes == 3
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


def test_sharded_mppi_controller_without_a_collective_is_refused(ctx):
    setup = Setup("mlp")
    with pytest.raises(_lib.L2AError, match="no reduce function and no communicator"):
        setup.controller(13, shard=(0, 2, None))
    with pytest.raises(_lib.L2AError, match="bad rank / world"):
        setup.controller(13, shard=(2, 2, lambda payload: None))


def test_mpc_controller_builds_and_steps_the_sharded_controller(ctx):
    """`MPCController(use_mppi=True, native_mppi_step=True)` on three loopback ranks: `_mppistep` serves the calls (its dry run of
    the collective is one more reduce, of zeros) and two steps equal ONE process's Python loop; with the keyword on and a C
    controller that does not apply, the existing "shard" error is raised."""
    setup = Setup("mlp")
    want = setup.python_steps(4242, 2)
    world_size = 3

    def reset(rank):
        torch.manual_seed(4242)
        restore_context(ctx)

    def program(rank, comm):
        ctrl = comm.install(setup.python(native_mppi_step=True))
        outs = []
        try:
            for k in range(2):
                try:
                    act, _ = ctrl.get_actions(setup.obs[k])
                except _lib.L2AError:
                    if comm.tainted:
                        return None
                    raise
                st = ctrl._mppistep
                assert st is not None and st.steps == k + 1 and st.shard == (rank, world_size)
                outs.append(dict(act=act.copy(), plan=dict(ctrl.last_plan)))
            return outs
        finally:
            if ctrl._mppistep is not None:
                ctrl._mppistep.close()
                ctrl._mppistep = None

    world = LoopbackWorld(world_size, reset=reset)
    outs = world.run(program)
    mn = setup.m * setup.n
    assert world.passes == 4 and world.calls == [3] * world_size
    assert all(c["kind"] == "reduce" and all(p.shape == (mn + 3,) for p in c["parts"]) for c in world.collectives)
    assert not np.stack(world.collectives[0]["parts"]).any()             # the dry run
    for rank, out in enumerate(outs):
        for k in range(2):
            assert bits(out[k]["act"]) == bits(want[k]["act"]), (rank, k)
            plan = out[k]["plan"]
            assert tuple(plan.pop("shard")) == _shard(setup.n, rank, world_size)
            assert set(plan) == set(want[k]["plan"])
            for key, ref in want[k]["plan"].items():
                assert plan[key].dtype == ref.dtype and bits(plan[key]) == bits(ref), (rank, k, key)
    # the keyword on, world > 1, a C controller that does not apply (a replaced normal hook): the "shard" error
    ctrl = setup.python(native_mppi_step=True)
    ctrl._dist = lambda: (0, 2)
    ctrl._mppi_normal_device = lambda shape, device: None
    with pytest.raises(_lib.L2AError, match="shard"):
        ctrl.get_actions(setup.obs[0])
    assert ctrl._mppistep is None


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
        import mppi_step_cases as msc
        setup = msc.Setup("mlp")
        torch.manual_seed(99)
        ctrl = setup.python(native_mppi_step=True)
        out = {}
        for k in range(2):
            act, _ = ctrl.get_actions(setup.obs[k])
            assert ctrl._mppistep is not None and ctrl._mppistep.steps == k + 1 and ctrl._mppistep.shard == (rank, world)
            plan = ctrl.last_plan
            out.update({"act_%d" % k: act, "idx_%d" % k: np.asarray(plan["best_index"]), "ret_%d" % k: np.asarray(plan["best_return"]),
                        "mean_%d" % k: plan["mppi_mean"], "ess_%d" % k: plan["mppi_ess"], "valid_%d" % k: plan["mppi_valid"],
                        "rets_%d" % k: plan["returns"]})
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
    ref = setup.python(native_mppi_step=True)
    outs = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    try:
        for k in range(2):
            want_act, _ = ref.get_actions(setup.obs[k])
            plan = ref.last_plan
            assert ref._mppistep is not None and ref._mppistep.shard is None
            for rank, o in enumerate(outs):
                assert bits(o["act_%d" % k]) == bits(want_act), (rank, k)
                assert np.array_equal(o["idx_%d" % k], plan["best_index"]), (rank, k)
                assert bits(o["ret_%d" % k]) == bits(plan["best_return"]), (rank, k)
                assert bits(o["mean_%d" % k]) == bits(plan["mppi_mean"]) and bits(o["ess_%d" % k]) == bits(plan["mppi_ess"]), (rank, k)
                assert np.array_equal(o["valid_%d" % k], plan["mppi_valid"]) and bits(o["rets_%d" % k]) == bits(plan["returns"]), (rank, k)
    finally:
        ref._mppistep.close()
        ref._mppistep = None
