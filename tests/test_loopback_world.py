"""The sequential loopback world (tests/loopback_world.py) itself, on the CPU: pure NumPy rank programs pin its replay rules, and the
controller's real host path (launch replaced by the oracle, as tests/test_distributed_cpu.py does) at world = 8 pins it against
the cases `test_many_rank_plan_equals_single_process_plan` runs on eight gloo processes - the helper reproduces real
`torch.distributed` semantics before tests/test_sharded_emulation_gpu.py trusts it with kernels."""

import numpy as np
import pytest
import torch

import cases
from loopback_world import LoopbackError, LoopbackWorld


def _shard(n, rank, world):
    return (rank * n) // world, ((rank + 1) * n) // world


# ---- pure NumPy rank programs ------------------------------------------------------------------------------------------------------
def test_one_max_reduce_takes_two_passes():
    data = np.random.RandomState(0).randint(-2 ** 40, 2 ** 40, size=(8, 5)).astype(np.int64)
    resets = []
    world = LoopbackWorld(8, reset=resets.append)
    outs = world.run(lambda rank, comm: comm.reduce_max(data[rank]))
    assert world.passes == 2 and world.calls == [1] * 8 and resets == list(range(8)) * 2
    for out in outs:
        assert out.dtype == np.int64 and np.array_equal(out, data.max(axis=0))
    assert np.array_equal(world.result(0), data.max(axis=0))
    # the first pass handed every rank its own words back and recorded them; the second one the true result
    for r in range(8):
        first, second = world.log[(1, r, 0)], world.log[(2, r, 0)]
        assert not first["known"] and np.array_equal(first["result"], data[r]) and np.array_equal(first["contribution"], data[r])
        assert second["known"] and np.array_equal(second["result"], data.max(axis=0))


def test_a_reduced_flag_that_triggers_a_second_reduce_takes_three_passes():
    """The relaunch protocol's shape: ONE rank raises a flag, the reduced flag makes EVERY rank issue a second collective."""
    world = LoopbackWorld(4)

    def program(rank, comm):
        key = 100 + 7 * rank
        first = comm.reduce_max(np.array([key, 1 if rank == 2 else 0], dtype=np.int64))
        if int(first[1]) == 0:
            return int(first[0]), comm.calls
        second = comm.reduce_max(np.array([key + 1000, 0], dtype=np.int64))      # what the repeated launch contributes
        return int(second[0]), comm.calls

    outs = world.run(program)
    assert world.passes == 3
    assert outs == [(1121, 2)] * 4
    # pass 1: only the flagged rank went on (on its own words - tainted, nothing recorded); pass 2: all of them
    assert [(1, r, 1) in world.log for r in range(4)] == [False, False, True, False]
    assert world.log[(1, 2, 1)]["tainted"] and all(not world.log[(2, r, 1)]["tainted"] for r in range(4))


def test_five_gathers_in_a_row():
    """CEM's shape: every iteration's input depends on the previous gather's result."""
    world = LoopbackWorld(3)

    def program(rank, comm):
        x = np.float32(rank + 1)
        seen = []
        for it in range(5):
            parts = comm.all_gather(np.array([[x, x * 2]], dtype=np.float32))
            assert len(parts) == 3 and all(p.shape == (1, 2) and p.dtype == np.float32 for p in parts)
            x = np.float32(sum(float(p[0, 0]) for p in parts) / 4 + rank)
            seen.append(x)
        return seen

    outs = world.run(program)
    assert world.passes == 6 and world.calls == [5, 5, 5]
    xs = [1.0, 2.0, 3.0]
    for it in range(5):
        total = np.float32(sum(xs))
        xs = [float(np.float32(float(total) / 4 + r)) for r in range(3)]
        assert [float(o[it]) for o in outs] == xs


@pytest.mark.parametrize("n,world_size", [(37, 8), (10, 3), (2, 5), (0, 3)])
def test_uneven_and_empty_shards_are_padded_and_cut_back(n, world_size):
    """The controller's gather of shards that differ by one candidate - or hold none: padded to the widest, cut back afterwards."""
    full = np.random.RandomState(n).randn(2, n).astype(np.float32)
    widths = [_shard(n, r, world_size)[1] - _shard(n, r, world_size)[0] for r in range(world_size)]
    wmax = max(widths)
    world = LoopbackWorld(world_size)

    def program(rank, comm):
        lo, hi = _shard(n, rank, world_size)
        mine = np.zeros((2, wmax), dtype=np.float32)
        mine[:, :hi - lo] = full[:, lo:hi]
        parts = comm.all_gather(mine)
        return np.concatenate([p[:, :w] for p, w in zip(parts, widths)], axis=1)

    for out in world.run(program):
        assert out.tobytes() == full.tobytes() and out.shape == full.shape
    assert world.passes == 2


def test_a_rank_program_that_is_not_deterministic_fails_the_bit_identity_check():
    state = {"calls": 0}

    def program(rank, comm):
        state["calls"] += 1
        noise = state["calls"] if rank == 1 else 0             # rank 1 contributes something else in every pass
        return comm.reduce_max(np.array([rank, noise], dtype=np.int64))

    with pytest.raises(LoopbackError, match="rank 1.*not bit-identical"):
        LoopbackWorld(3).run(program)
    # a NaN payload that is reproduced bit for bit is NOT a difference
    outs = LoopbackWorld(2).run(lambda rank, comm: comm.all_gather(np.array([np.nan, rank], dtype=np.float32)))
    assert all(np.isnan(o[r][0]) for o in outs for r in range(2))


def test_a_collective_count_that_differs_between_ranks_fails_instead_of_looping():
    def program(rank, comm):
        out = comm.reduce_max(np.array([rank], dtype=np.int64))
        if rank == 1:
            comm.reduce_max(np.array([5], dtype=np.int64))       # nobody else joins this one
        return out

    world = LoopbackWorld(3)
    with pytest.raises(LoopbackError, match="completed no collective"):
        world.run(program)
    assert world.passes == 2            # pass 1 completed the shared reduce, pass 2 nothing: refused there

    def mixed(rank, comm):
        return comm.reduce_max(np.array([1], dtype=np.int64)) if rank else comm.all_gather(np.array([1], dtype=np.int64))

    with pytest.raises(LoopbackError, match="a reduce on rank 1 and a gather"):
        LoopbackWorld(2).run(mixed)
    with pytest.raises(LoopbackError, match="contributes"):
        LoopbackWorld(2).run(lambda rank, comm: comm.reduce_max(np.zeros(2 + rank, dtype=np.int64)))


def test_the_tensor_reduce_works_in_place():
    world = LoopbackWorld(2)

    def program(rank, comm):
        t = torch.tensor([3 - rank, 10 * rank, -1], dtype=torch.int64)
        comm.reduce(t)
        return t.numpy().copy()

    for out in world.run(program):
        assert out.tolist() == [3, 10, -1]


# ---- the controller's real host path at world = 8, launch replaced by the oracle ---------------------------------------------------
def _controller_world(cid, world_size, monkeypatch):
    import oracle_backend
    case, seed = cases.split_id(cid)
    gold = cases.load_golden(cid)
    ctrl = oracle_backend.install(cases.product_controller(case), case)
    np.random.seed(seed)
    state0 = np.random.get_state()
    current = {}

    def all_reduce(tensor, op=None):
        # `_combine_keys` (the Python RS path) reaches its collective through torch.distributed directly
        assert op == torch.distributed.ReduceOp.MAX
        current["comm"].reduce(tensor)

    monkeypatch.setattr(torch.distributed, "all_reduce", all_reduce)

    def program(rank, comm):
        current["comm"] = comm
        comm.install(ctrl)
        actions, _ = ctrl.get_actions(gold["obs0"])
        return dict(actions=actions.copy(), best=np.array(ctrl.last_plan["best_index"]), rng_next=np.random.uniform(),
                    shard=ctrl.last_plan.get("shard"))

    world = LoopbackWorld(world_size, reset=lambda rank: np.random.set_state(state0))
    outs = world.run(program)
    if ctrl._ahead is not None:
        ctrl._ahead.stop()
    return case, gold, world, outs


def test_cem_host_path_on_eight_loopback_ranks_gives_the_golden_plan(monkeypatch):
    """`hc_cem_m2_n100_h4_s0` in shards of 12 / 13 candidates: per iteration one agreement and one all-gather (padded, cut back)
    through `_cem_iteration`'s own code - every rank must return the golden index and action and leave np.random where the
    reference leaves it."""
    case, gold, world, outs = _controller_world("hc_cem_m2_n100_h4_s0", 8, monkeypatch)
    iters = case["num_cem_iters"]
    assert world.calls == [2 * iters] * 8 and world.passes == 2 * iters + 1
    assert [c["kind"] for c in world.collectives] == ["reduce", "gather"] * iters
    for out in outs:
        assert np.array_equal(out["best"], gold["best"])
        np.testing.assert_array_equal(out["actions"], gold["chosen"])
        assert out["rng_next"] == float(gold["rng_next"])
    for k in range(0, 2 * iters, 2):                          # [flag, digest, MASK - digest]: nothing flagged, digests equal
        words = np.stack(world.collectives[k]["parts"])
        assert np.all(words[:, 0] == 0) and np.all(words == words[0]) and int(words[0, 1] + words[0, 2]) == 0x7FFFFFFFFFFF


def test_rs_host_path_on_eight_loopback_ranks_gives_the_golden_plan(monkeypatch):
    """`hc_rs_ragged_n37_h3_s0` in shards of 4 and 5 candidates through `_rs_parity_plan` / `_combine_keys`: one MAX all-reduce of
    `[key, flag, digest pair]`; the winning key comes from the rank that owns the golden candidate."""
    case, gold, world, outs = _controller_world("hc_rs_ragged_n37_h3_s0", 8, monkeypatch)
    m = case["m"]
    assert world.calls == [1] * 8 and world.passes == 2
    for rank, out in enumerate(outs):
        assert np.array_equal(out["best"], gold["best"])
        np.testing.assert_array_equal(out["actions"], gold["chosen"])
        assert out["rng_next"] == float(gold["rng_next"])
        assert tuple(out["shard"]) == _shard(case["n"], rank, 8)
    words = np.stack(world.collectives[0]["parts"])
    assert words.shape == (8, m + 3) and np.all(words[:, m] == 0) and np.all(words[:, m + 1:] == words[0, m + 1:])
    from learning_to_adapt_amd import _lib
    for i in range(m):
        best = int(gold["best"][i])
        owners = [r for r in range(8) if words[r, i] == words[:, i].max()]
        assert owners == [r for r in range(8) if _shard(case["n"], r, 8)[0] <= best < _shard(case["n"], r, 8)[1]]
        assert _lib.key_decode(words[:, i].max())[1] == best
