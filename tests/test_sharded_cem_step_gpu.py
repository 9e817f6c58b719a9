"""The sharded device-mode CEM plan step as ONE C call (``l2a_cem_controller_create_sharded_device``): every rank rolls out its
slice of the candidates, and every iteration's returns are gathered by the plan's one collective kind - the int64 MAX all-reduce,
here of ``m * n + 3`` words packed and unpacked on the device (``l2a_cem_shard_pack`` / ``_unpack``).

The ranks run one after another on ONE GPU through the sequential loopback world (tests/loopback_world.py), a fresh controller per
(pass, rank), so a rank launches the geometry it launches when it owns its GPU (config 5's shard: the member fan).  A *tainted*
pass - a rank whose collective is not fully known yet gets its own words back - sees holes and fails with ``L2AError``; the
programs tolerate that only while ``comm.tainted``.  Everything is compared bit for bit against the unsharded ``NativeCemStep``
(or the Python ``get_cem_action_device``) under the same seed.

Not covered here: RCCL with more than one rank, and timing."""

import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

import cases
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
from learning_to_adapt_amd.policies.mpc_controller import MPCController
from learning_to_adapt_amd.policies.native_cem_step import NativeCemStep
from loopback_world import LoopbackWorld

HERE = os.path.dirname(os.path.abspath(__file__))
DIGEST_MASK = 0x7FFFFFFFFFFF
PRESENT = 1 << 32

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


def _words_of(table):
    """Host model of the words of an fp32 table (``l2a_cem_word_encode`` element by element)."""
    return (np.ascontiguousarray(table, dtype=np.float32).view(np.uint32).astype(np.int64) | PRESENT).reshape(-1)


# ---- 1. the two kernels alone ---------------------------------------------------------------------------------------------------
def _returns_table(m, n, seed):
    rs = np.random.RandomState(seed)
    bits = (rs.randn(m, n) * 50.0).astype(np.float32).view(np.uint32)
    flat = bits.reshape(-1)
    for k, special in enumerate([0x7FC00000, 0x7FD12345, 0xFFFFFFFF, 0x7FA00001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                                 0x00000001, 0x807FFFFF]):
        flat[(5 * k + seed) % flat.size] = special
    return bits


def _pack(ctx, local_bits, m, n, lo, hi, digest):
    dev = torch.device("cuda", ctx.device)
    words = torch.full((m * n + 3,), -1, dtype=torch.int64, device=dev)            # (every word must be written: no memset in front)
    local = None
    if hi > lo:
        local = torch.from_numpy(np.ascontiguousarray(local_bits).view(np.int32)).to(dev).view(torch.float32)
    ctx.check(ctx.lib.l2a_cem_shard_pack(ctx.handle, _ptr(local), m, n, lo, hi, ctypes.c_ulonglong(digest), _ptr(words),
                                         _stream_ptr(dev)), "l2a_cem_shard_pack")
    torch.cuda.synchronize()
    return words


def _unpack(ctx, words, m, n, verdict):
    dev = words.device
    out = torch.full((m, n), 7.0, dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.l2a_cem_shard_unpack(ctx.handle, _ptr(words), m, n, _ptr(out), _ptr(verdict), _stream_ptr(dev)),
              "l2a_cem_shard_unpack")
    torch.cuda.synchronize()
    return out.view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("m,n,world_size", [(1, 13, 3), (2, 13, 16), (2, 1000, 7), (1, 4000, 8)])
def test_pack_and_unpack_kernels_against_the_host_helpers(m, n, world_size, ctx):
    """Uneven shards, empty shards (world > n) and non-finite returns: every rank's words are the host helper's, zeros outside the
    shard; the MAX of all ranks' words unpacks to the table bit for bit with a clean verdict; without one rank's part `holes` rises
    by exactly its width; the verdict accumulates over two calls."""
    lib = ctx.lib
    bits = _returns_table(m, n, 1 + m)
    digest = 0xFEDCBA9876543210
    d = digest & DIGEST_MASK
    parts = []
    for rank in range(world_size):
        lo, hi = _shard(n, rank, world_size)
        got = _pack(ctx, bits[:, lo:hi], m, n, lo, hi, digest).cpu().numpy()
        want = np.zeros((m * n + 3,), dtype=np.int64)
        for i in range(m):
            for j in range(lo, hi):
                value = ctypes.c_float.from_buffer_copy(bits[i, j:j + 1].tobytes())
                want[i * n + j] = int(lib.l2a_cem_word_encode(value))
        want[m * n:] = [0, d, DIGEST_MASK - d]
        assert np.array_equal(got, want), rank
        parts.append(got)
    if world_size > n:
        assert any(_shard(n, r, world_size)[0] == _shard(n, r, world_size)[1] for r in range(world_size))
    dev = torch.device("cuda", ctx.device)
    verdict = torch.zeros((3,), dtype=torch.int32, device=dev)
    reduced = torch.from_numpy(np.maximum.reduce(parts)).to(dev)
    table = _unpack(ctx, reduced, m, n, verdict)
    assert table.tobytes() == bits.tobytes()
    assert verdict.cpu().tolist() == [0, 0, 0]
    # a missing part: holes = exactly its width, decoded as 0.0f
    gone = max(range(world_size), key=lambda r: _shard(n, r, world_size)[1] - _shard(n, r, world_size)[0])
    lo, hi = _shard(n, gone, world_size)
    partial = torch.from_numpy(np.maximum.reduce([p for r, p in enumerate(parts) if r != gone])).to(dev)
    table = _unpack(ctx, partial, m, n, verdict)
    assert verdict.cpu().tolist() == [0, m * (hi - lo), 0]
    assert not table[:, lo:hi].any() and table[:, :lo].tobytes() == bits[:, :lo].tobytes() and table[:, hi:].tobytes() == bits[:, hi:].tobytes()
    _unpack(ctx, partial, m, n, verdict)                                 # NOT reset by the call
    assert verdict.cpu().tolist() == [0, 2 * m * (hi - lo), 0]


def test_status_word_and_digest_pair_reach_the_verdict(ctx):
    m, n = 2, 50
    bits = _returns_table(m, n, 5)
    dev = torch.device("cuda", ctx.device)
    ctx.check(ctx.lib.l2a_inject_status(ctx.handle, 1), "l2a_inject_status")
    try:
        flagged = _pack(ctx, bits, m, n, 0, n, 99)
    finally:
        assert ctx.launch_status_value() == 1                            # (the pack reads the word, it does not clear it)
    assert flagged.cpu().numpy()[m * n:].tolist() == [1, 99, DIGEST_MASK - 99]
    clean = _pack(ctx, bits, m, n, 0, n, 99)
    assert clean.cpu().numpy()[m * n:].tolist() == [0, 99, DIGEST_MASK - 99]
    verdict = torch.zeros((3,), dtype=torch.int32, device=dev)
    assert _unpack(ctx, flagged, m, n, verdict).tobytes() == bits.tobytes()
    assert verdict.cpu().tolist() == [1, 0, 0]
    _unpack(ctx, clean, m, n, verdict)
    assert verdict.cpu().tolist() == [1, 0, 0]                           # the flag stays: OR over the calls
    # two ranks with different digests: MAX of the pair no longer adds up
    other = _pack(ctx, bits, m, n, 0, n, 100)
    wrong = torch.maximum(clean, other)
    verdict.zero_()
    _unpack(ctx, wrong, m, n, verdict)
    assert verdict.cpu().tolist() == [0, 0, 1]
    _unpack(ctx, clean, m, n, verdict)
    assert verdict.cpu().tolist() == [0, 0, 1]


# ---- the controller -------------------------------------------------------------------------------------------------------------
class _Setup(object):
    def __init__(self, name, seed_id, cem_mode="reference"):
        self.case = dict(cases.CASES[name])
        self.gold = cases.load_golden("%s_s%d" % (name, seed_id))
        self.env, self.model = cases.product_model(self.case)
        self.native = self.model.planner_model()
        ctrl = cases.product_controller(self.case, model=self.model, env=self.env, rng="device", cem_mode=cem_mode)
        self.n, self.m, self.h, self.iters = self.case["n"], self.case["m"], self.case["h"], self.case["num_cem_iters"]
        self.num_elites = max(int(self.n * ctrl.percent_elites), 1)
        self.alpha, self.reward = ctrl.alpha, ctrl._reward_spec
        self.reference = cem_mode == "reference"
        self.cem_mode = cem_mode
        self.stream = torch.cuda.current_stream(self.native.device).cuda_stream
        rs = np.random.RandomState(8)
        self.obs = [self.gold["obs0"], self.gold["obs0"] + 0.01 * rs.randn(*self.gold["obs0"].shape)]

    def controller(self, seed, shard=None):
        return NativeCemStep(self.native, self.m, self.n, self.h, self.env.action_space.low, self.env.action_space.high,
                             self.case.get("discount", 1.0), self.reward, self.iters, self.num_elites, self.alpha, self.reference,
                             seed, shard=shard)

    def unsharded(self, seed, steps):
        st = self.controller(seed)
        try:
            return [self.snapshot(st, st.step(self.obs[k], self.stream)) for k in range(steps)]
        finally:
            st.close()

    @staticmethod
    def snapshot(st, rc):
        mean, std, rets = st.result()
        return dict(rc=rc, act=st.act.copy(), idx=st.idx.copy(), ret=st.ret.copy(), mean=mean, std=std, rets=rets)


def _same_step(got, want, where):
    assert got["act"].dtype == np.float64 and _bits(got["act"]) == _bits(want["act"]), where
    assert np.array_equal(got["idx"], want["idx"]), where
    assert _bits(got["ret"]) == _bits(want["ret"]), where
    assert _bits(got["mean"]) == _bits(want["mean"]) and _bits(got["std"]) == _bits(want["std"]), where
    assert got["rets"].shape == want["rets"].shape
    for it in range(want["rets"].shape[0]):                              # EVERY iteration's gathered [m, n] table
        assert _bits(got["rets"][it]) == _bits(want["rets"][it]), "%s, iteration %d" % (where, it)


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
                    rc = st.step(setup.obs[sum(1 for o in outs if "rc" in o)], setup.stream)     # (a refused step is repeated)
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
                out = setup.snapshot(st, rc)
                torch.cuda.synchronize()
                out.update(stats=st.stats(), degraded=bool(ctx.split_degraded),
                           status=ctx.launch_status_value(), collectives=comm.calls)
                outs.append(out)
            return outs
        finally:
            st.close()

    world = LoopbackWorld(world_size, reset=reset, max_collectives=64)
    return world, world.run(program)


def _assert_collectives(world, setup, world_size, wants):
    """Every collective is a reduce of m * n + 3 int64 words; rank r's contribution to iteration `it` holds exactly the words of its
    slice of the unsharded run's table, a clear flag and the shared digest pair."""
    m, n = setup.m, setup.n
    assert [c["kind"] for c in world.collectives] == ["reduce"] * len(wants)
    for k, table in enumerate(wants):
        parts = world.collectives[k]["parts"]
        want_words = _words_of(table).reshape(m, n)
        for rank, part in enumerate(parts):
            assert part.dtype == np.int64 and part.shape == (m * n + 3,), (k, rank)
            lo, hi = _shard(n, rank, world_size)
            mine = np.zeros((m, n), dtype=np.int64)
            mine[:, lo:hi] = want_words[:, lo:hi]
            assert np.array_equal(part[:m * n].reshape(m, n), mine), (k, rank)
            assert int(part[m * n]) == 0 and int(part[m * n + 1]) + int(part[m * n + 2]) == DIGEST_MASK, (k, rank)
            assert np.array_equal(part[m * n + 1:], parts[0][m * n + 1:]), (k, rank)


@pytest.mark.parametrize("cem_mode", ["reference", "fixed"])
@pytest.mark.parametrize("seed_id", [0, 1])
def test_config5_as_eight_ranks_of_the_sharded_cem_step(seed_id, cem_mode, ctx):
    """8 x 500 of config 5's 4000 candidates on the member fan: every rank's action, index, return, final mean / std and every
    iteration's [m, n] returns table are those of the unsharded C step under the same seed; five collectives, six passes."""
    setup = _Setup("c5_hc_cem_n4000_h30_e5", seed_id, cem_mode)
    case = setup.case
    cus = ctx.info()["compute_units"]
    for r in range(8):
        lo, hi = _shard(case["n"], r, 8)
        g = _lib.plan_geometry(setup.env.observation_space.shape[0], setup.env.action_space.shape[0], case["hidden"], case["E"],
                               case["mode"], case["m"], hi - lo, case["h"], cus=cus)
        assert hi - lo == 500 and case["h"] == 30 and (g["split"], g["fan"], g["nt"]) == (3, True, 1), g
    seed = 4242 + seed_id
    want = setup.unsharded(seed, 1)[0]
    world, outs = _run_world(ctx, setup, 8, seed)
    assert world.passes == setup.iters + 1 and world.calls == [setup.iters] * 8
    _assert_collectives(world, setup, 8, [want["rets"][it] for it in range(setup.iters)])
    for rank, out in enumerate(outs):
        assert len(out) == 1 and out[0]["rc"] == _lib.L2A_OK, rank
        _same_step(out[0], want, "rank %d" % rank)
        assert out[0]["stats"]["relaunches"] == 0 and out[0]["stats"]["steps"] == 1 and not out[0]["degraded"], rank
        assert out[0]["collectives"] == setup.iters


@pytest.mark.parametrize("world_size", [3, "n + 1"])
def test_uneven_and_empty_shards_over_two_consecutive_steps(world_size, ctx):
    """`hc_cem_m2_n100_h4` as 3 ranks (33 / 33 / 34) and as n + 1 ranks (one empty shard): two consecutive steps equal the
    unsharded controller's step for step - the Philox stream position carries over, and does not depend on the world size."""
    setup = _Setup("hc_cem_m2_n100_h4", 0, "reference")
    n = setup.n
    world_size = n + 1 if world_size == "n + 1" else world_size
    widths = [_shard(n, r, world_size)[1] - _shard(n, r, world_size)[0] for r in range(world_size)]
    assert (widths == [33, 33, 34]) if world_size == 3 else (sorted(set(widths)) == [0, 1] and widths.count(0) == 1)
    wants = setup.unsharded(31, 2)
    assert _bits(wants[0]["rets"]) != _bits(wants[1]["rets"])
    world, outs = _run_world(ctx, setup, world_size, 31, steps=2)
    assert world.passes == 2 * setup.iters + 1 and world.calls == [2 * setup.iters] * world_size
    _assert_collectives(world, setup, world_size, [w["rets"][it] for w in wants for it in range(setup.iters)])
    for rank, out in enumerate(outs):
        for k in range(2):
            assert out[k]["rc"] == _lib.L2A_OK
            _same_step(out[k], wants[k], "rank %d, step %d" % (rank, k))
        assert out[1]["stats"]["steps"] == 2 and out[1]["stats"]["relaunches"] == 0


def test_one_flagged_rank_makes_every_rank_repeat_the_step_unsplit(ctx):
    """ONE rank's status word is set (what a lost tile-split partner reports): the reduced flag makes all ranks switch the split
    off and repeat the whole step with the same offsets - 2 x iters collectives, L2A_STEP_UNSPLIT, one relaunch, the unflagged
    result - and the flagged rank's status word is consumed."""
    setup = _Setup("hc_cem_n400_h10", 0, "reference")
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
        # the split and the unsplit launch: the same words
        assert all(np.array_equal(a[:mn], b[:mn]) for a, b in zip(world.collectives[k]["parts"], world.collectives[k - iters]["parts"]))
    for rank, out in enumerate(outs):
        assert out[0]["rc"] == _lib.L2A_STEP_UNSPLIT, rank
        assert out[0]["stats"]["relaunches"] == 1 and out[0]["stats"]["steps"] == 1, rank
        assert out[0]["degraded"] and out[0]["status"] == 0, rank
        _same_step(out[0], want, "rank %d" % rank)
    _restore_context(ctx)                                                # the context is usable as before: the split is back on
    again = setup.unsharded(77, 1)[0]
    _same_step(again, want, "after the relaunch")


def test_a_rank_built_with_another_seed_fails_every_rank_and_consumes_nothing(ctx):
    """Digests that differ fail the step with L2A_ESTATE on EVERY rank; the stream position does not advance: the following step -
    the odd rank rebuilt with the right seed - reproduces step 1 of the unsharded run."""
    setup = _Setup("hc_cem_m2_n100_h4", 0, "fixed")
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


@pytest.mark.parametrize("cem_mode", ["reference", "fixed"])
def test_mpc_controller_builds_and_steps_the_sharded_cem_controller(cem_mode, ctx):
    """`MPCController(use_cem=True, rng="device", native_cem_step=True)` on eight loopback ranks: `_cemstep` serves the call (its
    dry run of the collective is one more reduce, of zeros) and the plan equals ONE process's Python `get_cem_action_device`."""
    cid = "c5_hc_cem_n4000_h30_e5_s0"
    case, seed = cases.split_id(cid)
    gold = cases.load_golden(cid)
    env, model = cases.product_model(case)
    torch_seed = 4242
    ref = cases.product_controller(case, model=model, env=env, rng="device", cem_mode=cem_mode)
    torch.manual_seed(torch_seed)
    want_act, _ = ref.get_actions(gold["obs0"])
    want = dict(ref.last_plan)
    assert ref._cemstep is None

    def reset(rank):
        torch.manual_seed(torch_seed)
        _restore_context(ctx)

    def program(rank, comm):
        ctrl = comm.install(cases.product_controller(case, model=model, env=env, rng="device", cem_mode=cem_mode, native_cem_step=True))
        try:
            try:
                act, _ = ctrl.get_actions(gold["obs0"])
            except _lib.L2AError:
                if comm.tainted:
                    return None
                raise
            st = ctrl._cemstep
            assert st is not None and st.steps == 1 and st.shard == (rank, 8)
            plan = ctrl.last_plan
            return dict(act=act.copy(), idx=np.array(plan["best_index"]), ret=np.array(plan["best_return"]), mean=plan["cem_mean"],
                        std=plan["cem_std"], trace=len(plan["cem_trace"]), shard=tuple(plan["shard"]), calls=ctrl._bufs["cem_calls"])
        finally:
            if ctrl._cemstep is not None:
                ctrl._cemstep.close()
                ctrl._cemstep = None

    world = LoopbackWorld(8, reset=reset)
    outs = world.run(program)
    iters, mn = case["num_cem_iters"], case["m"] * case["n"]
    assert world.passes == iters + 2 and world.calls == [iters + 1] * 8
    assert all(c["kind"] == "reduce" and all(p.shape == (mn + 3,) for p in c["parts"]) for c in world.collectives)
    assert not np.stack(world.collectives[0]["parts"]).any()             # the dry run
    for rank, out in enumerate(outs):
        assert _bits(out["act"]) == _bits(want_act), rank
        assert np.array_equal(out["idx"], want["best_index"]), rank
        assert _bits(np.asarray(out["ret"], dtype=np.float32)) == _bits(np.asarray(want["best_return"], dtype=np.float32)), rank
        assert _bits(out["mean"]) == _bits(want["cem_mean"]) and _bits(out["std"]) == _bits(want["cem_std"]), rank
        assert out["trace"] == iters and out["shard"] == _shard(case["n"], rank, 8) and out["calls"] == iters, rank


def test_one_rank_over_the_librarys_own_communicator(ctx):
    """`reduce` = NULL: the collective is `l2a_allreduce_best` on m * n + 3 words over a one-rank `l2a_comm_init` communicator
    (RCCL cannot run two ranks on one GPU).  Pack, collective and unpack all run; the step equals the unsharded one."""
    setup = _Setup("hc_cem_m2_n100_h4", 0, "reference")
    lib = ctx.lib
    wants = setup.unsharded(13, 2)
    buf = ctypes.create_string_buffer(128)
    ctx.check(lib.l2a_comm_unique_id(buf), "l2a_comm_unique_id")
    ctx.check(lib.l2a_comm_init(ctx.handle, 0, 1, buf.raw), "l2a_comm_init")
    try:
        st = setup.controller(13, shard=(0, 1, None))
        try:
            for k in range(2):
                out = setup.snapshot(st, st.step(setup.obs[k], setup.stream))
                assert out["rc"] == _lib.L2A_OK
                _same_step(out, wants[k], "step %d" % k)
        finally:
            st.close()
    finally:
        lib.l2a_comm_destroy(ctx.handle)


def test_sharded_cem_controller_without_a_collective_is_refused(ctx):
    setup = _Setup("hc_cem_m2_n100_h4", 0, "reference")
    with pytest.raises(_lib.L2AError, match="no reduce function and no communicator"):
        setup.controller(13, shard=(0, 2, None))
    with pytest.raises(_lib.L2AError, match="bad rank / world"):
        setup.controller(13, shard=(2, 2, lambda payload: None))


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
        import cases as _cases
        case = dict(_cases.CASES["hc_cem_m2_n100_h4"])
        gold = _cases.load_golden("hc_cem_m2_n100_h4_s0")
        torch.manual_seed(99)
        ctrl = _cases.product_controller(case, rng="device", cem_mode="reference", native_cem_step=True)
        out = {}
        for k in range(2):
            act, _ = ctrl.get_actions(gold["obs0"])
            assert ctrl._cemstep is not None and ctrl._cemstep.steps == k + 1 and ctrl._cemstep.shard == (rank, world)
            plan = ctrl.last_plan
            out.update({"act_%d" % k: act, "idx_%d" % k: np.asarray(plan["best_index"]), "ret_%d" % k: np.asarray(plan["best_return"]),
                        "mean_%d" % k: plan["cem_mean"], "std_%d" % k: plan["cem_std"],
                        "rets_%d" % k: np.stack([t["returns"] for t in plan["cem_trace"]])})
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
    case = dict(cases.CASES["hc_cem_m2_n100_h4"])
    gold = cases.load_golden("hc_cem_m2_n100_h4_s0")
    torch.manual_seed(99)
    ref = cases.product_controller(case, rng="device", cem_mode="reference", native_cem_step=True)
    outs = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    for k in range(2):
        want_act, _ = ref.get_actions(gold["obs0"])
        plan = ref.last_plan
        assert ref._cemstep is not None and ref._cemstep.shard is None
        for rank, o in enumerate(outs):
            assert _bits(o["act_%d" % k]) == _bits(want_act), (rank, k)
            assert np.array_equal(o["idx_%d" % k], plan["best_index"]), (rank, k)
            assert _bits(o["ret_%d" % k]) == _bits(plan["best_return"]), (rank, k)
            assert _bits(o["mean_%d" % k]) == _bits(plan["cem_mean"]) and _bits(o["std_%d" % k]) == _bits(plan["cem_std"]), (rank, k)
            assert _bits(o["rets_%d" % k]) == _bits(np.stack([t["returns"] for t in plan["cem_trace"]])), (rank, k)
