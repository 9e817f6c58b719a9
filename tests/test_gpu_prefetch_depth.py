"""The operand hand-over between the phases of the MFMA rollout kernel (csrc/l2a_mfma.h) at the smallest shapes where it can
go wrong: which weight fragments a phase requests for the phase after it, and at which scalar offset, depends on the hidden
width (HT = 8 / 16 / 32 k-groups, TH = 1 / 2 / 4 tiles per wave of a half member), on what precedes the half member (a layer 0,
a full set's output phase, an inner GEMM) and on the instance (HalfCheetah's O4 tile, the Ant's four input k-groups, one
hidden layer).

Every case: n = 24 candidates (two tiles, the second half filled; one case with a single tile) and h = 3 steps (both parities
of the exchange regions and one reuse).  As in test_tile_split_is_bit_identical_to_single_workgroup the two tile-split
geometries must reproduce the one-workgroup launch bit for bit, twice, with a clean launch status, and agree with the oracle.
"""

import numpy as np
import pytest
import torch

import cases
from learning_to_adapt_amd import _lib

pytestmark = pytest.mark.gpu

RTOL = 1e-4      # BASELINE.json north star, as in test_gpu_parity.py: |got - want| / max(1, |want|)

C2 = "c2_hc_rs_n2000_h30_e5"
CASES = (
    # HT = 8 / 16 / 32 and TH = 1 / 2 / 4; E = 1 is the half member alone (reached from a layer 0), E = 3 and 5 reach it from
    # a full set's output phase
    [(C2, dict(hidden=[w, w], E=e, n=24, h=3)) for w in (128, 256, 512) for e in (1, 3, 5)]
    # the half member reached from an inner GEMM
    + [(C2, dict(hidden=[256, 256, 256], E=e, n=24, h=3)) for e in (1, 3)]
    # one hidden layer: the N1 instances (whole sets only)
    + [(C2, dict(hidden=[128], E=3, n=24, h=3))]
    # a single candidate tile
    + [(C2, dict(hidden=[512, 512], E=5, n=16, h=3))]
    # the Ant's instance (KG0 = 4, K0L = 1): its layer-0 path with the scalar offsets
    + [("ant_rs_n300_h6_e3", dict(n=24, h=3))]
)


def _ids(c):
    name, over = c
    return "%s-%s" % (name.split("_")[0], "-".join("%s=%s" % (k, "x".join(map(str, v)) if isinstance(v, list) else v)
                                                  for k, v in sorted(over.items())))


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _plan_returns(native, case, env, obs0, actions):
    dev = native.device
    m, n = case["m"], case["n"]
    rets = torch.full((m, n), float("nan"), dtype=torch.float32, device=dev)
    best = torch.zeros((m,), dtype=torch.int64, device=dev)
    native.plan_rs(torch.from_numpy(np.ascontiguousarray(obs0, dtype=np.float32)).to(dev),
                   torch.from_numpy(np.ascontiguousarray(actions, dtype=np.float32)).to(dev),
                   m, n, case["h"], case.get("discount", 1.0), env.reward_spec, returns_out=rets, best_key=best)
    torch.cuda.synchronize()
    return rets.cpu().numpy(), best.cpu().numpy()


@pytest.mark.parametrize("name,over", CASES, ids=[_ids(c) for c in CASES])
def test_phase_handover_is_bit_identical_across_tile_splits(name, over):
    from oracle import make_reward
    from oracle.planner import rollout_returns, sample_rs_actions
    case = dict(cases.CASES[name], **over)
    env, model = cases.product_model(case)
    native = model.planner_model()
    np.random.seed(1)
    a = sample_rs_actions(env.action_space.low, env.action_space.high, case["n"], case["m"], case["h"])
    obs0 = np.random.RandomState(11).randn(case["m"], env.observation_space.shape[0])
    ctx = _lib.Context.get(0)
    out = {}
    try:
        ctx.set_kernel("mfma")
        ctx.set_micro(0)        # (plans this small would otherwise run on micro tiles: not the kernel under test)
        ctx.set_fan(0)          # (nor on the member fan)
        for policy in (1, 2, 0):
            ctx.set_split(policy)
            r1, k1 = _plan_returns(native, case, env, obs0, a)
            r2, k2 = _plan_returns(native, case, env, obs0, a)
            ctx.launch_status()                                  # raises unless clean
            assert not np.isnan(r1).any()
            assert np.array_equal(r1, r2) and np.array_equal(k1, k2), "policy %d: two launches differ" % policy
            out[policy] = (r1, k1)
    finally:
        ctx.set_split(1)
        ctx.set_fan(1)
        ctx.set_micro(1)
        ctx.set_kernel("auto")
    for policy in (1, 2):
        assert np.array_equal(out[policy][0], out[0][0]), "policy %d differs from the unsplit launch" % policy
        assert np.array_equal(out[policy][1], out[0][1])
    want = rollout_returns(cases.oracle_dynamics(case), make_reward(case["env"], env.dt), obs0, a, case["n"],
                           case.get("discount", 1.0)).reshape(case["m"], case["n"])
    for policy in (1, 2, 0):
        err = rel_err(out[policy][0], want)
        print("policy %d: rel_err %.3g" % (policy, err))
        assert err < RTOL
