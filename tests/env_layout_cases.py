"""Many envs per workgroup: the layout table that ``tests/test_env_layout_gpu.py`` runs on the GPU, and pure-Python restatements
of the two PER-ENV KEY REDUCTIONS (no GPU, no kernel arithmetic) with which ``tests/test_env_layout_cases.py`` proves on the CPU
that the table tells a correct reduction from a broken one.

Five kernels walk the flat ``m * n`` row axis in workgroups of ``W`` rows that ignore env boundaries (``W = 16 RT`` for
``l2a_value_mlp_k<RT>``, 64 for ``l2a_score_traj_k`` / ``l2a_score_term_k``, ``16 CT`` for ``l2a_score_mlp_k``), and reduce the
packed arg-max keys per env inside the workgroup before ONE ``atomicMax`` per (workgroup, env):

  ``value_reduce``   csrc/l2a_value.hip: waves 0 and 1 each reduce the envs ``e0 .. e1`` their 64 rows touch into ``swk[env][wave]``,
                     one thread per env combines the two words.  Mutants
                       ``"V1"``  ``wave < 2`` -> ``wave < 1``: wave 1 never reduces;
                       ``"V2"``  ``e1 = e0``: a wave reduces the first env of its rows only;
                       ``"V3"``  the final combine ignores ``swk[..][1]``.
  ``scorer_reduce``  csrc/l2a_score.hip, csrc/l2a_score_mlp.hip: the first row of every env run of the workgroup walks the run in
                     LDS.  Mutants
                       ``"S1"``  a run starts only at ``tid == 0`` or where ``tid % 16 == 0``;
                       ``"S2"``  the run walk stops at the next multiple of 64.
  ``gather_env``     the ``obs0`` row a scorer's row reads at ``t = 0``, ``(r0 + i) / n``.  Mutant
                       ``"G"``   ``obs0[r0 / n]`` of the row's 16-row tile for every row of the tile.

Every mutant indexes only what the kernel indexes (``swk[0 .. n_env - 1]``, ``skey`` / ``senv`` below ``nr``, ``obs0`` rows of envs
the workgroup touches, ``best_key`` of those envs): none reads or writes out of bounds.

V1 and V3 are the SAME function as the kernel wherever a workgroup has no row in wave 1, that is for every ``W <= 64``; S2
wherever ``W <= 64``.  The CPU test records both."""

from math import gcd

import numpy as np

N_LAYOUT = (1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129)
WS = (16, 32, 64, 128)
CUS = (32, 64, 256, 304)            # device sizes at which the table's structural claims are asserted without a GPU
CAND_OFFSETS = ("0", "1000", "top")   # "top": 2 ** 31 - 1 - n, the largest offset include/l2a.h allows
VALUE_MUTANTS = ("V1", "V2", "V3")
SCORER_MUTANTS = ("S1", "S2")

# the tail classes of ``rows mod W``
ONE = "one"         # the last workgroup holds one row
SHORT = "short"     # ... 2 .. 63 rows (below W): wave 0 only
LONG = "long"       # ... 65 .. W - 1 rows, W = 128: a ragged wave 1
CUT = "cut"         # ... 1 .. n - 1 rows: nothing but the end of an env that began in the workgroup before, its run cut by the launch's end
TAILS = (ONE, SHORT, LONG, CUT)

# the only (m, n) the direct kernel tests used before this table (tests/value_model_cases.py, tests/termination_cases.py,
# tests/test_reward_program_gpu.py, tests/test_reward_model_gpu.py)
OLD_SHAPES = ((1, 64), (1, 33), (3, 70), (2, 130), (1, 129))
OLD_VALUE_SHAPES = OLD_SHAPES[:4]


def cand_offset_of(name, n):
    return {"0": 0, "1000": 1000, "top": 2 ** 31 - 1 - n}[name]


def tail_ok(W, n, t, tail):
    """Whether a last workgroup of ``t = rows mod W`` rows is of class ``tail``."""
    if tail == ONE:
        return t == 1
    if tail == SHORT:
        return 2 <= t <= min(63, W - 1)
    if tail == LONG:
        return W == 128 and 65 <= t <= W - 1
    if tail == CUT:
        return 1 <= t <= n - 1
    raise ValueError(tail)


def tail_possible(W, n, tail):
    """``rows = m n`` leaves ``rows mod W`` a multiple of ``g = gcd(n, W)``, and every multiple occurs: a class is possible where
    it holds one."""
    g = gcd(n, W)
    return any(tail_ok(W, n, t, tail) for t in range(0, W, g))


def layout(W, n, min_rows, tail):
    """``(m, rows)``: the smallest ``m`` with ``rows = m n >= min_rows`` whose ``rows mod W`` is of class ``tail`` - or None
    where ``n`` makes the class impossible at this ``W`` (``tail_possible`` says so without a search).  ``rows`` stays below
    ``min_rows + W n``."""
    if not tail_possible(W, n, tail):
        return None
    m = max(1, -(-min_rows // n))
    for _ in range(W):                  # (m n mod W has period W / gcd(n, W) in m)
        if tail_ok(W, n, (m * n) % W, tail):
            return m, m * n
        m += 1
    raise AssertionError("tail_possible and the search disagree: W %d n %d %s" % (W, n, tail))


PLAIN = "plain"     # where n allows none of the classes: the smallest table (whole workgroups, or 64 rows left at n = 64, W = 128)


def layouts(W, n, min_rows):
    """Every possible tail class of ``(W, n)``: ``[(tail, m, rows)]`` - or, for the (W, n) that have none (W | n; n = 64 at
    W = 128), the one ``plain`` layout of ``ceil(min_rows / n)`` envs, so that no n leaves a table."""
    out = []
    for tail in TAILS:
        lay = layout(W, n, min_rows, tail)
        if lay is not None:
            out.append((tail,) + lay)
    if not out:
        m = max(1, -(-min_rows // n))
        out.append((PLAIN, m, m * n))
    return out


def v2_lost_rows(W, n, rows):
    """The rows whose key mutant V2 drops: those of another env than the first row of their wave (64 rows, or the workgroup)."""
    r = np.arange(rows, dtype=np.int64)
    span = min(W, 64)
    return (r // n) != ((r // span) * span) // n


def min_rows_small(W):
    """Three whole workgroups and a ragged one: what the reduction structure needs (the CPU table; the scorers' GPU table)."""
    return 3 * W + 37


# ---- the GPU tables ------------------------------------------------------------------------------------------------------------
VALUE_OBS, VALUE_HIDDEN = 20, (64,)                         # width 64: the accumulator budget allows RT = 8
VALUE_WIDE = (256, 256)                                     # its cap is 8 too; a 128 KiB image at RT = 8
RTS = (1, 2, 4, 8)


def value_min_rows(rt, cus):
    """The launcher picks the smallest RT with ``ceil(tiles / RT) <= cus``: RT > 1 takes more than ``16 cus (RT / 2)`` rows."""
    return 16 * cus * (rt // 2) + 1 if rt > 1 else min_rows_small(16)


def value_table(cus, rts=RTS, ns=N_LAYOUT):
    """``[(rt, n, tail, m, rows)]`` of the terminal-value kernel on a device of ``cus`` compute units."""
    return [(rt, n) + lay for rt in rts for n in ns for lay in layouts(16 * rt, n, value_min_rows(rt, cus))]


def value_rt(rows, cus, cap=8):
    """``choose_rt`` of csrc/l2a_value.hip where the LDS does not bind (asserted against ``l2a_value_model_geometry``)."""
    tiles = -(-rows // 16)
    rt = 1
    while rt < cap and -(-tiles // rt) > cus:
        rt *= 2
    return rt


def scorer_table(W=64, ns=N_LAYOUT):
    """``[(n, tail, m, rows)]`` of the trajectory scorers (64 rows per workgroup): ``rows >= 3 * 64 + 37``."""
    return [(n,) + lay for n in ns for lay in layouts(W, n, min_rows_small(W))]


# the reward-model scorer: ((RT, CT, S), a, h) - ``rows >= a * 16 * cus + 37`` as ``reward_model_geometries.plan_n`` sizes them
MODEL_GEOMETRIES = [((1, 1, 1), 0, 1), ((2, 2, 1), 1, 1), ((4, 4, 1), 2, 1), ((8, 8, 1), 4, 1), ((4, 2, 2), 1, 5), ((8, 4, 2), 2, 9)]
MODEL_NS = (1, 3, 5, 17, 33)
MODEL_OBS, MODEL_ACT, MODEL_HIDDEN = 20, 6, (64,)


def model_envs(a, cus, n):
    """``m = ceil(rows / n)`` of a reward-model case."""
    return -(-(a * 16 * cus + 37) // n)


# ---- the plan entries at many envs x few candidates --------------------------------------------------------------------------
PLAN_SHAPES = ((40, 5), (65, 1), (33, 3))
PLAN_MODELS = {"mean_e2": dict(env="half_cheetah", mode="mean", E=2, hidden=[128, 128]),
               "single": dict(env="half_cheetah", mode="single", E=1, hidden=[128, 128])}
PLAN_H = 3
PLAN_DISCOUNT = 0.9
# (model, m, n) -> (coordinate, lower quantile or None, upper quantile or None, seed of the candidates): found on the CPU with the
# float64 oracle alone, as tests/termination_cases.py PLAN_GUARDS were (tests/test_env_layout_cases.py checks the conditions
# again): at most 1 % of the rows ambiguous, at least 20 % terminate before h, at least 20 % survive
PLAN_GUARDS = {(model, m, n): (10, 30, None, 0) for model in PLAN_MODELS for m, n in PLAN_SHAPES}
_PLAN = {}


def plan_case(model, m, n):
    """The oracle's side of a plan case, built once and never modified - the dict ``termination_cases.plan_case`` returns."""
    key = (model, m, n)
    if key not in _PLAN:
        import cases
        from learning_to_adapt_amd.utils import synthetic
        from oracle.planner import rollout_trace, sample_rs_actions
        from oracle.rewards import make_reward
        coord, ql, qh, seed = PLAN_GUARDS[key]
        case = dict(PLAN_MODELS[model], m=m, n=n, h=PLAN_H, name="layout_%s_m%d_n%d" % key, planner="rs")
        env = cases.recipe(case)[0]
        np.random.seed(seed)
        actions = sample_rs_actions(env.action_space.low, env.action_space.high, n, m, PLAN_H)
        obs0 = synthetic.make_obs0(m, env.observation_space.shape[0])
        rf = make_reward(case["env"], env.dt)
        total, trace = rollout_trace(cases.oracle_dynamics(case), rf, obs0, actions, n, PLAN_DISCOUNT)
        lo = -float("inf") if ql is None else float(np.float32(np.percentile(trace[:, :, coord], ql)))
        hi = float("inf") if qh is None else float(np.float32(np.percentile(trace[:, :, coord], qh)))
        _PLAN[key] = dict(case=case, env=env, actions=actions, obs0=obs0, obs_rows=np.repeat(obs0, n, axis=0), trace=trace,
                          total=total, guards=[(coord, 1, lo, hi)], discount=PLAN_DISCOUNT, reward_fn=rf)
    return _PLAN[key]


# ---- keys -----------------------------------------------------------------------------------------------------------------------
def key_pack(returns, index):
    """``l2a_key_pack`` (csrc/l2a_kernels.h) over arrays: the return's bits in an order in which -inf < finite < +inf < NaN and
    -0 == +0, above ``2 ** 31 - 1 - index`` - the larger key is the better return, then the lower index."""
    r = np.asarray(returns, dtype=np.float32)
    shape = r.shape
    r = np.ascontiguousarray(r).reshape(-1)
    u = r.view(np.uint32).copy()
    u[r == 0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    order = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    order[np.isnan(r)] = np.uint32(0xFFFFFFFF)
    idx = np.broadcast_to(np.asarray(index, dtype=np.int64), shape).reshape(-1)
    assert np.all(idx >= 0) and np.all(idx <= 0x7FFFFFFF)
    return ((order.astype(np.uint64) << np.uint64(31)) | (np.int64(0x7FFFFFFF) - idx).astype(np.uint64)).reshape(shape)


def want_keys(returns, cand_offset):
    """The key of the plain NumPy arg-max (first maximum; a NaN is the maximum) of every env of ``returns [m, n]``."""
    returns = np.ascontiguousarray(returns, dtype=np.float32)
    j = np.argmax(returns, axis=1)
    return key_pack(returns[np.arange(returns.shape[0]), j], int(cand_offset) + j)


def row_keys(returns, cand_offset):
    """Every row's own key, ``[m * n]``: what a kernel's epilogue packs before it reduces."""
    m, n = returns.shape
    return key_pack(returns.reshape(-1), int(cand_offset) + np.tile(np.arange(n, dtype=np.int64), m))


# ---- the two reductions -------------------------------------------------------------------------------------------------------
def value_reduce(keys, n, W, mutant=None):
    """``l2a_value_mlp_k``'s key reduction over ``keys [m * n]`` (``row_keys``) in workgroups of ``W = 16 RT`` rows: per
    workgroup, per wave, the env range, the ``swk`` words, the combine, the ``atomicMax`` on the zeroed ``best_key``."""
    assert mutant is None or mutant in VALUE_MUTANTS
    assert W in WS
    keys = [int(k) for k in keys]
    rows = len(keys)
    m = rows // n
    assert m * n == rows
    best = [0] * m                                          # hipMemsetAsync(best_key, 0)
    for r0 in range(0, rows, W):
        nr = min(W, rows - r0)
        swk = [[0, 0] for _ in range(128)]                  # zeroed at the kernel's start
        env_lo = r0 // n
        for wave in range(1 if mutant == "V1" else 2):
            if 64 * wave < nr:
                first, last = 64 * wave, min(64 * wave + 63, nr - 1)
                e0, e1 = (r0 + first) // n, (r0 + last) // n
                if mutant == "V2":
                    e1 = e0
                for e in range(e0, e1 + 1):
                    k = 0                                   # the xor butterfly: the maximum over the wave's lanes, 0 where env != e
                    for i in range(first, last + 1):
                        if (r0 + i) // n == e and keys[r0 + i] > k:
                            k = keys[r0 + i]
                    assert 0 <= e - env_lo < nr
                    swk[e - env_lo][wave] = k
        n_env = (r0 + nr - 1) // n - env_lo + 1
        assert n_env <= nr
        for t in range(n_env):
            a, b = swk[t]
            word = a if mutant == "V3" else max(a, b)
            assert env_lo + t < m
            best[env_lo + t] = max(best[env_lo + t], word)
    return np.array(best, dtype=np.uint64)


def scorer_reduce(keys, n, W, mutant=None):
    """The scorers' key reduction (``skey``, ``senv``): the first row of every env run of a workgroup walks its run."""
    assert mutant is None or mutant in SCORER_MUTANTS
    keys = [int(k) for k in keys]
    rows = len(keys)
    m = rows // n
    assert m * n == rows
    best = [0] * m
    for r0 in range(0, rows, W):
        nr = min(W, rows - r0)
        senv = [(r0 + i) // n for i in range(nr)]
        skey = keys[r0:r0 + nr]
        for tid in range(nr):
            starts = tid == 0 or senv[tid - 1] != senv[tid]
            if mutant == "S1":
                starts = tid == 0 or (tid % 16 == 0 and senv[tid - 1] != senv[tid])
            if not starts:
                continue
            stop = min(nr, (tid // 64 + 1) * 64) if mutant == "S2" else nr
            b = skey[tid]
            i = tid + 1
            while i < stop and senv[i] == senv[tid]:
                b = max(b, skey[i])
                i += 1
            best[senv[tid]] = max(best[senv[tid]], b)
    return np.array(best, dtype=np.uint64)


def gather_env(rows, n, mutant=None):
    """The ``obs0`` row every row reads at ``t = 0``: its env - with ``"G"`` the env of its 16-row tile's first row (workgroups
    start at multiples of 16, so the tile's first row is ``row & ~15`` whatever ``W``; that row exists and its env is one the
    workgroup touches)."""
    assert mutant in (None, "G")
    r = np.arange(rows, dtype=np.int64)
    if mutant == "G":
        r = r & ~np.int64(15)
    return r // n


# ---- what a layout contains ---------------------------------------------------------------------------------------------------
def facts(W, n, rows):
    """The structural facts of one layout, as counts / booleans."""
    m = rows // n
    first = np.arange(m, dtype=np.int64) * n                # an env's first and last row
    last = first + n - 1
    wg_first, wg_last = first // W, last // W
    whole_wg = wg_first == wg_last                          # envs wholly inside one workgroup ...
    interior = whole_wg & (first % W != 0) & (last % W != W - 1) & (last != rows - 1)      # ... touching neither of its ends
    per_wg = np.bincount(wg_first[interior], minlength=-(-rows // W))
    nr_last = rows - (rows - 1) // W * W
    f = dict(interior_envs=int(per_wg.max()) if per_wg.size else 0,
             run1_first=bool(np.any(last % W == 0)),        # an env run of length 1 on a workgroup's first row
             run1_last=bool(np.any((first % W == W - 1) | ((first == rows - 1) & (n == 1)))),     # ... on its last row
             three_wgs=bool(np.any(wg_last - wg_first >= 2)),
             last_rows=int(nr_last))
    if W == 128:
        f.update(in_wave1=bool(np.any(whole_wg & (first % W >= 64))),
                 across_waves=bool(np.any(whole_wg & (first % W <= 63) & (last % W >= 64))))
    return f


# ---- returns patterns --------------------------------------------------------------------------------------------------------
PLANTS = ("win_first", "win_last", "twins_wg", "twins_wave", "all_ninf", "one_nan", "all_nan")


def base_returns(seed, m, n):
    """Random DISTINCT fp32 values, multiples of 1 / 128 in (-rows / 256, rows / 256): exact in fp32 below 2 ** 24 rows."""
    rows = m * n
    assert rows < 2 ** 24
    perm = np.random.RandomState(seed).permutation(rows)
    return ((perm.astype(np.float64) - rows // 2) / 128.0).astype(np.float32).reshape(m, n)


def plant(returns, W):
    """Plants the patterns into ``returns [m, n]`` in place, each in an env of its own while there are envs left (twins first,
    then all_ninf, one_nan, all_nan, win_last, win_first; envs taken from the back, so that the ragged last workgroups get
    theirs first), and returns ``{pattern: (env, row, ...)}`` of those planted.  ``twins_*`` need an env across the boundary in
    question; n = 1 has no twins.  ``big = rows`` lies above every drawn value.  The rows that must tie are in the record, for a
    caller that has to make their other inputs equal:

      win_first / win_last   the winner on the env's first / last row
      twins_wg               two equal winners in different workgroups: the lower index must win
      twins_wave             (W = 128) two equal winners on rows 63 | 64 of one workgroup: different waves
      all_ninf               every row -inf: the key is key_pack(-inf, cand_offset), not the memset's 0
      one_nan                one NaN row behind a large finite one: the NaN wins
      all_nan                every row NaN: index 0"""
    m, n = returns.shape
    rows = m * n
    big = np.float32(rows)
    first = np.arange(m, dtype=np.int64) * n
    last = first + n - 1
    taken = set()
    out = {}

    def pick(mask):
        for e in np.nonzero(mask)[0][::-1]:                 # from the back: the ragged last workgroups get patterns first
            if int(e) not in taken:
                taken.add(int(e))
                return int(e)
        return None

    every = np.ones(m, dtype=bool)
    if n >= 2:
        e = pick(first // W != last // W)
        if e is not None:
            b = (first[e] // W + 1) * W                     # the first workgroup boundary inside env e
            j_lo, j_hi = int(b - 1 - first[e]), int(b - first[e])
            returns[e, j_lo] = returns[e, j_hi] = big
            out["twins_wg"] = (e, j_lo, j_hi)
        if W == 128:
            e = pick((first // W == last // W) & (first % W <= 63) & (last % W >= 64))
            if e is not None:
                b = first[e] // W * W + 64
                j_lo, j_hi = int(b - 1 - first[e]), int(b - first[e])
                returns[e, j_lo] = returns[e, j_hi] = big
                out["twins_wave"] = (e, j_lo, j_hi)
    e = pick(every)
    if e is not None:
        returns[e] = -np.inf
        out["all_ninf"] = (e,)
    e = pick(every)
    if e is not None:
        j = n // 2
        returns[e, 0] = big
        returns[e, j] = np.nan
        out["one_nan"] = (e, j)
    e = pick(every)
    if e is not None:
        returns[e] = np.nan
        out["all_nan"] = (e,)
    e = pick(every)
    if e is not None:
        returns[e, n - 1] = big
        out["win_last"] = (e, n - 1)
    e = pick(every)
    if e is not None:
        returns[e, 0] = big
        out["win_first"] = (e, 0)
    return out


def check_plants(returns, keys, planted, cand_offset):
    """What the planted envs' keys must be, spelled out - on top of ``keys == want_keys(returns)``."""
    m, n = returns.shape
    for name, where in planted.items():
        e = where[0]
        if name in ("twins_wg", "twins_wave"):
            assert returns[e, where[1]] == returns[e, where[2]], name
            want = key_pack(returns[e, where[1]], cand_offset + where[1])
        elif name in ("win_first", "win_last"):
            want = key_pack(returns[e, where[1]], cand_offset + where[1])
        elif name == "all_ninf":
            assert np.all(returns[e] == -np.inf)
            want = key_pack(np.float32(-np.inf), cand_offset)
            assert int(want) == (0x007FFFFF << 31) | (0x7FFFFFFF - cand_offset) and int(want) != 0
        elif name == "one_nan":
            assert np.isnan(returns[e, where[1]])
            want = key_pack(np.float32(np.nan), cand_offset + where[1])
        else:
            assert np.all(np.isnan(returns[e]))
            want = key_pack(np.float32(np.nan), cand_offset)
        assert int(keys[e]) == int(want), (name, where, hex(int(keys[e])), hex(int(want)))
