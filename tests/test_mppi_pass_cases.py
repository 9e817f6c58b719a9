"""The pass-boundary table of ``tests/mppi_pass_cases.py`` judged on the CPU, before ``tests/test_mppi_kernels_gpu.py`` runs it on
the kernel: the restatement of ``l2a_mppi_sample_k``'s pass structure equals ``mppi_reference.sample_f32`` bit for bit on every
case, and each of its three one-line mutants (filter state reset at a pass start, shifted-mean clamp at the pass end, element
index without ``t0 * A``) differs from it on every case on which the mutant is another function at all (``mppi_pass_cases.shows``:
``beta = 1`` carries no state, an env that does not shift forward reads nothing ahead - there the mutant must EQUAL the reference, so
that ``shows`` cannot hide a survivor).  A case on which a mutant survives is a mistake of the table: change its seed, ``n`` or
``beta`` until it discriminates; no tolerance is involved."""

import functools

import numpy as np
import pytest

import mppi_pass_cases as pc
import mppi_reference as mr

IDS = ["%d_h%d_A%d_n%d_m%d" % ((k,) + c[:4]) for k, c in enumerate(pc.CASES)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(index):
    inp = pc.inputs(index)
    return mr.sample_f32(inp["mean"], inp["shift"], inp["z"], inp["sigma"], inp["beta"], inp["low"], inp["high"], inp["n"], inp["m"],
                         inp["h"], inp["ad"])


def _differs(got, want):
    return not (np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])))


@pytest.mark.parametrize("index", range(len(pc.CASES)), ids=IDS)
def test_case_is_multi_pass_and_rejects_every_mutant(index):
    case = pc.CASES[index]
    h, ad, n, m, shift, beta, zero_sigma, with_seq = case
    tc = pc.PASS_STEPS(ad)
    assert h > tc
    inp = pc.inputs(index)
    want = _reference(index)
    got = pc.restate(inp)
    assert np.array_equal(_bits(got[0]), _bits(want[0])), "mean_out"
    assert np.array_equal(_bits(got[1]), _bits(want[1])), "a_clip"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), "seq"
    # a later pass is visible: some sample of a step t >= tc is not clipped away
    late = want[1].reshape(n, m, h, ad)[:, :, tc:]
    assert ((late > inp["low"]) & (late < inp["high"])).any(), "every sample behind the first pass sits on a bound"
    for mutant in pc.MUTANTS:
        assert _differs(pc.restate(inp, mutant), want) == bool(pc.shows(case, mutant)), \
            "mutant %r %s on %s" % (mutant, "survives" if pc.shows(case, mutant) else "shows where it cannot", (case,))


def test_table_covers_every_axis_and_pass_length_class():
    cases = pc.CASES
    assert 40 <= len(cases) <= 60
    assert {(c[0], c[1]) for c in cases} == set(pc.SHAPES)
    assert pc.PASS_STEPS(16) == 32 and pc.PASS_STEPS(8) == 64 and pc.PASS_STEPS(6) == 85 and pc.PASS_STEPS(1) == 512
    lengths = {s: pc.pass_lengths(*s) for s in pc.SHAPES}
    assert any(len(p) == 2 and p[-1] == 1 for p in lengths.values()), "a second pass of one step"
    assert any(len(p) == 2 and p[-1] == p[0] for p in lengths.values()), "an exact multiple"
    assert any(len(p) == 3 for p in lengths.values()), "three passes"
    assert {p[-1] % 4 for p in lengths.values()} >= {1, 2, 3}, "a last pass with nt % 4 in (1, 2, 3)"
    assert {c[2] for c in cases} >= {1, 2, 5, 9}
    rows = {(c[2] * c[3]) % pc.ROWS for c in cases}
    assert rows == {0, 1, 2, 3}, "n * m is and is not a multiple of the workgroup's rows"
    assert {tuple(c[4]) for c in cases if c[3] == 1} == {(-1,), (1,), (0,)}
    assert {tuple(c[4]) for c in cases if c[3] == 3} == {tuple(v) for v in pc.SHIFTS3}
    assert {c[5] for c in cases} == set(pc.BETAS)
    assert {c[6] is None for c in cases} == {True, False} and {c[7] for c in cases} == {True, False}
    for shape in pc.SHAPES:
        mine = [c for c in cases if (c[0], c[1]) == shape]
        assert {c[5] for c in mine} == set(pc.BETAS), shape
        assert {c[3] for c in mine} == {1, 3}, shape
        # what the GPU test's parameter for this shape can reject: every mutant, in more than one launch
        for mutant in pc.MUTANTS:
            assert sum(1 for c in mine if pc.shows(c, mutant)) >= 2, (shape, mutant)


def test_shows_is_no_wider_than_the_arithmetic():
    """``shows`` excuses a mutant only where the kernel's own arithmetic makes it the same function: ``omb = 1 - beta`` is exactly
    0 at ``beta = 1`` (and a finite state times 0 is 0), and the clamp is only evaluated for ``shift > 0``."""
    assert np.float32(1.0) - np.float32(1.0) == 0.0
    for beta in pc.BETAS[1:]:
        assert np.float32(1.0) - np.float32(beta) > 0.0
    for case in pc.CASES:
        assert pc.shows(case, "index")
        assert pc.shows(case, "reset") == (case[5] != 1.0)
        assert pc.shows(case, "clamp") == (max(case[4]) > 0)
