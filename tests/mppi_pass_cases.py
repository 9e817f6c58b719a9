"""Horizons longer than one LDS pass of ``l2a_mppi_sample_k`` (``csrc/l2a_mppi.hip``): the case table that
``tests/test_mppi_kernels_gpu.py`` runs on the GPU, and a NumPy restatement of the kernel's PASS STRUCTURE (no GPU, no library
calls) with which ``tests/test_mppi_pass_cases.py`` proves on the CPU that the table tells a correct pass loop from a broken one.

The kernel gives a workgroup four sample rows and walks the horizon in passes of ``PASS_STEPS(act_dim)`` steps.  Between two passes
the filter state stays in a register, the element index of the normal picks up ``t0 * A``, a shifted mean reads ``mean_in`` at
``t + 1`` - the last step of a pass reads the first step of the next one - and ``mean_out``, ``a_clip`` and ``seq`` are stored pass by
pass.  ``mppi_reference.sample_f32`` knows nothing of passes; ``restate`` does, and takes one of three one-line mutants:

  ``"reset"``  the filter state is zeroed at each pass start;
  ``"clamp"``  the shifted mean's ``min(t + 1, h - 1)`` stops at the pass end instead of ``h - 1``;
  ``"index"``  the normal's element index drops ``t0 * A``.

Two of them are the SAME function as the kernel on part of the input space, whatever the horizon (``shows``): without a carried
state (``beta = 1``: ``1 - beta = 0`` multiplies it away) there is nothing to reset, and without an env that shifts forward nothing
is read ahead.  The table must cover ``beta = 1`` and the non-positive shifts all the same, so the CPU test holds every case to
"the mutant differs exactly where it can", and every ``(h, A)`` to several cases that reject each mutant."""

import numpy as np

ROWS = 4            # csrc/l2a_mppi.hip: L2A_MPPI_ROWS, the sample rows of one workgroup
TILE = 2048         # csrc/l2a_mppi.hip: L2A_MPPI_TILE, the floats of one LDS tile (ROWS x steps per pass x act_dim)
MUTANTS = ("reset", "clamp", "index")


def PASS_STEPS(act_dim):
    """Horizon steps per pass: ``L2A_MPPI_TILE / (L2A_MPPI_ROWS * act_dim) = 512 // act_dim``."""
    return TILE // (ROWS * act_dim)


# (h, A): a second pass of one step (its tail loop only) | two full passes | three passes, the last with nt % 4 = 2 | 85 + 1 |
# 85 + 85 + 5 (nt % 4 = 1) | 46 + 1 at a width that divides nothing | 512 + 1 at A = 1 | a last pass with nt % 4 = 3
SHAPES = ((33, 16), (64, 16), (70, 16), (86, 6), (175, 6), (47, 11), (513, 1), (35, 16))
# candidates: with m in (1, 3) the row counts 1 .. 27 leave partial last workgroups of 1, 2 and 3 rows; n = 4 adds the counts (4,
# 12) that are a multiple of the workgroup's four rows
NS = (1, 2, 5, 9, 4)
SHIFTS1 = ([-1], [1], [0])
SHIFTS3 = ([-1, 1, 0], [1, 0, -1], [0, -1, 1], [1, 1, 1], [0, 0, 0], [-1, -1, 1])
BETAS = (1.0, 0.6, 2.0 ** -10)
PER_SHAPE = 7       # launches per (h, A): 56 in all


def _table():
    """``(h, act_dim, n, m, shift, beta, zero_sigma, with_seq)``: not a product - one counter walks the axes with different periods
    (``tests/test_mppi_pass_cases.py`` states what the walk covers: every shape meets every beta and both ``m``; the table every
    shift vector and every row count modulo four).  ``sigma = 0`` in one dimension in every third case - never at A = 1, where it
    would silence the whole draw - and ``seq`` absent in every fifth."""
    out = []
    c = 0
    for h, ad in SHAPES:
        for j in range(PER_SHAPE):
            m = (1, 3)[j % 2]
            k = c // 2                      # moves on once per (m = 1, m = 3) pair
            n = NS[c % 5]
            shift = SHIFTS3[k % 6] if m == 3 else SHIFTS1[k % 3]
            beta = BETAS[(k + k // 3 + j % 2) % 3]
            zero_sigma = (c % ad) if (c % 3 == 0 and ad > 1) else None
            with_seq = c % 5 != 4
            out.append((h, ad, n, m, list(shift), beta, zero_sigma, with_seq))
            c += 1
    return tuple(out)


CASES = _table()


def seed_of(index):
    """The seed of ``CASES[index]``'s inputs, on the CPU and on the GPU."""
    return 5000 + index


def bounds(ad):
    """The action bounds of ``tests/test_mppi_kernels_gpu.py``."""
    return np.linspace(-0.8, -0.3, ad).astype(np.float32), np.linspace(0.4, 0.9, ad).astype(np.float32)


def inputs(index):
    """The inputs of ``CASES[index]`` as ``test_mppi_kernels_gpu.sample_inputs`` draws them (the dict ``run_sample`` takes)."""
    h, ad, n, m, shift, beta, zero_sigma, _ = CASES[index]
    rs = np.random.RandomState(seed_of(index))
    D = h * ad
    low, high = bounds(ad)
    sigma = (0.1 + 0.5 * rs.rand(ad)).astype(np.float32)
    if zero_sigma is not None:
        sigma[zero_sigma] = 0.0
    mean = (0.7 * rs.randn(m, D)).astype(np.float32)            # beyond both bounds in some dimensions
    z = rs.randn(n, m, D).astype(np.float32)
    return dict(n=n, m=m, h=h, ad=ad, beta=beta, shift=np.asarray(shift, dtype=np.int32), mean=mean, sigma=sigma, low=low, high=high,
                z=z, seed=0, off=0)


def shows(case, mutant):
    """Whether ``mutant`` is another function than the kernel on this case's inputs at all (module docstring)."""
    _, _, _, _, shift, beta, _, _ = case
    if mutant == "reset":
        return np.float32(beta) < np.float32(1.0)
    if mutant == "clamp":
        return any(s > 0 for s in shift)
    return True


def pass_lengths(h, ad):
    tc = PASS_STEPS(ad)
    return [min(tc, h - t0) for t0 in range(0, h, tc)]


def restate(inp, mutant=None):
    """``(mean_out [m, D], a_clip [n, m, D], seq [h, m * n, A])`` in ``np.float32``, computed the way the kernel walks: workgroups of
    four rows; per pass the tiles are filled (u = z * sigma, the shifted mean), the chains run over the tile with the state carried
    from the pass before, and the tile is stored - ``a_clip`` at ``t0 * A + rem``, ``seq`` at step ``t0 + tt``, the shifted mean by
    the rows of candidate 0.  Every output starts as NaN: an element no pass stores stays NaN."""
    assert mutant is None or mutant in MUTANTS
    f32 = np.float32
    n, m, h, A = inp["n"], inp["m"], inp["h"], inp["ad"]
    D = h * A
    rows = n * m
    tc = PASS_STEPS(A)
    z = np.ascontiguousarray(inp["z"], dtype=f32).reshape(-1)
    mean_in = np.ascontiguousarray(inp["mean"], dtype=f32).reshape(-1)
    sigma, low, high = (np.asarray(inp[k], dtype=f32) for k in ("sigma", "low", "high"))
    beta = f32(inp["beta"])
    omb = f32(f32(1.0) - beta)
    mean_out = np.full(m * D, np.nan, dtype=f32)
    a_clip = np.full(rows * D, np.nan, dtype=f32)
    seq = np.full(h * rows * A, np.nan, dtype=f32)
    kk = np.arange(A)
    for g0 in range(0, rows, ROWS):
        nr = min(ROWS, rows - g0)
        nz = np.zeros((nr, A), dtype=f32)                       # one register per chain (row, action dimension)
        for t0 in range(0, h, tc):
            nt = min(tc, h - t0)
            tile = np.empty((nr, nt, A), dtype=f32)
            mtile = np.empty((nr, nt, A), dtype=f32)
            rem = (np.arange(nt)[:, None] * A + kk[None, :])    # tt * A + k
            t = t0 + np.arange(nt)
            for r in range(nr):
                g = g0 + r
                i = g % m
                sh = int(inp["shift"][i])
                last = (t0 + nt - 1) if mutant == "clamp" else (h - 1)
                ts = np.minimum(t + 1, last) if sh > 0 else t
                mtile[r] = f32(0.0) if sh < 0 else mean_in[i * D + ts[:, None] * A + kk[None, :]]
                e = g * D + (0 if mutant == "index" else t0 * A) + rem
                tile[r] = z[e] * sigma[None, :]
            if mutant == "reset":
                nz = np.zeros((nr, A), dtype=f32)
            for tt in range(nt):
                bu = beta * tile[:, tt]
                kn = omb * nz
                nz = bu + kn
                a = mtile[:, tt] + nz
                tile[:, tt] = np.minimum(np.maximum(a, low), high)
                assert nz.dtype == f32 and a.dtype == f32
            for r in range(nr):
                g = g0 + r
                j, i = divmod(g, m)
                a_clip[g * D + t0 * A + rem] = tile[r]
                prow = i * n + j
                seq[((t[:, None]) * rows + prow) * A + kk[None, :]] = tile[r]
                if j == 0:
                    mean_out[i * D + t0 * A + rem] = mtile[r]
    return mean_out.reshape(m, D), a_clip.reshape(n, m, D), seq.reshape(h, rows, A)
