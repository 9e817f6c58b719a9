"""The plan rows of the MLP trajectory-rollout tests (tests/test_mlp_traj.py on the CPU, tests/test_mlp_traj_gpu.py on the GPU).

``n`` is a number, or ``("above", k)``: the smallest ragged plan whose m * ceil(n / 4) micro tiles are just above k times the CUs
that the envs share - workgroups of k + 1 and k micro tiles (``mc_r`` of the larger kind)."""

ROWS = [
    # one hidden layer forces the generic-activation instance; one ragged micro tile; 16-byte stores
    dict(id="h256x1_n3", hidden=(256,), act="relu", mode="single", E=1, od=20, ad=6, m=1, n=3, h=5),
    # dims 16 .. 19 summed per quarter (m_o4), ragged last quad, two envs of one set
    dict(id="h512x2_o4_n37", hidden=(512, 512), act="relu", mode="single", E=1, od=20, ad=6, m=2, n=37, h=2),
    # tanh, dword stores (obs_dim 17: one padding lane of three), workgroups of two and one micro tile
    dict(id="h256x2_tanh_above_cus", hidden=(256, 256), act="tanh", mode="single", E=1, od=17, ad=6, m=1, n=("above", 1), h=2),
    # per-block sets, Ant-like action width, obs_dim 18 (dword stores, two padding lanes), workgroups of three and two micro tiles
    dict(id="h512x3_pb_above_2cus", hidden=(512, 512, 512), act="relu", mode="per_block", E=2, od=18, ad=8, m=2, n=("above", 2), h=1),
    # mean of two sets, obs_dim 49: four observation tiles, more than three quarter blocks
    dict(id="h512x2_mean2_od49", hidden=(512, 512), act="relu", mode="mean", E=2, od=49, ad=6, m=1, n=37, h=5),
    # mean of three sets (groups A and B unequal), workgroups of two and one micro tile
    dict(id="h512x2_mean3_above_cus", hidden=(512, 512), act="relu", mode="mean", E=3, od=20, ad=6, m=1, n=("above", 1), h=2),
]


def row_n(row, cus):
    n = row["n"]
    if isinstance(n, tuple):
        quads = n[1] * (cus // row["m"]) + 1
        return 4 * quads - 1
    return n
