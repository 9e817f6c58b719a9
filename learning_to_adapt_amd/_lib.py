"""ctypes binding of ``libl2a_hip.so`` (C ABI: ``include/l2a.h``).

There is deliberately no fallback: if the shared library is missing or a call fails, an
exception is raised.  The CPU oracle under ``oracle/`` is test infrastructure and is never
imported from here.
"""

import ctypes
import json
import os

from .envs.reward_spec import RewardProgram, RewardSpec
from .envs.termination import TerminationProgram

_HERE = os.path.dirname(os.path.abspath(__file__))
# L2A_LIB_PATH: developer override for kernel A/B runs (tools/build_variant.py); the product loads the in-tree build
LIB_PATH = os.environ.get("L2A_LIB_PATH") or os.path.join(_HERE, "libl2a_hip.so")

# include/l2a.h
L2A_OK = 0
L2A_EINVAL = -1
L2A_ESTATE = -4
L2A_ESPLIT = -5
L2A_STEP_MISS = 1
L2A_STEP_UNSPLIT = 2
L2A_STEP_DREW = 3
ACT_CODES = {None: 0, "identity": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "swish": 4}
MODE_CODES = {"single": 0, "per_block": 1, "mean": 2}
KERNEL_CODES = {"auto": 0, "mfma": 1, "valu": 2}
CELL_CODES = {"lstm": 0, "gru": 1, "rnn": 2}

EXPORTED_SYMBOLS = (
    "l2a_init", "l2a_destroy", "l2a_last_error", "l2a_device_info", "l2a_set_kernel", "l2a_set_split", "l2a_set_batch", "l2a_set_xcd_align", "l2a_set_fan", "l2a_set_double_rounds", "l2a_set_seq3", "l2a_set_micro",
    "l2a_launch_status", "l2a_set_debug_buffer", "l2a_set_spin_limit", "l2a_inject_status",
    "l2a_model_create", "l2a_model_destroy", "l2a_model_set_weights", "l2a_model_set_weights_strided",
    "l2a_model_set_norm", "l2a_model_adapt_sgd", "l2a_model_adapt_sgd_host", "l2a_model_adapt_sgd_raw", "l2a_model_get_weights",
    "l2a_plan_rs", "l2a_plan_rs_sync", "l2a_plan_rs_chunk", "l2a_reward_program_check", "l2a_score_trajectory", "l2a_plan_rs_program",
    "l2a_reward_model_check", "l2a_reward_model_geometry", "l2a_reward_model_create", "l2a_reward_model_destroy", "l2a_reward_model_set_weights", "l2a_reward_model_set_norm",
    "l2a_reward_model_predict", "l2a_score_trajectory_model", "l2a_plan_rs_reward_model", "l2a_predict", "l2a_key_encode", "l2a_key_decode", "l2a_mfma_eligible", "l2a_plan_geometry", "l2a_plan_geometry_ex",
    "l2a_packed_layer_floats", "l2a_pack_layer_host", "l2a_micro_layout_floats", "l2a_micro_pack_layer_host",
    "l2a_comm_unique_id", "l2a_comm_init", "l2a_comm_destroy", "l2a_allreduce_best", "l2a_plan_payload",
    "l2a_cem_sample", "l2a_cem_refit", "l2a_cem_pick", "l2a_cem_refit_sample", "l2a_cem_refit_sample_fused",
    "l2a_mppi_sample", "l2a_mppi_update", "l2a_mppi_sample_shard",
    "l2a_icem_sample", "l2a_icem_refit",
    "l2a_mppi_controller_create_device", "l2a_mppi_controller_create_sharded_device", "l2a_mppi_controller_reset",
    "l2a_mppi_controller_reseed", "l2a_mppi_controller_result",
    "l2a_icem_sample_shard", "l2a_icem_controller_create_device", "l2a_icem_controller_create_sharded_device", "l2a_icem_controller_reset",
    "l2a_icem_controller_reseed", "l2a_icem_controller_result",
    "l2a_icem_noise_matrix", "l2a_icem_sample_noise", "l2a_icem_sample_noise_shard", "l2a_icem_controller_set_noise",
    "l2a_lstm_create", "l2a_rnn_create", "l2a_lstm_destroy", "l2a_lstm_set_weights", "l2a_lstm_set_norm", "l2a_lstm_plan_rs", "l2a_lstm_plan_rs_sync", "l2a_lstm_plan_rs_chunk",
    "l2a_lstm_predict", "l2a_lstm_advance", "l2a_lstm_mfma_eligible",
    "l2a_lstm_rollout_traj", "l2a_lstm_plan_rs_program", "l2a_lstm_plan_rs_reward_model", "l2a_lstm_traj_geometry", "l2a_lstm_plan_geometry",
    "l2a_rollout_traj", "l2a_mlp_traj_geometry",
    "l2a_value_model_check", "l2a_value_model_geometry", "l2a_value_model_create", "l2a_value_model_destroy", "l2a_value_model_set_weights",
    "l2a_value_model_set_norm", "l2a_value_model_predict", "l2a_value_terminal", "l2a_plan_rs_value", "l2a_plan_rs_program_value",
    "l2a_plan_rs_reward_model_value",
    "l2a_policy_model_check", "l2a_policy_model_geometry", "l2a_policy_model_create", "l2a_policy_model_destroy",
    "l2a_policy_model_set_weights", "l2a_policy_model_set_norm", "l2a_policy_act", "l2a_policy_propose",
    "l2a_termination_check", "l2a_score_trajectory_term", "l2a_plan_rs_term",
    "l2a_particle_score", "l2a_plan_rs_particles", "l2a_plan_rs_particles_program", "l2a_plan_rs_particles_reward_model",
    "l2a_particle_perm", "l2a_particle_shuffle", "l2a_plan_rs_particles_ts1",
    "l2a_particle_step", "l2a_plan_rs_particles_ts1_program", "l2a_plan_rs_particles_ts1_reward_model",
    "l2a_controller_create", "l2a_controller_create_sharded", "l2a_controller_create_sharded_device", "l2a_lstm_controller_create", "l2a_controller_create_device", "l2a_lstm_controller_create_device",
    "l2a_lstm_controller_create_sharded", "l2a_lstm_controller_create_sharded_device",
    "l2a_controller_destroy", "l2a_controller_step", "l2a_controller_begin", "l2a_lstm_controller_begin", "l2a_controller_finish",
    "l2a_lstm_controller_step", "l2a_controller_rearm", "l2a_controller_actions", "l2a_controller_stats",
    "l2a_cem_controller_create_device", "l2a_cem_controller_result",
    "l2a_cem_shard_pack", "l2a_cem_shard_unpack", "l2a_cem_word_encode", "l2a_cem_word_decode", "l2a_cem_controller_create_sharded_device",
    "l2a_cem_pick_act", "l2a_lstm_cem_controller_create_device", "l2a_lstm_cem_controller_create_sharded_device",
)


class L2AError(RuntimeError):
    pass


def lstm_traj_geometry(obs_dim, act_dim, units, m, n, h, micro=1, cus=0):
    """Which path ``l2a_lstm_rollout_traj`` takes for one LSTM layer of ``units`` (``l2a_lstm_traj_geometry``: the launcher's own
    decision function, no GPU needed) under micro policy ``micro`` on ``cus`` CUs (0: 256).  Returns a dict: single (one launch of
    the trajectory-writing micro-tile instance) or the carry chain, launches, workgroups, workgroups_per_env, micro_tiles (of the
    largest workgroup; 99: none fits), full_workgroups (per env, of that size)."""
    lib = load()
    out = (ctypes.c_int * 8)()
    rc = lib.l2a_lstm_traj_geometry(int(obs_dim), int(act_dim), int(units), int(m), int(n), int(h), int(micro), int(cus), out)
    if rc != L2A_OK:
        raise L2AError("l2a_lstm_traj_geometry failed (%d)" % rc)
    v = list(out)
    return dict(single=bool(v[0]), launches=v[1], workgroups=v[2], workgroups_per_env=v[3], micro_tiles=v[4], full_workgroups=v[5])


def mlp_traj_geometry(obs_dim, act_dim, n_hidden, hidden, mode, n_sets, m, n, h, micro=1, cus=0):
    """Which path ``l2a_rollout_traj`` takes for ``n_hidden`` layers of ``hidden`` units with ``n_sets`` weight sets in ``mode``
    ('single' | 'per_block' | 'mean') (``l2a_mlp_traj_geometry``: the launcher's own decision function, no GPU needed) under micro
    policy ``micro`` on ``cus`` CUs (0: 256).  Returns a dict: single (one launch of the trajectory-writing micro-tile instance) or
    the carry chain, launches, workgroups, workgroups_per_env, micro_tiles (of the largest workgroup; 99: none fits),
    full_workgroups (per env, of that size)."""
    lib = load()
    out = (ctypes.c_int * 8)()
    rc = lib.l2a_mlp_traj_geometry(int(obs_dim), int(act_dim), int(n_hidden), int(hidden), MODE_CODES[mode], int(n_sets), int(m), int(n),
                                   int(h), int(micro), int(cus), out)
    if rc != L2A_OK:
        raise L2AError("l2a_mlp_traj_geometry failed (%d)" % rc)
    v = list(out)
    return dict(single=bool(v[0]), launches=v[1], workgroups=v[2], workgroups_per_env=v[3], micro_tiles=v[4], full_workgroups=v[5])


def plan_geometry(obs_dim, act_dim, hidden, n_sets, mode, m, n, h, split=-1, fan=-1, micro=-1, cus=0, double=-1, batch=-1, seq3=-1):
    """The launch geometry the library would pick for this plan (``l2a_plan_geometry``: the launcher's own decision code, no
    GPU needed).  Returns a dict: kernel ('valu' | 'mfma16' | 'micro'), nt, split (0 none, 1 whole sets, 2 shared half member,
    3 member fan), split_from, fan, workgroups, lds_bytes, sets_per_batch, micro_tiles, placement_units, front_workgroups
    (double-tile workgroups of a launch IN FRONT of the described one: ``l2a_set_double_rounds``), whole_instance (the
    described launch runs on a whole-tiles-only kernel instance), seq3 (it runs on a static three-set-step instance:
    ``l2a_set_seq3``).  ``batch`` / ``seq3``: the policies of ``l2a_set_batch`` / ``l2a_set_seq3`` (-1 = their defaults)."""
    lib = load()
    hid = (ctypes.c_int * len(hidden))(*[int(x) for x in hidden])
    pol = (ctypes.c_int * 7)(int(split), int(fan), int(micro), int(cus), int(double), int(batch), int(seq3))
    out = (ctypes.c_int * 13)()
    if hasattr(lib, "l2a_plan_geometry_ex"):
        rc = lib.l2a_plan_geometry_ex(int(obs_dim), int(act_dim), len(hidden), hid, int(n_sets), MODE_CODES[mode], int(m), int(n), int(h),
                                      pol, 7, out, 13)
    else:       # (an older variant library selected with L2A_LIB_PATH: neither the two policies nor the field)
        rc = lib.l2a_plan_geometry(int(obs_dim), int(act_dim), len(hidden), hid, int(n_sets), MODE_CODES[mode], int(m), int(n), int(h), pol, out)
    if rc != L2A_OK:
        raise L2AError("l2a_plan_geometry failed (%d)" % rc)
    v = list(out)
    return dict(kernel=("valu", "mfma16", "micro")[v[0]], nt=v[1], split=v[2], split_from=v[3], fan=bool(v[4]), workgroups=v[5],
                lds_bytes=v[6], sets_per_batch=v[7], micro_tiles=v[8], placement_units=v[9], front_workgroups=v[10],
                whole_instance=bool(v[11]), seq3=bool(v[12]))


LSTM_FAMILIES = ("lstm_valu", "lstm_mfma16", "lstm_micro", "lstm_micro_traj", "generic_valu", "generic_mfma16", "generic_micro")
LSTM_REQUEST_BITS = {"per_row": 1, "state_out": 2, "no_results": 4, "no_split": 8, "traj": 16}


def lstm_plan_geometry(obs_dim, act_dim, units, cell, m, n, h, request=(), kernel="auto", split=-1, micro=-1, cus=0, lds=0):
    """The launch the recurrent launcher would pick (``l2a_lstm_plan_geometry``: its own plan function, no GPU needed) for the
    model ``l2a_rnn_create`` builds from ``units`` (a list: one entry per layer; an int: the model of ``l2a_lstm_create``).
    ``request``: names of ``LSTM_REQUEST_BITS``.  Returns a dict: family (``LSTM_FAMILIES``), mtm, split, workgroups, lds_bytes,
    tiles_per_env, mc_w, mc_hi, mc_r, exchange_bytes, publish."""
    lib = load()
    layers = [int(units)] if isinstance(units, int) else [int(x) for x in units]
    arr = (ctypes.c_int * len(layers))(*layers)
    pol = (ctypes.c_int * 5)(KERNEL_CODES[kernel], int(split), int(micro), int(cus), int(lds))
    out = (ctypes.c_int * 12)()
    rc = lib.l2a_lstm_plan_geometry(int(obs_dim), int(act_dim), 0 if isinstance(units, int) else len(layers), arr, CELL_CODES[cell],
                                    int(m), int(n), int(h), sum(LSTM_REQUEST_BITS[r] for r in request), pol, out)
    if rc != L2A_OK:
        raise L2AError("l2a_lstm_plan_geometry failed (%d)" % rc)
    v = list(out)
    return dict(family=LSTM_FAMILIES[v[0]], mtm=v[1], split=v[2], workgroups=v[3], lds_bytes=v[4], tiles_per_env=v[5], mc_w=v[6],
                mc_hi=v[7], mc_r=v[8], exchange_bytes=v[9], publish=bool(v[10]))


def reward_model_check(obs_dim, act_dim, hidden, hidden_act):
    """``l2a_reward_model_check`` (host only, no GPU): ``None`` when the matrix-core reward scorer takes this network, else the
    library's reason.  ``hidden_act``: a nonlinearity name (``ACT_CODES``) or an integer code."""
    lib = load()
    hid = (ctypes.c_int * max(len(hidden), 1))(*[int(x) for x in hidden])
    code = hidden_act if isinstance(hidden_act, int) else ACT_CODES.get(hidden_act, -1)
    rc = lib.l2a_reward_model_check(int(obs_dim), int(act_dim), len(hidden), hid, int(code))
    return None if rc == L2A_OK else lib.l2a_last_error(None).decode()


def reward_model_geometry(obs_dim, act_dim, hidden, rows, h, cus=0, lds_per_block=160 * 1024):
    """The launch geometry of the reward-model scorer (``l2a_reward_model_geometry``: the launcher's own decision function, no
    GPU needed) for ``rows`` candidates over ``h`` steps on ``cus`` CUs (0: 256) with ``lds_per_block`` bytes of LDS.  Returns a
    dict: RT (row tiles per pass), CT (candidate tiles per workgroup), S (steps per pass), workgroups, passes, lds_bytes."""
    lib = load()
    hid = (ctypes.c_int * max(len(hidden), 1))(*[int(x) for x in hidden])
    out = (ctypes.c_int * 8)()
    rc = lib.l2a_reward_model_geometry(int(obs_dim), int(act_dim), len(hidden), hid, int(rows), int(h), int(cus), int(lds_per_block), out)
    if rc != L2A_OK:
        raise L2AError("l2a_reward_model_geometry failed (%d): %s" % (rc, lib.l2a_last_error(None).decode()))
    v = list(out)
    return dict(RT=v[0], CT=v[1], S=v[2], workgroups=v[3], passes=v[4], lds_bytes=v[5])


def value_model_check(obs_dim, hidden, hidden_act):
    """``l2a_value_model_check`` (host only, no GPU): ``None`` when the terminal-value kernel takes this network, else the
    library's reason.  ``hidden_act``: a nonlinearity name (``ACT_CODES``) or an integer code."""
    lib = load()
    hid = (ctypes.c_int * max(len(hidden), 1))(*[int(x) for x in hidden])
    code = hidden_act if isinstance(hidden_act, int) else ACT_CODES.get(hidden_act, -1)
    rc = lib.l2a_value_model_check(int(obs_dim), len(hidden), hid, int(code))
    return None if rc == L2A_OK else lib.l2a_last_error(None).decode()


def value_model_geometry(obs_dim, hidden, rows, cus=0, lds_per_block=160 * 1024):
    """The launch geometry of the terminal-value kernel (``l2a_value_model_geometry``: the launcher's own decision function, no
    GPU needed) for ``rows`` states on ``cus`` CUs (0: 256) with ``lds_per_block`` bytes of LDS.  Returns a dict: RT (row tiles
    of 16 rows per workgroup), workgroups, lds_bytes."""
    lib = load()
    hid = (ctypes.c_int * max(len(hidden), 1))(*[int(x) for x in hidden])
    out = (ctypes.c_int * 8)()
    rc = lib.l2a_value_model_geometry(int(obs_dim), len(hidden), hid, int(rows), int(cus), int(lds_per_block), out)
    if rc != L2A_OK:
        raise L2AError("l2a_value_model_geometry failed (%d): %s" % (rc, lib.l2a_last_error(None).decode()))
    v = list(out)
    return dict(RT=v[0], workgroups=v[1], lds_bytes=v[2])


def _policy_symbols(lib):
    if not hasattr(lib, "l2a_policy_model_create"):
        raise L2AError("the loaded library (%s) has no l2a_policy_model_* entries: it predates policy priors - rebuild it" % LIB_PATH)


def policy_model_check(obs_dim, act_dim, hidden, hidden_act):
    """``l2a_policy_model_check`` (host only, no GPU): ``None`` when the policy kernel takes this network, else the library's
    reason.  ``hidden_act``: a nonlinearity name (``ACT_CODES``) or an integer code."""
    lib = load()
    _policy_symbols(lib)
    hid = (ctypes.c_int * max(len(hidden), 1))(*[int(x) for x in hidden])
    code = hidden_act if isinstance(hidden_act, int) else ACT_CODES.get(hidden_act, -1)
    rc = lib.l2a_policy_model_check(int(obs_dim), int(act_dim), len(hidden), hid, int(code))
    return None if rc == L2A_OK else lib.l2a_last_error(None).decode()


def policy_model_geometry(obs_dim, act_dim, hidden, rows, cus=0, lds_per_block=160 * 1024):
    """The launch geometry of the policy kernel (``l2a_policy_model_geometry``: the launcher's own decision function, no GPU
    needed) for ``rows`` states on ``cus`` CUs (0: 256) with ``lds_per_block`` bytes of LDS.  Returns a dict: RT (row tiles of 16
    rows per workgroup), workgroups, lds_bytes."""
    lib = load()
    _policy_symbols(lib)
    hid = (ctypes.c_int * max(len(hidden), 1))(*[int(x) for x in hidden])
    out = (ctypes.c_int * 8)()
    rc = lib.l2a_policy_model_geometry(int(obs_dim), int(act_dim), len(hidden), hid, int(rows), int(cus), int(lds_per_block), out)
    if rc != L2A_OK:
        raise L2AError("l2a_policy_model_geometry failed (%d): %s" % (rc, lib.l2a_last_error(None).decode()))
    v = list(out)
    return dict(RT=v[0], workgroups=v[1], lds_bytes=v[2])


_lib = None


def load():
    """Load the shared library (once) and declare every prototype of include/l2a.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise L2AError(
            "%s not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    # PyTorch-ROCm brings its own HIP runtime and has to be in the process FIRST: loaded behind libl2a_hip.so (which pulls in the
    # system's), the process holds two runtimes and l2a_init finds "no ROCm-capable device" once torch has opened the GPU
    # (`build()` followed by `smoke()` in one interpreter did).  Importing torch touches no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass            # plain C-ABI use without PyTorch
    lib = ctypes.CDLL(LIB_PATH)
    c = ctypes
    vp, i32, f32 = c.c_void_p, c.c_int, c.c_float
    lib.l2a_init.argtypes = [i32, c.POINTER(vp)]
    lib.l2a_init.restype = i32
    lib.l2a_destroy.argtypes = [vp]
    lib.l2a_destroy.restype = None
    lib.l2a_last_error.argtypes = [vp]
    lib.l2a_last_error.restype = c.c_char_p
    lib.l2a_device_info.argtypes = [vp, c.c_char_p, i32]
    lib.l2a_device_info.restype = i32
    lib.l2a_set_kernel.argtypes = [vp, i32]
    lib.l2a_set_kernel.restype = i32
    lib.l2a_set_split.argtypes = [vp, i32]
    lib.l2a_set_split.restype = i32
    if os.environ.get("L2A_LIB_PATH") and not hasattr(lib, "l2a_set_batch"):
        lib.l2a_set_batch = lambda handle, sets: 0         # developer A/B against a library of an earlier round
    else:
        lib.l2a_set_batch.argtypes = [vp, i32]
        lib.l2a_set_batch.restype = i32
    if os.environ.get("L2A_LIB_PATH") and not hasattr(lib, "l2a_set_micro"):
        lib.l2a_set_micro = lambda handle, policy: 0
    else:
        lib.l2a_set_micro.argtypes = [vp, i32]
        lib.l2a_set_micro.restype = i32
    if os.environ.get("L2A_LIB_PATH") and not hasattr(lib, "l2a_set_fan"):
        lib.l2a_set_fan = lambda handle, on: 0
    else:
        lib.l2a_set_fan.argtypes = [vp, i32]
        lib.l2a_set_fan.restype = i32
    if os.environ.get("L2A_LIB_PATH") and not hasattr(lib, "l2a_set_seq3"):
        lib.l2a_set_seq3 = lambda handle, on: 0
    else:
        lib.l2a_set_seq3.argtypes = [vp, i32]
        lib.l2a_set_seq3.restype = i32
    if os.environ.get("L2A_LIB_PATH") and not hasattr(lib, "l2a_set_double_rounds"):
        lib.l2a_set_double_rounds = lambda handle, on: 0
    else:
        lib.l2a_set_double_rounds.argtypes = [vp, i32]
        lib.l2a_set_double_rounds.restype = i32
    if os.environ.get("L2A_LIB_PATH") and not hasattr(lib, "l2a_set_xcd_align"):
        lib.l2a_set_xcd_align = lambda handle, on: 0
    else:
        lib.l2a_set_xcd_align.argtypes = [vp, i32]
        lib.l2a_set_xcd_align.restype = i32
    lib.l2a_launch_status.argtypes = [vp, c.POINTER(i32)]
    lib.l2a_launch_status.restype = i32
    lib.l2a_set_debug_buffer.argtypes = [vp, vp]
    lib.l2a_set_debug_buffer.restype = i32
    lib.l2a_set_spin_limit.argtypes = [vp, c.c_uint]
    lib.l2a_set_spin_limit.restype = i32
    lib.l2a_inject_status.argtypes = [vp, i32]
    lib.l2a_inject_status.restype = i32
    lib.l2a_model_create.argtypes = [vp, i32, i32, i32, c.POINTER(i32), i32, i32, i32, i32, c.POINTER(vp)]
    lib.l2a_model_create.restype = i32
    lib.l2a_model_destroy.argtypes = [vp]
    lib.l2a_model_destroy.restype = None
    lib.l2a_model_set_weights.argtypes = [vp, i32, c.POINTER(vp), vp]
    lib.l2a_model_set_weights.restype = i32
    lib.l2a_model_set_weights_strided.argtypes = [vp, i32, i32, c.POINTER(vp), c.POINTER(c.c_longlong), vp]
    lib.l2a_model_set_weights_strided.restype = i32
    lib.l2a_model_adapt_sgd.argtypes = [vp, c.POINTER(vp), vp, vp, i32, i32, f32, vp]
    lib.l2a_model_adapt_sgd.restype = i32
    lib.l2a_model_adapt_sgd_host.argtypes = [vp, c.POINTER(vp), vp, vp, i32, i32, f32, vp]
    lib.l2a_model_adapt_sgd_host.restype = i32
    lib.l2a_model_adapt_sgd_raw.argtypes = [vp, c.POINTER(vp), vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp]
    lib.l2a_model_adapt_sgd_raw.restype = i32
    lib.l2a_model_get_weights.argtypes = [vp, i32, c.POINTER(vp), vp]
    lib.l2a_model_get_weights.restype = i32
    dp = c.POINTER(c.c_double)
    lib.l2a_model_set_norm.argtypes = [vp, i32, dp, dp, dp, dp, dp, dp, vp]
    lib.l2a_model_set_norm.restype = i32
    lib.l2a_plan_rs.argtypes = [vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardSpec), i32, vp, vp, vp]
    lib.l2a_plan_rs.restype = i32
    lib.l2a_plan_rs_sync.argtypes = [vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardSpec), i32, vp, vp, vp]
    lib.l2a_plan_rs_sync.restype = i32
    lib.l2a_plan_rs_chunk.argtypes = [vp, vp, i32, vp, i32, i32, i32, i32, c.c_double, c.POINTER(RewardSpec), i32, vp, vp, vp, vp, vp]
    lib.l2a_plan_rs_chunk.restype = i32
    lib.l2a_reward_program_check.argtypes = [c.POINTER(RewardProgram), i32, i32]
    lib.l2a_reward_program_check.restype = i32
    lib.l2a_score_trajectory.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, c.c_double, c.POINTER(RewardProgram), i32, vp, vp, vp]
    lib.l2a_score_trajectory.restype = i32
    lib.l2a_plan_rs_program.argtypes = [vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardProgram), i32, vp, vp, vp, vp]
    lib.l2a_plan_rs_program.restype = i32
    if hasattr(lib, "l2a_termination_check"):           # (absent from older variant libraries selected with L2A_LIB_PATH)
        tp = c.POINTER(TerminationProgram)
        lib.l2a_termination_check.argtypes = [tp, i32]
        lib.l2a_termination_check.restype = i32
        lib.l2a_score_trajectory_term.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, c.c_double, c.POINTER(RewardProgram), tp,
                                                  vp, c.c_double, i32, vp, vp, vp, vp]
        lib.l2a_score_trajectory_term.restype = i32
        lib.l2a_plan_rs_term.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardProgram), tp, c.c_double, i32,
                                         vp, vp, vp, vp, vp]
        lib.l2a_plan_rs_term.restype = i32
    if hasattr(lib, "l2a_value_model_create"):          # (absent from older variant libraries selected with L2A_LIB_PATH)
        dbl = c.c_double
        lib.l2a_value_model_check.argtypes = [i32, i32, c.POINTER(i32), i32]
        lib.l2a_value_model_check.restype = i32
        lib.l2a_value_model_geometry.argtypes = [i32, i32, c.POINTER(i32), c.c_longlong, i32, i32, c.POINTER(i32)]
        lib.l2a_value_model_geometry.restype = i32
        lib.l2a_value_model_create.argtypes = [vp, i32, i32, c.POINTER(i32), i32, c.POINTER(vp)]
        lib.l2a_value_model_create.restype = i32
        lib.l2a_value_model_destroy.argtypes = [vp]
        lib.l2a_value_model_destroy.restype = None
        lib.l2a_value_model_set_weights.argtypes = [vp, c.POINTER(vp), vp]
        lib.l2a_value_model_set_weights.restype = i32
        lib.l2a_value_model_set_norm.argtypes = [vp, dp, dp, dp, dp, vp]
        lib.l2a_value_model_set_norm.restype = i32
        lib.l2a_value_model_predict.argtypes = [vp, vp, i32, vp, vp]
        lib.l2a_value_model_predict.restype = i32
        lib.l2a_value_terminal.argtypes = [vp, vp, vp, i32, i32, i32, dbl, dbl, i32, vp, vp, vp]
        lib.l2a_value_terminal.restype = i32
        lib.l2a_plan_rs_value.argtypes = [vp, vp, vp, vp, i32, i32, i32, dbl, c.POINTER(RewardSpec), dbl, i32, vp, vp, vp]
        lib.l2a_plan_rs_value.restype = i32
        lib.l2a_plan_rs_program_value.argtypes = [vp, vp, vp, vp, i32, i32, i32, dbl, c.POINTER(RewardProgram), dbl, i32, vp, vp, vp, vp]
        lib.l2a_plan_rs_program_value.restype = i32
        lib.l2a_plan_rs_reward_model_value.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, dbl, dbl, i32, vp, vp, vp, vp]
        lib.l2a_plan_rs_reward_model_value.restype = i32
    if hasattr(lib, "l2a_policy_model_create"):         # (absent from older variant libraries selected with L2A_LIB_PATH)
        u64 = c.c_ulonglong
        lib.l2a_policy_model_check.argtypes = [i32, i32, i32, c.POINTER(i32), i32]
        lib.l2a_policy_model_check.restype = i32
        lib.l2a_policy_model_geometry.argtypes = [i32, i32, i32, c.POINTER(i32), c.c_longlong, i32, i32, c.POINTER(i32)]
        lib.l2a_policy_model_geometry.restype = i32
        lib.l2a_policy_model_create.argtypes = [vp, i32, i32, i32, c.POINTER(i32), i32, c.POINTER(vp)]
        lib.l2a_policy_model_create.restype = i32
        lib.l2a_policy_model_destroy.argtypes = [vp]
        lib.l2a_policy_model_destroy.restype = None
        lib.l2a_policy_model_set_weights.argtypes = [vp, c.POINTER(vp), vp]
        lib.l2a_policy_model_set_weights.restype = i32
        lib.l2a_policy_model_set_norm.argtypes = [vp, dp, dp, dp, dp, vp]
        lib.l2a_policy_model_set_norm.restype = i32
        lib.l2a_policy_act.argtypes = [vp, vp, i32, vp, u64, u64, vp, vp, vp, vp, vp]
        lib.l2a_policy_act.restype = i32
        lib.l2a_policy_propose.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, u64, u64, vp, vp, vp, vp, vp, i32, vp]
        lib.l2a_policy_propose.restype = i32
    if hasattr(lib, "l2a_reward_model_create"):         # (absent from older variant libraries selected with L2A_LIB_PATH)
        lib.l2a_reward_model_check.argtypes = [i32, i32, i32, c.POINTER(i32), i32]
        lib.l2a_reward_model_check.restype = i32
        if hasattr(lib, "l2a_reward_model_geometry"):
            lib.l2a_reward_model_geometry.argtypes = [i32, i32, i32, c.POINTER(i32), c.c_longlong, i32, i32, i32, c.POINTER(i32)]
            lib.l2a_reward_model_geometry.restype = i32
        lib.l2a_reward_model_create.argtypes = [vp, i32, i32, i32, c.POINTER(i32), i32, c.POINTER(vp)]
        lib.l2a_reward_model_create.restype = i32
        lib.l2a_reward_model_destroy.argtypes = [vp]
        lib.l2a_reward_model_destroy.restype = None
        lib.l2a_reward_model_set_weights.argtypes = [vp, c.POINTER(vp), vp]
        lib.l2a_reward_model_set_weights.restype = i32
        lib.l2a_reward_model_set_norm.argtypes = [vp, dp, dp, dp, dp, dp, dp, dp, dp, vp]
        lib.l2a_reward_model_set_norm.restype = i32
        lib.l2a_reward_model_predict.argtypes = [vp, vp, vp, vp, i32, vp, vp]
        lib.l2a_reward_model_predict.restype = i32
        lib.l2a_score_trajectory_model.argtypes = [vp, vp, vp, vp, i32, i32, i32, c.c_double, i32, vp, vp, vp]
        lib.l2a_score_trajectory_model.restype = i32
        lib.l2a_plan_rs_reward_model.argtypes = [vp, vp, vp, vp, i32, i32, i32, c.c_double, i32, vp, vp, vp, vp]
        lib.l2a_plan_rs_reward_model.restype = i32
    lib.l2a_predict.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.l2a_predict.restype = i32
    lib.l2a_key_encode.argtypes = [f32, i32]
    lib.l2a_key_encode.restype = c.c_ulonglong
    lib.l2a_key_decode.argtypes = [c.c_ulonglong, c.POINTER(f32), c.POINTER(i32)]
    lib.l2a_key_decode.restype = None
    lib.l2a_mfma_eligible.argtypes = [i32, i32, i32, c.POINTER(i32)]
    lib.l2a_mfma_eligible.restype = i32
    lib.l2a_plan_geometry.argtypes = [i32, i32, i32, c.POINTER(i32), i32, i32, i32, i32, i32, c.POINTER(i32), c.POINTER(i32)]
    lib.l2a_plan_geometry.restype = i32
    if hasattr(lib, "l2a_plan_geometry_ex") or not os.environ.get("L2A_LIB_PATH"):
        lib.l2a_plan_geometry_ex.argtypes = [i32, i32, i32, c.POINTER(i32), i32, i32, i32, i32, i32, c.POINTER(i32), i32, c.POINTER(i32), i32]
        lib.l2a_plan_geometry_ex.restype = i32
    lib.l2a_packed_layer_floats.argtypes = [i32, i32]
    lib.l2a_packed_layer_floats.restype = c.c_longlong
    lib.l2a_pack_layer_host.argtypes = [c.POINTER(f32), i32, i32, c.POINTER(f32)]
    lib.l2a_pack_layer_host.restype = i32
    if hasattr(lib, "l2a_micro_layout_floats"):         # (absent from older variant libraries selected with L2A_LIB_PATH)
        lib.l2a_micro_layout_floats.argtypes = [i32, i32, i32, i32]
        lib.l2a_micro_layout_floats.restype = c.c_longlong
        lib.l2a_micro_pack_layer_host.argtypes = [c.POINTER(f32), i32, i32, i32, i32, i32, c.POINTER(f32)]
        lib.l2a_micro_pack_layer_host.restype = i32
    lib.l2a_comm_unique_id.argtypes = [c.c_char_p]
    lib.l2a_comm_unique_id.restype = i32
    lib.l2a_comm_init.argtypes = [vp, i32, i32, c.c_char_p]
    lib.l2a_comm_init.restype = i32
    lib.l2a_comm_destroy.argtypes = [vp]
    lib.l2a_comm_destroy.restype = i32
    lib.l2a_allreduce_best.argtypes = [vp, vp, i32, vp]
    lib.l2a_allreduce_best.restype = i32
    lib.l2a_lstm_create.argtypes = [vp, i32, i32, i32, i32, i32, c.POINTER(vp)]
    lib.l2a_lstm_create.restype = i32
    lib.l2a_rnn_create.argtypes = [vp, i32, i32, i32, c.POINTER(i32), i32, i32, i32, c.POINTER(vp)]
    lib.l2a_rnn_create.restype = i32
    lib.l2a_lstm_destroy.argtypes = [vp]
    lib.l2a_lstm_destroy.restype = None
    lib.l2a_lstm_set_weights.argtypes = [vp, c.POINTER(vp), vp]
    lib.l2a_lstm_set_weights.restype = i32
    lib.l2a_lstm_set_norm.argtypes = [vp, dp, dp, dp, dp, dp, dp, vp]
    lib.l2a_lstm_set_norm.restype = i32
    lib.l2a_lstm_plan_rs.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardSpec), i32, vp, vp, vp]
    lib.l2a_lstm_plan_rs.restype = i32
    lib.l2a_cem_sample.argtypes = [vp, vp, c.c_ulonglong, c.c_ulonglong, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32,
                                   vp, vp, vp, vp]
    lib.l2a_cem_sample.restype = i32
    lib.l2a_cem_refit.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp]
    lib.l2a_cem_refit.restype = i32
    lib.l2a_cem_pick.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.l2a_cem_pick.restype = i32
    if hasattr(lib, "l2a_cem_refit_sample"):
        lib.l2a_cem_refit_sample.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp, c.c_ulonglong, c.c_ulonglong, vp, vp,
                                             i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.l2a_cem_refit_sample.restype = i32
        lib.l2a_cem_refit_sample_fused.argtypes = [vp, i32, i32, i32, i32, i32, i32]
        lib.l2a_cem_refit_sample_fused.restype = i32
    if hasattr(lib, "l2a_mppi_sample"):
        lib.l2a_mppi_sample.argtypes = [vp, vp, c.c_ulonglong, c.c_ulonglong, vp, vp, vp, f32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
        lib.l2a_mppi_sample.restype = i32
        lib.l2a_mppi_update.argtypes = [vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp]
        lib.l2a_mppi_update.restype = i32
    if hasattr(lib, "l2a_icem_sample"):         # the iCEM planner's kernels (absent from older variant libraries)
        lib.l2a_icem_sample.argtypes = [vp, vp, c.c_ulonglong, c.c_ulonglong, vp, vp, vp, vp, vp, vp, f32, vp, vp, i32, i32, i32, i32, i32,
                                        i32, vp, vp, vp, vp, vp]
        lib.l2a_icem_sample.restype = i32
        lib.l2a_icem_refit.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp]
        lib.l2a_icem_refit.restype = i32
    lib.l2a_lstm_plan_rs_sync.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardSpec), i32, vp, vp, vp, vp]
    lib.l2a_lstm_plan_rs_sync.restype = i32
    lib.l2a_lstm_plan_rs_chunk.argtypes = [vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, c.c_double, c.POINTER(RewardSpec), i32,
                                           vp, vp, vp, vp, vp, vp, vp]
    lib.l2a_lstm_plan_rs_chunk.restype = i32
    lib.l2a_lstm_predict.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.l2a_lstm_predict.restype = i32
    if hasattr(lib, "l2a_lstm_advance"):
        lib.l2a_lstm_advance.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp]
        lib.l2a_lstm_advance.restype = i32
    if os.environ.get("L2A_LIB_PATH") and not hasattr(lib, "l2a_plan_payload"):
        pass                                               # developer A/B against a library of an earlier round
    else:
        lib.l2a_plan_payload.argtypes = [vp, vp, i32, c.c_ulonglong, vp, vp]
        lib.l2a_plan_payload.restype = i32
    lib.l2a_lstm_mfma_eligible.argtypes = [i32, i32, i32]
    lib.l2a_lstm_mfma_eligible.restype = i32
    if hasattr(lib, "l2a_lstm_rollout_traj"):           # (absent from older variant libraries selected with L2A_LIB_PATH)
        lib.l2a_lstm_rollout_traj.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
        lib.l2a_lstm_rollout_traj.restype = i32
        lib.l2a_lstm_plan_rs_program.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardProgram), i32, vp, vp, vp, vp]
        lib.l2a_lstm_plan_rs_program.restype = i32
        lib.l2a_lstm_plan_rs_reward_model.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, c.c_double, i32, vp, vp, vp, vp]
        lib.l2a_lstm_plan_rs_reward_model.restype = i32
        lib.l2a_lstm_traj_geometry.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, c.POINTER(i32)]
        lib.l2a_lstm_traj_geometry.restype = i32
    if hasattr(lib, "l2a_lstm_plan_geometry"):          # (absent from older variant libraries selected with L2A_LIB_PATH)
        lib.l2a_lstm_plan_geometry.argtypes = [i32, i32, i32, c.POINTER(i32), i32, i32, i32, i32, i32, c.POINTER(i32), c.POINTER(i32)]
        lib.l2a_lstm_plan_geometry.restype = i32
    if hasattr(lib, "l2a_rollout_traj"):                # (absent from older variant libraries selected with L2A_LIB_PATH)
        lib.l2a_rollout_traj.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp]
        lib.l2a_rollout_traj.restype = i32
        lib.l2a_mlp_traj_geometry.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, c.POINTER(i32)]
        lib.l2a_mlp_traj_geometry.restype = i32
    if hasattr(lib, "l2a_particle_score"):              # (absent from older variant libraries selected with L2A_LIB_PATH)
        tail = [f32, i32, vp, vp, vp, vp, vp]           # lambda, cand_offset, score_out, spread_out, member_returns_out, best_key, stream
        lib.l2a_particle_score.argtypes = [vp, vp, i32, i32, i32, f32, i32, vp, vp, vp, vp]
        lib.l2a_particle_score.restype = i32
        lib.l2a_plan_rs_particles.argtypes = [vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardSpec)] + tail
        lib.l2a_plan_rs_particles.restype = i32
        lib.l2a_plan_rs_particles_program.argtypes = [vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardProgram)] + tail
        lib.l2a_plan_rs_particles_program.restype = i32
        lib.l2a_plan_rs_particles_reward_model.argtypes = [vp, vp, vp, vp, i32, i32, i32, c.c_double] + tail
        lib.l2a_plan_rs_particles_reward_model.restype = i32
    if hasattr(lib, "l2a_plan_rs_particles_ts1"):       # (absent from older variant libraries selected with L2A_LIB_PATH)
        u64 = c.c_ulonglong
        lib.l2a_particle_perm.argtypes = [u64, u64, i32, i32, i32, i32, i32, i32, i32, vp]
        lib.l2a_particle_perm.restype = i32
        # ctx, state_in, ret_in, state_out, ret_out, perm, seed, offset, t, m, E, n, obs_dim, cand_offset, stream
        lib.l2a_particle_shuffle.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, i32, i32, i32, i32, i32, vp]
        lib.l2a_particle_shuffle.restype = i32
        # model, obs0, actions, m, n, h, discount, reward, lambda, seed, offset, perm, cand_offset, score_out, spread_out,
        # particle_returns_out, best_key, stream
        lib.l2a_plan_rs_particles_ts1.argtypes = [vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardSpec), f32, u64, u64, vp,
                                                  i32, vp, vp, vp, vp, vp]
        lib.l2a_plan_rs_particles_ts1.restype = i32
    if hasattr(lib, "l2a_particle_step"):               # (absent from older variant libraries selected with L2A_LIB_PATH)
        u64 = c.c_ulonglong
        # ctx, pre, pre_per_row, post, actions, act_env_stride, rewards, program, disc_t, ret_in, state_out, ret_out, perm, seed,
        # offset, t, m, E, n, obs_dim, act_dim, cand_offset, stream
        lib.l2a_particle_step.argtypes = [vp, vp, i32, vp, vp, c.c_longlong, vp, c.POINTER(RewardProgram), c.c_double, vp, vp, vp, vp,
                                          u64, u64, i32, i32, i32, i32, i32, i32, i32, vp]
        lib.l2a_particle_step.restype = i32
        # l2a_plan_rs_particles_ts1's arguments with the program, or the reward model, in place of the reward
        ts1_tail = [f32, u64, u64, vp, i32, vp, vp, vp, vp, vp]
        lib.l2a_plan_rs_particles_ts1_program.argtypes = [vp, vp, vp, i32, i32, i32, c.c_double, c.POINTER(RewardProgram)] + ts1_tail
        lib.l2a_plan_rs_particles_ts1_program.restype = i32
        lib.l2a_plan_rs_particles_ts1_reward_model.argtypes = [vp, vp, vp, vp, i32, i32, i32, c.c_double] + ts1_tail
        lib.l2a_plan_rs_particles_ts1_reward_model.restype = i32
    if os.environ.get("L2A_LIB_PATH") and not hasattr(lib, "l2a_controller_step"):
        pass                                               # developer A/B against a library of an earlier round
    else:
        lib.l2a_controller_create.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), vp, i32, c.POINTER(vp)]
        # the caller's collective of a sharded step: int fn(void* arg, uint64* payload_dev, int words, void* stream)
        lib.REDUCE_FN = c.CFUNCTYPE(i32, vp, vp, i32, vp)
        lib.l2a_controller_create.restype = i32
        lib.l2a_lstm_controller_create.argtypes = lib.l2a_controller_create.argtypes
        lib.l2a_lstm_controller_create.restype = i32
        lib.l2a_controller_create_device.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), c.c_ulonglong, c.POINTER(vp)]
        lib.l2a_controller_create_device.restype = i32
        lib.l2a_lstm_controller_create_device.argtypes = lib.l2a_controller_create_device.argtypes
        lib.l2a_lstm_controller_create_device.restype = i32
        lib.l2a_controller_destroy.argtypes = [vp]
        lib.l2a_controller_destroy.restype = None
        lib.l2a_controller_step.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.l2a_controller_step.restype = i32
        lib.l2a_lstm_controller_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.l2a_lstm_controller_step.restype = i32
        lib.l2a_controller_rearm.argtypes = [vp]
        lib.l2a_controller_rearm.restype = i32
        lib.l2a_controller_create_sharded.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), vp, i32, i32, i32,
                                                      vp, vp, c.POINTER(vp)]
        lib.l2a_controller_create_sharded.restype = i32
        lib.l2a_controller_create_sharded_device.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), c.c_ulonglong, i32, i32,
                                                             vp, vp, c.POINTER(vp)]
        lib.l2a_controller_create_sharded_device.restype = i32
        lib.l2a_controller_begin.argtypes = [vp, vp, vp]
        lib.l2a_controller_begin.restype = i32
        lib.l2a_lstm_controller_begin.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        lib.l2a_lstm_controller_begin.restype = i32
        lib.l2a_controller_finish.argtypes = [vp, vp, vp, vp]
        lib.l2a_controller_finish.restype = i32
        lib.l2a_controller_actions.argtypes = [vp]
        lib.l2a_controller_actions.restype = vp
        lib.l2a_controller_stats.argtypes = [vp, dp, i32]
        lib.l2a_controller_stats.restype = i32
    if hasattr(lib, "l2a_lstm_controller_create_sharded"):       # the sharded recurrent step (absent from older variant libraries)
        lib.l2a_lstm_controller_create_sharded.argtypes = lib.l2a_controller_create_sharded.argtypes
        lib.l2a_lstm_controller_create_sharded.restype = i32
        lib.l2a_lstm_controller_create_sharded_device.argtypes = lib.l2a_controller_create_sharded_device.argtypes
        lib.l2a_lstm_controller_create_sharded_device.restype = i32
    if hasattr(lib, "l2a_cem_controller_create_device"):
        lib.l2a_cem_controller_create_device.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), i32, i32, f32, i32,
                                                         c.c_ulonglong, c.POINTER(vp)]
        lib.l2a_cem_controller_create_device.restype = i32
        lib.l2a_cem_controller_result.argtypes = [vp, vp, vp, vp]
        lib.l2a_cem_controller_result.restype = i32
    if hasattr(lib, "l2a_cem_controller_create_sharded_device"):
        lib.l2a_cem_shard_pack.argtypes = [vp, vp, i32, i32, i32, i32, c.c_ulonglong, vp, vp]
        lib.l2a_cem_shard_pack.restype = i32
        lib.l2a_cem_shard_unpack.argtypes = [vp, vp, i32, i32, vp, vp, vp]
        lib.l2a_cem_shard_unpack.restype = i32
        lib.l2a_cem_word_encode.argtypes = [f32]
        lib.l2a_cem_word_encode.restype = c.c_ulonglong
        lib.l2a_cem_word_decode.argtypes = [c.c_ulonglong, c.POINTER(f32)]
        lib.l2a_cem_word_decode.restype = i32
        lib.l2a_cem_controller_create_sharded_device.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), i32, i32, f32, i32,
                                                                 c.c_ulonglong, i32, i32, vp, vp, c.POINTER(vp)]
        lib.l2a_cem_controller_create_sharded_device.restype = i32
    if hasattr(lib, "l2a_lstm_cem_controller_create_device"):
        lib.l2a_cem_pick_act.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
        lib.l2a_cem_pick_act.restype = i32
        lib.l2a_lstm_cem_controller_create_device.argtypes = lib.l2a_cem_controller_create_device.argtypes
        lib.l2a_lstm_cem_controller_create_device.restype = i32
        lib.l2a_lstm_cem_controller_create_sharded_device.argtypes = lib.l2a_cem_controller_create_sharded_device.argtypes
        lib.l2a_lstm_cem_controller_create_sharded_device.restype = i32
    if hasattr(lib, "l2a_mppi_controller_create_device"):    # the MPPI step as one call (absent from older variant libraries)
        lib.l2a_mppi_sample_shard.argtypes = [vp, vp, c.c_ulonglong, c.c_ulonglong, vp, vp, vp, f32, vp, vp, i32, i32, i32, i32, i32, i32,
                                              vp, vp, vp, vp]
        lib.l2a_mppi_sample_shard.restype = i32
        lib.l2a_mppi_controller_create_device.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), i32, f32, f32, vp,
                                                          c.c_ulonglong, c.POINTER(vp)]
        lib.l2a_mppi_controller_create_device.restype = i32
        lib.l2a_mppi_controller_create_sharded_device.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), i32, f32, f32, vp,
                                                                  c.c_ulonglong, i32, i32, vp, vp, c.POINTER(vp)]
        lib.l2a_mppi_controller_create_sharded_device.restype = i32
        lib.l2a_mppi_controller_reset.argtypes = [vp, vp]
        lib.l2a_mppi_controller_reset.restype = i32
        lib.l2a_mppi_controller_reseed.argtypes = [vp, c.c_ulonglong]
        lib.l2a_mppi_controller_reseed.restype = i32
        lib.l2a_mppi_controller_result.argtypes = [vp, vp, vp, vp, vp]
        lib.l2a_mppi_controller_result.restype = i32
    if hasattr(lib, "l2a_icem_controller_create_device"):    # the iCEM step as one call (absent from older variant libraries)
        lib.l2a_icem_sample_shard.argtypes = [vp, vp, c.c_ulonglong, c.c_ulonglong, vp, vp, vp, vp, vp, vp, f32, vp, vp, i32, i32, i32, i32,
                                              i32, i32, i32, i32, vp, vp, vp, vp, vp]
        lib.l2a_icem_sample_shard.restype = i32
        lib.l2a_icem_controller_create_device.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), i32, vp, i32, i32,
                                                          f32, f32, vp, i32, c.c_ulonglong, c.POINTER(vp)]
        lib.l2a_icem_controller_create_device.restype = i32
        lib.l2a_icem_controller_create_sharded_device.argtypes = [vp, i32, i32, i32, vp, vp, c.c_double, c.POINTER(RewardSpec), i32, vp, i32,
                                                                  i32, f32, f32, vp, i32, c.c_ulonglong, i32, i32, vp, vp, c.POINTER(vp)]
        lib.l2a_icem_controller_create_sharded_device.restype = i32
        lib.l2a_icem_controller_reset.argtypes = [vp, vp]
        lib.l2a_icem_controller_reset.restype = i32
        lib.l2a_icem_controller_reseed.argtypes = [vp, c.c_ulonglong]
        lib.l2a_icem_controller_reseed.restype = i32
        lib.l2a_icem_controller_result.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        lib.l2a_icem_controller_result.restype = i32
    if hasattr(lib, "l2a_icem_sample_noise"):    # iCEM's noise as a matrix (absent from older variant libraries)
        lib.l2a_icem_noise_matrix.argtypes = [i32, c.c_double, vp]
        lib.l2a_icem_noise_matrix.restype = i32
        # (l2a_icem_sample's / l2a_icem_sample_shard's arguments with `float rho` replaced by the device matrix)
        lib.l2a_icem_sample_noise.argtypes = [vp, vp, c.c_ulonglong, c.c_ulonglong, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32,
                                              i32, i32, vp, vp, vp, vp, vp]
        lib.l2a_icem_sample_noise.restype = i32
        lib.l2a_icem_sample_noise_shard.argtypes = [vp, vp, c.c_ulonglong, c.c_ulonglong, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32,
                                                    i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
        lib.l2a_icem_sample_noise_shard.restype = i32
        lib.l2a_icem_controller_set_noise.argtypes = [vp, vp]
        lib.l2a_icem_controller_set_noise.restype = i32
    _lib = lib
    return lib


def key_decode(key):
    """``best_key`` -> (return as float, global candidate index)."""
    lib = load()
    ret, idx = ctypes.c_float(), ctypes.c_int()
    lib.l2a_key_decode(ctypes.c_ulonglong(int(key) & 0xFFFFFFFFFFFFFFFF), ctypes.byref(ret), ctypes.byref(idx))
    return ret.value, idx.value


class Context(object):
    """One ``l2a_ctx`` per (process, device).  Created lazily by the models (never at import
    or construction time: the reference forks env workers before touching the accelerator,
    ``samplers/sampler.py:37`` vs ``trainers/mb_trainer.py:46-48``)."""

    _by_device = {}

    def __init__(self, device=0):
        self.lib = load()
        handle = ctypes.c_void_p()
        rc = self.lib.l2a_init(int(device), ctypes.byref(handle))
        if rc != L2A_OK:
            raise L2AError("l2a_init(device=%d) failed (%d): %s" % (
                device, rc, self.lib.l2a_last_error(None).decode()))
        self.handle = handle
        self.device = int(device)
        self.pid = os.getpid()

    @classmethod
    def get(cls, device=0):
        ctx = cls._by_device.get(device)
        if ctx is None or ctx.pid != os.getpid():
            ctx = cls(device)
            cls._by_device[device] = ctx
            kind = os.environ.get("L2A_KERNEL")
            if kind:
                ctx.set_kernel(kind)
        return ctx

    def check(self, rc, what):
        if rc != L2A_OK:
            raise L2AError("%s failed (%d): %s" % (what, rc, self.lib.l2a_last_error(self.handle).decode()))

    def info(self):
        buf = ctypes.create_string_buffer(512)
        self.check(self.lib.l2a_device_info(self.handle, buf, 512), "l2a_device_info")
        return json.loads(buf.value.decode())

    def set_kernel(self, kind):
        self.check(self.lib.l2a_set_kernel(self.handle, KERNEL_CODES[kind]), "l2a_set_kernel")

    def set_split(self, policy):
        """0 = never, 1 = auto (default; shares the middle set of odd ensembles), 2 = whole sets only."""
        self.check(self.lib.l2a_set_split(self.handle, int(policy)), "l2a_set_split")

    def set_batch(self, sets):
        """Sets per batch of the MFMA rollout: 0 = as many as fit the LDS (default), 1 = one at a time (bit-identical)."""
        self.check(self.lib.l2a_set_batch(self.handle, int(sets)), "l2a_set_batch")

    def set_micro(self, policy):
        """Micro-tile kernels: 0 = never, 1 = where they fill the chip better (default), 2 = whenever eligible.  Bit-identical to
        the 16-candidate matrix-core kernels; a generic recurrent stack too large for those (policy 0: VALU kernel) agrees to the
        fp32 tolerance only (include/l2a.h)."""
        self.check(self.lib.l2a_set_micro(self.handle, int(policy)), "l2a_set_micro")

    def set_xcd_align(self, on):
        """Split launches: ensemble group A on XCDs 0-3, B on 4-7 exactly (padded grid; default on; bit-identical)."""
        self.check(self.lib.l2a_set_xcd_align(self.handle, int(bool(on))), "l2a_set_xcd_align")

    def set_fan(self, on):
        """Member fan: small mean-ensemble plans on one workgroup per (candidate tile, member) - default on; bit-identical."""
        self.check(self.lib.l2a_set_fan(self.handle, int(bool(on))), "l2a_set_fan")

    def set_seq3(self, on):
        """Static three-set step: five-set mean ensembles under the shared-set tile split (2 x 512) run kernel instances that know
        the full, full, shared sequence at compile time - default on; bit-identical."""
        self.check(self.lib.l2a_set_seq3(self.handle, int(bool(on))), "l2a_set_seq3")

    def set_double_rounds(self, on):
        """Double rounds: multi-round plans at width 512 run their first rounds on two-tile workgroups - default on; bit-identical."""
        self.check(self.lib.l2a_set_double_rounds(self.handle, int(bool(on))), "l2a_set_double_rounds")

    def launch_status_value(self):
        """Status word of the launches since the last call (stream must be synchronised); reading clears it."""
        st = ctypes.c_int()
        self.check(self.lib.l2a_launch_status(self.handle, ctypes.byref(st)), "l2a_launch_status")
        return st.value

    def launch_status(self):
        """Status of the launches since the last call (stream must be synchronised).  Raises when a
        member-split exchange timed out - results of those launches are invalid."""
        st = self.launch_status_value()
        if st != 0:
            raise L2AError("rollout launch reported status 0x%x (member-split exchange timed out; "
                           "set L2A_SPLIT=0 to disable the split)" % st)
        return st

    def check_or_degrade(self):
        """After a stream sync: True when every launch since the last check was fine.  A tile-split exchange
        that timed out (the two workgroups of a tile were not co-resident, e.g. another process shares the GPU)
        invalidates those launches: the context is switched to the unsplit launch geometry for good - same
        bits, fewer busy CUs - and False is returned so that the caller relaunches.  Raises only when launches
        fail although the split is already off."""
        st = self.launch_status_value()
        if st == 0:
            return True
        if getattr(self, "split_degraded", False):
            raise L2AError("rollout launch reported status 0x%x with the tile split disabled" % st)
        self.set_split(0)
        self.split_degraded = True
        return False

    def force_unsplit(self):
        """A rank of a sharded plan was told by the collective that SOME rank's launch lost its tile-split partner: all
        ranks clear their status word, switch to the unsplit geometry (bit-identical results) and repeat the launch
        together.  Never raises: a rank that had already degraded on its own (a single-GPU call between two sharded
        plans) must stay in step with the others - a launch that fails again is caught by the caller's second look at the
        REDUCED flag, which raises on every rank alike."""
        self.launch_status_value()
        if not getattr(self, "split_degraded", False):
            self.set_split(0)
            self.split_degraded = True

    def plan_payload(self, best_key, m, digest, payload, stream_ptr):
        """Pack what a sharded plan all-reduces (``l2a_plan_payload``): keys, this rank's launch flag, the digest pair -
        on the device, in stream order behind the launch, no host synchronisation.  ``best_key`` / ``payload``: int64 CUDA
        tensors of ``m`` / ``m + 3`` elements.  Shared by every planner model (MLP and recurrent)."""
        assert best_key.is_cuda and payload.is_cuda and str(best_key.dtype) == "torch.int64" and str(payload.dtype) == "torch.int64"
        assert best_key.numel() == m and payload.numel() == m + 3
        rc = self.lib.l2a_plan_payload(self.handle, ctypes.c_void_p(best_key.data_ptr()), int(m), ctypes.c_ulonglong(int(digest)),
                                       ctypes.c_void_p(payload.data_ptr()), stream_ptr)
        self.check(rc, "l2a_plan_payload")

    def score_trajectory(self, obs0, traj, actions, m, n, h, discount, program, cand_offset=0, returns_out=None,
                         best_key=None, stream_ptr=None):
        """Score trajectories that are already on the device with a reward program (``l2a_score_trajectory``): ``obs0``
        ``[m, obs_dim]``, ``traj`` ``[h, m * n, obs_dim]``, ``actions`` ``[h, m * n, act_dim]`` fp32 CUDA tensors."""
        import torch
        assert isinstance(program, RewardProgram)
        for t in (obs0, traj, actions):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        obs_dim, act_dim = int(obs0.shape[-1]), int(actions.shape[-1])
        assert obs0.numel() == m * obs_dim and traj.numel() == h * m * n * obs_dim and actions.numel() == h * m * n * act_dim
        if returns_out is not None:
            assert returns_out.is_cuda and returns_out.dtype == torch.float32 and returns_out.numel() == m * n
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        if stream_ptr is None:
            stream_ptr = ctypes.c_void_p(torch.cuda.current_stream(obs0.device).cuda_stream)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)    # noqa: E731
        rc = self.lib.l2a_score_trajectory(self.handle, ptr(obs0), ptr(traj), ptr(actions), int(m), int(n), int(h), obs_dim,
                                           act_dim, float(discount), ctypes.byref(program), int(cand_offset), ptr(returns_out),
                                           ptr(best_key), stream_ptr)
        self.check(rc, "l2a_score_trajectory")

    def score_trajectory_term(self, obs0, traj, actions, m, n, h, discount, termination, program=None, step_rewards=None,
                              terminal_values=None, value_coef=1.0, cand_offset=0, returns_out=None, steps_alive_out=None,
                              best_key=None, stream_ptr=None):
        """Score trajectories that are already on the device under a termination program (``l2a_score_trajectory_term``): exactly
        one of ``program`` (a ``RewardProgram``; ``obs0`` / ``actions`` as ``score_trajectory``) and ``step_rewards`` (fp32 CUDA
        ``[h, m * n]``; ``obs0`` and ``actions`` may be ``None``).  ``terminal_values``: fp32 CUDA ``[m * n]`` or ``None``;
        ``steps_alive_out``: int32 CUDA ``[m, n]`` or ``None``."""
        import torch
        assert isinstance(termination, TerminationProgram)
        assert program is None or isinstance(program, RewardProgram)
        assert traj.is_cuda and traj.dtype == torch.float32 and traj.is_contiguous()
        obs_dim = int(traj.shape[-1])
        assert traj.numel() == h * m * n * obs_dim
        act_dim = int(actions.shape[-1]) if actions is not None else 1
        if program is not None:
            for t in (obs0, actions):
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            assert obs0.numel() == m * obs_dim and actions.numel() == h * m * n * act_dim
        if step_rewards is not None:
            assert step_rewards.is_cuda and step_rewards.dtype == torch.float32 and step_rewards.is_contiguous()
            assert step_rewards.numel() == h * m * n
        if terminal_values is not None:
            assert terminal_values.is_cuda and terminal_values.dtype == torch.float32 and terminal_values.is_contiguous()
            assert terminal_values.numel() == m * n
        if returns_out is not None:
            assert returns_out.is_cuda and returns_out.dtype == torch.float32 and returns_out.numel() == m * n
        if steps_alive_out is not None:
            assert steps_alive_out.is_cuda and steps_alive_out.dtype == torch.int32 and steps_alive_out.numel() == m * n
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        if stream_ptr is None:
            stream_ptr = ctypes.c_void_p(torch.cuda.current_stream(traj.device).cuda_stream)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)    # noqa: E731
        rc = self.lib.l2a_score_trajectory_term(self.handle, ptr(obs0), ptr(traj), ptr(actions), ptr(step_rewards), int(m), int(n),
                                                int(h), obs_dim, act_dim, float(discount),
                                                ctypes.byref(program) if program is not None else None, ctypes.byref(termination),
                                                ptr(terminal_values), float(value_coef), int(cand_offset), ptr(returns_out),
                                                ptr(steps_alive_out), ptr(best_key), stream_ptr)
        self.check(rc, "l2a_score_trajectory_term")

    def set_spin_limit(self, polls):
        """Developer / test knob: polls a split workgroup waits for its partner per launch (0 = default)."""
        self.check(self.lib.l2a_set_spin_limit(self.handle, int(polls)), "l2a_set_spin_limit")
