"""ctypes binding of libmeshenv_hip.so: one row of SIGNATURES per function the public headers in include/ declare
(tests/test_capi_signatures_cpu.py holds the rows, the Structure classes and the constants against those headers).  Fails loudly when
the library is missing: there is no CPU fallback anywhere in this package."""
from __future__ import annotations

import ctypes as C
import os

from .build import LIB_PATH

OBS_DIM = 18
ACT_DIM = 3

ST_NO_REFERENCE = 1
ST_LOG_OVERFLOW = 2
MOVE_OK, MOVE_NONE, MOVE_RAISES, MOVE_NEEDS_SMOOTHING, MOVE_SMOOTH_RAISES = 0, 1, 2, 3, 4
SMOOTH_SKIPPED, SMOOTH_LOG_OVERFLOW, SMOOTH_DEGREE, SMOOTH_NOT_FINISHED, SMOOTH_INDEX_ERROR, SMOOTH_RAISES = -1, -2, -3, -4, -5, -6
SMOOTH_NONFINITE = -7
E_ARG, E_HIP, E_RANGE, E_STATE = -1, -2, -3, -4

# the constants of the other headers, in the order of SIGNATURES below
OPTIM_PROGRAMS, OPTIM_BLOCKS, OPTIM_CHUNK = 8, 4, 1024
OPTIM_ADAM, OPTIM_POLYAK, OPTIM_ADAM_POLYAK, OPTIM_RMSPROP = 1, 2, 3, 4
TD3_ACTOR_GRAD_FLOATS = 71488
PPO_GRAD_FLOATS = {64: 11072, 128: 38464}
PPO_GRAD_OUTPUTS, PPO_GRAD_PARTS = 8, 5
ROLLOUT_FIELDS, ROLLOUT_CHUNK, ROLLOUT_MAX_ROWS = 6, 1024, 2 ** 24 - 16
TRAIN_OUTPUTS, TRAIN_MAX_MINIBATCHES = 12, 65536
LEARN_WORDS, LEARN_MAX_ENTRIES = 3, 2 ** 20
LEARN_WORD_N_UPDATES, LEARN_WORD_ERROR, LEARN_WORD_STEPS = 0, 1, 2
OFFTRAIN_OUTPUTS, OFFTRAIN_MAX_STEPS = 8, 65536
OFFTRAIN_SAMPLE_FLOATS, REPLAY_BATCHES_MAX_SAMPLES = 41, 2 ** 24
UNIFORM_PHILOX_TAG, EPISODE_RING_DOUBLES = 4, 3
EVAL_ROW_DOUBLES, EVAL_STATE_DOUBLES, KEEP_BEST_MAX_ENTRIES = 9, 4, 64
EVAL_COLUMNS = ("num_timesteps", "mean_reward", "std_reward", "mean_ep_length", "recorded", "short", "complete_rate",
                "mean_n_elements", "improved")
TOPOLOGY_DIM = 16
TOPO_OK, TOPO_MASKED, TOPO_LOG_OVERFLOW, TOPO_DEGREE, TOPO_NOT_ARCHIVED = 0, 1, 2, 3, 4
FNN_TENSORS, FNN_PACKED_FLOATS, MOVE_SKIPPED = 14, 21568, 255
FNN_GRAD_FLOATS, FNN_GRAD_OUTPUTS, FNN_GRAD_MAX_GROUPS = 20544, 4, 128
AUGMENT_PHILOX_TAG, AUGMENT_BINS, AUGMENT_TYPES, AUGMENT_MAX_ACTIONS, AUGMENT_UNIFORMS = 5, 11, 3, 20, 57
AUGMENT_MAX_POOL, AUGMENT_MAX_ROUND, AUGMENT_MAX_ROUNDS, AUGMENT_STATS = 1024, 2 ** 20, 4095, 4
DDPG_GRAD_ACTOR_FLOATS, DDPG_GRAD_CRITIC_FLOATS, DDPG_GRAD_MAX_ROWS = 128832, 129408, 65536


class MeshEnvParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("neighbor_num", C.c_int32), ("radius_num", C.c_int32),
        ("fail_limit", C.c_int32), ("log_capacity", C.c_int32), ("reserved", C.c_int32),
        ("radius", C.c_double), ("max_ref_angle", C.c_double), ("key_lambda", C.c_double),
        ("min_degree", C.c_double), ("max_degree", C.c_double), ("same_point_eps", C.c_double),
        ("ray_length", C.c_double),
    ]


class MeshEvalBuffers(C.Structure):
    """include/meshenv.h MeshEvalBuffers: device pointers (torch data_ptr()), NULL = None."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32)] + [
        (name, C.c_void_p) for name in (
            "target_dev", "offset_dev", "count_dev", "length_dev", "seen_dev", "return_dev", "return_raw_dev", "short_dev",
            "ep_env_dev", "ep_domain_dev", "ep_step_dev", "ep_length_dev", "ep_flags_dev", "ep_n_elements_dev",
            "ep_archive_dev", "ep_return_dev", "ep_return_raw_dev", "ep_quality_dev", "obs_dev", "reward_dev", "done_dev",
            "complete_dev")]


class MeshKeepEntry(C.Structure):
    """include/meshenv_eval_callback.h MeshKeepEntry: one tensor of a meshenv_keep_best call."""
    _fields_ = [("src_dev", C.c_void_p), ("dst_offset", C.c_int64), ("numel", C.c_int64)]


class MeshOptimScalars(C.Structure):
    """include/meshenv_optim.h MeshOptimScalars: the host-computed scalars of one step, a kernel argument."""
    _fields_ = [(name, C.c_float * OPTIM_BLOCKS) for name in ("step_size", "bc2_sqrt", "w1", "beta2", "w2", "eps")] + [
        ("tau", C.c_float), ("one_minus_tau", C.c_float)]


class MeshOptimCounted(C.Structure):
    """include/meshenv_onpolicy_learn.h MeshOptimCounted: the scalars of every step of one counted train()."""
    _fields_ = [("lr", C.c_double * OPTIM_BLOCKS)] + [(name, C.c_float * OPTIM_BLOCKS) for name in ("w1", "beta2", "w2", "eps")] + [
        ("tau", C.c_float), ("one_minus_tau", C.c_float)]


class MeshEnvError(RuntimeError):
    pass


_lib = None

# the types of the rows below.  vp: a handle, a stream or a device pointer (torch data_ptr()); vpp: a host array of those, or the
# handle a create returns
i, i64, u64, f32, f64, vp, cstr = C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_void_p, C.c_char_p
vpp, i32p, i64p, u64p, f32p, f64p = (C.POINTER(t) for t in (vp, C.c_int32, i64, u64, f32, f64))
params_p, eval_p, keep_p = C.POINTER(MeshEnvParams), C.POINTER(MeshEvalBuffers), C.POINTER(MeshKeepEntry)
scalars_p, counted_p = C.POINTER(MeshOptimScalars), C.POINTER(MeshOptimCounted)


def _family(prefix, *extra, parts=("create", "destroy", "set_stream", "last_error")):
    """The rows every handle type has: <prefix>_create(device, stream, <extra>, out), _destroy, _set_stream, _last_error."""
    rows = {"create": (i, [i, vp, *extra, vpp]), "destroy": (None, [vp]), "set_stream": (i, [vp, vp]), "last_error": (cstr, [vp])}
    return {f"{prefix}_{part}": rows[part] for part in parts}


# {public header: {function: (restype, argtypes)}}: every function the headers declare, once.  load() sets exactly these.
SIGNATURES = {
    "meshenv.h": {
        "meshenv_default_params": (None, [params_p]),
        "meshenv_abi_version": (i, []),
        "meshenv_device_count": (i, []),
        "meshenv_libm_exact": (i, [vp]),
        "meshenv_atan2_exact": (i, []),
        "meshenv_selftest": (i, [i, i, i, i, vp, vp]),
        "meshenv_create": (i, [i, i, i32p, f64p, f64p, i, i32p, params_p, vp, vpp]),
        "meshenv_create_random": (i, [i, i, u64, i, f64, params_p, vp, vpp]),
        "meshenv_create_random_density": (i, [i, i, u64, vp, i, f64, f64, params_p, vp, vpp, vp]),
        "meshenv_density_rings": (i, [i, i, vp, vp, i, vp, f64, vp, vp, vp, i64]),
        "meshenv_destroy": (None, [vp]),
        "meshenv_last_error": (cstr, [vp]),
        "meshenv_set_stream": (i, [vp, vp]),
        "meshenv_num_envs": (i, [vp]),
        "meshenv_max_ring": (i, [vp]),
        "meshenv_group_size": (i, [vp]),
        "meshenv_step_kernel": (i, [vp]),
        "meshenv_rollout_kernel": (i, [vp]),
        "meshenv_step_kernel_name": (cstr, [vp]),
        "meshenv_rollout_kernel_name": (cstr, [vp]),
        "meshenv_set_timing": (i, [vp, i]),
        "meshenv_kernel_times": (i, [vp, vp, i, i32p]),
        "meshenv_counters": (i, [vp, u64p]),
        "meshenv_set_packed_output": (i, [vp, vp]),
        "meshenv_reset": (i, [vp, vp, vp]),
        "meshenv_reset_static": (i, [vp, vp, vp, i]),
        "meshenv_step": (i, [vp] * 7 + [i]),
        "meshenv_rollout": (i, [vp, i] + [vp] * 5 + [i]),
        "meshenv_move": (i, [vp] * 7),
        "meshenv_get_status": (i, [vp, vp]),
        "meshenv_get_state": (i, [vp, i] + [vp] * 6),
        "meshenv_get_domain": (i, [vp, i, vp, i, i32p, vp]),
        "meshenv_get_elements": (i, [vp, i, vp, i, vp, i, i32p, i32p]),
        "meshenv_get_last_episode": (i, [vp, i, vp, i, vp, i, i32p, i32p, i32p, i32p]),
        "meshenv_get_not_valid": (i, [vp, i, vp, i, i32p]),
        "meshenv_get_not_valid_ids": (i, [vp, i, vp, i, i32p, vp]),
        "meshenv_element_quality": (i, [vp, i, vp, vp, vp]),
        "meshenv_quad_quality": (i, [vp, i, vp, i, vp]),
        "meshenv_smooth": (i, [vp, i, vp, i, i, i, vp, vp, vp]),
        "meshenv_smooth_final": (i, [vp, i, vp, i, f64, f64, vp, vp]),
        "meshenv_extract_samples": (i, [vp, i, vp, i, i, f64, i, f64] + [vp] * 6),
        "meshenv_gae": (i, [vp, i] + [vp] * 5 + [f64, f64, vp, vp, vp]),
        # the SAC actor; its last_error came later, with meshenv_offpolicy_learn.h
        **_family("meshenv_actor", parts=("create", "destroy", "set_stream")),
        "meshenv_actor_load": (i, [vp] * 13),
        "meshenv_actor_forward": (i, [vp, i, vp, vp, vp]),
        "meshenv_actor_sample": (i, [vp, i, vp, u64, u64, vp, vp]),
        "meshenv_step_actor": (i, [vp] * 8 + [i, i, u64, u64, vp, vp]),
        "meshenv_step_actor_multi": (i, [vp, vp, i] + [vp] * 6 + [i, i, u64, u64, vp]),
        # the PPO / A2C / TD3 policy
        **_family("meshenv_policy"),
        "meshenv_policy_load": (i, [vp, i, i, i] + [vp] * 15),
        "meshenv_policy_forward": (i, [vp, i, vp, vp, i, u64, u64] + [vp] * 5),
        "meshenv_step_policy_multi": (i, [vp, vp, i, vp, i, u64, u64] + [vp] * 11 + [i]),
        # the evaluation
        "meshenv_eval_begin": (i, [vp, eval_p]),
        "meshenv_eval_tally": (i, [vp, eval_p, i, vp, vp, vp]),
        "meshenv_evaluate": (i, [vp, vp, vp, i, u64, u64, i, i, eval_p, i32p, i32p]),
        # the replay buffer
        "meshenv_replay_record_floats": (i, []),
        "meshenv_replay_add": (i, [vp, i] + [vp] * 7 + [f32p, i, vp, i, i]),
        "meshenv_replay_sample": (i, [vp, vp, i, i, i, u64, u64] + [vp] * 9),
        # the SAC / TD3 TD target, critic loss gradient and SAC actor loss gradient
        **_family("meshenv_target", i, f32, f32, f32, f32),
        "meshenv_target_bind": (i, [vp, vpp, i, vpp, vpp, i, vp]),
        "meshenv_target_refresh": (i, [vp]),
        "meshenv_target_forward": (i, [vp, i, vp, vp, vp, vp, i, u64, u64] + [vp] * 6),
        **_family("meshenv_critic_grad", i),
        "meshenv_critic_grad_bind": (i, [vp, vpp, vpp, i, vp, i64]),
        "meshenv_critic_grad_backward": (i, [vp, i] + [vp] * 6 + [vpp, vpp]),
        **_family("meshenv_actor_grad", f32, f32),
        "meshenv_actor_grad_bind": (i, [vp, vpp, i, vpp, vpp, i, vp, vp, i64]),
        "meshenv_actor_grad_backward": (i, [vp, i, vp, vp, i, u64, u64, vp, vp, vpp, vpp]),
    },
    "meshenv_optim.h": {    # the optimiser step
        **_family("meshenv_optim"),
        "meshenv_optim_bind": (i, [vp, i, i] + [vpp] * 5 + [i64p, i32p, i32p, i32p]),
        "meshenv_optim_step": (i, [vp, i, scalars_p]),
    },
    "meshenv_td3_actor_grad.h": {   # the TD3 actor loss gradient (meshenv_actor_grad_* of meshenv.h is the SAC statement)
        **_family("meshenv_td3_actor_grad"),
        "meshenv_td3_actor_grad_bind": (i, [vp, vpp, i, vpp, i, vp, i64]),
        "meshenv_td3_actor_grad_backward": (i, [vp, i, vp, vp, vpp, vpp]),
    },
    "meshenv_ppo_grad.h": {     # the PPO / A2C loss gradient, and the refresh of a loaded policy from its live tensors
        **_family("meshenv_ppo_grad"),
        "meshenv_ppo_grad_bind": (i, [vp, i, i, vpp, i, vp, i64]),
        "meshenv_ppo_grad_backward": (i, [vp, i] + [vp] * 5 + [i, f64, f32, f32, i, i, f32, vp, vpp, vpp]),
        "meshenv_policy_bind": (i, [vp, vpp, i]),
        "meshenv_policy_refresh": (i, [vp]),
    },
    "meshenv_rollout.h": {      # the on-policy rollout buffer (one gather launch per epoch)
        **_family("meshenv_rollout"),
        "meshenv_rollout_gather": (i, [vp, i, i, vp, i, vpp, vpp, i]),
    },
    "meshenv_onpolicy_train.h": {   # PPO.train / A2C.train as one call
        **_family("meshenv_onpolicy_train"),
        "meshenv_onpolicy_train_run": (i, [vp, vp, vp, i, vp,           # t, g, o, program, r
                                           vp, i, i, vpp, vpp,          # policy, T, n_envs, in_dev, gather_dev
                                           vp, i, i, i, i, f64,         # perm_dev, perm_bytes, n_epochs, batch_size, a2c, clip_range
                                           f32, f32, i, i, f32,         # ent_coef, vf_coef, normalize_advantage, clip_grad, max_grad_norm
                                           f64, scalars_p, i, vp]),     # target_kl, scalars, n_scalars, out_dev
    },
    "meshenv_onpolicy_learn.h": {   # the counted train() of a PPO learn loop with a target_kl
        **_family("meshenv_onpolicy_learn"),
        "meshenv_onpolicy_learn_bind": (i, [vp, f64p, i, i, vp, i64]),
        "meshenv_onpolicy_learn_run": (i, [vp, vp, vp, vp, i,           # l, t, g, o, program
                                           vp, vp, i, i, vpp,           # r, policy, T, n_envs, in_dev
                                           vpp, vp, i, i, i, i,         # gather_dev, perm_dev, perm_bytes, n_epochs, batch_size, a2c
                                           f64, f32, f32, i, i,         # clip_range, ent_coef, vf_coef, normalize_advantage, clip_grad
                                           f32, f64, counted_p, vp,     # max_grad_norm, target_kl, counted, history_dev
                                           i, i]),                      # iteration, iterations
    },
    "meshenv_offpolicy_train.h": {  # SAC.train / TD3.train as one call, and the draw of all its minibatches
        **_family("meshenv_offpolicy_train"),
        "meshenv_offpolicy_train_run": (i, [vp] * 7 + [                 # t, env, target, cg, sac_ag, td3_ag, o
                                            i, vp, i, i,                # critic_program, store_dev, rows, size
                                            i, i, u64, u64, vpp, i,     # batch, K, seed, counter0, sample_dev, chunk
                                            vp, i32p, scalars_p,        # target_dev, actor_program, critic_scalars
                                            scalars_p, i, vp]),         # actor_scalars, n_actor_scalars, out_dev
        "meshenv_replay_sample_batches": (i, [vp, vp, i, i, i, i, u64, u64] + [vp] * 7),
    },
    "meshenv_offpolicy_learn.h": {  # the live SAC behaviour actor, the warm-up actions and their steps, the episode statistics
        "meshenv_actor_bind": (i, [vp, vpp, i]),
        "meshenv_actor_refresh": (i, [vp]),
        **_family("meshenv_actor", parts=("last_error",)),
        "meshenv_uniform_actions": (i, [vp, i, u64, u64, f32p, vp, vp]),
        "meshenv_step_actions_multi": (i, [vp, i] + [vp] * 6 + [i]),
        **_family("meshenv_episode_stats"),
        "meshenv_episode_stats_update": (i, [vp, i, i, i] + [vp] * 9),
    },
    "meshenv_eval_callback.h": {    # the queued evaluation, the reduction of its records with the best-mean gate, the gated copy
        "meshenv_evaluate_queued": (i, [vp, vp, vp, i, u64, u64, i, eval_p]),
        **_family("meshenv_eval_callback"),
        "meshenv_eval_reduce": (i, [vp, i, i, eval_p, i, i, f64, vp, vp, vp]),
        "meshenv_keep_best": (i, [vp, keep_p, i, vp, i64, vp]),
    },
    "meshenv_topology.h": {     # the topology report, its attachment to the tally, the counting on logs the caller wrote
        "meshenv_mesh_topology": (i, [vp, i, vp, vp, vp]),
        "meshenv_eval_set_topology": (i, [vp, vp]),
        "meshenv_topology_selftest": (i, [i, i, vp, vp, vp, vp, i, vp, vp]),
    },
    "meshenv_fnn.h": {      # the forward of the supervised element-extraction network and the meshing loop around meshenv_move
        **_family("meshenv_fnn"),
        "meshenv_fnn_pack": (i, [vpp, vp, vp]),
        "meshenv_fnn_load": (i, [vp, vpp, vp]),
        "meshenv_fnn_forward": (i, [vp, i] + [vp] * 6),
        "meshenv_move_fnn_multi": (i, [vp, vp, i] + [vp] * 13),
    },
    "meshenv_fnn_train.h": {    # the loss gradient of the supervised network, and the refresh of a loaded FusedFNN
        **_family("meshenv_fnn_grad"),
        "meshenv_fnn_grad_bind": (i, [vp, vpp, vp, i64]),
        "meshenv_fnn_grad_backward": (i, [vp, i, i] + [vp] * 5),
        "meshenv_fnn_bind": (i, [vp, vpp]),
        "meshenv_fnn_refresh": (i, [vp]),
    },
    "meshenv_augment.h": {      # the synthetic training samples of the supervised network (MeshAugmentation.sampling)
        **_family("meshenv_augment"),
        "meshenv_augment_score": (i, [vp, i, vp, vp, f64, vp, vp, vp, vp]),
        "meshenv_augment_propose": (i, [vp, i] + [vp] * 9),
        "meshenv_augment_sample": (i, [vp, i64, f64, u64, i, i, i, i64] + [vp] * 6),
    },
    "meshenv_ddpg.h": {     # the load of DDPG's [400, 300] actor into a MeshPolicy
        "meshenv_policy_load_widths": (i, [vp, i, i, i, i] + [vp] * 9),
    },
    "meshenv_ddpg_grad.h": {    # DDPG's two gradient statements at [400, 300]
        **_family("meshenv_ddpg_grad", f32),
        "meshenv_ddpg_grad_bind": (i, [vp, vpp, i, vpp, i, vp, i64]),
        "meshenv_ddpg_grad_critic_backward": (i, [vp, i, vp, vp, vp, vp, vpp]),
        "meshenv_ddpg_grad_actor_backward": (i, [vp, i, vp, vp, vpp, vpp]),
    },
}

# every symbol include/meshenv.h declares, and the same for each later header
EXPORTS = list(SIGNATURES["meshenv.h"])
EXPORTS_OPTIM = list(SIGNATURES["meshenv_optim.h"])
EXPORTS_TD3_ACTOR_GRAD = list(SIGNATURES["meshenv_td3_actor_grad.h"])
EXPORTS_PPO_GRAD = list(SIGNATURES["meshenv_ppo_grad.h"])
EXPORTS_ROLLOUT = list(SIGNATURES["meshenv_rollout.h"])
EXPORTS_ONPOLICY_TRAIN = list(SIGNATURES["meshenv_onpolicy_train.h"])
EXPORTS_ONPOLICY_LEARN = list(SIGNATURES["meshenv_onpolicy_learn.h"])
EXPORTS_OFFPOLICY_TRAIN = list(SIGNATURES["meshenv_offpolicy_train.h"])
EXPORTS_OFFPOLICY_LEARN = list(SIGNATURES["meshenv_offpolicy_learn.h"])
EXPORTS_EVAL_CALLBACK = list(SIGNATURES["meshenv_eval_callback.h"])
EXPORTS_TOPOLOGY = list(SIGNATURES["meshenv_topology.h"])
EXPORTS_FNN = list(SIGNATURES["meshenv_fnn.h"])
EXPORTS_FNN_TRAIN = list(SIGNATURES["meshenv_fnn_train.h"])
EXPORTS_AUGMENT = list(SIGNATURES["meshenv_augment.h"])
EXPORTS_DDPG = list(SIGNATURES["meshenv_ddpg.h"])
EXPORTS_DDPG_GRAD = list(SIGNATURES["meshenv_ddpg_grad.h"])


def load():
    """Load the HIP library (no GPU needed for loading; compute calls need one)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MESHENV_LIB", LIB_PATH)  # A/B builds of the same library
    if not os.path.exists(path) and path == LIB_PATH:
        try:  # a fresh checkout: compile the library in-tree (needs hipcc); never a substitute implementation
            from .build import build
            build(force=True)
        except Exception as exc:
            raise MeshEnvError(f"{LIB_PATH} is missing and could not be built ({exc}); this package has no CPU "
                               "fallback") from exc
    if not os.path.exists(path):
        raise MeshEnvError(
            f"{path} is missing: build it with `python -m reinforcementlearning4meshgeneration_amd.build` "
            "(hipcc, gfx950).  This package has no CPU fallback.")
    try:
        # torch ships its own copy of the HIP runtime; loading it first makes this library bind to the same one (two
        # runtimes in one process do not share the device: torch.cuda.is_available() turns False if ours initialises first)
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    for rows in SIGNATURES.values():
        for name, (restype, argtypes) in rows.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def default_params() -> MeshEnvParams:
    p = MeshEnvParams()
    load().meshenv_default_params(C.byref(p))
    return p


def topology_selftest(meshes, n0, n_new, width, valence_fill=None, report_fill=0, device=0):
    """meshenv_topology_selftest (include/meshenv_topology.h): the counting of k_mesh_topology / k_eval_topology on element logs
    the caller wrote.  meshes: one [n, 4] id array per mesh (domain vertex i -> i, k-th generated vertex -> n0 + k), n0 / n_new:
    one int per mesh.  Returns (rc, report int32 [M, 16], valence uint8 [M, width] or None); the two arrays start as
    report_fill / valence_fill (None = no valence rows), so what the kernel did not write keeps that value."""
    import numpy as np
    quads = [np.asarray(q, np.int32).reshape(-1, 4) for q in meshes]
    offsets = np.concatenate([[0], np.cumsum([len(q) for q in quads])]).astype(np.int32)
    flat = np.ascontiguousarray(np.concatenate(quads + [np.zeros((1, 4), np.int32)]))    # never an empty buffer
    n0 = np.ascontiguousarray(n0, np.int32)
    n_new = np.ascontiguousarray(n_new, np.int32)
    if not (len(quads) == len(n0) == len(n_new)):
        raise ValueError("topology_selftest: one n0 and one n_new per mesh")
    report = np.full((len(quads), TOPOLOGY_DIM), report_fill, np.int32)
    valence = None if valence_fill is None else np.full((len(quads), max(int(width), 0)), valence_fill, np.uint8)
    rc = load().meshenv_topology_selftest(device, len(quads), offsets.ctypes.data, flat.ctypes.data, n0.ctypes.data, n_new.ctypes.data,
                                          int(width), report.ctypes.data, None if valence is None else valence.ctypes.data)
    return rc, report, valence


def check(handle, rc: int, what: str):
    if rc != 0:
        msg = load().meshenv_last_error(handle)
        raise MeshEnvError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
