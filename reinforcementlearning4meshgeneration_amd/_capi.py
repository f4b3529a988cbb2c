"""ctypes binding of libmeshenv_hip.so (include/meshenv.h, meshenv_optim.h, meshenv_td3_actor_grad.h,
meshenv_ppo_grad.h, meshenv_rollout.h, meshenv_onpolicy_train.h, meshenv_onpolicy_learn.h, meshenv_offpolicy_train.h, meshenv_offpolicy_learn.h, meshenv_eval_callback.h, meshenv_topology.h, meshenv_fnn.h, meshenv_fnn_train.h, meshenv_augment.h, meshenv_ddpg.h, meshenv_ddpg_grad.h).  Fails loudly when the library is missing:
there is no CPU fallback anywhere in this package."""
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


class MeshEnvError(RuntimeError):
    pass


_lib = None

# every symbol include/meshenv.h declares
EXPORTS = [
    "meshenv_default_params", "meshenv_abi_version", "meshenv_device_count", "meshenv_create", "meshenv_destroy",
    "meshenv_last_error", "meshenv_set_stream", "meshenv_num_envs", "meshenv_max_ring", "meshenv_group_size", "meshenv_reset",
    "meshenv_step", "meshenv_rollout", "meshenv_get_status", "meshenv_get_state", "meshenv_get_elements",
    "meshenv_counters", "meshenv_set_timing", "meshenv_kernel_times", "meshenv_selftest", "meshenv_set_packed_output",
    "meshenv_actor_create", "meshenv_actor_destroy", "meshenv_actor_set_stream", "meshenv_actor_load",
    "meshenv_actor_forward", "meshenv_actor_sample", "meshenv_get_last_episode", "meshenv_element_quality",
    "meshenv_reset_static", "meshenv_move", "meshenv_get_not_valid", "meshenv_step_kernel", "meshenv_rollout_kernel",
    "meshenv_create_random", "meshenv_get_domain", "meshenv_smooth", "meshenv_smooth_final", "meshenv_get_not_valid_ids", "meshenv_step_actor",
    "meshenv_libm_exact", "meshenv_create_random_density", "meshenv_density_rings",
    "meshenv_step_actor_multi", "meshenv_extract_samples", "meshenv_atan2_exact", "meshenv_quad_quality",
    "meshenv_policy_create", "meshenv_policy_destroy", "meshenv_policy_set_stream", "meshenv_policy_load",
    "meshenv_policy_forward", "meshenv_step_policy_multi", "meshenv_policy_last_error", "meshenv_gae",
    "meshenv_eval_begin", "meshenv_eval_tally", "meshenv_evaluate",
    "meshenv_replay_record_floats", "meshenv_replay_add", "meshenv_replay_sample",
    "meshenv_target_create", "meshenv_target_destroy", "meshenv_target_set_stream", "meshenv_target_last_error",
    "meshenv_target_bind", "meshenv_target_refresh", "meshenv_target_forward",
    "meshenv_critic_grad_create", "meshenv_critic_grad_destroy", "meshenv_critic_grad_set_stream",
    "meshenv_critic_grad_last_error", "meshenv_critic_grad_bind", "meshenv_critic_grad_backward",
    "meshenv_actor_grad_create", "meshenv_actor_grad_destroy", "meshenv_actor_grad_set_stream",
    "meshenv_actor_grad_last_error", "meshenv_actor_grad_bind", "meshenv_actor_grad_backward",
    "meshenv_step_kernel_name", "meshenv_rollout_kernel_name",
]

# every symbol include/meshenv_optim.h declares (the optimiser step has a header of its own)
EXPORTS_OPTIM = [
    "meshenv_optim_create", "meshenv_optim_destroy", "meshenv_optim_set_stream", "meshenv_optim_last_error",
    "meshenv_optim_bind", "meshenv_optim_step",
]
OPTIM_PROGRAMS, OPTIM_BLOCKS, OPTIM_CHUNK = 8, 4, 1024
OPTIM_ADAM, OPTIM_POLYAK, OPTIM_ADAM_POLYAK, OPTIM_RMSPROP = 1, 2, 3, 4

# every symbol include/meshenv_td3_actor_grad.h declares (meshenv_actor_grad_* of meshenv.h is the SAC statement)
EXPORTS_TD3_ACTOR_GRAD = [
    "meshenv_td3_actor_grad_create", "meshenv_td3_actor_grad_destroy", "meshenv_td3_actor_grad_set_stream",
    "meshenv_td3_actor_grad_last_error", "meshenv_td3_actor_grad_bind", "meshenv_td3_actor_grad_backward",
]
TD3_ACTOR_GRAD_FLOATS = 71488

# every symbol include/meshenv_ppo_grad.h declares: the PPO / A2C statement, and the refresh of a loaded policy from its live tensors
EXPORTS_PPO_GRAD = [
    "meshenv_ppo_grad_create", "meshenv_ppo_grad_destroy", "meshenv_ppo_grad_set_stream", "meshenv_ppo_grad_last_error",
    "meshenv_ppo_grad_bind", "meshenv_ppo_grad_backward", "meshenv_policy_bind", "meshenv_policy_refresh",
]
PPO_GRAD_FLOATS = {64: 11072, 128: 38464}
PPO_GRAD_OUTPUTS, PPO_GRAD_PARTS = 8, 5

# every symbol include/meshenv_rollout.h declares: the on-policy rollout buffer (one gather launch per epoch)
EXPORTS_ROLLOUT = [
    "meshenv_rollout_create", "meshenv_rollout_destroy", "meshenv_rollout_set_stream", "meshenv_rollout_last_error",
    "meshenv_rollout_gather",
]
ROLLOUT_FIELDS, ROLLOUT_CHUNK, ROLLOUT_MAX_ROWS = 6, 1024, 2 ** 24 - 16

# every symbol include/meshenv_onpolicy_train.h declares: PPO.train / A2C.train as one call
EXPORTS_ONPOLICY_TRAIN = [
    "meshenv_onpolicy_train_create", "meshenv_onpolicy_train_destroy", "meshenv_onpolicy_train_set_stream",
    "meshenv_onpolicy_train_last_error", "meshenv_onpolicy_train_run",
]
TRAIN_OUTPUTS, TRAIN_MAX_MINIBATCHES = 12, 65536

# every symbol include/meshenv_onpolicy_learn.h declares: the counted train() of a PPO learn loop with a target_kl
EXPORTS_ONPOLICY_LEARN = [
    "meshenv_onpolicy_learn_create", "meshenv_onpolicy_learn_destroy", "meshenv_onpolicy_learn_set_stream",
    "meshenv_onpolicy_learn_last_error", "meshenv_onpolicy_learn_bind", "meshenv_onpolicy_learn_run",
]
LEARN_WORDS, LEARN_MAX_ENTRIES = 3, 2 ** 20
LEARN_WORD_N_UPDATES, LEARN_WORD_ERROR, LEARN_WORD_STEPS = 0, 1, 2

# every symbol include/meshenv_offpolicy_train.h declares: SAC.train / TD3.train as one call, and the draw of all its minibatches
EXPORTS_OFFPOLICY_TRAIN = [
    "meshenv_offpolicy_train_create", "meshenv_offpolicy_train_destroy", "meshenv_offpolicy_train_set_stream",
    "meshenv_offpolicy_train_last_error", "meshenv_offpolicy_train_run", "meshenv_replay_sample_batches",
]
OFFTRAIN_OUTPUTS, OFFTRAIN_MAX_STEPS = 8, 65536
OFFTRAIN_SAMPLE_FLOATS, REPLAY_BATCHES_MAX_SAMPLES = 41, 2 ** 24

# every symbol include/meshenv_offpolicy_learn.h declares: the live SAC behaviour actor, the warm-up actions and their steps, the
# episode statistics
EXPORTS_OFFPOLICY_LEARN = [
    "meshenv_actor_bind", "meshenv_actor_refresh", "meshenv_actor_last_error", "meshenv_uniform_actions",
    "meshenv_step_actions_multi", "meshenv_episode_stats_create", "meshenv_episode_stats_destroy",
    "meshenv_episode_stats_set_stream", "meshenv_episode_stats_last_error", "meshenv_episode_stats_update",
]
UNIFORM_PHILOX_TAG, EPISODE_RING_DOUBLES = 4, 3

# every symbol include/meshenv_eval_callback.h declares: the queued evaluation, the reduction of its records with the best-mean
# gate, the gated copy of the live parameters
EXPORTS_EVAL_CALLBACK = [
    "meshenv_evaluate_queued", "meshenv_eval_callback_create", "meshenv_eval_callback_destroy", "meshenv_eval_callback_set_stream",
    "meshenv_eval_callback_last_error", "meshenv_eval_reduce", "meshenv_keep_best",
]
EVAL_ROW_DOUBLES, EVAL_STATE_DOUBLES, KEEP_BEST_MAX_ENTRIES = 9, 4, 64
EVAL_COLUMNS = ("num_timesteps", "mean_reward", "std_reward", "mean_ep_length", "recorded", "short", "complete_rate",
                "mean_n_elements", "improved")

# every symbol include/meshenv_topology.h declares: the topology report of the generated meshes, its attachment to the tally, and
# the test entry point that runs the counting on element logs the caller wrote
EXPORTS_TOPOLOGY = ["meshenv_mesh_topology", "meshenv_eval_set_topology", "meshenv_topology_selftest"]
TOPOLOGY_DIM = 16
TOPO_OK, TOPO_MASKED, TOPO_LOG_OVERFLOW, TOPO_DEGREE, TOPO_NOT_ARCHIVED = 0, 1, 2, 3, 4

# every symbol include/meshenv_fnn.h declares: the forward of the supervised element-extraction network and the meshing loop
# around meshenv_move
EXPORTS_FNN = [
    "meshenv_fnn_create", "meshenv_fnn_destroy", "meshenv_fnn_set_stream", "meshenv_fnn_last_error", "meshenv_fnn_pack",
    "meshenv_fnn_load", "meshenv_fnn_forward", "meshenv_move_fnn_multi",
]
FNN_TENSORS, FNN_PACKED_FLOATS, MOVE_SKIPPED = 14, 21568, 255

# every symbol include/meshenv_fnn_train.h declares: the loss gradient of the supervised network (train_ch3) and the refresh of a
# loaded FusedFNN from its live tensors
EXPORTS_FNN_TRAIN = [
    "meshenv_fnn_grad_create", "meshenv_fnn_grad_destroy", "meshenv_fnn_grad_set_stream", "meshenv_fnn_grad_last_error",
    "meshenv_fnn_grad_bind", "meshenv_fnn_grad_backward", "meshenv_fnn_bind", "meshenv_fnn_refresh",
]
FNN_GRAD_FLOATS, FNN_GRAD_OUTPUTS, FNN_GRAD_MAX_GROUPS = 20544, 4, 128

# every symbol include/meshenv_augment.h declares: the synthetic training samples of the supervised network (MeshAugmentation.sampling)
EXPORTS_AUGMENT = [
    "meshenv_augment_create", "meshenv_augment_destroy", "meshenv_augment_set_stream", "meshenv_augment_last_error",
    "meshenv_augment_score", "meshenv_augment_propose", "meshenv_augment_sample",
]
AUGMENT_PHILOX_TAG, AUGMENT_BINS, AUGMENT_TYPES, AUGMENT_MAX_ACTIONS, AUGMENT_UNIFORMS = 5, 11, 3, 20, 57
AUGMENT_MAX_POOL, AUGMENT_MAX_ROUND, AUGMENT_MAX_ROUNDS, AUGMENT_STATS = 1024, 2 ** 20, 4095, 4

# every symbol include/meshenv_ddpg.h declares: the load of DDPG's [400, 300] actor into a MeshPolicy
EXPORTS_DDPG = ["meshenv_policy_load_widths"]

# every symbol include/meshenv_ddpg_grad.h declares: DDPG's two gradient statements at [400, 300]
EXPORTS_DDPG_GRAD = [
    "meshenv_ddpg_grad_create", "meshenv_ddpg_grad_destroy", "meshenv_ddpg_grad_set_stream", "meshenv_ddpg_grad_last_error",
    "meshenv_ddpg_grad_bind", "meshenv_ddpg_grad_critic_backward", "meshenv_ddpg_grad_actor_backward",
]
DDPG_GRAD_ACTOR_FLOATS, DDPG_GRAD_CRITIC_FLOATS, DDPG_GRAD_MAX_ROWS = 128832, 129408, 65536


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
    vp, i32p, f64p, u8p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p, C.c_void_p
    L.meshenv_default_params.argtypes = [C.POINTER(MeshEnvParams)]
    L.meshenv_default_params.restype = None
    L.meshenv_abi_version.restype = C.c_int
    L.meshenv_device_count.restype = C.c_int
    L.meshenv_create.argtypes = [C.c_int, C.c_int, i32p, f64p, f64p, C.c_int, i32p, C.POINTER(MeshEnvParams), vp,
                                 C.POINTER(vp)]
    L.meshenv_create.restype = C.c_int
    L.meshenv_create_random.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_double, C.POINTER(MeshEnvParams), vp,
                                        C.POINTER(vp)]
    L.meshenv_create_random.restype = C.c_int
    L.meshenv_create_random_density.argtypes = [C.c_int, C.c_int, C.c_uint64, vp, C.c_int, C.c_double, C.c_double,
                                                C.POINTER(MeshEnvParams), vp, C.POINTER(vp), vp]
    L.meshenv_create_random_density.restype = C.c_int
    L.meshenv_density_rings.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_double, vp, vp, vp, C.c_int64]
    L.meshenv_density_rings.restype = C.c_int
    L.meshenv_get_domain.argtypes = [vp, C.c_int, vp, C.c_int, i32p, vp]
    L.meshenv_get_domain.restype = C.c_int
    L.meshenv_destroy.argtypes = [vp]
    L.meshenv_destroy.restype = None
    L.meshenv_last_error.argtypes = [vp]
    L.meshenv_last_error.restype = C.c_char_p
    L.meshenv_set_stream.argtypes = [vp, vp]
    L.meshenv_num_envs.argtypes = [vp]
    L.meshenv_max_ring.argtypes = [vp]
    L.meshenv_group_size.argtypes = [vp]
    L.meshenv_group_size.restype = C.c_int
    L.meshenv_step_kernel.argtypes = [vp]
    L.meshenv_step_kernel.restype = C.c_int
    L.meshenv_rollout_kernel.argtypes = [vp]
    L.meshenv_rollout_kernel.restype = C.c_int
    L.meshenv_step_kernel_name.argtypes = [vp]
    L.meshenv_step_kernel_name.restype = C.c_char_p
    L.meshenv_rollout_kernel_name.argtypes = [vp]
    L.meshenv_rollout_kernel_name.restype = C.c_char_p
    L.meshenv_libm_exact.argtypes = [vp]
    L.meshenv_libm_exact.restype = C.c_int
    L.meshenv_atan2_exact.argtypes = []
    L.meshenv_atan2_exact.restype = C.c_int
    L.meshenv_reset.argtypes = [vp, u8p, f32p]
    L.meshenv_reset_static.argtypes = [vp, u8p, f32p, C.c_int]
    L.meshenv_move.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.meshenv_get_not_valid.argtypes = [vp, C.c_int, vp, C.c_int, i32p]
    L.meshenv_get_not_valid_ids.argtypes = [vp, C.c_int, vp, C.c_int, i32p, vp]
    L.meshenv_get_not_valid_ids.restype = C.c_int
    L.meshenv_step_actor.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, vp]
    L.meshenv_step_actor.restype = C.c_int
    L.meshenv_step_actor_multi.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.meshenv_step_actor_multi.restype = C.c_int
    L.meshenv_extract_samples.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, vp, vp, vp, vp, vp, vp]
    L.meshenv_extract_samples.restype = C.c_int
    L.meshenv_smooth.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.meshenv_smooth.restype = C.c_int
    L.meshenv_smooth_final.argtypes = [vp, C.c_int, vp, C.c_int, C.c_double, C.c_double, vp, vp]
    L.meshenv_smooth_final.restype = C.c_int
    L.meshenv_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int]
    L.meshenv_rollout.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int]
    L.meshenv_get_status.argtypes = [vp, vp]
    L.meshenv_get_state.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.meshenv_get_elements.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, i32p, i32p]
    L.meshenv_get_last_episode.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, i32p, i32p, i32p, i32p]
    L.meshenv_element_quality.argtypes = [vp, C.c_int, vp, vp, vp]
    L.meshenv_quad_quality.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    L.meshenv_quad_quality.restype = C.c_int
    L.meshenv_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.meshenv_set_timing.argtypes = [vp, C.c_int]
    L.meshenv_kernel_times.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int32)]
    L.meshenv_selftest.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.meshenv_selftest.restype = C.c_int
    L.meshenv_set_packed_output.argtypes = [vp, vp]
    L.meshenv_set_packed_output.restype = C.c_int
    # the handle families: <prefix>_create(device, stream, <extra>, out), _destroy, _set_stream and (all but the actor) _last_error
    f32 = C.c_float
    for prefix, extra, has_last_error in (("meshenv_actor", [], False), ("meshenv_policy", [], True),
                                          ("meshenv_target", [C.c_int, f32, f32, f32, f32], True),
                                          ("meshenv_critic_grad", [C.c_int], True), ("meshenv_actor_grad", [f32, f32], True),
                                          ("meshenv_optim", [], True), ("meshenv_td3_actor_grad", [], True),
                                          ("meshenv_ppo_grad", [], True), ("meshenv_rollout", [], True),
                                          ("meshenv_onpolicy_train", [], True), ("meshenv_onpolicy_learn", [], True),
                                          ("meshenv_offpolicy_train", [], True),
                                          ("meshenv_episode_stats", [], True), ("meshenv_eval_callback", [], True),
                                          ("meshenv_fnn", [], True), ("meshenv_fnn_grad", [], True),
                                          ("meshenv_augment", [], True), ("meshenv_ddpg_grad", [f32], True)):
        fn = lambda name: getattr(L, f"{prefix}_{name}")   # noqa: E731
        fn("create").argtypes, fn("create").restype = [C.c_int, vp] + extra + [C.POINTER(vp)], C.c_int
        fn("destroy").argtypes, fn("destroy").restype = [vp], None
        fn("set_stream").argtypes, fn("set_stream").restype = [vp, vp], C.c_int
        if has_last_error:
            fn("last_error").argtypes, fn("last_error").restype = [vp], C.c_char_p
    L.meshenv_actor_load.argtypes = [vp] + [vp] * 12
    L.meshenv_actor_forward.argtypes = [vp, C.c_int, vp, vp, vp]
    L.meshenv_actor_sample.argtypes = [vp, C.c_int, vp, C.c_uint64, C.c_uint64, vp, vp]
    L.meshenv_policy_load.argtypes = [vp, C.c_int, C.c_int, C.c_int] + [vp] * 15
    L.meshenv_policy_load_widths.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 9
    L.meshenv_policy_forward.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp]
    L.meshenv_step_policy_multi.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_uint64, C.c_uint64] + [vp] * 11 + [C.c_int]
    L.meshenv_gae.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp]
    L.meshenv_gae.restype = C.c_int
    evp = C.POINTER(MeshEvalBuffers)
    L.meshenv_eval_begin.argtypes = [vp, evp]
    L.meshenv_eval_begin.restype = C.c_int
    L.meshenv_eval_tally.argtypes = [vp, evp, C.c_int, vp, vp, vp]
    L.meshenv_eval_tally.restype = C.c_int
    L.meshenv_evaluate.argtypes = [vp, vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, evp, i32p, i32p]
    L.meshenv_evaluate.restype = C.c_int
    L.meshenv_replay_record_floats.argtypes = []
    L.meshenv_replay_record_floats.restype = C.c_int
    L.meshenv_replay_add.argtypes = [vp, C.c_int] + [vp] * 7 + [C.POINTER(C.c_float), C.c_int, vp, C.c_int, C.c_int]
    L.meshenv_replay_add.restype = C.c_int
    L.meshenv_replay_sample.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64] + [vp] * 9
    L.meshenv_replay_sample.restype = C.c_int
    L.meshenv_target_bind.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, vp]
    L.meshenv_target_refresh.argtypes = [vp]
    L.meshenv_target_forward.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_uint64, C.c_uint64] + [vp] * 6
    L.meshenv_critic_grad_bind.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, vp, C.c_int64]
    L.meshenv_critic_grad_backward.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    L.meshenv_actor_grad_bind.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, vp, vp, C.c_int64]
    L.meshenv_actor_grad_backward.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_uint64, C.c_uint64, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    L.meshenv_td3_actor_grad_bind.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, vp, C.c_int64]
    L.meshenv_td3_actor_grad_backward.argtypes = [vp, C.c_int, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    L.meshenv_ddpg_grad_bind.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, vp, C.c_int64]
    L.meshenv_ddpg_grad_critic_backward.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.POINTER(vp)]
    L.meshenv_ddpg_grad_actor_backward.argtypes = [vp, C.c_int, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    L.meshenv_ddpg_grad_bind.restype = L.meshenv_ddpg_grad_critic_backward.restype = L.meshenv_ddpg_grad_actor_backward.restype = C.c_int
    L.meshenv_ppo_grad_bind.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp), C.c_int, vp, C.c_int64]
    L.meshenv_ppo_grad_backward.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_double, f32, f32, C.c_int, C.c_int, f32, vp,
                                            C.POINTER(vp), C.POINTER(vp)]
    L.meshenv_policy_bind.argtypes = [vp, C.POINTER(vp), C.c_int]
    L.meshenv_policy_refresh.argtypes = [vp]
    L.meshenv_optim_bind.argtypes = [vp, C.c_int, C.c_int] + [C.POINTER(vp)] * 5 + [C.POINTER(C.c_int64)] + [C.POINTER(C.c_int32)] * 3
    L.meshenv_optim_step.argtypes = [vp, C.c_int, C.POINTER(MeshOptimScalars)]
    L.meshenv_rollout_gather.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int]
    L.meshenv_onpolicy_train_run.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), vp, C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.c_double, f32, f32, C.c_int, C.c_int, f32, C.c_double,
                                             C.POINTER(MeshOptimScalars), C.c_int, vp]
    L.meshenv_onpolicy_learn_bind.argtypes = [vp, C.POINTER(C.c_double), C.c_int, C.c_int, vp, C.c_int64]
    L.meshenv_onpolicy_learn_run.argtypes = [vp] + L.meshenv_onpolicy_train_run.argtypes[:22] + [C.POINTER(MeshOptimCounted), vp, C.c_int,
                                                                                              C.c_int]
    L.meshenv_onpolicy_learn_bind.restype = L.meshenv_onpolicy_learn_run.restype = C.c_int
    L.meshenv_replay_sample_batches.argtypes =[vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64] + [vp] * 7
    L.meshenv_offpolicy_train_run.argtypes = [vp] * 7 + [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                              C.POINTER(vp), C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(MeshOptimScalars),
                                              C.POINTER(MeshOptimScalars), C.c_int, vp]
    L.meshenv_actor_bind.argtypes = [vp, C.POINTER(vp), C.c_int]
    L.meshenv_actor_refresh.argtypes = [vp]
    L.meshenv_actor_last_error.argtypes, L.meshenv_actor_last_error.restype = [vp], C.c_char_p
    L.meshenv_uniform_actions.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_float), vp, vp]
    L.meshenv_step_actions_multi.argtypes = [vp, C.c_int] + [vp] * 6 + [C.c_int]
    L.meshenv_episode_stats_update.argtypes = [vp, C.c_int, C.c_int, C.c_int] + [vp] * 9
    L.meshenv_evaluate_queued.argtypes = [vp, vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int, evp]
    L.meshenv_eval_reduce.argtypes = [vp, C.c_int, C.c_int, evp, C.c_int, C.c_int, C.c_double, vp, vp, vp]
    L.meshenv_keep_best.argtypes = [vp, C.POINTER(MeshKeepEntry), C.c_int, vp, C.c_int64, vp]
    L.meshenv_mesh_topology.argtypes, L.meshenv_mesh_topology.restype = [vp, C.c_int, vp, vp, vp], C.c_int
    L.meshenv_eval_set_topology.argtypes, L.meshenv_eval_set_topology.restype = [vp, vp], C.c_int
    L.meshenv_topology_selftest.argtypes, L.meshenv_topology_selftest.restype = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp], C.c_int
    L.meshenv_fnn_pack.argtypes = [C.POINTER(vp), vp, vp]
    L.meshenv_fnn_load.argtypes = [vp, C.POINTER(vp), vp]
    L.meshenv_fnn_forward.argtypes = [vp, C.c_int] + [vp] * 6
    L.meshenv_move_fnn_multi.argtypes = [vp, vp, C.c_int] + [vp] * 13
    L.meshenv_fnn_grad_bind.argtypes = [vp, C.POINTER(vp), vp, C.c_int64]
    L.meshenv_fnn_grad_backward.argtypes = [vp, C.c_int, C.c_int] + [vp] * 5
    L.meshenv_fnn_bind.argtypes = [vp, C.POINTER(vp)]
    L.meshenv_fnn_refresh.argtypes = [vp]
    L.meshenv_augment_score.argtypes = [vp, C.c_int, vp, vp, C.c_double, vp, vp, vp, vp]
    L.meshenv_augment_propose.argtypes = [vp, C.c_int] + [vp] * 9
    L.meshenv_augment_sample.argtypes = [vp, C.c_int64, C.c_double, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.meshenv_augment_score.restype = L.meshenv_augment_propose.restype = L.meshenv_augment_sample.restype = C.c_int
    for name in ("meshenv_fnn_pack", "meshenv_fnn_load", "meshenv_fnn_forward", "meshenv_move_fnn_multi", "meshenv_fnn_grad_bind",
                 "meshenv_fnn_grad_backward", "meshenv_fnn_bind", "meshenv_fnn_refresh"):
        getattr(L, name).restype = C.c_int
    for name in ("meshenv_actor_bind", "meshenv_actor_refresh", "meshenv_uniform_actions", "meshenv_step_actions_multi",
                 "meshenv_episode_stats_update", "meshenv_evaluate_queued", "meshenv_eval_reduce", "meshenv_keep_best"):
        getattr(L, name).restype = C.c_int
    for name in ("meshenv_replay_sample_batches", "meshenv_offpolicy_train_run", "meshenv_target_bind", "meshenv_target_refresh", "meshenv_target_forward", "meshenv_critic_grad_bind",
                 "meshenv_critic_grad_backward", "meshenv_actor_grad_bind", "meshenv_actor_grad_backward", "meshenv_optim_bind",
                 "meshenv_optim_step", "meshenv_policy_load", "meshenv_policy_load_widths", "meshenv_policy_forward", "meshenv_step_policy_multi",
                 "meshenv_actor_load", "meshenv_actor_forward", "meshenv_actor_sample", "meshenv_td3_actor_grad_bind",
                 "meshenv_td3_actor_grad_backward", "meshenv_ppo_grad_bind", "meshenv_ppo_grad_backward", "meshenv_policy_bind",
                 "meshenv_policy_refresh", "meshenv_rollout_gather", "meshenv_onpolicy_train_run"):
        getattr(L, name).restype = C.c_int
    for name in ("meshenv_reset_static", "meshenv_move", "meshenv_get_not_valid", "meshenv_set_stream", "meshenv_num_envs", "meshenv_max_ring", "meshenv_reset", "meshenv_step",
                 "meshenv_rollout", "meshenv_get_status", "meshenv_get_state", "meshenv_get_elements",
                 "meshenv_counters", "meshenv_set_timing", "meshenv_kernel_times", "meshenv_get_last_episode",
                 "meshenv_element_quality"):
        getattr(L, name).restype = C.c_int
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
