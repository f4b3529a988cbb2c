"""MI355X-native vectorised BoudaryEnv (quad element extraction) -- the step()/reset() hot path of
ZhuoQiuMcgill/ReinforcementLearning4MeshGeneration as hand-written HIP kernels behind a C-ABI.

    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, SB3MeshVecEnv, BoudaryEnv, boundary, read_polygon
"""
from .domains import boundary, domain_constants, generate_polygon, random_domain, read_polygon  # noqa: F401

__all__ = ["MeshVecEnv", "SB3MeshVecEnv", "BoudaryEnv", "boundary", "read_polygon", "domain_constants", "generate_polygon",
           "random_domain", "MeshEnvError", "FusedActor", "FusedPolicy", "EvalResult", "evaluate_policy",
           "DeviceReplayBuffer", "ReplayBufferSamples", "FusedTDTarget", "TDTargetSpec", "FusedCriticGrad", "CriticGradSpec",
           "FusedActorGrad", "ActorGradSpec", "FusedOptimStep", "OptimStepSpec", "FusedTD3ActorGrad", "TD3ActorGradSpec",
           "FusedPPOGrad", "PPOGradSpec", "DeviceRolloutBuffer", "RolloutBufferSamples", "FusedOnPolicyTrain", "OnPolicyTrainSpec",
           "TrainLogs", "FusedOffPolicyTrain", "OffPolicyTrainSpec", "OffPolicyTrainLogs", "FusedOffPolicyLearn",
           "OffPolicyLearnSpec", "OffPolicyLearnLogs", "EpisodeStats", "DeviceEvalCallback", "FusedOnPolicyLearn",
           "OnPolicyLearnSpec", "OnPolicyLearnLogs", "StepCounter", "FusedFNN", "FNNSpec", "FNNMeshResult",
           "FusedFNNTrain", "FNNTrainSpec", "FNNTrainLog", "DeviceMeshAugmentation", "AugmentScore", "FusedDDPGGrad", "DDPGGradSpec"]


def __getattr__(name):  # torch / the HIP library are only needed once an environment is built
    if name == "MeshVecEnv":
        from .vec_env import MeshVecEnv
        return MeshVecEnv
    if name == "SB3MeshVecEnv":
        from .vec_env import SB3MeshVecEnv
        return SB3MeshVecEnv
    if name == "BoudaryEnv":
        from .boundary_env import BoudaryEnv
        return BoudaryEnv
    if name == "MeshEnvError":
        from ._capi import MeshEnvError
        return MeshEnvError
    if name == "FusedActor":
        from .actor import FusedActor
        return FusedActor
    if name == "FusedPolicy":
        from .policy import FusedPolicy
        return FusedPolicy
    if name in ("EvalResult", "evaluate_policy"):
        from . import evaluation
        return getattr(evaluation, name)
    if name in ("DeviceReplayBuffer", "ReplayBufferSamples"):
        from . import replay
        return getattr(replay, name)
    if name in ("FusedTDTarget", "TDTargetSpec"):
        from . import td_target
        return getattr(td_target, name)
    if name in ("FusedCriticGrad", "CriticGradSpec"):
        from . import critic_grad
        return getattr(critic_grad, name)
    if name in ("FusedActorGrad", "ActorGradSpec"):
        from . import actor_grad
        return getattr(actor_grad, name)
    if name in ("FusedOptimStep", "OptimStepSpec"):
        from . import optim_step
        return getattr(optim_step, name)
    if name in ("FusedTD3ActorGrad", "TD3ActorGradSpec"):
        from . import td3_actor_grad
        return getattr(td3_actor_grad, name)
    if name in ("FusedPPOGrad", "PPOGradSpec"):
        from . import ppo_grad
        return getattr(ppo_grad, name)
    if name in ("DeviceRolloutBuffer", "RolloutBufferSamples"):
        from . import rollout_buffer
        return getattr(rollout_buffer, name)
    if name in ("FusedOnPolicyTrain", "OnPolicyTrainSpec", "TrainLogs"):
        from . import onpolicy_train
        return getattr(onpolicy_train, name)
    if name in ("FusedOffPolicyTrain", "OffPolicyTrainSpec", "OffPolicyTrainLogs"):
        from . import offpolicy_train
        return getattr(offpolicy_train, name)
    if name in ("FusedOffPolicyLearn", "OffPolicyLearnSpec", "OffPolicyLearnLogs", "EpisodeStats"):
        from . import offpolicy_learn
        return getattr(offpolicy_learn, name)
    if name in ("FusedOnPolicyLearn", "OnPolicyLearnSpec", "OnPolicyLearnLogs", "StepCounter"):
        from . import onpolicy_learn
        return getattr(onpolicy_learn, name)
    if name in ("FusedFNN", "FNNSpec", "FNNMeshResult"):
        from . import fnn
        return getattr(fnn, name)
    if name in ("FusedFNNTrain", "FNNTrainSpec", "FNNTrainLog"):
        from . import fnn_train
        return getattr(fnn_train, name)
    if name in ("DeviceMeshAugmentation", "AugmentScore"):
        from . import augmentation
        return getattr(augmentation, name)
    if name in ("FusedDDPGGrad", "DDPGGradSpec"):
        from . import ddpg_grad
        return getattr(ddpg_grad, name)
    if name == "DeviceEvalCallback":
        from .eval_callback import DeviceEvalCallback
        return DeviceEvalCallback
    raise AttributeError(name)
