"""gmpe — MI355X-native batched GraphMPE step engine (package dir: contracts-marl-aam-corridors_amd/).

Host side is Python (the reference is Python): `vec_env.BatchedGraphMPEVecEnv` keeps the surface of
`GraphSubprocVecEnv` (onpolicy/envs/env_wrappers.py:959-1037) and drives hand-written HIP kernels
for gfx950 through the C ABI of include/gmpe.h (ctypes). There is no CPU fallback: without the
built libgmpe.so the engine raises.
"""
from . import config  # noqa: F401
from .config import make_config, config_from_args  # noqa: F401

__all__ = ["config", "make_config", "config_from_args"]


def __getattr__(name):
    # torch / HIP-dependent modules are imported on first use
    if name in ("engine", "vec_env", "spaces", "_lib", "sharding", "rollout", "minibatch", "evaluate", "ppo_loss", "act", "learner_shards", "gru", "mlp", "gnn", "head", "value", "policy", "optim", "infos"):
        import importlib
        return importlib.import_module("." + name, __name__)
    if name in ("BatchedGraphMPEVecEnv", "MultiDeviceGraphMPEVecEnv", "GraphMPEEnv", "make_train_env", "make_eval_env"):
        from . import vec_env
        return getattr(vec_env, name)
    if name == "BatchedEvaluator":
        from . import evaluate
        return evaluate.BatchedEvaluator
    if name in ("ppo_losses", "PPOLosses", "ppo_losses_popart", "PPOPopArtLosses", "ppo_losses_begin", "ppo_losses_finish"):
        from . import ppo_loss
        return getattr(ppo_loss, name)
    if name == "sample_actions":
        from . import act
        return act.sample_actions
    if name in ("rnn_layer", "rnn_workspace_bytes"):
        from . import gru
        return getattr(gru, name)
    if name in ("mlp_base", "mlp_workspace_bytes"):
        from . import mlp
        return getattr(mlp, name)
    if name in ("gnn_base", "gnn_base_from_table", "gnn_workspace_bytes", "gnn_base_wide", "gnn_base_wide_from_table"):
        from . import gnn
        return getattr(gnn, name)
    if name in ("action_logits", "act_head", "head_workspace_bytes"):
        from . import head
        return getattr(head, name)
    if name in ("value_head", "value_workspace_bytes"):
        from . import value
        return getattr(value, name)
    if name in ("clip_and_step", "clip_and_step_begin", "clip_and_step_finish"):
        from . import optim
        return getattr(optim, name)
    if name in ("env_infos", "eval_step", "eval_mean"):
        from . import infos
        return getattr(infos, name)
    if name in ("GmpeEngine", "compute_returns_begin", "compute_returns_finish"):
        from . import engine
        return getattr(engine, name)
    if name == "ProcessGroupExchange":
        from . import learner_shards
        return learner_shards.ProcessGroupExchange
    raise AttributeError(name)
