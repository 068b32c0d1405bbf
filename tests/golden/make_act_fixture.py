"""Golden vectors for the rollout half of the action head (gmpe_act_sample), produced by RUNNING the reference on the CPU:

    python tests/golden/make_act_fixture.py        # writes tests/golden/act_head.npz

What runs (the reference's own code; imports and stubs as in make_ppo_loss_fixture.py): `ACTLayer.forward` (onpolicy/algorithms/utils/act.py:107-113)
of an `ACTLayer(Discrete(K), K, ...)` whose `Categorical` (distributions.py:84-91) has its linear layer set to the identity, so x is the logits; once
with deterministic=True (FixedCategorical.mode) and once sampled under torch.manual_seed. torch's sampler is not the project's: the sampled actions
are stored to be used as GIVEN actions, whose log-probs the reference computed. Inputs are the seeded families of tests/act_lib.py (stop rows and
single-action rows included); the vectors are data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_buffer_fixture as MB  # noqa: E402
import act_lib as AL  # noqa: E402

# name -> (K, family, avail)
CASES = {"a": (5, "unit", "mixed"), "b": (25, "wide", "mixed"), "c": (5, "wide", "none"), "d": (25, "unit", "none"), "e": (25, "unit", "mixed"),
         "f": (5, "wide", "mixed")}
ROWS, TORCH_SEED = 96, 1234


def main():
    MB.load_reference()
    import gym
    import torch
    from onpolicy.algorithms.utils.act import ACTLayer
    d = {}
    for name, (K, fam, kind) in CASES.items():
        logits, avail = AL.family(fam, ROWS, K, seed=200, avail=kind)
        act = ACTLayer(gym.spaces.Discrete(K), K, True, 0.01)
        with torch.no_grad():
            act.action_out.linear.weight.copy_(torch.eye(K))
            act.action_out.linear.bias.zero_()
            av = None if avail is None else torch.from_numpy(avail)
            mode, mode_lp = act.forward(torch.from_numpy(logits.copy()), av, deterministic=True)
            torch.manual_seed(TORCH_SEED)
            sampled, sampled_lp = act.forward(torch.from_numpy(logits.copy()), av, deterministic=False)
        d[name + "_K"] = K
        d[name + "_logits"] = logits
        d[name + "_has_avail"] = avail is not None
        d[name + "_avail"] = avail if avail is not None else np.ones((ROWS, K), np.float32)
        d[name + "_mode"] = mode.numpy().copy()
        d[name + "_mode_log_probs"] = mode_lp.numpy().copy()
        d[name + "_sampled"] = sampled.numpy().copy()
        d[name + "_sampled_log_probs"] = sampled_lp.numpy().copy()
    p = os.path.join(HERE, "act_head.npz")
    np.savez_compressed(p, **d)
    print(p, os.path.getsize(p), len(d))


if __name__ == "__main__":
    main()
