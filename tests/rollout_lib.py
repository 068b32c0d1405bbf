"""What the generator and the test of the policy-in-the-loop rollout share (tests/golden/make_rollout_fixture.py, tests/test_gpu_rollout_policy.py): the
engine config whose shapes the prescribed env outputs take, the cases, the names of the stored arrays, mirror modules that load the reference's state_dict
strictly at that config's observation size, and the fixture loader. The rule is tests/trainer_lib.py's: err(a, t) = max|a - t| / max|t| per array,
err_dev <= 4 * err_ref + 2^-23 with err_ref <= 1e-5 from the reference's own float32 run."""
import functools
import json
import os

import numpy as np
import torch

import gmpe
import gnn_lib as G
import trainer_lib as TL
from optim_lib import CAP, bound, err  # noqa: F401  (the rule, shared)
from test_gpu_policy import _Net

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, A, T = 2, 3, 6
SCENARIO = "nav_graph_metered_single_corridor_rot_inv"      # a 7-feature scenario: the shipped actor and critic GNNBase read F = 7
CASES = ("valuenorm", "popart")
EXACT = ("actions", "available_actions", "masks", "active_masks")
CLOSE = ("values", "action_log_probs", "rnn_states", "rnn_states_critic", "value_preds", "returns")
ENV = ("obs", "agent_id", "node_obs", "adj", "rewards", "dones")        # [T + 1, ...] for the first four (slot 0: the reset), [T, ...] for the last two
RETURNS_ARGS = dict(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False)


def config():
    """the engine config the shapes are taken from (no device is touched)"""
    return gmpe.make_config(scenario_name=SCENARIO, num_envs=N, num_agents=A, episode_length=25, seed=5)


def shapes():
    c = config()
    assert int(c.node_feats) == 7
    return dict(D=int(c.obs_dim), E=int(c.num_entities), K=int(c.n_actions), F=7)


class Net(_Net):
    """tests/trainer_lib.py's Net at another observation size: _Net with the reference's fc_h and its two recurrence flags; head 'act', 'v_out' or
    'popart'. The weights come from load_state_dict."""

    def __init__(self, head, obs_dim):
        super().__init__(G.ACTOR if head == "act" else G.CRITIC, obs_dim, "v_out" if head == "popart" else head)
        nn = torch.nn
        self.base.mlp.fc_h = nn.Sequential(nn.Linear(64, 64), nn.ReLU(), nn.LayerNorm(64))
        self._use_recurrent_policy, self._use_naive_recurrent_policy = True, False
        if head == "popart":
            self.v_out = PopArt()


class PopArt(TL.PopArt):
    def debiased_mean_var(self):                            # popart.py:85-89
        mean = self.mean / self.debiasing_term.clamp(min=self.epsilon)
        var = (self.mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)
        return mean, var


class ValueNorm(TL.ValueNorm):
    def running_mean_var(self):                             # valuenorm.py:48-55
        mean = self.running_mean / self.debiasing_term.clamp(min=self.epsilon)
        var = (self.running_mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)
        return mean, var


@functools.lru_cache(maxsize=None)
def load(case):
    """{'env': {name: array}, 'init': {network: state_dict}, 'norm': the normaliser's statistics, 'truth': {name: float64 or exact array},
    'err_ref': {name: float}, 'args': dict}"""
    with np.load(os.path.join(GOLDEN, "rollout_%s.npz" % case)) as d:
        raw = {k: d[k] for k in d.files}
    fx = dict(env={}, init={}, norm={}, truth={}, err_ref={}, args=json.loads(str(raw["args"])))
    for k, v in raw.items():
        parts = k.split(":")
        if parts[0] == "init":
            fx["init"].setdefault(parts[1], {})[parts[2]] = v
        elif parts[0] in ("env", "norm", "truth"):
            fx[parts[0]][parts[1]] = v
        elif parts[0] == "err_ref":
            fx["err_ref"][parts[1]] = float(v)
    return fx


def nets(fx, case, device):
    """(actor, critic, value normaliser) from the fixture's initial state, loaded strictly, on `device` in float32"""
    D = fx["env"]["obs"].shape[-1]
    actor, critic = Net("act", D), Net("popart" if case == "popart" else "v_out", D)
    actor.load_state_dict({k: torch.from_numpy(v) for k, v in fx["init"]["actor"].items()}, strict=True)
    critic.load_state_dict({k: torch.from_numpy(v) for k, v in fx["init"]["critic"].items()}, strict=True)
    actor, critic = actor.to(device), critic.to(device)
    if case == "popart":
        vn = critic.v_out
    else:
        vn = ValueNorm(device)
        for k, v in fx["norm"].items():
            getattr(vn, k).copy_(torch.from_numpy(v).reshape(getattr(vn, k).shape))
    return actor, critic, vn
