"""Float32 NumPy restatement of GraphReplayBuffer.compute_returns (onpolicy/utils/graph_buffer.py:285-366), GR_MAPPO.train's advantage lines
(onpolicy/algorithms/graph_mappo.py:294-304) and the runner's stop-action rule (graph_mpe_runner.py:73-141, 263-335), used by the tests to check
the device kernels at shapes the golden fixtures do not cover. It is pinned to the reference itself by tests/test_returns_host.py, which compares it
bit for bit with tests/golden/returns_advantages.npz and available_actions.npz (both made by running the reference)."""
import numpy as np


def np_returns(rewards, masks, value_preds, returns, next_value, gamma, gae_lambda, use_gae, use_proper_time_limits, bad_masks=None, denorm=None):
    """-> (returns, value_preds) after compute_returns. The expressions keep the reference's operand order: a Python float meets a float32 array as
    float32(value), and gamma * gae_lambda is a double product rounded once. denorm: (mean, std) float32 scalars: x * std + mean, two roundings."""
    f32 = np.float32
    vp, ret = value_preds.astype(f32, copy=True), returns.astype(f32, copy=True)
    nv = next_value.astype(f32).reshape(vp.shape[1:])
    g, gl = f32(gamma), f32(gamma * gae_lambda)
    dn = (lambda x: x * f32(denorm[1]) + f32(denorm[0])) if denorm is not None else (lambda x: x)
    T = rewards.shape[0]
    if use_gae:
        vp[-1] = nv
        gae = np.zeros_like(nv)
        for s in reversed(range(T)):
            delta = rewards[s] + g * dn(vp[s + 1]) * masks[s + 1] - dn(vp[s])
            gae = delta + (gl * gae * masks[s + 1] if (use_proper_time_limits and denorm is not None) else gl * masks[s + 1] * gae)
            if use_proper_time_limits:
                gae = gae * bad_masks[s + 1]
            ret[s] = gae + dn(vp[s])
    else:
        ret[-1] = nv
        for s in reversed(range(T)):
            if use_proper_time_limits:
                ret[s] = (ret[s + 1] * g * masks[s + 1] + rewards[s]) * bad_masks[s + 1] + (f32(1) - bad_masks[s + 1]) * dn(vp[s])
            else:
                ret[s] = ret[s + 1] * g * masks[s + 1] + rewards[s]
    return ret, vp


def np_advantages(returns, value_preds, denorm=None):
    f32 = np.float32
    dv = value_preds[:-1] * f32(denorm[1]) + f32(denorm[0]) if denorm is not None else value_preds[:-1]
    return returns[:-1] - dv


def np_normalized(adv, active_masks):
    """(adv - mean) / (std + 1e-5) over the entries with active_masks != 0 (and not NaN), population std; statistics in double, as the kernels."""
    a = adv.astype(np.float64)
    keep = (active_masks[:-1] != 0) & ~np.isnan(a)
    if not keep.any():
        return np.full_like(adv, np.nan)
    m = a[keep].mean()
    sd = np.sqrt(((a[keep] - m) ** 2).mean())
    return (adv - np.float32(m)) / (np.float32(sd) + np.float32(1e-5))


def np_available_actions(dones, n_actions):
    """[T, ...lanes] dones -> [T, ...lanes, n_actions]: position t = ones at t = 0, else the stop row (one-hot at n_actions // 2) where dones[t - 1]."""
    out = np.ones(dones.shape + (n_actions,), np.float32)
    for t in range(1, dones.shape[0]):
        d = dones[t - 1].astype(bool)
        out[t][d] = 0.0
        out[t][d, n_actions // 2] = 1.0
    return out
