"""NumPy restatement of the learner's fields of GMPERunner.insert + GraphReplayBuffer.insert / after_update (graph_mpe_runner.py:384-392,
graph_buffer.py:229-234, 253-283): what gmpe_insert_learner and DeviceRolloutBuffer.after_update must reproduce. Pinned to the reference's own vectors
(tests/golden/learner_buffer_*.npz) by tests/test_learner_buffer_host.py."""
import numpy as np


def np_insert(inputs, T, N, A, R, H, Hc=None, k=1):
    """inputs: dict of [T, ...] arrays in_values [N, A, 1], in_actions int64 [N, A, k], in_action_log_probs, in_rnn_states [N, A, R, H],
    in_rnn_states_critic, in_dones bool [N, A]. Returns the five buffer arrays after T inserts from zero-initialised storage."""
    Hc = H if Hc is None else Hc
    f32 = np.float32
    out = dict(rnn_states=np.zeros((T + 1, N, A, R, H), f32), rnn_states_critic=np.zeros((T + 1, N, A, R, Hc), f32),
               actions=np.zeros((T, N, A, k), f32), action_log_probs=np.zeros((T, N, A, k), f32), value_preds=np.zeros((T + 1, N, A, 1), f32))
    for t in range(T):
        d = inputs["in_dones"][t].astype(bool)
        out["value_preds"][t] = inputs["in_values"][t]
        out["actions"][t] = inputs["in_actions"][t].astype(f32)
        out["action_log_probs"][t] = inputs["in_action_log_probs"][t]
        for name in ("rnn_states", "rnn_states_critic"):
            out[name][t + 1] = np.where(d[:, :, None, None], f32(0), inputs["in_" + name][t])
    return out


def np_after_update(bufs):
    """after_update: slot 0 of the [T+1] learner arrays takes the last slot; actions / log-probs have no slot T."""
    out = {k: v.copy() for k, v in bufs.items()}
    for name in ("rnn_states", "rnn_states_critic"):
        out[name][0] = out[name][-1]
    return out
