"""NumPy restatement of what follows the env step of a rollout step (include/gmpe.h gmpe_step_tail): GraphReplayBuffer.insert's mask rules
(graph_buffer.py:223-251, graph_mpe_runner.py:395-405), collect_with_mask's stop rows (graph_mpe_runner.py:263-335), GMPERunner.insert's learner fields
(graph_mpe_runner.py:384-392, graph_buffer.py:229-234) and the draw counter. Pinned to hand-written dones by tests/test_step_tail_host.py; the GPU
tests (tests/test_gpu_step_tail.py) compare the C entry with it bit for bit.
Arrays are kept as the kernel sees them: 2-D [slots, stride] float32 (dones: uint8), a slot's rows in the first `slot` elements of its line, so that
the padding between slots is part of every comparison."""
import numpy as np

F32 = np.float32
SENTINEL = F32(-77.25)


def np_masks(done, A):
    """done: [lanes] of any integer / bool type, != 0 is done; lanes of an env are consecutive -> (masks, active_masks), float32 [lanes]"""
    d = np.asarray(done).reshape(-1) != 0
    whole = np.repeat(d.reshape(-1, A).all(axis=1), A)
    return np.where(d, F32(0), F32(1)), np.where(d & ~whole, F32(0), F32(1))


def np_stop_rows(done_prev, lanes, n):
    """done_prev: the dones of the step before, or None at step 0 -> float32 [lanes, n]: one-hot at n // 2 for a lane that was done, ones otherwise"""
    out = np.ones((lanes, n), F32)
    if done_prev is not None:
        d = np.asarray(done_prev).reshape(-1) != 0
        out[d] = 0
        out[d, n // 2] = 1
    return out


def np_step_tail(t, dones, A, bufs, inputs, n=0, counter=None, draw_inc=0):
    """One gmpe_step_tail on NumPy arrays, in place.
    dones uint8 [T, stride_d]; bufs: name -> [slots, stride] float32 or absent, of masks, active_masks, available_actions (the WHOLE [T + 1] array:
    position t is slot t + 1), value_preds, actions, action_log_probs, rnn_states, rnn_states_critic; inputs: name -> the policy's outputs of this step
    with `lanes` rows (values, actions int64 / float32, action_log_probs, rnn_states, rnn_states_critic), absent = skipped.
    counter: None or a one-element uint64 array. lanes = len of an input, or of dones' slot."""
    lanes = inputs["_lanes"]
    d = dones[t, :lanes]
    done = d != 0
    m, a = np_masks(d, A)
    if bufs.get("masks") is not None:
        bufs["masks"][t + 1, :lanes] = m
    if bufs.get("active_masks") is not None:
        bufs["active_masks"][t + 1, :lanes] = a
    if bufs.get("available_actions") is not None:
        bufs["available_actions"][t + 1, :lanes * n] = np_stop_rows(dones[t - 1, :lanes] if t else None, lanes, n).reshape(-1)
    for name, dst, slot in (("values", "value_preds", t), ("actions", "actions", t), ("action_log_probs", "action_log_probs", t),
                            ("rnn_states", "rnn_states", t + 1), ("rnn_states_critic", "rnn_states_critic", t + 1)):
        x = inputs.get(name)
        if x is None:
            continue
        x = np.asarray(x).reshape(lanes, -1)
        if name.startswith("rnn"):
            x = np.where(done[:, None], F32(0), x.astype(F32))
        bufs[dst][slot, :x.size] = x.astype(F32).reshape(-1)            # int64 actions: NumPy's cast, as GraphReplayBuffer stores them
    if counter is not None:
        counter[0] += np.uint64(draw_inc)
