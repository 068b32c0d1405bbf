"""NumPy restatements for gmpe.infos / gmpe_infos.hip, and the fixture they are held to (tests/golden/run_log.npz, made by the reference's own
process_infos, log_env and eval: tests/golden/make_run_log_fixture.py).

np_mean restates the order in which float64 NumPy sums a contiguous list, add by add in Python floats: consecutive chunks of CHUNK values (the reduce
buffer), each by pairwise_sum (fewer than 8 values sequentially from -0.0; up to LEAF values by eight accumulators, their tree, then the tail; more
split at n2 = n/2 - (n/2) % 8), the chunk sums added in order to +0.0, then one division. tests/test_infos_host.py holds it to np.mean itself.
"""
import collections
import os

import numpy as np

CHUNK, LEAF = 8192, 128
INFO_KEYS = ["individual_reward", "Dist_to_goal", "Time_req_to_goal", "Num_agent_collisions", "Num_obst_collisions", "Distance_mean",
             "Distance_variance", "Mean_by_variance", "Dists_traveled", "Time_taken", "Time_mean", "Time_stddev", "Time_mean_by_stddev",
             "Conformance", "Delta_spacing", "Spacing_violations", "Min_time_to_goal", "Phase_reached"]
# process_infos' dict order (base_runner.py:271-288) -> the info key each list is filled from; formation_dist is filled from a key no scenario writes
NAMES = [("individual_rewards", "individual_reward"), ("time_to_goal", "Time_req_to_goal"), ("min_time_to_goal", "Min_time_to_goal"),
         ("dist_to_goal", "Dist_to_goal"), ("num_agent_collisions", "Num_agent_collisions"), ("num_obstacle_collisions", "Num_obst_collisions"),
         ("distance_mean", "Distance_mean"), ("distance_variance", "Distance_variance"), ("mean_variance", "Mean_by_variance"),
         ("dists_traveled", "Dists_traveled"), ("time_taken", "Time_taken"), ("formation_dist", "Formation_dist"), ("time_mean", "Time_mean"),
         ("time_variance", "Time_stddev"), ("time_mn_by_stddev", "Time_mean_by_stddev"), ("conformance_percentages", "Conformance"),
         ("delta_space", "Delta_spacing"), ("spacing_violations", "Spacing_violations")]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_log.npz")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def _leaf(x):
    n = len(x)
    if n < 8:
        r = -0.0
        for v in x:
            r = r + v
        return r
    r = [x[j] for j in range(8)]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] = r[j] + x[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + x[i]
        i += 1
    return res


def pairwise(x):
    """NumPy's pairwise_sum over a list of Python floats"""
    n = len(x)
    if n <= LEAF:
        return _leaf(x)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(x[:n2]) + pairwise(x[n2:])


def np_sum(values, chunk=CHUNK):
    """np.add.reduce of a contiguous 1-D float64 array; chunk=None: plain recursion over the whole array (the mutant: not NumPy's order past CHUNK)"""
    x = [float(v) for v in np.asarray(values, dtype=np.float64).ravel()]
    if chunk is None:
        return 0.0 + pairwise(x)
    acc = 0.0
    for s in range(0, len(x), chunk):
        acc = acc + pairwise(x[s:s + chunk])
    return acc


def np_mean(values, chunk=CHUNK):
    return np.float64(np_sum(values, chunk)) / np.float64(np.asarray(values).size)


def np_mean_columns(x):
    """np_mean of every column of a float64 [N, C] array at once: the same adds in the same order, each one elementwise over the C columns"""
    x = np.asarray(x, dtype=np.float64)
    acc = np.zeros(x.shape[1], dtype=np.float64)
    for s in range(0, x.shape[0], CHUNK):
        acc = acc + pairwise(x[s:s + CHUNK])
    return acc / np.float64(x.shape[0])


def leaves(m):
    """[(offset, size)] of pairwise_sum's leaves over m values, in order, and the depth of its recursion"""
    out, depth = [], [0]

    def go(off, n, d):
        depth[0] = max(depth[0], d)
        if n <= LEAF:
            out.append((off, n))
            return
        n2 = n // 2
        n2 -= n2 % 8
        go(off, n2, d + 1)
        go(off + n2, n - n2, d + 1)
    go(0, m, 1)
    return out, depth[0]


def env_infos(info, episode_length, dt, include_min_time=True):
    """process_infos + log_env on float32 info rows [N, A, 18]: ordered dict 'agent{a}/<name>' -> np.float64, the keys whose list is non-empty"""
    info = np.asarray(info, dtype=np.float32)
    N, A, _ = info.shape
    means = info_means(info, episode_length, dt)
    out = collections.OrderedDict()
    for a in range(A):
        for name, key in NAMES:
            if key not in INFO_KEYS or (key == "Min_time_to_goal" and not include_min_time):
                continue
            out["agent%d/%s" % (a, name)] = means[a, INFO_KEYS.index(key)]
    return out


def info_means(info, episode_length, dt):
    """float64 [A, 18]: the mean over envs of every info column as np.mean gives it for the list of Python floats, -1 times replaced first"""
    x = np.asarray(info, dtype=np.float32).astype(np.float64)
    N, A, K = x.shape
    ttg = x[:, :, INFO_KEYS.index("Time_req_to_goal")]
    ttg[ttg == -1.0] = np.float64(episode_length) * np.float64(dt)         # a view: written into x
    return np_mean_columns(x.reshape(N, A * K)).reshape(A, K)


def eval_episode(rewards, dones, rnn_shape=None):
    """GMPERunner.eval's bookkeeping on rewards [T, N, A] and dones [T, N, A]: (sums [N, A] float64, their mean, the masks [T, N, A, 1] after each step,
    per step the envs whose RNN rows are zeroed [T, N] bool)"""
    rewards, dones = np.asarray(rewards), np.asarray(dones, dtype=bool)
    T, N, A = rewards.shape
    sums = np.zeros((N, A), dtype=np.float64)
    masks, zeroed = [], []
    for t in range(T):
        sums = sums + rewards[t].astype(np.float64)
        all_done = dones[t].all(axis=1)
        m = np.ones((N, A, 1), dtype=np.float32)
        m[all_done] = 0.0
        masks.append(m)
        zeroed.append(all_done)
    return sums, np_mean(sums), np.array(masks), np.array(zeroed)


def load():
    return np.load(FIXTURE, allow_pickle=False)
