"""NumPy restatement of gmpe_episode_record_series (include/gmpe.h) and the inputs of its tests — test helper, not a conftest.

Written from the rules, as a plain loop over the envs: every env carries its own episode index, step count and running returns, and books R
episodes back to back. `Series(..., variant=...)` restates six cheap wrong readings of the rules; tests/test_eval_series_host.py shows that the
inputs below tell each of them from the truth.
"""
import numpy as np

VARIANTS = ["ret not cleared", "terminal reward to the next episode", "env-major rows", "any-done ends", "global time limit", "records past R"]


class Series(object):
    """Per-env record state of R back-to-back episodes, driven call by call."""

    def __init__(self, N, A, T, R, n_actions=25, width=18, variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.N, self.A, self.T, self.R, self.n_actions, self.variant = N, A, T, R, n_actions, variant
        self.episode = np.zeros(N, np.int32)
        self.t_in_ep = np.zeros(N, np.int32)
        self.ret = np.zeros((N, A), np.float64)
        self.steps = np.zeros((R, N), np.int32)
        self.ret_out = np.zeros((R, N, A), np.float64)
        self.final_info = np.zeros((R, N, A, width), np.float32)
        self.calls = 0

    def _row(self, e, n):
        """Flat episode row of (episode e, env n): e * N + n."""
        if self.variant == "env-major rows":
            return n * self.R + e
        return (e % self.R) * self.N + n           # e < R always, except in the variant that records past R (it wraps)

    def step(self, reward, done, info):
        """reward f32 [N, A], done bool [N, A], info f32 [N, A, W]; returns (masks [N, A, 1], available_actions [N, A, n_actions])."""
        N, A, T, R, v = self.N, self.A, self.T, self.R, self.variant
        done = np.asarray(done, bool)
        self.calls += 1
        steps, ret_out, final = self.steps.reshape(-1), self.ret_out.reshape(R * N, A), self.final_info.reshape(R * N, A, -1)
        for n in range(N):
            e = int(self.episode[n])
            if e >= R and v != "records past R":
                continue
            r = np.asarray(reward[n]).astype(np.float64)
            late = v == "terminal reward to the next episode"
            if not late:
                self.ret[n] = self.ret[n] + r
            self.t_in_ep[n] += 1
            limit = self.calls % T == 0 if v == "global time limit" else self.t_in_ep[n] == T
            over = done[n].any() if v == "any-done ends" else done[n].all()
            if over or limit:
                row = self._row(e, n)
                steps[row] = self.t_in_ep[n]
                ret_out[row] = self.ret[n]
                final[row] = info[n]
                self.episode[n] = e + 1
                self.t_in_ep[n] = 0
                if v != "ret not cleared":
                    self.ret[n] = 0.0
            if late:
                self.ret[n] = self.ret[n] + r
        masks = np.ones((N, A, 1), np.float32)
        all_done = done.all(axis=1)
        masks[done] = 0.0
        masks[all_done] = 1.0
        avail = np.ones((N, A, self.n_actions), np.float32)
        stop = np.zeros(self.n_actions, np.float32)
        stop[self.n_actions // 2] = 1.0
        avail[masks[..., 0] == 0] = stop
        return masks, avail

    def finished(self):
        return bool((self.episode >= self.R).all())

    def arrays(self):
        """The compared arrays: states and outputs (final_info as bits)."""
        return dict(episode=self.episode.copy(), t_in_ep=self.t_in_ep.copy(), ret=self.ret.copy(), steps=self.steps.copy(),
                    ret_out=self.ret_out.copy(), final_info=self.final_info.view(np.int32).copy())


def replay(rew, done, info, T, R, n_actions=25, variant=None):
    """Every call of a recorded sequence through Series; returns (the Series, [arrays() after each call])."""
    S, N, A = rew.shape
    rec = Series(N, A, T, R, n_actions=n_actions, width=info.shape[-1], variant=variant)
    trace = []
    for s in range(S):
        rec.step(rew[s], done[s], info[s])
        trace.append(rec.arrays())
    return rec, trace


ENV_PATTERNS = ["first step", "time limit only", "drawn lengths", "short then long", "drawn lengths"]


def series_inputs(N, A, T, R, seed):
    """(reward f32 [S, N, A], done bool [S, N, A], info f32 [S, N, A, 18]) for S = R * T calls. Env i follows ENV_PATTERNS[(i + seed) % 5]:

    first step: all agents done at every call, so each of its episodes ends at its first step and the env is frozen after R calls;
    time limit only: some agents done at random, never all: every episode runs T steps, the env finishes at call R * T;
    drawn lengths: per episode a length L uniform in 1 .. T + 2: all agents done at the episode's L-th step when L <= T, else never;
    short then long: its first episode ends by all-done at step max(T // 2, 1), the later ones run to the time limit (so its time limits do
      not fall on multiples of T calls when T > 1).
    Between ends a random subset of the agents, never all of them, is done. Once an env has played R episodes its rows stay random, all-done
    rows among them: a record that does not freeze it shows. info holds NaNs (two payloads) and -0.0 among random values."""
    rng = np.random.RandomState(seed)
    S = R * T
    rew = (rng.randn(S, N, A) * 3).astype(np.float32)
    done = np.zeros((S, N, A), bool)
    for i in range(N):
        pat = ENV_PATTERNS[(i + seed) % 5]
        t, ep, L = 0, 0, None
        for s in range(S):
            if ep >= R:                                            # frozen: anything goes
                done[s, i] = rng.rand(A) < 0.5
                if rng.rand() < 0.3:
                    done[s, i] = True
                continue
            if t == 0:
                L = {"first step": 1, "time limit only": T + 1, "drawn lengths": rng.randint(1, T + 3),
                     "short then long": max(T // 2, 1) if ep == 0 else T + 1}[pat]
            t += 1
            if t == L:
                done[s, i] = True
            else:
                d = rng.rand(A) < 0.4
                d[rng.randint(A)] = False
                done[s, i] = d
            if t == L or t == T:
                t, ep = 0, ep + 1
    info = (rng.rand(S, N, A, 18) * 4 - 1).astype(np.float32)
    r = rng.rand(S, N, A, 18)
    iv = info.view(np.int32)
    iv[r < 0.05] = 0x7fc00000
    iv[(r >= 0.05) & (r < 0.1)] = np.int32(-4079307)          # 0xffc1c0f5: a NaN with the sign bit and a payload
    iv[(r >= 0.1) & (r < 0.15)] = np.int32(-2 ** 31)          # -0.0
    return rew, done, info


SERIES_SHAPES = [(1, 1), (15, 64), (16, 64), (17, 64), (33, 5), (1000, 3), (4099, 10)]
SERIES_EPISODES = [1, 2, 3, 7]
SERIES_STEPS = [1, 2, 25]
SERIES_ACTIONS = [1, 2, 24, 25]
SERIES_RNN_ROWS = [None, 1, 7, 64, 1025]


def series_cases():
    """[(N, A, R, T, n_actions, rnn_row)]: every shape with every R and every T; the action count and the RNN row width rotate so that each
    of them meets each shape, each R and each T."""
    out = []
    for i, (N, A) in enumerate(SERIES_SHAPES):
        for j, R in enumerate(SERIES_EPISODES):
            for k, T in enumerate(SERIES_STEPS):
                out.append((N, A, R, T, SERIES_ACTIONS[(i + j + k) % 4], SERIES_RNN_ROWS[(i + 2 * j + k) % 5]))
    return out


# --- the engine-driven scenarios: a deterministic goal seeker in three of every four envs, the stop action in the fourth

ENGINE_SCENARIOS = {
    "tube_july": dict(scenario_name="nav_metered_one_goal_graph_rotate_tube_july", num_agents=3, world_size=2.0, episode_length=40, seed=7),
    "navigation_graph": dict(scenario_name="navigation_graph", num_agents=3, num_obstacles=3, world_size=4.0, episode_length=40, seed=7),
}
ENGINE_ENVS, ENGINE_EPISODES = 32, 3


def seek_actions(obs, n_actions, env0=0):
    """int32 [N, A] actions from the observations [N, A, D] (columns 2:4 the velocity, 4:6 the goal's relative position): head for the goal.
    Force dynamics (5 actions): push along the axis with the larger goal offset. Kinematic (25 = 5 turn rates x 5 accelerations): full turn
    towards the goal's bearing beyond 0.2 rad, full acceleration. Every fourth env (by global index env0 + n) takes the no-op / stop action."""
    obs = np.asarray(obs, np.float64)
    gx, gy, vx, vy = obs[..., 4], obs[..., 5], obs[..., 2], obs[..., 3]
    if n_actions == 5:
        a = np.where(np.abs(gx) >= np.abs(gy), np.where(gx > 0, 1, 2), np.where(gy > 0, 3, 4))
        idle = 0
    else:
        err = np.arctan2(gy, gx) - np.arctan2(vy, vx)
        err = (err + np.pi) % (2 * np.pi) - np.pi
        a = np.where(np.abs(err) < 0.2, 2, np.where(err > 0, 4, 0)) * 5 + 4
        idle = n_actions // 2
    a = a.astype(np.int32)
    a[(env0 + np.arange(obs.shape[0])) % 4 == 3] = idle
    return a


def end_shares(steps, T):
    """(share of episodes that end before T, share that end at T) of recorded episode lengths."""
    s = np.asarray(steps).reshape(-1)
    return float((s < T).mean()), float((s == T).mean())
