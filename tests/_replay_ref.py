"""numpy restatement of csrc/tma_replay.hip (include/tma.h, ABI 224) for tests/test_replay_buffer_cpu.py and tests/test_replay_buffer_gpu.py:
the index draw, the n-step window (a plain Python loop per sample), the epsilon-greedy pick and the ring write.  Importable without a GPU."""
import numpy as np

ENV_KEY = 0x5EEDBA5E     # tma_replay_sample: the env draw hashes seed ^ this
PICK_KEY = 0xE9517EED    # tma_egreedy_actions: the random action hashes rng_seed ^ this


def mix32(seed, i, t):
    """csrc/tma_common.h mix32, as tools/gen_golden.py states it: all arithmetic mod 2**32 (vectorised over i)"""
    with np.errstate(over="ignore"):
        x = (np.uint32(seed) * np.uint32(0x9E3779B1)) ^ (np.asarray(i, np.uint32) * np.uint32(0x85EBCA77)) ^ (np.uint32(t) * np.uint32(0xC2B2AE3D))
        x = np.asarray(x, np.uint32)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
    return x


def draw_indices(seed, draw, count, size, n_envs):
    """(t, i) int32 [count]: t = (uint64(mix32(seed, b, draw)) * size) >> 32, i = mix32(seed ^ ENV_KEY, b, draw) % n_envs"""
    b = np.arange(count, dtype=np.uint32)
    t = (mix32(seed, b, draw).astype(np.uint64) * np.uint64(size)) >> np.uint64(32)
    i = mix32((seed ^ ENV_KEY) & 0xFFFFFFFF, b, draw) % np.uint32(n_envs)
    return t.astype(np.int32), i.astype(np.int32)


def window(rewards, terminated, truncated, t, i, newest, n_step, gamma):
    """The n-step window that starts at row t of env i.  rewards f32 / flags u8 [R, N].  Returns (last row, reward f32, done f32,
    discount f32, steps included, why it ended: 'n' | 'done' | 'timeout' | 'head')."""
    R = rewards.shape[0]
    row, acc, g, steps = int(t), 0.0, 1.0, 0
    while True:
        r = float(rewards[row, i])
        acc = r if steps == 0 else acc + g * r  # float64, in k order
        g = g * float(gamma)                    # gamma ** (steps included), by repeated multiplication
        steps += 1
        if terminated[row, i]:
            why = "done"
        elif truncated[row, i]:
            why = "timeout"
        elif row == newest:
            why = "head"
        elif steps == n_step:
            why = "n"
        else:
            row = (row + 1) % R
            continue
        return row, np.float32(acc), np.float32(1.0 if terminated[row, i] else 0.0), np.float32(g), steps, why


def sample(planes, size, newest, n_step, gamma, seed, draw, count):
    """planes: dict of obs / next_obs [R, N, D], actions [R, N] | [R, N, A], rewards, terminated, truncated [R, N] (numpy).  Returns a dict
    of the eight outputs of tma_replay_sample plus 'why', the list of the reasons the windows ended."""
    N = planes["rewards"].shape[1]
    t, i = draw_indices(seed, draw, count, size, N)
    out = {"rows": t, "envs": i, "obs": planes["obs"][t, i], "actions": planes["actions"][t, i]}
    last, rew, done, disc, why = [], [], [], [], []
    for tb, ib in zip(t, i):
        row, r, d, g, _, w = window(planes["rewards"], planes["terminated"], planes["truncated"], tb, ib, newest, n_step, gamma)
        last.append(row), rew.append(r), done.append(d), disc.append(g), why.append(w)
    out["next_obs"] = planes["next_obs"][np.asarray(last), i]
    out["rewards"], out["dones"], out["discounts"] = np.asarray(rew, np.float32), np.asarray(done, np.float32), np.asarray(disc, np.float32)
    out["why"] = why
    return out


def egreedy(q, eps, rng_seed, rng_step, env_offset=0):
    """tma_egreedy_actions on q f32 [n, A]: int32 [n]"""
    n, A = q.shape
    env = (np.arange(n, dtype=np.uint64) + np.uint64(env_offset)).astype(np.uint32)
    u = (mix32(rng_seed, env, rng_step) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    pick = (mix32((rng_seed ^ PICK_KEY) & 0xFFFFFFFF, env, rng_step) % np.uint32(A)).astype(np.int32)
    greedy = np.zeros(n, np.int32)
    for r in range(n):  # the first maximal column; a NaN never wins, a row of NaNs gives 0
        a, m = 0, q[r, 0]
        for c in range(1, A):
            v = q[r, c]
            if v > m or (np.isnan(m) and not np.isnan(v)):
                a, m = c, v
        greedy[r] = a
    return np.where(u < np.float32(eps), pick, greedy).astype(np.int32)


class Ring:
    """tma_replay_add replayed in numpy: the planes, last_obs, pos and full after every add"""

    def __init__(self, R, N, D, A, continuous):
        self.obs, self.next_obs = np.zeros((R, N, D), np.float32), np.zeros((R, N, D), np.float32)
        self.actions = np.zeros((R, N, A), np.float32) if continuous else np.zeros((R, N), np.int32)
        self.rewards = np.zeros((R, N), np.float32)
        self.terminated, self.truncated = np.zeros((R, N), np.uint8), np.zeros((R, N), np.uint8)
        self.last_obs = np.zeros((N, D), np.float32)
        self.R, self.pos, self.full = R, 0, False

    def add(self, actions, step_obs, rewards, term, trunc, term_obs):
        p = self.pos
        ended = ((term | trunc) != 0)[:, None]
        self.obs[p] = self.last_obs
        self.next_obs[p] = np.where(ended, term_obs, step_obs)
        self.actions[p], self.rewards[p], self.terminated[p], self.truncated[p] = actions, rewards, term, trunc
        self.last_obs = step_obs.copy()
        self.pos = (p + 1) % self.R
        self.full = self.full or self.pos == 0

    def planes(self):
        return {k: getattr(self, k) for k in ("obs", "next_obs", "actions", "rewards", "terminated", "truncated")}
