"""Action scripts that end Crawler / Ant episodes by `unhealthy` (z < 0.38, |pitch| > 1, |roll| > 1; oracle/tma_oracle.c chain_step), found on
the CPU with the oracle alone.  N(0, 1) actions never do: 64 envs x 1040 steps end 0 episodes that way.  Only the parameters are committed;
the oracle regenerates actions and states at test time.

A script is (pattern, amplitude, steps): the same constant action row for every env and step,
  const  +a on every joint: the joints run into their +1.2 stop, mean cos(q) falls, z = 0.25 + k * sum cos(q) drops under 0.38;
  alt    +a / -a on even / odd joints: sum side * sin(q) drives the pitch past 1 on its first overshoot while |q| stays under the z limit.
Reached: Crawler z (step 13 of every env) and pitch (step 28); Ant z (step 13).  NOT reached by any script tried -- const / alt / half-and-half
patterns, amplitudes 0.3 .. 1.0, constant or sign-flipping every 10 .. 32 steps, 120 steps: Ant's pitch (8 joints give 0.3 * asym <= 2.2, a
static pitch of 0.36, and resonance does not triple it) and the roll of both (driven by 0.05 * thrust_y only).  Those two comparisons are reached
by `attitude_states` instead: oracle states with the root's pitch / roll overwritten on both sides of 1."""
import numpy as np

from oracle import oracle as orc

SCRIPTS = {
    ("crawler", "z"): ("const", 1.0, 13),
    ("crawler", "pitch"): ("alt", 0.7, 28),
    ("ant", "z"): ("const", 1.0, 13),
}


def action_row(task, pattern, amp):
    nj = orc.act_dim(task)
    j = np.arange(nj)
    row = {"const": np.ones(nj), "alt": np.where(j & 1, -1.0, 1.0)}[pattern]
    return (amp * row).astype(np.float32)


def script_actions(task, which, n, extra=2):
    pattern, amp, steps = SCRIPTS[(task, which)]
    return np.broadcast_to(action_row(task, pattern, amp), (steps + extra, n, orc.act_dim(task))).copy()


def why_unhealthy(task, pre_state, action):
    """Which of the three conditions the oracle's step from `pre_state` meets: a set out of {"z", "pitch", "roll"}."""
    nj = orc.act_dim(task)
    st, _, _, _ = orc.legacy_step(task, pre_state, action)
    z, pitch, roll = (np.float32(st[3 * nj + k]) for k in (0, 3, 4))
    return {n for n, hit in (("z", z < np.float32(0.38)), ("pitch", abs(pitch) > 1), ("roll", abs(roll) > 1)) if hit}


def pre_unhealthy_states(task, which, n, seed, leads):
    """Env i's state `leads[i % len(leads)]` steps before the script ends its episode (every env ends on the script's last step)."""
    pattern, amp, steps = SCRIPTS[(task, which)]
    env = orc.OracleVecEnv(task, n, seed=seed)
    env.reset()
    act = np.broadcast_to(action_row(task, pattern, amp), (n, orc.act_dim(task))).copy()
    snaps = []
    for t in range(steps):
        snaps.append(env.get_state())
        o = env.step(act)
        assert bool(o["term"].all()) == (t == steps - 1) and not o["trunc"].any(), (task, which, t)
    return np.stack([snaps[steps - leads[i % len(leads)]][i] for i in range(n)])


def attitude_states(task, n, seed, two_steps=False):
    """Oracle states three steps into an episode with pitch or roll (rates zeroed) set to +-1.05 / +-0.9: one step takes them to about
    +-1.034 (unhealthy) and +-0.886 (healthy).  Returns (states, which) with which[i] in {"pitch", "roll"}.
    two_steps: +-0.93 with a rate of +-1.5 instead -- about +-0.987 after one step and +-1.025 after two, whatever the actions (they move
    the attitude by ~1e-3 a step): every such env ends on its second step."""
    nj = orc.act_dim(task)
    env = orc.OracleVecEnv(task, n, seed=seed)
    env.reset()
    rng = np.random.default_rng(5)
    for _ in range(3):
        env.step(rng.uniform(-1, 1, (n, nj)).astype(np.float32))
    st = env.get_state()
    which = []
    for i in range(n):
        k, v = (3, 5) if i % 2 == 0 else (4, 6)
        if two_steps:
            sign = 1.0 if (i // 2) % 2 == 0 else -1.0
            st[i, 3 * nj + k], st[i, 3 * nj + v] = np.float32(0.93 * sign), np.float32(1.5 * sign)
        else:
            st[i, 3 * nj + k] = np.float32([1.05, -1.05, 0.9, -0.9][(i // 2) % 4])
            st[i, 3 * nj + v] = 0.0
        which.append("pitch" if k == 3 else "roll")
    return st, which
