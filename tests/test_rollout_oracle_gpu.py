"""The kernels bench.py times, checked directly against the CPU oracle at BASELINE.json's config sizes.

`tma_rollout_collect` runs the fused rollout chunks (`rollout_chunk2_h64_kernel`, `rollout_chunk_wide_bf_kernel`,
`rollout_chunk_wide_cont_kernel`, the per-step composition for the f32 256-wide nets); their env step is inlined in those kernels.
Here the actions a fused rollout RECORDED are replayed through `orc.OracleVecEnv` (the C restatement of
backend/examples/{gridworld.py:67-95, ball3d.py:74-113, push.py:62-125}, backend/mlagents/envs.py:60-84,125-152 with DummyVecEnv /
Monitor semantics, pinned bit-exact to the reference fixtures by tests/test_oracle_golden.py) with the same seed and env offset, and
every buffer the rollout wrote is compared with what the oracle produces: observations of every slot, rewards before the timeout
bootstrap (and the bootstrap re-applied from the oracle's terminal observations), terminated / truncated flags, the Monitor
(return, length) of every finished episode in per-env order, and the final episode index of every env.

Integer tasks (GridWorld, Push, Basic): bit-exact.  Ball3D: <= 1e-5 (north_star) with a bounded count of elements that are not
bit-identical (device sin(double) vs glibc).  Crawler: against the build's own C port -- parity UNPINNED (MuJoCo Ant-v5 is not
importable) -- same tolerance.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5  # north_star: float tasks within 1e-5

# (task, n_envs, n_steps, hidden, mfma_dtype, env_offset): BASELINE.json configs[1], [2], [3] (one GPU's shard), [0], [4] (shard, shortened)
CASES = [
    pytest.param("gridworld", 4096, 1024, 64, "f32", 0, id="gridworld-4096x1024-h64-f32"),
    pytest.param("ball3d", 4096, 1024, 256, "bf16", 0, id="ball3d-4096x1024-h256-bf16"),
    pytest.param("push", 2048, 2048, 256, "bf16", 2048, id="push-2048x2048-h256-bf16-shard1"),
    pytest.param("basic", 8, 1024, 256, "f32", 0, id="basic-8x1024-h256-f32"),
    pytest.param("crawler", 2048, 256, 256, "bf16", 4096, id="crawler-2048x256-h256-bf16-shard2-unpinned"),
    # (Crawler episodes run to the 1000-step limit: a narrower vector long enough for every env to finish one, timeout bootstrap included)
    pytest.param("crawler", 512, 1040, 256, "bf16", 4096, id="crawler-512x1040-h256-bf16-shard2-unpinned"),
    pytest.param("ant", 512, 1040, 256, "bf16", 0, id="ant-105x8-512x1040-h256-bf16-unpinned"),
    # ... and the configs[4] shard at its full size (round 4: the policy-only chunk on 16-env blocks, values / bootstrap on the side stream):
    # 2048 envs x 2048 steps, every env through two time limits
    pytest.param("crawler", 2048, 2048, 256, "bf16", 4096, id="crawler-2048x2048-h256-bf16-shard2-unpinned-config-size"),
    # the reference's default net and dtype (f32 256 x 256) at the headline size: the policy-only fused chunk + batched values / bootstrap
    pytest.param("gridworld", 4096, 256, 256, "f32", 0, id="gridworld-4096x256-h256-f32"),
    # the other fused H = 64 instantiations at the headline size
    pytest.param("push", 4096, 512, 64, "f32", 0, id="push-4096x512-h64-f32"),
    pytest.param("ball3d", 4096, 512, 64, "f32", 0, id="ball3d-4096x512-h64-f32"),
]


def _replay(task, N, T, hidden, mfma, env_offset, seed=1, start=None):
    """start = (states, actions, index of `steps` in a state): behind the reset both sides are given `states` and take one per-step step with `actions`, so that the
    rollout's observation row 0 belongs to the injected trajectory (it is compared with the oracle's like every other row)."""
    from three_mlagents_amd import _lib
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv

    exact = task in ("gridworld", "push", "basic")
    env = HipVecEnv(task, N, seed=seed, env_offset=env_offset)  # default ring depth: the configuration bench.py runs
    eng = env.engine
    eng.episode_log(1 << 21)
    model = PPO("MlpPolicy", env, n_steps=T, batch_size=max(256, N * T // 32), n_epochs=1, seed=seed,
                policy_kwargs={"net_arch": [hidden, hidden], "mfma_dtype": mfma})
    ref = orc.OracleVecEnv(task, N, seed=seed, env_offset=env_offset, threads=8)
    first_obs = ref.reset()
    if start is not None:
        eng.reset(model.buf["obs"][0])
        eng.set_state(start[0])
        ref.set_state(start[0])
        pre = eng.step(torch.from_numpy(start[1]).cuda())
        first = ref.step(start[1])
        assert not (first["term"] | first["trunc"]).any()  # the start states are one step before anything happens
        model.buf["obs"][T].copy_(pre["obs"][0])  # what collect_rollouts() carries over from a previous rollout
        model._last_obs_valid = True
        first_obs = first["obs"]
        # Monitor's episode length is the adapter's step count, which the kernels read from the state: an injected episode has already run
        # `steps` steps (the edge fixtures set the adapter's counter to the inner env's for the same reason); the oracle counts from its reset
        age = start[0][:, start[2]].astype(np.int32)  # start[2]: where the flat state keeps `steps`
    assert model.collect_rollouts()
    ran = (C.c_int32 * 3)()
    _lib.check(_lib.lib().tma_debug_last_rollout_plan(ran))
    b = {k: v.cpu().numpy() for k, v in model.buf.items() if k in ("obs", "actions", "rewards", "values", "terminated", "truncated")}
    log_r, log_l, log_e, seen = eng.pop_episode_log()
    assert seen == len(log_r)  # the log did not overflow
    ep_index = eng.episode_index().cpu().numpy().astype(np.uint32)

    if start is None:
        age = np.zeros(N, np.int32)
    inexact, compared = 0, 0
    events = dict(terminated=0, truncated=0, terminal_rewards=set(), limit_rewards=set(), unhealthy=set(), waypoint=set())  # what the ORACLE's side of the replay went through

    def cmp(name, got, want, t):
        nonlocal inexact, compared
        if exact:
            assert np.array_equal(got, want), (task, name, t)
        else:
            assert np.allclose(got, want, rtol=0, atol=TOL), (task, name, t, float(np.abs(got - want).max()))
            inexact += int((got != want).sum())
        compared += got.size

    cmp("first obs", b["obs"][0], first_obs, 0)
    trunc_rows = []  # (t, env) of every timeout, with the oracle's terminal observation and pre-bootstrap reward
    ep_events = []   # (env, return, length) of every finished episode, in (t, env) order
    for t in range(T):
        pre_state = ref.get_state() if start is not None else None
        r = ref.step(b["actions"][t])
        if pre_state is not None:
            # the invariant behind `age`: Monitor's length of an episode is the adapter's step count at its end, i.e. the state's `steps`
            ended = np.flatnonzero(r["term"] | r["trunc"])
            assert np.array_equal(r["ep_len"][ended] + age[ended], pre_state[ended, start[2]].astype(np.int32) + 1), (task, t)
        if task == "glider" and pre_state is not None:  # waypoint index changes inside the rollout, from the oracle's states
            going = np.flatnonzero((r["term"] | r["trunc"]) == 0)
            post = ref.get_state()
            events["waypoint"] |= {(int(a), int(c)) for a, c in zip(pre_state[going, 12], post[going, 12]) if a != c}
        if pre_state is not None and task in ("crawler", "ant"):  # which `unhealthy` condition ended each chain episode, from the oracle
            from _chain_scripts import why_unhealthy

            for i in np.flatnonzero(r["term"]):
                events["unhealthy"] |= why_unhealthy(task, pre_state[i], b["actions"][t, i])
        assert np.array_equal(b["terminated"][t], r["term"]) and np.array_equal(b["truncated"][t], r["trunc"]), (task, t)
        cmp("obs", b["obs"][t + 1], r["obs"], t)
        keep = r["trunc"] == 0
        cmp("rewards (no timeout)", b["rewards"][t][keep], r["rew32"][keep], t)
        idx = np.nonzero(r["trunc"])[0]
        if idx.size:
            trunc_rows.append((np.full(idx.size, t), idx, r["term_obs"][idx].copy(), r["rew32"][idx].copy()))
        done = np.nonzero(r["term"] | r["trunc"])[0]
        events["terminated"] += int(r["term"].sum())
        events["truncated"] += int(r["trunc"].sum())
        events["terminal_rewards"] |= set(r["rew64"][r["term"] != 0].tolist())
        events["limit_rewards"] |= set(r["rew64"][r["trunc"] != 0].tolist())
        if done.size:
            ep_events.append((done, r["ep_ret"][done].copy(), r["ep_len"][done] + age[done]))
            age[done] = 0
    assert np.array_equal(ep_index, ref.episode_index()), task

    # timeout bootstrap (SB3 collect_rollouts: rewards[i] += gamma * V(terminal_obs_i)): the library's bootstrap entry point applied to the
    # ORACLE's rewards and terminal observations of every timed-out (t, env) must give the rewards the fused rollout stored
    n_trunc = sum(len(x[0]) for x in trunc_rows)
    if n_trunc:
        tt = np.concatenate([x[0] for x in trunc_rows])
        ii = np.concatenate([x[1] for x in trunc_rows])
        tobs = torch.from_numpy(np.concatenate([x[2] for x in trunc_rows])).cuda().contiguous()
        rew = torch.from_numpy(np.concatenate([x[3] for x in trunc_rows])).cuda().contiguous()
        flags = torch.ones(n_trunc, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib().tma_policy_bootstrap(_lib.ptr(model.policy.params), C.byref(model.policy.dims), _lib.ptr(tobs), _lib.ptr(flags), n_trunc,
                                                   model.gamma, _lib.ptr(rew), _lib.stream_ptr()))
        cmp("rewards (timeout bootstrap)", b["rewards"][tt, ii], rew.cpu().numpy(), "all")

    # Monitor rows: the device episode log holds (return, length, env) of every finished episode; per env they must be the oracle's, in order
    n_events = sum(len(x[0]) for x in ep_events)
    assert len(log_r) == n_events, (len(log_r), n_events)
    if n_events:
        oe = np.concatenate([x[0] for x in ep_events])
        orr = np.concatenate([x[1] for x in ep_events])  # f64: Monitor's Python-float sum of the episode's rewards
        ol = np.concatenate([x[2] for x in ep_events])
        o_order = np.argsort(oe, kind="stable")
        g_order = np.argsort(log_e, kind="stable")
        assert np.array_equal(log_e[g_order], oe[o_order]) and np.array_equal(log_l[g_order], ol[o_order]), task
        cmp("episode returns", log_r[g_order], orr[o_order], "all")
    env.close()
    return dict(inexact=inexact, compared=compared, timeouts=n_trunc, episodes=n_events, events=events,
                plan=(_lib.ROLLOUT_FAMILIES[ran[0]], ran[1], ran[2]))


@pytest.mark.parametrize("task,N,T,hidden,mfma,env_offset", CASES)
def test_fused_rollout_replayed_through_the_oracle(task, N, T, hidden, mfma, env_offset):
    st = _replay(task, N, T, hidden, mfma, env_offset)
    print(f"[{task} {N}x{T} H={hidden} {mfma}] compared {st['compared']} elements, not bit-identical {st['inexact']}, "
          f"timeouts {st['timeouts']}, episodes {st['episodes']}")
    if T >= orc.max_episode_steps(task):
        assert st["episodes"] > 0 and st["timeouts"] > 0  # Monitor rows and the bootstrap branch were exercised
    if task in ("gridworld", "push", "basic"):
        assert st["inexact"] == 0
    else:
        # bounded so that "a visible fraction of the elements differs in the last bit" cannot pass: 0.1 % of the compared elements
        assert st["inexact"] <= 64 + st["compared"] // 1000, st


# ---- the fused families through the branches a random policy never reaches from a reset (the per-step kernels: tests/test_env_float_tasks_gpu.py
# on tests/golden/*_edges.npz, tests/test_env_gpu.py on the scripts of tests/_chain_scripts.py).  N = 40 (ragged 8-, 16- and 32-env tiles),
# T = 12; (family, waves per tile, envs per tile) as tests/test_rollout_plan_cpu.py tables them.
SUCCESS = {"bicycle": 50.0, "brickbreak": 10.0}
FAILURE = {"bicycle": -10.0, "brickbreak": -1.0, "glider": -50.0}
EDGE_N, EDGE_T = 40, 12
EDGE_CASES = [
    pytest.param("bicycle", 64, "f32", ("H64", 8, 16), id="bicycle-h64-f32"),
    pytest.param("bicycle", 256, "bf16", ("BF16_DISC", 0, 16), id="bicycle-h256-bf16"),
    pytest.param("bicycle", 256, "f32", ("F32_DISC", 0, 8), id="bicycle-h256-f32"),
    pytest.param("glider", 64, "f32", ("H64", 4, 16), id="glider-h64-f32"),
    pytest.param("glider", 256, "bf16", ("BF16_DISC", 0, 16), id="glider-h256-bf16"),
    pytest.param("glider", 256, "f32", ("F32_DISC", 0, 8), id="glider-h256-f32"),
    pytest.param("brickbreak", 256, "f32", ("F32_DISC", 0, 8), id="brickbreak-h256-f32"),
    pytest.param("crawler", 256, "bf16", ("BF16_BOX_PI", 0, 16), id="crawler-h256-bf16"),
    pytest.param("crawler", 256, "f32", ("F32_BOX", 0, 8), id="crawler-h256-f32"),
    pytest.param("ant", 256, "bf16", ("BF16_BOX_PI", 0, 16), id="ant-h256-bf16"),
    pytest.param("ant", 256, "f32", ("F32_BOX", 0, 8), id="ant-h256-f32"),
]
_START = {}


def _edge_start(task, golden):
    """(states, actions, index of `steps`) for the pre-step, one env in four per kind: a success-type ending on the rollout's first step (the failure where the task
    has no success), a failure ending on it, a healthy state 3 .. 10 steps short of the time limit, and the first two kinds again with the time
    limit on the same step.  Float tasks:
    the `pre_<x>` rows of the edge fixtures, whose next state ends the same way under every action (tests/_edges.py).  Chain tasks: the oracle's
    states two to four steps before a script of tests/_chain_scripts.py ends the episode (most end within three steps under zero action,
    tests/test_oracle_golden.py), reset states for the time limit, and in place of the far-from-anything kind attitude_states(two_steps=True):
    pitch or roll past 1 on the rollout's first step; the pre-step's action is zero."""
    if task in _START:
        return _START[task]
    N = EDGE_N
    limit = orc.max_episode_steps(task)
    if task in ("crawler", "ant"):
        from _chain_scripts import SCRIPTS, attitude_states, pre_unhealthy_states

        kinds = [w for (t, w) in SCRIPTS if t == task]
        fresh = orc.OracleVecEnv(task, N, seed=1)
        fresh.reset()
        st = fresh.get_state()
        for k, which in enumerate(kinds):
            st[k::4] = pre_unhealthy_states(task, which, N, seed=1, leads=(2, 3, 4))[k::4]
        st[3::4] = attitude_states(task, N, seed=1, two_steps=True)[0][: len(st[3::4])]  # |pitch| / |roll| > 1 on the rollout's first step
        act = np.zeros((N, orc.act_dim(task)), np.float32)
    else:
        from _edges import STEPS_AT, start_row

        g = golden(task + "_edges")
        tags = {"bicycle": ("goal", "fall"), "brickbreak": ("win", "lost"), "glider": ("wp_reached", "crash")}[task]
        rows = [start_row(g, tags[0]), start_row(g, tags[1]), start_row(g, "continue" if task != "glider" else "cruise")]
        pick = [i % 4 if i % 4 < 3 else (i // 4) % 2 for i in range(N)]  # (the fourth kind: the first two again, aged below)
        st = np.stack([rows[k][0] for k in pick])
        act = np.array([rows[k][1] for k in pick], np.int32)
        st[3::4, STEPS_AT[task]] = limit - 2  # the ending and the time limit on one step: truncated, not terminated, the reward kept
    at = st.shape[1] - 1 if task in ("crawler", "ant") else STEPS_AT[task]
    st[2::4, at] = [limit - (3 + k % 8) for k in range(len(st[2::4]))]
    _START[task] = (st, act, at)
    return _START[task]


@pytest.mark.parametrize("task,hidden,mfma,plan", EDGE_CASES)
def test_fused_rollout_through_the_edge_branches(golden, task, hidden, mfma, plan):
    """Every fused family that inlines a float or chain task's step, started from the edge states: endings of every kind fall inside the chunk
    at different steps, so the reset, the timeout bootstrap and the episode log follow inside the kernel -- replayed through the oracle like
    the cases above (every observation row, rewards, flags, bootstrap, Monitor rows, final episode index)."""
    st = _replay(task, EDGE_N, EDGE_T, hidden, mfma, 0, start=_edge_start(task, golden))
    ev = st["events"]
    print(f"[{task} edges {EDGE_N}x{EDGE_T} H={hidden} {mfma}] {st['plan']}: compared {st['compared']} elements, not bit-identical {st['inexact']}, "
          f"terminated {ev['terminated']} ({sorted(ev['unhealthy']) or sorted(ev['terminal_rewards'])}), waypoint {sorted(ev['waypoint'])}, truncated {ev['truncated']} (with a terminal reward: {sorted(set(ev['limit_rewards']) & {SUCCESS.get(task), FAILURE.get(task)})}), episodes {st['episodes']}")
    assert st["plan"] == plan, st["plan"]
    # from the oracle's side of the replay: the case went through what it is about
    assert ev["truncated"] > 0 and ev["terminated"] > 0 and st["timeouts"] == ev["truncated"], ev
    if task in SUCCESS:
        assert SUCCESS[task] in ev["terminal_rewards"], ev
    if task in FAILURE:
        assert FAILURE[task] in ev["terminal_rewards"], ev
        assert FAILURE[task] in ev["limit_rewards"] and SUCCESS.get(task, FAILURE[task]) in ev["limit_rewards"], ev  # ... and at the limit, as truncations
    if task == "glider":
        assert (1, 0) in ev["waypoint"], ev  # the waypoint was reached and its index wrapped inside the chunk
    if task == "brickbreak":
        assert st["inexact"] == 0, st  # add / multiply / compare only: bit for bit, the resets' cos / sin after the float32 cast included
    if task in ("crawler", "ant"):  # each of the three `unhealthy` conditions, in the lane-parallel step the Box chunks run
        assert ev["unhealthy"] == {"z", "pitch", "roll"}, ev
    assert st["inexact"] <= 64 + st["compared"] // 1000, st
