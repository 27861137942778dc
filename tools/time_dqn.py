#!/usr/bin/env python3
"""Time the DQN kernels (csrc/tma_dqn.hip, ABI 225) against the compositions they replace, with HIP events, at (D, A) = (21, 3) and (4, 5), H = 128
(ReLU), B = 64 -- the reference's DQN table on Basic and GridWorld:
  * td_grad:   `tma_dqn_td_grad` (two launches) against what tools/dqn_example.py runs for the same gradient: two `policy.head` forwards (the
               target's under no_grad), torch smooth_l1_loss on the gathered column, and its backward (one tma_policy_head_vjp call behind
               torch autograd's own kernels);
  * opt_step:  sample + TD gradient + clip + Adam, natively (`DQN.train(1)`) against the example's (rb.sample, the composition above,
               clip_grad_norm_, torch.optim.Adam.step);
  * collect:   one collected vector step, three launches (tma_dqn_act -> tma_env_step -> tma_replay_add) against `ReplayBuffer.collect`'s four
               (head -> tma_egreedy_actions -> env step -> add), one env;
  * learn:     env-steps per second of `DQN.learn(25 000)` at one env (wall clock, synchronised) against tools/dqn_example.py on the same
               schedule in the same session (a child process; its own figure includes ten evaluations, so it is also run with --evals 1).
A timed window is `reps` back-to-back calls between two events; the figure is the window over reps, median of 5 windows, the smaller of two
interleaved rounds.  No ratio is asserted.  Prints one JSON object; `python tools/time_dqn.py OUT.json` also writes it."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.dqn import DQN  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402

DEV = torch.device("cuda", 0)
L = _lib.lib()
TASKS = [("basic", 21, 3), ("gridworld", 4, 5)]
TABLE = dict(learning_rate=3e-4, buffer_size=25_000, learning_starts=1_250, batch_size=64, gamma=0.99, train_freq=4, gradient_steps=1,
             target_update_interval=1_000, exploration_fraction=0.25, exploration_final_eps=0.03, policy_kwargs={"net_arch": [128, 128]})


def window_us(fn, reps, warm=2, rounds=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    out.sort()
    return out[len(out) // 2]


def best_of_two(variants, reps):
    us = {}
    for _ in range(2):
        for name, fn in variants:
            t = window_us(fn, reps)
            us[name] = min(us.get(name, t), t)
    return us


def task_timing(task, D, A):
    env = HipVecEnv(task, 1, seed=1)
    model = DQN("MlpPolicy", env, seed=1, **TABLE)
    model.learn(2_000)  # a filled ring, trained weights, a target that differs from the online net
    pol, tgt, rb, b, st = model.policy, model.q_net_target, model.replay_buffer, model.buf, _lib.stream_ptr(DEV)
    B = model.batch_size
    s = rb.sample(B)
    ws = b["td_ws"]

    def td_grad():
        _lib.check(L.tma_dqn_td_grad(_lib.ptr(pol.params), _lib.ptr(tgt.params), C.byref(pol.dims), _lib.ptr(s.observations), _lib.ptr(s.actions),
                                     _lib.ptr(s.next_observations), _lib.ptr(s.dones), _lib.ptr(s.rewards), _lib.ptr(s.discounts), B, _lib.ptr(model.grad), None,
                                     None, _lib.ptr(ws), ws.numel(), st))

    # the composition, on a policy of its own with the same weights (parameters() makes the head differentiable)
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    q2, t2 = (HipActorCriticPolicy(D, A, False, 128, DEV, seed=1, activation="relu", ortho_init=False) for _ in range(2))
    q2.load_state_dict(pol.state_dict()), t2.load_state_dict(tgt.state_dict())
    params = q2.parameters()
    opt = torch.optim.Adam(params, lr=3e-4)
    idx = s.actions.long()[:, None]

    def composition(data=s, index=idx):
        with torch.no_grad():
            y = data.rewards + (1.0 - data.dones) * data.discounts * t2.head(data.next_observations)[0].max(dim=1).values
        loss = F.smooth_l1_loss(q2.head(data.observations)[0].gather(1, index).squeeze(1), y)
        opt.zero_grad()
        loss.backward()

    def example_step():
        data = rb.sample(B)
        composition(data, data.actions.long()[:, None])
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        opt.step()

    # the two gradients agree before either is timed
    td_grad()
    composition()
    err = float((model.grad[: pol.offsets[6]] - params[0].grad[: pol.offsets[6]]).abs().max())
    assert err < 1e-5, err
    grad_us = best_of_two((("tma_dqn_td_grad", td_grad), ("head_head_vjp_torch_huber", composition)), 2048)
    step_us = best_of_two((("native_train_1", lambda: model.train(1)), ("example_step", example_step)), 1024)

    # one collected vector step
    eng, N = env.engine, 1
    counter = {"k": 0}

    def collect3():
        counter["k"] += 1
        _lib.check(L.tma_dqn_act(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(rb.last_obs), N, 0.1, 1, counter["k"], 0, _lib.ptr(b["actions"]), None, st))
        _lib.check(L.tma_env_step(eng._h, _lib.ptr(b["actions"]), _lib.ACT_I32, 0, 0, 1, _lib.ptr(b["step_obs"]), _lib.ptr(b["rewards"]), _lib.ptr(b["term"]),
                                  _lib.ptr(b["trunc"]), _lib.ptr(b["term_obs"]), None, None, st))
        _lib.check(L.tma_replay_add(C.byref(rb._view), rb.pos, _lib.ptr(rb.last_obs), _lib.ptr(b["actions"]), _lib.ptr(b["step_obs"]), _lib.ptr(b["rewards"]),
                                    _lib.ptr(b["term"]), _lib.ptr(b["trunc"]), _lib.ptr(b["term_obs"]), st))

    q_fn = lambda obs: pol.head(obs)[0]  # noqa: E731
    collect_us = best_of_two((("act_step_add_3_launches", collect3), ("replay_buffer_collect_4_launches", lambda: rb.collect(env, q_fn, 1, 0.1))), 2048)
    env.close()
    return {"D": D, "A": A, "H": 128, "B": B, "grad_max_abs_difference": err, "td_grad_us": grad_us,
            "composition_over_td_grad": grad_us["head_head_vjp_torch_huber"] / grad_us["tma_dqn_td_grad"], "opt_step_us": step_us,
            "example_over_native_step": step_us["example_step"] / step_us["native_train_1"], "collected_step_us": collect_us,
            "collect_over_three_launches": collect_us["replay_buffer_collect_4_launches"] / collect_us["act_step_add_3_launches"]}


def learn_timing(task, steps=25_000):
    env = HipVecEnv(task, 1, seed=1)
    model = DQN("MlpPolicy", env, seed=1, **TABLE)
    model.learn(1_000)  # warm: allocations, first launches
    torch.cuda.synchronize()
    t0 = time.time()
    model.learn(steps)
    torch.cuda.synchronize()
    native = time.time() - t0
    env.close()
    out = {"steps": steps, "native_learn_seconds": native, "native_env_steps_per_s": steps / native, "n_updates": model._n_updates}
    for evals in (1, 10):
        t0 = time.time()
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dqn_example.py"), "--task", task, "--timesteps", str(steps), "--evals", str(evals)],
                       check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=600)
        out[f"example_process_seconds_evals{evals}"] = time.time() - t0
    # the child's start-up (imports, context, library load) is not the loop's: a run of 4 steps measures it
    t0 = time.time()
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dqn_example.py"), "--task", task, "--timesteps", "4", "--evals", "1"], check=True, cwd=ROOT,
                   stdout=subprocess.DEVNULL, timeout=600)
    out["example_process_startup_seconds"] = time.time() - t0
    loop = out["example_process_seconds_evals1"] - out["example_process_startup_seconds"]
    out["example_env_steps_per_s"] = steps / max(loop, 1e-9)
    out["native_over_example"] = out["native_env_steps_per_s"] / out["example_env_steps_per_s"]
    return out


def main():
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("TMA_COMMIT", "unknown")
    res = {"what": "HIP-event time per call in microseconds (median of 5 windows of back-to-back calls, the smaller of two interleaved rounds); learn: wall "
                   "clock of 25 000 env steps at one env, synchronised, against tools/dqn_example.py as a child process less its start-up",
           "device": torch.cuda.get_device_name(0), "commit": commit, "abi": int(L.tma_version()),
           "kernels": {task: task_timing(task, D, A) for task, D, A in TASKS}, "learn": {task: learn_timing(task) for task, _, _ in TASKS}}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
