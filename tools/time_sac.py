#!/usr/bin/env python3
"""Time the SAC kernels (csrc/tma_sac.hip, ABI 226) with HIP events at H = 256 (ReLU), B = 256 -- the reference's SAC table -- on two shapes:
`ant` (105 observations, 8 actions: the one Box task of this build whose shape the kernels take) and 6 / 2 (Ball3D's observation width with a
two-dimensional Box action: a shape only, the task itself has a Discrete action space):
  * act:         `tma_sac_act` on one row (a collected step's forward) and on B rows;
  * critic_grad, actor_grad: the two gradient calls (two launches each) on one sampled batch;
  * step:        a whole gradient step, `SAC.train(1)` (sample, critic, Adam, actor, Adam, ent_coef, Adam, polyak: 10 launches), against the
                 restatement of the same step (tests/_sac_ref.py Trainer: torch autograd and three torch Adams) in float32 on the same GPU;
  * collect:     one collected vector step of `ant` at one env, three launches (tma_sac_act -> tma_env_step -> tma_replay_add);
  * learn:       env-steps per second of `SAC.learn` on `ant` at one env with the reference's table (wall clock, synchronised).
A timed window is `reps` back-to-back calls between two events; the figure is the window over reps, median of 5 windows, the smaller of two
interleaved rounds.  No ratio is asserted.  Prints one JSON object; `python tools/time_sac.py OUT.json` also writes it."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import _sac_ref as ref  # noqa: E402  (the torch restatement: the baseline)
from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.replay_buffer import ReplayBuffer  # noqa: E402
from three_mlagents_amd.sac import SAC  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402

DEV = torch.device("cuda", 0)
L = _lib.lib()
p = _lib.ptr
H, B = 256, 256
TABLE = dict(learning_rate=3e-4, buffer_size=100_000, learning_starts=1_000, batch_size=B, gamma=0.99, tau=0.005, train_freq=1, gradient_steps=1)


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


def shape_timing(D, A, env=None):
    """The kernels on a model of shape (D, A): trained on `env` where there is one, else on a ring filled with random transitions."""
    if env is not None:
        model = SAC("MlpPolicy", env, seed=1, **TABLE)
        model.learn(2_000)
    else:
        model = SAC("MlpPolicy", None, seed=1, **TABLE)
        model.device = DEV
        model._make_policy(D, A, H, "relu", DEV)
        g = torch.Generator().manual_seed(1)
        rb = model.replay_buffer = ReplayBuffer(4096, D, (A, True), DEV, n_envs=1, seed=1)
        for _ in range(2048):
            rb.add(torch.randn(1, D, generator=g).to(DEV), torch.randn(1, D, generator=g).to(DEV), (torch.rand(1, A, generator=g) * 2 - 1).to(DEV),
                   torch.randn(1, generator=g).to(DEV), (torch.rand(1, generator=g) < 0.05).to(torch.uint8).to(DEV), torch.zeros(1, dtype=torch.uint8, device=DEV))
        need = int(L.tma_sac_workspace_bytes(C.byref(model.policy.dims), B))
        model.buf = dict(ws=torch.zeros(need, dtype=torch.uint8, device=DEV), critic_stats=torch.zeros(4, dtype=torch.float64, device=DEV),
                         actor_stats=torch.zeros(3, dtype=torch.float64, device=DEV))
        model.train(8)
    pol, rb, b, st = model.policy, model.replay_buffer, model.buf, _lib.stream_ptr(DEV)
    d, ws = C.byref(pol.dims), b["ws"]
    s = rb.sample(B)
    one, acts1, actsB = s.observations[:1].contiguous(), torch.empty((1, A), device=DEV), torch.empty((B, A), device=DEV)
    gc, ga = torch.empty(pol.n_critic, device=DEV), torch.empty(pol.n_actor, device=DEV)

    def act(obs, out, n):
        _lib.check(L.tma_sac_act(p(pol.actor), d, p(obs), n, _lib.SAC_SAMPLE, 1, 2, 0, None, p(out), None, None, None, st))

    def critic_grad():
        _lib.check(L.tma_sac_critic_grad(p(pol.actor), p(pol.critic), p(pol.critic_target), p(pol.log_ent_coef), d, p(s.observations), p(s.actions),
                                         p(s.next_observations), p(s.dones), p(s.rewards), p(s.discounts), B, 1, 2, None, p(gc), None, None, None, None, None,
                                         p(ws), ws.numel(), st))

    def actor_grad():
        _lib.check(L.tma_sac_actor_grad(p(pol.actor), p(pol.critic), p(pol.log_ent_coef), d, p(s.observations), B, 1, 2, None, p(ga), None, None, None, None,
                                        None, p(ws), ws.numel(), st))

    # the baseline: the restatement's whole step in float32 on this GPU, on the same weights, with torch's own noise
    trainer = ref.Trainer(pol.state_dict(), float(pol.log_ent_coef.cpu()[0]), lr=3e-4, tau=0.005, target_entropy=-float(A), dtype=torch.float32, device=DEV)

    def torch_step():
        data = rb.sample(B)
        trainer.step(dict(obs=data.observations, actions=data.actions, next_obs=data.next_observations, dones=data.dones, rewards=data.rewards,
                          discounts=data.discounts, noise_next=torch.randn((B, A), device=DEV), noise_pi=torch.randn((B, A), device=DEV)))

    kernels = best_of_two((("tma_sac_act_1_row", lambda: act(one, acts1, 1)), ("tma_sac_act_B_rows", lambda: act(s.observations, actsB, B)),
                           ("tma_sac_critic_grad", critic_grad), ("tma_sac_actor_grad", actor_grad)), 1024)
    step = best_of_two((("native_train_1", lambda: model.train(1)), ("torch_float32_step", torch_step)), 256)
    out = {"D": D, "A": A, "H": H, "B": B, "kernels_us": kernels, "gradient_step_us": step,
           "torch_over_native_step": step["torch_float32_step"] / step["native_train_1"]}
    if env is not None:
        eng, counter = env.engine, {"k": 0}

        def collect3():
            counter["k"] += 1
            _lib.check(L.tma_sac_act(p(pol.actor), d, p(rb.last_obs), 1, _lib.SAC_SAMPLE, 1, counter["k"], 0, None, p(b["actions"]), None, None, None, st))
            _lib.check(L.tma_env_step(eng._h, p(b["actions"]), _lib.ACT_F32, 0, 0, 1, p(b["step_obs"]), p(b["rewards"]), p(b["term"]), p(b["trunc"]),
                                      p(b["term_obs"]), None, None, st))
            _lib.check(L.tma_replay_add(C.byref(rb._view), rb.pos, p(rb.last_obs), p(b["actions"]), p(b["step_obs"]), p(b["rewards"]), p(b["term"]),
                                        p(b["trunc"]), p(b["term_obs"]), st))

        out["collected_step_us"] = best_of_two((("act_step_add_3_launches", collect3),), 1024)
    return out


def learn_timing(steps=20_000):
    env = HipVecEnv("ant", 1, seed=1)
    model = SAC("MlpPolicy", env, seed=1, **TABLE)
    model.learn(2_000)  # warm: allocations, first launches, past learning_starts
    torch.cuda.synchronize()
    t0 = time.time()
    model.learn(steps, reset_num_timesteps=False)
    torch.cuda.synchronize()
    took = time.time() - t0
    env.close()
    return {"task": "ant", "steps": steps, "native_learn_seconds": took, "native_env_steps_per_s": steps / took, "n_updates": model._n_updates}


def main():
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("TMA_COMMIT", "unknown")
    env = HipVecEnv("ant", 1, seed=1)
    res = {"what": "HIP-event time per call in microseconds (median of 5 windows of back-to-back calls, the smaller of two interleaved rounds); learn: wall "
                   "clock of 20 000 env steps of ant at one env, synchronised, one optimizer step per env step",
           "device": torch.cuda.get_device_name(0), "commit": commit, "abi": int(L.tma_version()),
           "shapes": {"ant_105_8": shape_timing(105, 8, env), "obs6_act2": shape_timing(6, 2)}}
    env.close()
    res["learn"] = learn_timing()
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
