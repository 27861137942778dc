#!/usr/bin/env python3
"""Time the TD3 kernels (csrc/tma_td3.hip, ABI 227) with HIP events on the `ant` shape (105 observations, 8 actions), ReLU, at H in {64, 256} x
B in {64, 256}, and in the SAME process the `tma_sac_*` calls at the same shapes and the restatement (tests/_td3_ref.py Trainer, torch autograd
and two torch Adams) in float32 on the same GPU:
  * critic_grad, actor_grad: the two gradient calls (two launches each) on one sampled batch, TD3's and SAC's;
  * step:        a whole gradient step with the delayed block, `TD3.train(1)` at policy_delay = 1 (sample, critic, Adam, actor, Adam, two polyak
                 updates: 9 launches), the average step at policy_delay = 2, and the restatement's step at policy_delay = 1;
  * collect:     one collected vector step of `ant` at one env, three launches (tma_td3_act with action noise -> tma_env_step -> tma_replay_add).
A timed window is `reps` back-to-back calls between two events; a repeat is the median of 5 windows; every figure is the median of 5 repeats, the
repeats of the variants interleaved, and `spread_us` is max - min over the 5 repeats.  The expectation recorded: tma_td3_critic_grad does strictly less
work per row than tma_sac_critic_grad (no log-std head, no log-probability), so it should not be slower; `td3_not_slower` is median(TD3) <=
median(SAC) + spread(SAC).  Prints one JSON object; `python tools/time_td3.py OUT.json` also writes it."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _td3_ref as ref  # noqa: E402  (the torch restatement: the baseline)
from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.replay_buffer import ReplayBuffer  # noqa: E402
from three_mlagents_amd.sac import SAC  # noqa: E402
from three_mlagents_amd.td3 import TD3, NormalActionNoise  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402

DEV = torch.device("cuda", 0)
L = _lib.lib()
p = _lib.ptr
D, A = 105, 8
REPEATS = 5


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


def repeats(variants, reps):
    """{name: {median_us, spread_us, repeats_us}} over REPEATS interleaved repeats"""
    us = {name: [] for name, _ in variants}
    for _ in range(REPEATS):
        for name, fn in variants:
            us[name].append(window_us(fn, reps))
    return {name: {"median_us": float(np.median(v)), "spread_us": max(v) - min(v), "repeats_us": v} for name, v in us.items()}


def fill(model, cls_dims, H, B, stats):
    """A model without an env: policy, a ring of random transitions, the buffers train() uses."""
    model.device = DEV
    model._make_policy(D, A, H, "relu", DEV)
    g = torch.Generator().manual_seed(1)
    rb = model.replay_buffer = ReplayBuffer(4096, D, (A, True), DEV, n_envs=1, seed=1)
    for _ in range(1024):
        rb.add(torch.randn(1, D, generator=g).to(DEV), torch.randn(1, D, generator=g).to(DEV), (torch.rand(1, A, generator=g) * 2 - 1).to(DEV),
               torch.randn(1, generator=g).to(DEV), (torch.rand(1, generator=g) < 0.05).to(torch.uint8).to(DEV), torch.zeros(1, dtype=torch.uint8, device=DEV))
    need = int(cls_dims(C.byref(model.policy.dims), B))
    model.buf = dict(ws=torch.zeros(need, dtype=torch.uint8, device=DEV), critic_stats=torch.zeros(4, dtype=torch.float64, device=DEV),
                     actor_stats=torch.zeros(stats, dtype=torch.float64, device=DEV))
    model.train(4)
    return model


def shape_timing(H, B):
    kw = dict(learning_rate=3e-4, batch_size=B, seed=1, policy_kwargs=dict(net_arch=[H, H]))
    td3 = fill(TD3("MlpPolicy", None, policy_delay=1, **kw), L.tma_td3_workspace_bytes, H, B, 2)
    td3_d2 = fill(TD3("MlpPolicy", None, policy_delay=2, **kw), L.tma_td3_workspace_bytes, H, B, 2)
    sac = fill(SAC("MlpPolicy", None, **kw), L.tma_sac_workspace_bytes, H, B, 3)
    st = _lib.stream_ptr(DEV)
    tp, sp, rb = td3.policy, sac.policy, td3.replay_buffer
    s = rb.sample(B)
    gc, ga, gs = torch.empty(tp.n_critic, device=DEV), torch.empty(tp.n_actor, device=DEV), torch.empty(sp.n_actor, device=DEV)
    tws, sws = td3.buf["ws"], sac.buf["ws"]
    batch = (p(s.observations), p(s.actions), p(s.next_observations), p(s.dones), p(s.rewards), p(s.discounts))

    def td3_critic():
        _lib.check(L.tma_td3_critic_grad(p(tp.actor_target), p(tp.critic), p(tp.critic_target), C.byref(tp.dims), *batch, B, 0.2, 0.5, 1, 2, None, p(gc), None,
                                         None, None, None, None, p(tws), tws.numel(), st))

    def td3_actor():
        _lib.check(L.tma_td3_actor_grad(p(tp.actor), p(tp.critic), C.byref(tp.dims), batch[0], B, p(ga), None, None, None, p(tws), tws.numel(), st))

    def sac_critic():
        _lib.check(L.tma_sac_critic_grad(p(sp.actor), p(sp.critic), p(sp.critic_target), p(sp.log_ent_coef), C.byref(sp.dims), *batch, B, 1, 2, None, p(gc), None,
                                         None, None, None, None, p(sws), sws.numel(), st))

    def sac_actor():
        _lib.check(L.tma_sac_actor_grad(p(sp.actor), p(sp.critic), p(sp.log_ent_coef), C.byref(sp.dims), batch[0], B, 1, 2, None, p(gs), None, None, None, None,
                                        None, p(sws), sws.numel(), st))

    trainer = ref.Trainer(tp.state_dict(), lr=3e-4, tau=0.005, policy_delay=1, policy_noise=0.2, noise_clip=0.5, dtype=torch.float32, device=DEV)

    def torch_step():
        data = rb.sample(B)
        trainer.step(dict(obs=data.observations, actions=data.actions, next_obs=data.next_observations, dones=data.dones, rewards=data.rewards,
                          discounts=data.discounts, noise=torch.randn((B, A), device=DEV)))

    kernels = repeats((("tma_td3_critic_grad", td3_critic), ("tma_sac_critic_grad", sac_critic), ("tma_td3_actor_grad", td3_actor),
                       ("tma_sac_actor_grad", sac_actor)), 512)
    step = repeats((("td3_train_1_policy_delay_1", lambda: td3.train(1)), ("td3_train_2_policy_delay_2_per_step", lambda: td3_d2.train(2)),
                    ("sac_train_1", lambda: sac.train(1)), ("torch_float32_td3_step_policy_delay_1", torch_step)), 128)
    for k in ("median_us", "spread_us"):
        step["td3_train_2_policy_delay_2_per_step"][k] /= 2.0
    step["td3_train_2_policy_delay_2_per_step"]["repeats_us"] = [v / 2.0 for v in step["td3_train_2_policy_delay_2_per_step"]["repeats_us"]]
    t, s_ = kernels["tma_td3_critic_grad"], kernels["tma_sac_critic_grad"]
    return {"D": D, "A": A, "H": H, "B": B, "kernels": kernels, "gradient_step": step,
            "critic_grad_td3_over_sac": t["median_us"] / s_["median_us"], "td3_not_slower": bool(t["median_us"] <= s_["median_us"] + s_["spread_us"]),
            "torch_over_native_step": step["torch_float32_td3_step_policy_delay_1"]["median_us"] / step["td3_train_1_policy_delay_1"]["median_us"]}


def collect_timing(H):
    env = HipVecEnv("ant", 1, seed=1)
    model = TD3("MlpPolicy", env, seed=1, learning_starts=100, buffer_size=10_000, batch_size=64, action_noise=NormalActionNoise(np.zeros(A), 0.1 * np.ones(A)),
                policy_kwargs=dict(net_arch=[H, H]))
    model.learn(300)
    pol, rb, b, st, eng, counter = model.policy, model.replay_buffer, model.buf, _lib.stream_ptr(DEV), env.engine, {"k": 0}

    def collect3():
        counter["k"] += 1
        _lib.check(L.tma_td3_act(p(pol.actor), C.byref(pol.dims), p(rb.last_obs), 1, _lib.TD3_NOISY, C.byref(model._noise), 1, counter["k"], 0, None,
                                 p(b["actions"]), None, None, st))
        _lib.check(L.tma_env_step(eng._h, p(b["actions"]), _lib.ACT_F32, 0, 0, 1, p(b["step_obs"]), p(b["rewards"]), p(b["term"]), p(b["trunc"]),
                                  p(b["term_obs"]), None, None, st))
        _lib.check(L.tma_replay_add(C.byref(rb._view), rb.pos, p(rb.last_obs), p(b["actions"]), p(b["step_obs"]), p(b["rewards"]), p(b["term"]), p(b["trunc"]),
                                    p(b["term_obs"]), st))

    out = repeats((("act_step_add_3_launches", collect3),), 512)["act_step_add_3_launches"]
    env.close()
    return out


def main():
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("TMA_COMMIT", "unknown")
    res = {"what": "HIP-event time per call in microseconds: windows of back-to-back calls, a repeat = the median of 5 windows, median and spread (max - min) "
                   "of 5 interleaved repeats; ant shape (105 + 8), ReLU",
           "device": torch.cuda.get_device_name(0), "commit": commit, "abi": int(L.tma_version()),
           "shapes": {f"H{H}_B{B}": shape_timing(H, B) for H in (64, 256) for B in (64, 256)},
           "collected_step": {f"H{H}": collect_timing(H) for H in (64, 256)}}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
