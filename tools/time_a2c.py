#!/usr/bin/env python3
"""Time A2C at the reference's schedule (8 envs x 5 steps, SB3's default 64 x 64 nets) with HIP events, for basic / gridworld / ball3d:
  * us per iteration through the per-iteration path (collect_rollouts() + train()) and through tma_a2c_iterations_local, and env-steps/s;
  * us of each piece of one iteration (rollout, GAE, sample records, gradient + policy-loss reduction, RMSprop step), each in a chain of its own;
  * us of the RMSprop step next to the Adam step, per optimizer kernel shape (tma_debug_plan_dispatch(TMA_PLAN_OPT)).
Prints one JSON object; `python tools/time_a2c.py OUT.json` also writes it there."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.a2c import A2C, RMSPROP_ALPHA  # noqa: E402
from three_mlagents_amd.harness import make_vector_env  # noqa: E402
from three_mlagents_amd.ppo import HipActorCriticPolicy  # noqa: E402

DEV = torch.device("cuda", 0)
L = _lib.lib()


def chain_us(fn, reps, warm=20, rounds=5):
    """median over `rounds` of (HIP-event time of `reps` back-to-back calls) / reps"""
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


def native(m, n):
    eng, b, pol = m.env.engine, m.buf, m.policy
    carry = 1 if m._last_obs_valid else 0
    if not carry:
        eng.reset(b["obs"][0])
        m._last_obs_valid = True
    _lib.check(L.tma_a2c_iterations_local(eng._h, _lib.ptr(pol.params), C.byref(pol.dims), C.byref(m._rb), _lib.ptr(b["advantages"]), _lib.ptr(b["returns"]),
                                          _lib.ptr(m._packed) if m._packed is not None else None, m.n_steps, m.seed & 0xFFFFFFFF, m._rollout_counter & 0xFFFFFFFF,
                                          eng.env_offset & 0xFFFFFFFF, m.gamma, m.gae_lambda, carry, n, C.byref(m._a2c_hp), _lib.ptr(m.grad), _lib.ptr(m.square_avg),
                                          m.learning_rate, RMSPROP_ALPHA, m.rms_prop_eps, m.max_grad_norm, _lib.ptr(m.workspace), m._stream()))
    m._rollout_counter += n


def task_timing(task):
    env = make_vector_env(task, n_envs=8, seed=1)
    m = A2C("MlpPolicy", env, seed=1)
    pol, b, eng, st = m.policy, m.buf, env.engine, m._stream()
    T, N = m.n_steps, m.n_envs

    def per_iteration():
        m.collect_rollouts(None)
        m.train()

    res = {"per_iteration_path_us": chain_us(per_iteration, 200), "native_path_us": chain_us(lambda: native(m, 100), 2, warm=2) / 100}
    res["env_steps_per_s"] = {k: T * N / (res[k + "_us"] * 1e-6) for k in ("per_iteration_path", "native_path")}

    def rollout():
        _lib.check(L.tma_rollout_collect(eng._h, _lib.ptr(pol.params), C.byref(pol.dims), C.byref(m._rb), 0, T, T, 1, 0, 0, m.gamma, 1, 0, st))

    def gae():
        _lib.check(L.tma_gae_flags(_lib.ptr(b["rewards"]), _lib.ptr(b["values"]), _lib.ptr(b["terminated"]), _lib.ptr(b["truncated"]), _lib.ptr(b["last_values"]),
                                   m.gamma, m.gae_lambda, T, N, _lib.ptr(b["advantages"]), _lib.ptr(b["returns"]), st))

    def pack():
        _lib.check(L.tma_ppo_pack_samples(C.byref(m._rollout_view), C.byref(pol.dims), _lib.ptr(m._packed), st))

    def grad():
        _lib.check(L.tma_a2c_grad(_lib.ptr(pol.params), C.byref(pol.dims), C.byref(m._rollout_view), C.byref(m._a2c_hp), _lib.ptr(m.grad), _lib.ptr(m.workspace), st))

    def step():
        _lib.check(L.tma_rmsprop_step_local(_lib.ptr(pol.params), _lib.ptr(m.grad), _lib.ptr(m.square_avg), C.byref(pol.dims), 0.0, RMSPROP_ALPHA, m.rms_prop_eps,
                                            m.max_grad_norm, _lib.ptr(m.workspace), st, T * N))

    pieces = {"rollout_collect": rollout, "gae_flags": gae, "a2c_grad": grad, "rmsprop_step_local": step}
    if m._packed is not None:
        pieces["pack_samples"] = pack
    res["pieces_us"] = {k: chain_us(f, 200) for k, f in pieces.items()}
    fwd, gr, op = C.c_int32(), C.c_int32(), C.c_int32()
    L.tma_debug_last_dispatch(C.byref(fwd), C.byref(gr), C.byref(op))
    res["dispatch"] = {"grad": gr.value, "opt": op.value}
    env.close()
    return res


def optimizer_timing():
    out = {}
    for name, (D, H, A, cont, dtype) in {"scatter_h64": (4, 64, 5, False, "f32"), "scatter_wide": (6, 256, 5, False, "f32"), "scatter_wide_bf16": (6, 256, 5, False, "bf16"),
                                         "small": (7, 64, 3, True, "f32"), "small_loop": (21, 64, 3, False, "f32"), "generic": (8, 512, 4, False, "f32")}.items():
        pol = HipActorCriticPolicy(D, A, cont, H, DEV, seed=1, mfma_dtype=dtype)
        P = pol.n_trainable
        grad, sq, m, v = (torch.zeros(P, device=DEV) for _ in range(4))
        sq.fill_(1.0)
        ws = torch.zeros(int(L.tma_ppo_workspace_bytes(C.byref(pol.dims))), dtype=torch.uint8, device=DEV)
        st = _lib.stream_ptr()
        pid = C.c_int32()
        L.tma_debug_plan_dispatch(C.byref(pol.dims), 2, 0, C.byref(pid), None, None, None)

        def rms():
            _lib.check(L.tma_rmsprop_step(_lib.ptr(pol.params), _lib.ptr(grad), _lib.ptr(sq), C.byref(pol.dims), 7e-4, 0.99, 1e-5, 0.5, 1.0, _lib.ptr(ws), st))

        def adam():
            _lib.check(L.tma_ppo_adam_step(_lib.ptr(pol.params), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), C.byref(pol.dims), 1, 7e-4, 0.9, 0.999, 1e-5, 0.5, 1.0,
                                           _lib.ptr(ws), st))

        # interleaved A / B / A / B: both see the same clocks
        a1, r1, a2, r2 = chain_us(adam, 200), chain_us(rms, 200), chain_us(adam, 200), chain_us(rms, 200)
        out[name] = {"plan_id": pid.value, "n_trainable": P, "adam_us": min(a1, a2), "rmsprop_us": min(r1, r2), "ratio": min(r1, r2) / min(a1, a2)}
    return out


def main():
    res = {"schedule": "8 envs x 5 steps, net_arch [64, 64]", "tasks": {t: task_timing(t) for t in ("basic", "gridworld", "ball3d")},
           "optimizer_step_whole_entry_us": optimizer_timing()}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
