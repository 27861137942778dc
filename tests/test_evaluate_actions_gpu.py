"""HipActorCriticPolicy.evaluate_actions / tma_policy_evaluate_actions on the GPU: SB3's ActorCriticPolicy.evaluate_actions (values, log-probability
of GIVEN actions, entropy) as a further MODE of the three forward kernel templates.

  * against the torch-CPU restatement (oracle/sb3_ref.py evaluate_actions), at the tolerances tests/test_ppo_gpu.py holds the forward pass to;
  * the same bits as `act` -- values always, the log-probability of the actions `act` drew -- for every forward family, also above the grid caps;
  * NULL outputs, out-of-range Discrete actions;
  * the rollout audit: what the fused rollout kernels wrote into the buffer against what the launch-path forward gives for those rows.
"""
import ctypes as C

import pytest
import torch

from oracle import sb3_ref

pytestmark = pytest.mark.gpu

V_TOL = dict(rtol=1e-5, atol=1e-5)   # values (tests/test_ppo_gpu.py test_forward_matches_torch_reference)
LP_TOL = dict(rtol=1e-5, atol=5e-5)  # log-probability and entropy (same test, the stochastic branch)

CONFIGS = [(4, 64, 5, False), (6, 256, 5, False), (21, 64, 3, False), (172, 256, 20, True), (4, 128, 5, False),  # tests/test_ppo_gpu.py CONFIGS
           (105, 256, 8, True), (45, 256, 3, False)]
# the H = 64 image path beyond 4 observations: DT = 6 (Ball3D), a runtime width with one zero-padded column (Bicycle) and four full k-steps (Glider)
H64_MORE = [(6, 64, 5, False), (7, 64, 3, False), (16, 64, 5, False)]
CONFIGS += H64_MORE

# (D, H, A, continuous, mfma_dtype, TMA_DISPATCH_FWD_* family the shape runs in)
FAMILIES = [
    (4, 64, 5, False, "f32", "FWD_H64"),
    (4, 128, 5, False, "f32", "FWD_F32_NTW2_DISCRETE"), (6, 256, 5, False, "f32", "FWD_F32_NTW4_DISCRETE"), (105, 256, 8, True, "f32", "FWD_F32_NTW4_BOX"),
    (6, 256, 5, False, "bf16", "FWD_BF16_NTW4_DISCRETE"), (105, 256, 8, True, "bf16", "FWD_BF16_NTW4_BOX"),
    (4, 320, 3, False, "f32", "FWD_GENERIC"), (6, 64, 4, True, "f32", "FWD_GENERIC"),
    (6, 256, 5, False, "bf16x3", "FWD_F32_NTW4_DISCRETE"),  # mfma_dtype 2: the exact-f32 kernels, as `act`
] + [(*c, "f32", "FWD_H64") for c in H64_MORE]
# one run per family above its grid cap (wide: 4096 groups of 32 rows; generic: 8192 blocks of 4 tiles of 16 rows; H = 64: 2048 blocks)
CAPPED = [
    (4, 64, 5, False, "f32", 131072 + 17, "FWD_H64"),
    (6, 128, 3, True, "f32", 32 * 4096 + 17, "FWD_F32_NTW2_BOX|GRID_CAPPED"), (6, 256, 5, False, "f32", 32 * 4096 + 17, "FWD_F32_NTW4_DISCRETE|GRID_CAPPED"),
    (6, 256, 5, False, "bf16", 32 * 4096 + 17, "FWD_BF16_NTW4_DISCRETE|GRID_CAPPED"),
    (4, 64, 2, True, "f32", 16 * 4 * 8192 + 17, "FWD_GENERIC_W4|GRID_CAPPED"), (21, 64, 3, False, "f32", 16 * 4 * 8192 + 17, "FWD_GENERIC_W4|GRID_CAPPED"),
] + [(*c, "f32", 131072 + 17, "FWD_H64") for c in H64_MORE]


def _policy(D, H, A, cont, seed=5, mfma="f32"):
    """tests/test_ppo_gpu.py _policy: heads made non-trivial (gain 0.01 init gives almost uniform logits), non-zero biases and log_std."""
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    pol = HipActorCriticPolicy(D, A, cont, H, torch.device("cuda", 0), seed=seed, mfma_dtype=mfma)
    sd = pol.state_dict()
    if cont:
        sd["log_std"] = torch.linspace(-0.7, 0.3, A)
    g = torch.Generator().manual_seed(seed)
    sd["action_net.weight"] = sd["action_net.weight"] * 40 + 0.05 * torch.randn(sd["action_net.weight"].shape, generator=g)
    sd["action_net.bias"] = 0.1 * torch.randn(sd["action_net.bias"].shape, generator=g)
    for k in list(sd):
        if k.endswith("bias") and k != "action_net.bias":
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    pol.load_state_dict(sd)
    return pol, sd


def _cpu_actions(sd, obs, A, cont, seed):
    """Actions drawn on the CPU: uniform for Discrete, mean + sigma * z with |z| <= 3 for Box."""
    g = torch.Generator().manual_seed(seed)
    n = obs.shape[0]
    if not cont:
        return torch.randint(0, A, (n,), generator=g, dtype=torch.int32)
    mean, _ = sb3_ref.forward(sd, obs)
    z = torch.randn(n, A, generator=g).clamp(-3.0, 3.0)
    return (mean + sd["log_std"].exp() * z).to(torch.float32)


def _last_fwd_dispatch():
    from three_mlagents_amd import _lib

    f, g, o = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    _lib.check(_lib.lib().tma_debug_last_dispatch(C.byref(f), C.byref(g), C.byref(o)))
    return f.value


def _dispatch_value(name):
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tma.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bTMA_DISPATCH_([A-Z0-9_]+)\s*=\s*(\d+)", text)}
    v = 0
    for part in name.split("|"):
        v |= ids[part]
    return v


def _ulps(a: torch.Tensor, b: torch.Tensor) -> int:
    """Largest distance of two float32 tensors in units in the last place (ordered-integer distance of the bit patterns)."""
    def key(x):
        i = x.detach().cpu().contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)

    return int((key(a) - key(b)).abs().max())


@pytest.mark.parametrize("D,H,A,cont", CONFIGS)
def test_matches_the_torch_reference(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    n = 101
    obs = torch.randn(n, D, generator=torch.Generator().manual_seed(1))
    actions = _cpu_actions(sd, obs, A, cont, seed=2)
    v_ref, lp_ref, ent_ref = sb3_ref.evaluate_actions(sd, obs, actions)
    v, lp, ent = pol.evaluate_actions(obs.cuda(), actions.cuda())
    assert v.shape == lp.shape == ent.shape == (n,) and v.is_cuda and lp.is_cuda and ent.is_cuda
    print(f"{D}x{H}x{A}{'C' if cont else 'D'}: max |dv| {float((v.cpu() - v_ref).abs().max()):.3g}  max |dlogp| {float((lp.cpu() - lp_ref).abs().max()):.3g}"
          f"  max |dent| {float((ent.cpu() - ent_ref).abs().max()):.3g}")
    assert torch.allclose(v.cpu(), v_ref, **V_TOL), float((v.cpu() - v_ref).abs().max())
    assert torch.allclose(lp.cpu(), lp_ref, **LP_TOL), float((lp.cpu() - lp_ref).abs().max())
    assert torch.allclose(ent.cpu(), ent_ref, **LP_TOL), float((ent.cpu() - ent_ref).abs().max())


def _check_same_bits_as_act(pol, cont, obs_d, expect_dispatch):
    a, v_act, lp_act = pol.act(obs_d, rng_seed=9, rng_step=3, deterministic=False)
    d_act = _last_fwd_dispatch()
    v, lp, ent = pol.evaluate_actions(obs_d, a)
    d_eval = _last_fwd_dispatch()
    assert d_eval == d_act, (d_eval, d_act)  # the family `act` ran, under its existing id
    if "|" in expect_dispatch or not expect_dispatch.endswith("GENERIC"):
        assert d_eval == _dispatch_value(expect_dispatch), (d_eval, expect_dispatch)
    assert torch.equal(v, v_act)
    if cont:  # (`act` may form the Box log-probability from its noise)
        assert torch.allclose(lp, lp_act, **LP_TOL), float((lp - lp_act).abs().max())
    else:
        assert torch.equal(lp, lp_act)
    assert bool(torch.isfinite(ent).all())
    a2, v_det, _ = pol.forward(obs_d, deterministic=True)  # SB3's name for `act`
    a3, v_det3, _ = pol.act(obs_d, deterministic=True)
    assert torch.equal(a2, a3) and torch.equal(v_det, v_det3) and torch.equal(v_det, v)
    return a, v, lp, ent


@pytest.mark.parametrize("D,H,A,cont,mfma,family", FAMILIES, ids=[f"{f[0]}x{f[1]}x{f[2]}{'C' if f[3] else 'D'}-{f[4]}" for f in FAMILIES])
def test_same_bits_as_act_and_null_outputs(D, H, A, cont, mfma, family):
    from three_mlagents_amd import _lib

    pol, _ = _policy(D, H, A, cont, mfma=mfma)
    for n in (1, 17, 101, 1000):
        obs_d = torch.randn(n, D, generator=torch.Generator().manual_seed(n)).cuda()
        a, v, lp, ent = _check_same_bits_as_act(pol, cont, obs_d, family)
        # any output passed as NULL leaves the others unchanged (buffers pre-filled with a sentinel: a skipped output must stay untouched)
        L = _lib.lib()
        for mask in range(1, 7):
            outs = [torch.full((n,), -12345.0, device="cuda") for _ in range(3)]
            ptrs = [_lib.ptr(outs[i]) if mask & (1 << i) else None for i in range(3)]
            _lib.check(L.tma_policy_evaluate_actions(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs_d), _lib.ptr(a), n, *ptrs, _lib.stream_ptr()))
            for i, full in enumerate((v, lp, ent)):
                if mask & (1 << i):
                    assert torch.equal(outs[i], full), (n, mask, i)
                else:
                    assert bool((outs[i] == -12345.0).all()), (n, mask, i)
        with pytest.raises(ValueError):
            _lib.check(L.tma_policy_evaluate_actions(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs_d), _lib.ptr(a), n, None, None, None,
                                                     _lib.stream_ptr()))


@pytest.mark.parametrize("D,H,A,cont,mfma,n,dispatch", CAPPED, ids=[f"{c[0]}x{c[1]}x{c[2]}{'C' if c[3] else 'D'}-{c[4]}-{c[5]}" for c in CAPPED])
def test_same_bits_as_act_above_the_grid_caps(D, H, A, cont, mfma, n, dispatch):
    pol, _ = _policy(D, H, A, cont, mfma=mfma)
    obs_d = torch.randn(n, D, generator=torch.Generator().manual_seed(3)).cuda()
    _check_same_bits_as_act(pol, cont, obs_d, dispatch)


@pytest.mark.parametrize("D,H,A,mfma", [(4, 64, 5, "f32"), (4, 64, 16, "f32"), (6, 256, 5, "f32"), (6, 256, 5, "bf16"), (4, 320, 3, "f32"), (21, 64, 2, "f32")]
                         + [(*c[:3], "f32") for c in H64_MORE])
def test_out_of_range_discrete_actions_give_nan_and_touch_nothing_else(D, H, A, mfma):
    pol, _ = _policy(D, H, A, False, mfma=mfma)
    n = 203
    obs_d = torch.randn(n, D, generator=torch.Generator().manual_seed(4)).cuda()
    a = torch.randint(0, A, (n,), generator=torch.Generator().manual_seed(5), dtype=torch.int32).cuda()
    v0, lp0, ent0 = pol.evaluate_actions(obs_d, a)
    bad = a.clone()
    rows_lo, rows_hi = [0, 16, 37, n - 1], [5, 31, 32, 100]
    bad[rows_lo] = -1
    bad[rows_hi] = A
    bad[50], bad[51] = 2 ** 31 - 1, -2 ** 31  # (a value that would be far outside any buffer if it were ever used as an index)
    v1, lp1, ent1 = pol.evaluate_actions(obs_d, bad)
    nan_rows = torch.zeros(n, dtype=torch.bool, device="cuda")
    nan_rows[rows_lo + rows_hi + [50, 51]] = True
    assert bool(torch.isnan(lp1[nan_rows]).all())
    assert torch.equal(lp1[~nan_rows], lp0[~nan_rows]) and bool(torch.isfinite(lp0).all())
    assert torch.equal(v1, v0) and torch.equal(ent1, ent0)


def test_python_surface_checks_rows_dtypes_and_shapes():
    pol, _ = _policy(6, 256, 5, False)
    box, _ = _policy(8, 128, 3, True)
    obs = torch.randn(10, 6).cuda()
    with pytest.raises(ValueError):
        pol.evaluate_actions(obs, torch.zeros(10, dtype=torch.int64, device="cuda"))  # SB3's long actions: not the buffer's dtype
    with pytest.raises(ValueError):
        pol.evaluate_actions(obs, torch.zeros(10, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        pol.evaluate_actions(obs, torch.zeros(9, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        pol.evaluate_actions(obs, torch.zeros(10, 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        pol.evaluate_actions(torch.randn(10, 7).cuda(), torch.zeros(10, dtype=torch.int32, device="cuda"))  # the row check of `act`
    with pytest.raises(ValueError):
        pol.evaluate_actions(obs, [0] * 10)
    bobs = torch.randn(10, 8).cuda()
    with pytest.raises(ValueError):
        box.evaluate_actions(bobs, torch.zeros(10, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        box.evaluate_actions(bobs, torch.zeros(10, 3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        box.evaluate_actions(bobs, torch.zeros(10, 4, dtype=torch.float32, device="cuda"))
    v, lp, ent = box.evaluate_actions(bobs, torch.zeros(10, 3, dtype=torch.float32, device="cuda"))
    assert v.shape == lp.shape == ent.shape == (10,)


# (task, hidden, mfma_dtype, n_envs, family): one collect_rollouts() of PPO, then the launch-path forward over the buffer's rows
AUDIT = [("gridworld", 64, "f32", 64, "h64"), ("ball3d", 256, "f32", 64, "wide f32 discrete"), ("ball3d", 256, "bf16", 64, "wide bf16 discrete"),
         ("ant", 256, "f32", 64, "wide f32 box")]


@pytest.mark.parametrize("task,hidden,mfma,n_envs,family", AUDIT, ids=[f"{a[0]}-{a[1]}-{a[2]}" for a in AUDIT])
def test_rollout_audit(task, hidden, mfma, n_envs, family):
    """The contract DESIGN.md section 6 relies on (`approx_kl == 0` in the first epoch): the values and log-probabilities a rollout kernel wrote are
    the ones the policy gives for those rows.  The forward tolerances are asserted first; the largest distance in ulps is printed.  Measured on
    MI355X: 0 ulps for values and log-probabilities on every case of every family (H = 64 fused chunk, 256-wide f32 and bf16 Discrete chunks, the
    f32 Box chunk with its batched value pass), so equality is asserted for all of them."""
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv

    T = 32
    env = HipVecEnv(task, n_envs, seed=3)
    try:
        model = PPO("MlpPolicy", env, n_steps=T, batch_size=512, n_epochs=1, seed=7, policy_kwargs={"net_arch": [hidden, hidden], "mfma_dtype": mfma})
        assert model.collect_rollouts()
        buf = model.buf
        obs = buf["obs"][:T].flatten(0, 1)
        actions = buf["actions"].flatten(0, 1)
        v, lp, _ = model.policy.evaluate_actions(obs, actions)
        bv, blp = buf["values"].flatten(), buf["log_probs"].flatten()
        uv, ulp = _ulps(v, bv), _ulps(lp, blp)
        print(f"rollout audit {task} {hidden}x{hidden} {mfma} ({family}): max ulps values {uv}, log_probs {ulp}; "
              f"max |dv| {float((v - bv).abs().max()):.3g}, max |dlogp| {float((lp - blp).abs().max()):.3g}")
        assert torch.allclose(v, bv, **V_TOL), float((v - bv).abs().max())
        assert torch.allclose(lp, blp, **LP_TOL), float((lp - blp).abs().max())
        assert torch.equal(v, bv) and torch.equal(lp, blp), (uv, ulp)
    finally:
        env.close()
