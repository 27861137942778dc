"""policy_kwargs activation_fn (tma_policy_dims.activation, ABI 220) without a GPU: the field and its refusals, the routing of a ReLU layout to
the generic kernel families in the pure plan functions (csrc/tma_policy_plan.h) with every tanh plan unchanged, the constructor's refusals, the
two initialisation kwargs that belong to the ReLU recipe (log_std_init, ortho_init=False), the zip `data` round trip of the three at JSON level,
and tests/_relu_ref.py against plain torch modules."""
import ctypes as C
import json
import math
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _relu_ref  # noqa: E402
from three_mlagents_amd import _lib, sb3_format  # noqa: E402
from three_mlagents_amd.ppo import initial_state_dict, orthogonal_init, policy_dims  # noqa: E402

ROOT = os.path.dirname(HERE)
SHAPES = [(4, 64, 5, 0), (6, 256, 5, 0), (105, 256, 8, 1), (6, 128, 5, 0)]
PLAN_WHICH = {"fwd": 0, "grad": 1, "opt": 2, "opt_local": 3}  # TMA_PLAN_* of include/tma.h


def _ids():
    text = open(os.path.join(ROOT, "include", "tma.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\bTMA_DISPATCH_([A-Z0-9_]+)\s*=\s*(\d+)", text)}


def _name(v):
    return next(k for k, x in _ids().items() if x == v & 0xFF and k != "GRID_CAPPED")


def _planned(dims, which, n):
    i, g, b, l = C.c_int32(-1), C.c_int64(-1), C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().tma_debug_plan_dispatch(C.byref(dims), PLAN_WHICH[which], n, C.byref(i), C.byref(g), C.byref(b), C.byref(l))
    return rc, i.value, g.value, b.value, l.value


def test_abi_and_the_dims_field():
    assert _lib.lib().tma_version() >= 220
    assert _lib.PolicyDims._fields_[-1][0] == "activation"
    d = _lib.PolicyDims(4, 64, 5, 0, 0, -1)  # every positional construction from before the field: tanh
    assert d.activation == 0 and C.sizeof(_lib.PolicyDims) == 7 * 4
    header = open(os.path.join(ROOT, "include", "tma.h")).read()
    assert re.search(r"int activation;[^}]*\}\s*tma_policy_dims;", header, re.S), "activation must be the LAST member of tma_policy_dims"
    assert "#define TMA_ACT_TANH 0" in header and "#define TMA_ACT_RELU 1" in header


@pytest.mark.parametrize("D,H,A,cont", SHAPES)
def test_a_relu_layout_plans_the_generic_families_and_tanh_plans_are_unchanged(D, H, A, cont):
    tanh, explicit, relu = _lib.PolicyDims(D, H, A, cont, 0, -1), _lib.PolicyDims(D, H, A, cont, 0, -1, 0), _lib.PolicyDims(D, H, A, cont, 0, -1, 1)
    tuned = 0
    for n in (1, 48, 272, 4096, 131072):
        for which in PLAN_WHICH:
            assert _planned(tanh, which, n) == _planned(explicit, which, n)
        rc, fid, grid, block, lds = _planned(relu, "fwd", n)
        assert rc == _lib.TMA_OK and _name(fid).startswith("FWD_GENERIC_W") and grid >= 1 and block in (64, 128, 256) and 0 < lds <= 160 * 1024
        rc, gid, grid, block, lds = _planned(relu, "grad", n)
        assert rc == _lib.TMA_OK and _name(gid).startswith("GRAD_GENERIC_W") and grid >= 2 and 0 < lds <= 160 * 1024
        # the optimizer step behind a generic gradient: never the "local" kernels that read a slab reduction's partials
        rc, oid, *_ = _planned(relu, "opt_local", n)
        assert rc == _lib.TMA_OK and not _name(oid).startswith("OPT_LOCAL_"), _name(oid)
        assert _planned(relu, "opt", n)[:2] == _planned(tanh, "opt", n)[:2]
        tuned += not _name(_planned(tanh, "fwd", n)[1]).startswith("FWD_GENERIC") or not _name(_planned(tanh, "grad", n)[1]).startswith("GRAD_GENERIC")
    assert tuned >= 3  # these shapes DO have tuned tanh kernels: the condition above is not vacuous


def test_sizes_do_not_depend_on_the_activation():
    L = _lib.lib()
    for D, H, A, cont in SHAPES + [(4, 320, 3, 0)]:
        got = []
        for act in (0, 1):
            d = _lib.PolicyDims(D, H, A, cont, 0, -1, act)
            nt, ntot, offs = C.c_int64(0), C.c_int64(0), (C.c_int32 * 13)()
            assert L.tma_policy_param_count(C.byref(d), C.byref(nt), C.byref(ntot)) == _lib.TMA_OK
            assert L.tma_policy_param_offsets(C.byref(d), offs) == _lib.TMA_OK
            got.append((nt.value, ntot.value, list(offs), int(L.tma_ppo_workspace_bytes(C.byref(d))), int(L.tma_policy_vjp_workspace_bytes(C.byref(d), 77))))
        assert got[0] == got[1]
    # the H = 64 sample records feed the LDS-image gradient kernels only: none for a layout that never runs them
    assert L.tma_ppo_packed_floats(C.byref(_lib.PolicyDims(4, 64, 5, 0, 0, -1, 0)), 16, 8) > 0
    assert L.tma_ppo_packed_floats(C.byref(_lib.PolicyDims(4, 64, 5, 0, 0, -1, 1)), 16, 8) == 0


def test_rollout_norm_plan_is_per_step_for_relu():
    L = _lib.lib()
    ant, grid = 9, 1  # TMA_TASK_ANT, TMA_TASK_GRIDWORLD
    for task, dims in ((ant, (105, 256, 8, 1)), (grid, (None, 256, 5, 0))):
        D = dims[0] if dims[0] is not None else int(L.tma_task_obs_dim(task))
        for training in (0, 1):
            tanh = L.tma_rollout_norm_plan(task, C.byref(_lib.PolicyDims(D, *dims[1:], 0, -1, 0)), 8, training)
            relu = L.tma_rollout_norm_plan(task, C.byref(_lib.PolicyDims(D, *dims[1:], 0, -1, 1)), 8, training)
            assert tanh in (_lib.ROLLOUT_NORM_FUSED_DISC_F32, _lib.ROLLOUT_NORM_FUSED_CONT_F32) and relu == _lib.ROLLOUT_NORM_PER_STEP, (task, tanh, relu)


BAD = [(4, 64, 5, 0, 0, -1, 2), (4, 64, 5, 0, 0, -1, -1), (6, 256, 5, 0, 1, -1, 1), (6, 256, 5, 0, 2, -1, 1)]


@pytest.mark.parametrize("bad", BAD)
def test_bad_activations_are_refused_before_any_hip_call(bad):
    """host memory stands in for every buffer: the refusal comes back before anything is read or launched"""
    L, d, buf = _lib.lib(), _lib.PolicyDims(*bad), (C.c_float * 16)()
    nt, ntot = C.c_int64(0), C.c_int64(0)
    calls = {
        "tma_policy_param_count": lambda: L.tma_policy_param_count(C.byref(d), C.byref(nt), C.byref(ntot)),
        "tma_policy_head": lambda: L.tma_policy_head(buf, C.byref(d), buf, 16, buf, buf, None),
        "tma_policy_evaluate_actions_backward": lambda: L.tma_policy_evaluate_actions_backward(buf, C.byref(d), buf, buf, 16, buf, None, None, buf, buf, 64, None),
    }
    for name, call in calls.items():
        L.tma_policy_param_count(None, None, None)  # leaves ANOTHER message behind
        assert call() == _lib.TMA_ERR_INVALID, name
        msg = _lib.last_error()
        assert "activation" in msg, (name, msg)
        if bad[4] != 0:
            assert "bf16" in msg and "ReLU" in msg, msg  # says that the bf16 / bf16x3 kernels have no ReLU form
        with pytest.raises(ValueError):
            _lib.check(call())
    assert L.tma_rollout_norm_plan(1, C.byref(d), 8, 1) == -_lib.TMA_ERR_INVALID


def test_constructor_kwargs():
    assert sb3_format.parse_activation(None) == sb3_format.parse_activation(torch.nn.Tanh) == sb3_format.parse_activation("tanh") == "tanh"
    assert sb3_format.parse_activation(torch.nn.ReLU) == sb3_format.parse_activation("relu") == "relu"
    for other in (torch.nn.ELU, torch.nn.LeakyReLU, "gelu", torch.relu, 1):
        with pytest.raises(ValueError, match="Tanh.*ReLU"):
            sb3_format.parse_activation(other)
        with pytest.raises(ValueError, match="Tanh.*ReLU"):
            policy_dims(4, 64, 5, False, "f32", -1, other)
    for mfma in ("bf16", "bf16x3"):
        with pytest.raises(ValueError, match="f32"):
            policy_dims(6, 256, 5, False, mfma, -1, torch.nn.ReLU)
        assert policy_dims(6, 256, 5, False, mfma, -1, torch.nn.Tanh).activation == 0
    for act, want in ((torch.nn.ReLU, 1), ("relu", 1), (torch.nn.Tanh, 0), ("tanh", 0), (None, 0)):
        d = policy_dims(4, 64, 5, False, "f32", 0, act)
        nt, ntot = C.c_int64(0), C.c_int64(0)
        assert d.activation == want and d.device == 0 and _lib.lib().tma_policy_param_count(C.byref(d), C.byref(nt), C.byref(ntot)) == _lib.TMA_OK
    with pytest.raises(ValueError):
        policy_dims(4, 64, 5, False, "f16")


def test_initialisation_kwargs_on_the_cpu():
    D, H, A = 6, 64, 4
    ortho = orthogonal_init(D, H, A, True, 3)
    same = initial_state_dict(D, H, A, True, 3)
    assert all(torch.equal(ortho[k], same[k]) for k in ortho)  # the defaults are the initialisation there has always been
    filled = initial_state_dict(D, H, A, True, 3, log_std_init=-2.0)
    assert torch.equal(filled["log_std"], torch.full((A,), -2.0)) and all(torch.equal(ortho[k], filled[k]) for k in ortho if k != "log_std")
    assert "log_std" not in initial_state_dict(D, H, A, False, 3, log_std_init=-2.0)
    a, b, c = (initial_state_dict(D, H, A, True, s, log_std_init=-1.0, ortho_init=False) for s in (3, 3, 4))
    assert set(a) == set(ortho) and torch.equal(a["log_std"], torch.full((A,), -1.0))
    for k, w in a.items():
        assert w.shape == ortho[k].shape and torch.equal(w, b[k])  # deterministic per seed
        if k == "log_std":
            continue
        assert not torch.equal(w, c[k]) and not torch.equal(w, ortho[k])  # another seed, another draw; not the orthogonal one
        fan_in = a[k.replace("bias", "weight")].shape[1]
        bound = 1.0 / math.sqrt(fan_in)
        assert float(w.abs().max()) <= bound and bool((w != 0).all())  # biases too: torch's nn.Linear default
        assert w.numel() < 16 or float(w.abs().max()) > 0.5 * bound  # ... and the bound is the scale of the draw, not merely above it


def test_zip_data_round_trip_of_the_three_kwargs():
    # SB3's defaults leave data["policy_kwargs"] what it has always been
    assert sb3_format.policy_kwargs_data(64) == {"net_arch": [64, 64]}
    pk = sb3_format.policy_kwargs_data(256, "relu", -2.0, False)
    assert pk == {"net_arch": [256, 256], "activation_fn": "<class 'torch.nn.modules.activation.ReLU'>", "log_std_init": -2.0, "ortho_init": False}
    assert pk["activation_fn"] == str(torch.nn.ReLU) and sb3_format.activation_repr("tanh") == str(torch.nn.Tanh)
    data = json.loads(json.dumps({"policy_kwargs": pk, "tma": {"activation": "relu"}}))
    assert sb3_format.policy_kwargs_from_data(data) == {"activation_fn": "relu", "log_std_init": -2.0, "ortho_init": False}
    # a zip SB3 wrote: the blob, and the str() of each member beside it; no "tma"
    sb3 = {"policy_kwargs": {":type:": "<class 'dict'>", ":serialized:": "gAWV", "activation_fn": str(torch.nn.ReLU), "net_arch": "{'pi': [256, 256], 'vf': [256, 256]}",
                             "log_std_init": "-2", "ortho_init": "False"}}
    assert sb3_format.policy_kwargs_from_data(sb3) == {"activation_fn": "relu", "log_std_init": 0.0, "ortho_init": True}  # (strings are not values: the weights come from the zip)
    sb3["policy_kwargs"]["activation_fn"] = str(torch.nn.Tanh)
    assert sb3_format.policy_kwargs_from_data(sb3)["activation_fn"] == "tanh"
    # from before the entry existed, or a blob alone: tanh
    for old in ({}, {"policy_kwargs": {"net_arch": [64, 64]}}, {"policy_kwargs": "gAWV"}, {"policy_kwargs": None, "tma": {"mfma_dtype": "f32"}}):
        assert sb3_format.policy_kwargs_from_data(old) == {"activation_fn": "tanh", "log_std_init": 0.0, "ortho_init": True}
    for unknown in (str(torch.nn.ELU), str(torch.nn.LeakyReLU), "<class 'torch.nn.modules.activation.ReLU6'>"):
        with pytest.raises(ValueError, match="Tanh.*ReLU"):
            sb3_format.policy_kwargs_from_data({"policy_kwargs": {"activation_fn": unknown}})
    with pytest.raises(ValueError):
        sb3_format.policy_kwargs_from_data({"tma": {"activation": "elu"}})


@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 64, 4, True)])
def test_the_relu_reference_is_the_plain_torch_net(D, H, A, cont):
    sd = {k: v.double() for k, v in _relu_ref.policy_sd(D, H, A, cont).items()}
    n = 33
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(n, D, generator=g, dtype=torch.float64)

    def net(base):
        seq = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU()).double()
        seq.requires_grad_(False)
        seq.load_state_dict({"0.weight": sd[_relu_ref.KEYS[base]], "0.bias": sd[_relu_ref.KEYS[base + 1]], "2.weight": sd[_relu_ref.KEYS[base + 2]],
                             "2.bias": sd[_relu_ref.KEYS[base + 3]]})
        return seq

    lin = torch.nn.functional.linear
    out_ref, v_ref = lin(net(0)(obs), sd["action_net.weight"], sd["action_net.bias"]), lin(net(6)(obs), sd["value_net.weight"], sd["value_net.bias"]).flatten()
    out, v = _relu_ref.forward(sd, obs, "relu")
    assert float((out - out_ref).abs().max()) <= 1e-12 and float((v - v_ref).abs().max()) <= 1e-12
    if cont:
        actions = out_ref + 0.3 * torch.randn(n, A, generator=g, dtype=torch.float64)
        dist = torch.distributions.Normal(out_ref, sd["log_std"].exp().expand_as(out_ref))
        lp_ref, ent_ref = dist.log_prob(actions).sum(1), dist.entropy().sum(1)
    else:
        actions = torch.randint(0, A, (n,), generator=g, dtype=torch.int32)
        dist = torch.distributions.Categorical(logits=out_ref)
        lp_ref, ent_ref = dist.log_prob(actions.long()), dist.entropy()
    v2, lp, ent = _relu_ref.evaluate_actions(sd, obs, actions, "relu")
    assert torch.equal(v2, v) and float((lp - lp_ref).abs().max()) <= 1e-12 and float((ent - ent_ref).abs().max()) <= 1e-12
    # the tanh branch is oracle/sb3_ref.py's function, and a different one
    from oracle import sb3_ref

    out_t, v_t = _relu_ref.forward(sd, obs, "tanh")
    assert torch.equal(out_t, sb3_ref.forward(sd, obs)[0]) and torch.equal(v_t, sb3_ref.forward(sd, obs)[1]) and float((v_t - v).abs().max()) > 1e-3
    # the pre-activations are the ones the masks are taken from, and the screened rows are clear of the kink
    z = _relu_ref.preactivations(sd, obs)
    assert len(z) == 4 and all(t.shape == (n, H) for t in z)
    assert torch.equal(torch.relu(lin(torch.relu(z[0]), sd[_relu_ref.KEYS[2]], sd[_relu_ref.KEYS[3]])), net(0)(obs))
    clear = _relu_ref.clear_obs(sd, D, 77, seed=2)
    assert clear.shape == (77, D) and clear.dtype == torch.float32 and _relu_ref.kink_margin(sd, clear) >= _relu_ref.KINK_MARGIN
    assert torch.equal(clear, _relu_ref.clear_obs(sd, D, 77, seed=2))
