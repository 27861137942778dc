"""tma_replay_add / tma_replay_sample / tma_egreedy_actions (csrc/tma_replay.hip, ABI 224) and three-mlagents_amd/replay_buffer.py on the device,
against the numpy restatement tests/_replay_ref.py.  Every comparison is exact: the kernels are copies plus one float64 sum in a fixed order.
Shapes are the smallest that reach each index path: rows of 21 floats (dwords, 16-row wave blocks, more than one workgroup at B = 67), rows of 8
(float4 where the bases are aligned, 64-row blocks) with Box actions, rows of 105 with 8 Box actions; a ring before and after its wrap."""
import ctypes as C

import numpy as np
import pytest
import torch

import _replay_ref as ref
from three_mlagents_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
R, N = 11, 3
GEOMS = {"d21_discrete": (21, 5, False), "d8_box": (8, 3, True)}      # name -> (D, A, Box actions)
FILLS = {"before_wrap": (7, 6), "after_wrap": (R, 4)}                  # name -> (size, newest): pos 7 of an unwrapped ring; pos 5 of a full one
F_CANARY, I_CANARY, TAIL = -12345.5, -77, 64
SEED = 2024


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# (row, env) of the flags: in rows 0 .. 6 (all an unwrapped ring holds) env 0 has a done, env 1 a time-out and a step that is both, env 2 nothing,
# so that windows of five end there by their length; the rows behind hold one more of each
TERMINATED, TRUNCATED = ((2, 0), (5, 1), (9, 1), (10, 2)), ((1, 1), (5, 1), (8, 0))


def _flag_plane(cells):
    plane = np.zeros((R, N), np.uint8)
    for row, env in cells:
        plane[row, env] = 1
    return plane


def _make_planes(D, A, cont, seed):
    rng = np.random.default_rng(seed)
    return dict(obs=rng.normal(size=(R, N, D)).astype(np.float32), next_obs=rng.normal(size=(R, N, D)).astype(np.float32),
                actions=rng.normal(size=(R, N, A)).astype(np.float32) if cont else rng.integers(0, A, (R, N)).astype(np.int32),
                rewards=rng.normal(size=(R, N)).astype(np.float32),
                terminated=_flag_plane(TERMINATED), truncated=_flag_plane(TRUNCATED))


@pytest.fixture(scope="module")
def rings():
    """name -> (numpy planes, device planes, tma_replay view): built once, never written"""
    out = {}
    for k, (name, (D, A, cont)) in enumerate(GEOMS.items()):
        host = _make_planes(D, A, cont, 100 + k)
        dev = {key: _dev(v) for key, v in host.items()}
        view = _lib.Replay(*(_lib.ptr(dev[key]) for key in ("obs", "next_obs", "actions", "rewards", "terminated", "truncated")), R, N, D, A, int(cont))
        out[name] = (host, dev, view)
    return out


OUTS = ("obs", "actions", "next_obs", "dones", "rewards", "discounts", "rows", "envs")


def _launch_sample(view, size, newest, n_step, gamma, seed, draw, B, want=OUTS, shift=0):
    """One tma_replay_sample call into canary-filled tensors with TAIL elements behind each output's end (`shift`: the outputs start that many
    elements into their tensors).  Returns name -> numpy array of the asked outputs, after checking that nothing outside them was written."""
    D, A, cont = view.obs_dim, view.act_dim, bool(view.continuous)
    width = {"obs": D, "next_obs": D, "actions": A if cont else 1}
    bufs = {}
    for name in want:
        is_int = name in ("rows", "envs") or (name == "actions" and not cont)
        n = B * width.get(name, 1)
        bufs[name] = torch.full((shift + n + TAIL,), I_CANARY if is_int else F_CANARY, dtype=torch.int32 if is_int else torch.float32, device=DEV)
    ptrs = [C.c_void_p(bufs[name].data_ptr() + 4 * shift) if name in bufs else None for name in OUTS]
    _lib.check(_lib.lib().tma_replay_sample(C.byref(view), size, newest, n_step, gamma, seed, draw, B, *ptrs, _lib.stream_ptr(DEV)))
    got = {}
    for name, t in bufs.items():
        h = t.cpu().numpy()
        n = B * width.get(name, 1)
        canary = h.dtype.type(I_CANARY if h.dtype == np.int32 else F_CANARY)
        assert (h[:shift] == canary).all() and (h[shift + n:] == canary).all(), f"{name}: written outside its {n} elements"
        body = h[shift:shift + n]
        got[name] = body.reshape(B, width[name]) if name in ("obs", "next_obs") or (name == "actions" and cont) else body
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _assert_equal_bits(got, want, names):
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(_bits(got[name]), _bits(want[name])), name


@pytest.mark.parametrize("n_step", [1, 3, 5])
@pytest.mark.parametrize("B", [1, 67, 256])
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_sample_equals_the_reference(rings, geom, fill, B, n_step):
    host, _, view = rings[geom]
    size, newest = FILLS[fill]
    gamma, draw = 0.97, 10 * n_step + B
    want = ref.sample(host, size, newest, n_step, gamma, SEED, draw, B)
    if B >= 67:  # (from the reference, not from the kernel) every way a window can end is in the batch
        assert set(want["why"]) == {"n", "done", "timeout", "head"}, sorted(set(want["why"]))
        assert want["rows"].min() == 0 and want["rows"].max() == size - 1 and set(want["envs"]) == {0, 1, 2}
    got = _launch_sample(view, size, newest, n_step, gamma, SEED, draw, B)
    _assert_equal_bits(got, want, OUTS)
    if n_step == 1:  # the plain buffer: the stored reward, terminated, gamma
        t, i = want["rows"], want["envs"]
        assert np.array_equal(_bits(got["rewards"]), _bits(host["rewards"][t, i])) and np.array_equal(got["dones"], host["terminated"][t, i].astype(np.float32))
        assert (got["discounts"] == np.float32(gamma)).all() and np.array_equal(_bits(got["next_obs"]), _bits(host["next_obs"][t, i]))


@pytest.mark.parametrize("want", [("next_obs", "rewards", "envs"), ("obs",), ("actions", "dones"), ("discounts", "rows"), ("rows",)])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_null_outputs_are_skipped(rings, geom, want):
    host, _, view = rings[geom]
    expect = ref.sample(host, R, 4, 3, 0.9, SEED, 3, 67)
    _assert_equal_bits(_launch_sample(view, R, 4, 3, 0.9, SEED, 3, 67, want=want), expect, want)


def test_rows_of_eight_floats_on_misaligned_outputs_take_the_dword_path(rings):
    """D = 8 moves as float4 only while every base is 16-byte aligned: outputs that start one float into their tensors must come out the same."""
    host, _, view = rings["d8_box"]
    expect = ref.sample(host, R, 4, 3, 0.9, SEED, 8, 256)
    _assert_equal_bits(_launch_sample(view, R, 4, 3, 0.9, SEED, 8, 256, shift=1), expect, OUTS)
    _assert_equal_bits(_launch_sample(view, R, 4, 3, 0.9, SEED, 8, 256, shift=4), expect, OUTS)


def test_the_same_draw_gives_the_same_bits_and_the_next_draw_others(rings):
    _, _, view = rings["d21_discrete"]
    a, b, c = (_launch_sample(view, R, 4, 3, 0.9, SEED, draw, 256) for draw in (5, 5, 6))
    _assert_equal_bits(a, b, OUTS)
    assert not np.array_equal(a["rows"], c["rows"]) and not np.array_equal(a["envs"], c["envs"]) and not np.array_equal(a["obs"], c["obs"])


# ---- add ---------------------------------------------------------------------------------------------------------------------------------
def _fake_steps(D, A, cont, n, seed):
    """n vector steps as step_device would return them (leading axis of one), flags on chosen envs: a done, a time-out, both at once"""
    rng = np.random.default_rng(seed)
    flags = {1: (0, 1, 0), 3: (2, 0, 1), 5: (1, 1, 1), 6: (0, 0, 1)}  # step -> (env, terminated, truncated)
    steps = []
    for k in range(n):
        term, trunc = np.zeros((1, N), np.uint8), np.zeros((1, N), np.uint8)
        if k in flags:
            env, term[0, env], trunc[0, env] = flags[k][0], flags[k][1], flags[k][2]
        steps.append(dict(actions=rng.normal(size=(N, A)).astype(np.float32) if cont else rng.integers(0, A, N).astype(np.int32),
                          obs=rng.normal(size=(1, N, D)).astype(np.float32), rew=rng.normal(size=(1, N)).astype(np.float32), term=term, trunc=trunc,
                          term_obs=rng.normal(size=(1, N, D)).astype(np.float32)))
    return steps


def _assert_ring(rb, ring):
    got = dict(obs=rb.observations, next_obs=rb.next_observations, actions=rb.actions, rewards=rb.rewards, terminated=rb.terminated, truncated=rb.truncated)
    for name, plane in ring.planes().items():
        assert np.array_equal(_bits(got[name].cpu().numpy()), _bits(plane)), name
    assert np.array_equal(_bits(rb.last_obs.cpu().numpy()), _bits(ring.last_obs))
    assert (rb.pos, rb.full, rb.size()) == (ring.pos, ring.full, ring.R if ring.full else ring.pos)


@pytest.mark.parametrize("D,A,cont", [(21, 5, False), (105, 8, True)])
def test_add_step_writes_the_ring_like_the_numpy_replay(D, A, cont):
    from three_mlagents_amd.replay_buffer import ReplayBuffer

    rows = 5
    rb = ReplayBuffer(rows * N, D, (A, cont), DEV, n_envs=N, n_steps=3, gamma=0.9, seed=SEED)
    ring = ref.Ring(rows, N, D, A, cont)
    assert (rb.buffer_size, rb.observations.shape, rb.actions.shape) == (rows, (rows, N, D), (rows, N, A) if cont else (rows, N))
    first = np.random.default_rng(1).normal(size=(N, D)).astype(np.float32)
    rb.start(_dev(first))
    ring.last_obs = first.copy()
    for k, s in enumerate(_fake_steps(D, A, cont, 7, 50 + D)):
        rb.add_step(_dev(s["actions"]), {key: _dev(s[key]) for key in ("obs", "rew", "term", "trunc", "term_obs")})
        ring.add(s["actions"], s["obs"][0], s["rew"][0], s["term"][0], s["trunc"][0], s["term_obs"][0])
        if k in (3, 6):  # before the wrap (pos 4) and after it
            _assert_ring(rb, ring)
    assert rb.pos == 2 and rb.full and rb.size() == rows
    # next_obs is the terminal row where a flag is set, the stepped row elsewhere -- from the inputs, not through the replay
    last = _fake_steps(D, A, cont, 7, 50 + D)[6]  # written to row 1: env 0 timed out
    assert np.array_equal(rb.next_observations[1, 0].cpu().numpy(), last["term_obs"][0, 0]) and np.array_equal(rb.next_observations[1, 1].cpu().numpy(), last["obs"][0, 1])
    # sample() through the Python surface: the draw counter advances per call, the windows are the reference's on the ring as it stands
    for draw in (0, 1):
        data, t, i = rb.sample(67, return_indices=True)
        want = ref.sample(ring.planes(), rows, 1, 3, 0.9, SEED, draw, 67)
        got = dict(zip(OUTS, (x.cpu().numpy() for x in (*data, t, i))))
        _assert_equal_bits(got, want, OUTS)
    assert type(data).__name__ == "ReplayBufferSamples" and data.observations.shape == (67, D) and data.dones.shape == (67,)
    rb.reset()
    assert (rb.pos, rb.full, rb.size()) == (0, False, 0)
    with pytest.raises(ValueError, match="empty"):
        rb.sample(4)


def test_add_with_the_callers_tensors_and_the_value_errors():
    from three_mlagents_amd.replay_buffer import ReplayBuffer

    D, A = 4, 5
    rb = ReplayBuffer(4 * N, D, A, DEV, n_envs=N)
    rng = np.random.default_rng(3)
    obs, nxt = rng.normal(size=(N, D)).astype(np.float32), rng.normal(size=(N, D)).astype(np.float32)
    act, rew = np.array([4, 0, 2]), rng.normal(size=N).astype(np.float32)
    term, trunc = np.array([True, False, False]), np.array([False, False, True])
    with pytest.raises(ValueError, match="empty"):
        rb.sample(1)
    rb.add(_dev(obs), _dev(nxt), _dev(act), _dev(rew), _dev(term), _dev(trunc))  # int64 actions, bool flags
    assert (rb.pos, rb.full, rb.size()) == (1, False, 1)
    assert np.array_equal(rb.observations[0].cpu().numpy(), obs) and np.array_equal(rb.next_observations[0].cpu().numpy(), nxt)  # next_obs as given
    assert rb.actions[0].tolist() == [4, 0, 2] and rb.terminated[0].tolist() == [1, 0, 0] and rb.truncated[0].tolist() == [0, 0, 1]
    assert np.array_equal(rb.rewards[0].cpu().numpy(), rew) and np.array_equal(rb.last_obs.cpu().numpy(), nxt)
    data = rb.sample(5)
    assert np.array_equal(data.rewards.cpu().numpy(), rew[ref.draw_indices(0, 0, 5, 1, N)[1]]) and (data.discounts == np.float32(0.99)).all()
    for bad in (0, -2):
        with pytest.raises(ValueError, match="batch_size"):
            rb.sample(bad)
    good = dict(obs=_dev(obs), next_obs=_dev(nxt), actions=_dev(act), rewards=_dev(rew), terminated=_dev(term), truncated=_dev(trunc))
    for key, wrong in (("obs", _dev(obs[:2])), ("obs", _dev(obs.astype(np.float64))), ("next_obs", _dev(nxt[:, :3])), ("actions", _dev(act.astype(np.float32))),
                       ("actions", _dev(act[:2])), ("rewards", _dev(rew.astype(np.float64))), ("terminated", _dev(term.astype(np.int32))),
                       ("truncated", _dev(trunc[:1])), ("obs", torch.from_numpy(obs))):
        with pytest.raises(ValueError, match=key):
            rb.add(**{**good, key: wrong})
    assert rb.pos == 1  # nothing was stored by the refused calls


# ---- epsilon-greedy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", [1, 67])
@pytest.mark.parametrize("A", [2, 5, 16])
def test_egreedy_equals_the_reference(A, n, eps):
    rng = np.random.default_rng(A * 100 + n)
    q = np.round(rng.normal(size=(n, A)), 1).astype(np.float32)  # one decimal: ties
    q[rng.random((n, A)) < 0.15] = np.nan
    q[rng.random((n, A)) < 0.05] = -np.inf
    if n > 1:
        q[3], q[4], q[5, 1:] = np.nan, 0.5, np.nan  # a row of NaNs, a row of equals, one number in front of NaNs
    offset = 0xFFFFFFF0 if n > 1 else 1000  # (env_offset + row wraps mod 2^32 inside the batch)
    want = ref.egreedy(q, eps, 9, 4, offset)
    if n > 1 and eps == 0.0:
        assert want[3] == 0 and want[4] == 0 and want[5] == 0
    out = torch.full((n + TAIL,), I_CANARY, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().tma_egreedy_actions(_lib.ptr(_dev(q)), n, A, eps, 9, 4, offset, _lib.ptr(out), _lib.stream_ptr(DEV)))
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], want) and (got[n:] == I_CANARY).all()


# ---- the pieces together ---------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """A vector env that keeps device copies of what each step returned (step_device's own tensors are overwritten by the next step)."""

    def __init__(self, env):
        self.env, self.engine, self.steps = env, env.engine, []

    def step_device(self, actions):
        out = self.env.step_device(actions)
        self.steps.append({"actions": actions.clone(), **{k: out[k][0].clone() for k in ("obs", "rew", "term", "trunc", "term_obs")}})
        return out


def test_collect_on_gridworld_then_one_td_step(monkeypatch):
    import torch.nn.functional as F

    from three_mlagents_amd.ppo import HipActorCriticPolicy
    from three_mlagents_amd.replay_buffer import ReplayBuffer
    from three_mlagents_amd.vec_env import HipVecEnv

    n_envs, T, eps = 3, 40, 0.3
    env = HipVecEnv("gridworld", n_envs, seed=1)
    policy = HipActorCriticPolicy(4, 5, False, 64, DEV, seed=3)
    rb = ReplayBuffer(64 * n_envs, 4, env.action_space, DEV, n_envs=n_envs, seed=11)
    rec = _Recorder(env)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with monkeypatch.context() as m, torch.cuda.stream(side):
        def no_host_copy(self, *a, **k):
            raise AssertionError("the collect loop copied a tensor to the host")

        m.setattr(torch.Tensor, "cpu", no_host_copy)
        first = rb.start(env.reset_device()).clone()
        rb.collect(rec, lambda obs: policy.head(obs)[0], T, eps)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert (rb.pos, rb.full, rb.size(), len(rec.steps)) == (T, False, T, T)
    obs, nxt = rb.observations[:T], rb.next_observations[:T]
    ended = (rb.terminated[:T] | rb.truncated[:T]).bool()
    assert torch.equal(obs[0], first)
    assert torch.equal(nxt[:-1][~ended[:-1]], obs[1:][~ended[:-1]])  # wherever no flag is set the next observation is the next row's observation
    for t, s in enumerate(rec.steps):
        assert torch.equal(rb.actions[t], s["actions"]) and torch.equal(rb.rewards[t], s["rew"])
        assert torch.equal(rb.terminated[t], s["term"]) and torch.equal(rb.truncated[t], s["trunc"])
        assert torch.equal(nxt[t], torch.where(ended[t][:, None], s["term_obs"], s["obs"]))  # the terminal row where a flag is set
        assert torch.equal(obs[t + 1] if t + 1 < T else rb.last_obs, s["obs"])
        q = policy.head(obs[t])[0].cpu().numpy()
        assert np.array_equal(rb.actions[t].cpu().numpy(), ref.egreedy(q, eps, 11, t, 0)), t
    # one DQN update on a sampled batch: Huber TD loss on policy.head, torch Adam on policy.parameters()
    params = policy.parameters()
    before = params[0].detach().clone()
    opt = torch.optim.Adam(params, lr=3e-4)
    data = rb.sample(64)
    with torch.no_grad():
        target = data.rewards + (1.0 - data.dones) * data.discounts * policy.head(data.next_observations)[0].max(dim=1).values
    q_taken = policy.head(data.observations)[0].gather(1, data.actions.long()[:, None]).squeeze(1)
    loss = F.smooth_l1_loss(q_taken, target)
    loss.backward()
    opt.step()
    after = params[0].detach()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(after).all()) and not torch.equal(after, before)
    env.close()
