"""Data-parallel path on the one-GPU box.

* RCCL itself: `dist.init_from_env(backend="nccl")` at world size 1 (a one-rank communicator) + all-reduce of a gradient-sized tensor.
* Two ranks on ONE GPU (gloo backend carrying the device tensors; RCCL needs one device per rank): the complete data-parallel PPO
  path -- env sharding by env_offset, the per-epoch all-reduce of the minibatch advantage sums, the per-minibatch gradient
  all-reduce, 1/world scaling inside the Adam kernel -- for the three kernel families (GridWorld 64x64 f32; the BASELINE configs[3]
  shape Push 256x256; configs[4] Crawler-shape 256x256 bf16), asserting that the replicas stay bit-identical and that every rank
  normalised with the same GLOBAL advantage statistics.  On the 8-GPU node the same code runs with backend nccl (`bench.py --gpus N`).
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _nccl_single(port, q):
    os.environ.update({"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                       "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    from three_mlagents_amd import dist

    rk, lr, ws = dist.init_from_env(backend="nccl", single_rank_group=True)
    import torch.distributed as td

    g = torch.arange(9350, dtype=torch.float32, device="cuda:0")  # the 64x64 policy's flat gradient size
    dist.allreduce_sum_(g)  # world 1: the helper skips the collective ...
    td.all_reduce(g)        # ... so drive RCCL directly as PPO.train does
    torch.cuda.synchronize()
    q.put((rk, ws, td.get_backend(), float(g.double().sum().item()), dist.allreduce_max_float(3.5, device="cuda:0")))
    td.destroy_process_group()


@pytest.mark.timeout(300)
def test_rccl_backend_initialises_and_all_reduces():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_single, args=(_free_port(), q))
    p.start()
    rk, ws, backend, total, mx = q.get(timeout=240)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert (rk, ws, backend) == (0, 1, "nccl") and total == float(sum(range(9350))) and mx == 3.5


def _native_comm_single(port, q):
    """World size 1, real RCCL twice in one process: torch.distributed's communicator (nccl backend) and the library's own (tma_comm_*)."""
    os.environ.update({"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                       "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    from three_mlagents_amd import _lib, dist

    dist.init_from_env(backend="nccl", single_rank_group=True)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    comm = dist.NativeComm(dev)
    g32 = torch.arange(9350, dtype=torch.float32, device=dev) * 0.5
    g64 = torch.arange(64, dtype=torch.float64, device=dev) + 0.25
    want32, want64 = g32.clone(), g64.clone()
    comm.timing(3)
    side = torch.cuda.Stream(dev)  # the collective runs on the stream it is given, ordered with the kernels queued there
    with torch.cuda.stream(side):
        g32.mul_(2.0)
        comm.all_reduce_(g32, _lib.stream_ptr(dev))
        g32.mul_(0.5)
        comm.all_reduce_(g64, _lib.stream_ptr(dev))
    side.synchronize()
    us, calls = comm.pop_timing()
    ok_collectives = bool(torch.equal(g32, want32) and torch.equal(g64, want64)) and len(us) == 2 and calls == 2 and all(u > 0 for u in us)
    # the PPO data-parallel epoch loop with the native communicator (TMA_DP_PATH: the multi-GPU loop at world size 1) against the callback
    # path into torch.distributed and against the single-GPU epoch call: same parameters, moments and statistics, bit for bit
    from three_mlagents_amd.harness import make_vector_env
    from three_mlagents_amd.ppo import PPO

    def run(mode):
        for k in ("TMA_DP_PATH", "TMA_NATIVE_RCCL", "TMA_NO_NATIVE_RCCL"):
            os.environ.pop(k, None)
        if mode != "local":
            os.environ["TMA_DP_PATH"] = "1"
        if mode == "native":
            os.environ["TMA_NATIVE_RCCL"] = "1"
        env = make_vector_env("gridworld", n_envs=256, seed=5)
        m = PPO("MlpPolicy", env, n_steps=64, batch_size=2048, n_epochs=3, seed=5, policy_kwargs={"net_arch": [64, 64]})
        if mode == "native":
            assert m._native_comm is not None
            m._native_comm.timing(8)
        m.collect_rollouts()
        m.train()
        st = m.pop_train_stats()
        tim = m.dp_timing_collect() if mode == "native" else None
        out = (m.policy.params.cpu(), m.exp_avg.cpu(), m.exp_avg_sq.cpu(), st, tim, m._native_comm is not None)
        env.close()
        return out

    p_n, m_n, v_n, s_n, tim, used_n = run("native")
    p_c, m_c, v_c, s_c, _, used_c = run("callback")
    p_l, m_l, v_l, s_l, _, _ = run("local")
    same = bool(torch.equal(p_n, p_c) and torch.equal(m_n, m_c) and torch.equal(v_n, v_c)) and all(s_n[k] == s_c[k] for k in s_c)
    near_local = bool(torch.allclose(p_n, p_l, rtol=0, atol=1e-6))
    q.put((ok_collectives, used_n, used_c, same, near_local, tim["grad_allreduce_us"]["calls_timed"], tim["grad_allreduce_us"]["allreduces_issued"],
           tim["grad_allreduce_us"]["path"]))
    comm.close()
    import torch.distributed as td

    td.destroy_process_group()


@pytest.mark.timeout(300)
def test_native_rccl_communicator_at_world_size_one():
    """include/tma.h tma_comm_*: the library's own RCCL communicator (ncclCommInitRank from a unique id, ncclAllReduce on the caller's stream)
    next to torch.distributed's in one process; the data-parallel epoch loop with tma_comm_allreduce_cb as its collective -- no Python call
    per minibatch -- gives the bits of the callback path (3 epochs x 8 minibatches = 24 all-reduces issued natively).  One GPU: world size 1;
    more ranks need more devices (RCCL allows one rank per device), which only the driver's scaling run has."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_native_comm_single, args=(_free_port(), q))
    p.start()
    ok, used_n, used_c, same, near_local, timed, issued, path = q.get(timeout=240)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert ok and used_n and not used_c and same and near_local
    assert timed == 8 and issued == 2 + 24 and path.startswith("native")  # (2: the construction-time self-check, one f32 and one f64 sum)


def _worker(rank, world, port, q, task, hidden, mfma, N, T, p2p=False):
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": "0", "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                       "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    os.environ.pop("TMA_P2P", None)
    if p2p:
        os.environ["TMA_P2P"] = "1"
    from three_mlagents_amd import dist

    dist.init_from_env(backend="gloo")
    torch.cuda.set_device(0)
    from three_mlagents_amd.harness import make_vector_env
    from three_mlagents_amd.ppo import PPO

    env = make_vector_env(task, n_envs=N, seed=1, env_offset=rank * N)
    model = PPO("MlpPolicy", env, n_steps=T, batch_size=N * T // 2, n_epochs=2, seed=1, policy_kwargs={"net_arch": [hidden, hidden], "mfma_dtype": mfma})
    assert model.world_size == world and model.rank == rank
    first_obs = env.engine.reset().cpu()
    model._last_obs_valid = False
    model.learn(2 * world * N * T)
    adv = model.buf["advantages"].double().cpu().numpy()
    if p2p:  # every collective of the run went through the peer exchange: 2 probes + per iteration 2 epochs x (1 advantage-sum + 2 gradient) all-reduces
        st = model._native_comm.p2p_status()
        assert model._native_comm is not None and not model._native_comm.has_rccl and st["enabled"] and not st["timed_out"], st
        assert st["calls"] == 2 + 2 * 2 * (1 + 2), st
    else:
        assert model._native_comm is None
    q.put((rank, model.policy.params[: model.policy.n_trainable].cpu().numpy(), first_obs.numpy(), model.num_timesteps,
           model._adv_sums.cpu().numpy(), float(adv.sum()), float((adv * adv).sum())))  # numpy: pickled by value
    env.close()
    dist.barrier()
    import torch.distributed as td

    td.destroy_process_group()


def _run_two_ranks(task, hidden, mfma, N, T, p2p=False, world=2):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, task, hidden, mfma, N, T, p2p)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=400) for _ in range(world)), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.timeout(600)
@pytest.mark.parametrize("task,hidden,mfma,N,T", [("gridworld", 64, "f32", 256, 64), ("push", 256, "f32", 256, 64), ("crawler", 256, "bf16", 128, 32),
                                                   ("gridworld", 256, "bf16x3", 256, 64)])  # (bf16x3: minibatches of 8 192 samples take the three-term split kernel)
def test_two_ranks_one_gpu_replicas_stay_identical(task, hidden, mfma, N, T):
    (r0, p0, o0, t0, s0, a0, q0), (r1, p1, o1, t1, s1, a1, q1) = _run_two_ranks(task, hidden, mfma, N, T)
    assert np.array_equal(p0, p1)  # same all-reduced gradient, same global advantage statistics, same Adam state -> bit-identical replicas
    assert not np.array_equal(o0, o1)  # the shards really are different envs (global indices 0..N-1 vs N..2N-1)
    assert t0 == t1 == 2 * 2 * N * T  # num_timesteps counts the whole job
    # both ranks hold the same all-reduced per-minibatch (sum, sumsq) pairs, and they add up to the two shards' last-rollout advantages
    assert np.array_equal(s0, s1) and s0.shape == (4,)
    assert np.isclose(s0[0] + s0[2], a0 + a1, rtol=1e-9, atol=1e-6) and np.isclose(s0[1] + s0[3], q0 + q1, rtol=1e-9, atol=1e-6)
    if task != "gridworld":
        return
    # the shards are the two halves of one 2N-env engine
    from three_mlagents_amd.vec_env import HipEnvEngine

    big = HipEnvEngine(task, 2 * N, seed=1)
    ob = big.reset().cpu().numpy()
    assert np.array_equal(ob[:N], o0) and np.array_equal(ob[N:], o1)
    # a single-rank run on the same data takes different steps (it sees half of each global batch)
    from three_mlagents_amd.harness import make_vector_env
    from three_mlagents_amd.ppo import PPO

    env = make_vector_env(task, n_envs=N, seed=1)
    solo = PPO("MlpPolicy", env, n_steps=T, batch_size=N * T // 2, n_epochs=2, seed=1, policy_kwargs={"net_arch": [64, 64]})
    solo.learn(2 * N * T)
    assert not np.array_equal(solo.policy.params[: solo.policy.n_trainable].cpu().numpy(), p0)


@pytest.mark.timeout(600)
def test_two_ranks_one_gpu_peer_exchange_equals_the_gloo_collectives():
    """The peer exchange (include/tma.h tma_comm_p2p_*) carrying EVERY collective of a two-rank run -- both ranks on this one GPU, their inboxes
    mapped into each other through HIP IPC handles, the gradient sum fused into slab_reduce_kernel (stores into both inboxes) and the
    sum-of-squares pass (reads its own inbox), the f64 advantage sums through the stand-alone push / pull kernels -- against the same run over
    gloo: at two ranks a + b is the same float whichever side adds, so parameters and advantage sums must agree bit for bit.
    (Two PROCESSES is as far as one GPU goes: a receiver kernel spins on words a sender kernel of another process stores, and from four
    processes on the scheduler no longer keeps every process's queues resident -- measured round 6: 120 s time-outs at world 4 / 8, with
    the default four hardware queues per process and with one.  The world sizes of a node run in ONE process, a stream per rank:
    test_peer_exchange_protocol_at_node_world_sizes_in_one_process.)"""
    if os.environ.get("TMA_NO_NATIVE_RCCL"):
        pytest.skip("TMA_NO_NATIVE_RCCL keeps every collective on the torch.distributed callback: no native communicator to carry the exchange")
    a = _run_two_ranks("gridworld", 64, "f32", 256, 64, p2p=True)
    b = _run_two_ranks("gridworld", 64, "f32", 256, 64, p2p=False)
    assert np.array_equal(a[0][1], a[1][1])  # replicas identical
    assert np.array_equal(a[0][1], b[0][1]) and np.array_equal(a[0][4], b[0][4])  # and identical to the run over gloo


def _p2p_raw_worker(rank, world, port, q, mode):
    """tma_comm_* with the peer exchange only (no RCCL side), driven directly."""
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": "0", "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                       "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    if mode == "timeout":
        os.environ["TMA_P2P_TIMEOUT_S"] = "0.5"
    import time

    from three_mlagents_amd import _lib, dist

    dist.init_from_env(backend="gloo")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    comm = dist.NativeComm(dev, rccl=False)
    comm.p2p_setup(16384)
    comm.p2p_enable(True)
    sp = _lib.stream_ptr(dev)
    out = {}
    if mode == "sums":
        gen = torch.Generator(device="cpu").manual_seed(7)  # same stream of test vectors on every rank
        ok, n_calls = True, 0
        for it in range(300):
            n = int(torch.randint(1, 16385, (1,), generator=gen).item())
            base = torch.randn(world, n, generator=gen, dtype=torch.float32)
            if it % 3 == 2:  # f64 messages (two words per element)
                n = min(n, 8192)
                x = base[rank, :n].double().to(dev) * 1.0000001
                want = base[0, :n].double() * 1.0000001
                for r in range(1, world):
                    want = want + base[r, :n].double() * 1.0000001
            else:
                x = base[rank].to(dev)
                want = base[0].clone()
                for r in range(1, world):
                    want = want + base[r]  # rank order
            if (it + rank) % 7 == 0:
                time.sleep(0.003)  # skew: one rank arrives late, the other's receiver waits
            comm.all_reduce_(x, sp)
            n_calls += 1
            if it % 10 == 0:  # (mostly back to back without a host sync: the two-parity argument is what keeps consecutive exchanges apart)
                ok = ok and bool(torch.equal(x.cpu(), want))
        torch.cuda.synchronize()
        ok = ok and bool(torch.equal(x.cpu(), want))
        st = comm.p2p_status()
        out = {"ok": ok, "calls": st["calls"], "n": n_calls, "timed_out": st["timed_out"]}
        dist.barrier()
    else:  # rank 1 never sends its words for the second exchange: rank 0's receiver gives up after TMA_P2P_TIMEOUT_S and says so
        x = torch.ones(1000, dtype=torch.float32, device=dev)
        comm.all_reduce_(x, sp)
        torch.cuda.synchronize()
        first = bool((x == float(world)).all())
        err = ""
        if rank == 0:
            t0 = time.perf_counter()
            comm.all_reduce_(x, sp)
            torch.cuda.synchronize()
            waited = time.perf_counter() - t0
            try:
                comm.all_reduce_(x, sp)
            except RuntimeError as exc:
                err = str(exc)
            out = {"first": first, "waited": waited, "timed_out": comm.p2p_status()["timed_out"], "err": err}
        else:
            out = {"first": first}
        dist.barrier()
    q.put((rank, out))
    dist.barrier()
    comm.close()
    import torch.distributed as td

    td.destroy_process_group()


def _run_p2p_raw(mode, world=2):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_p2p_raw_worker, args=(r, world, port, q, mode)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.timeout(400)
def test_peer_exchange_sums_in_rank_order_under_skew():
    """300 consecutive all-reduces of random lengths (f32 and f64) between two processes on this GPU, most of them without a host
    synchronisation in between and with one rank arriving late every few calls: every checked result equals the rank-ordered sum bit for bit."""
    res = _run_p2p_raw("sums")
    for r in (0, 1):
        assert res[r]["ok"] and res[r]["calls"] == res[r]["n"] == 300 and not res[r]["timed_out"], res


_NODE_WORLDS_PROGRAM = r"""
import ctypes as C, json, os, sys
import torch
sys.path.insert(0, sys.argv[1])
from three_mlagents_amd import _lib
L = _lib.lib()
dev = torch.device("cuda", 0)
out = {}
for world in (4, 8):
    comms = []
    for r in range(world):
        h = C.c_void_p()
        _lib.check(L.tma_comm_create_p2p(world, r, 0, C.byref(h)))
        ticket = (C.c_ubyte * 128)()
        _lib.check(L.tma_comm_p2p_prepare(h, 16384, ticket))
        comms.append(h)
    arr = (C.c_void_p * world)(*[c.value for c in comms])
    for h in comms:
        _lib.check(L.tma_comm_p2p_attach_local(h, arr))
        _lib.check(L.tma_comm_p2p_enable(h, 1))
    streams = [torch.cuda.Stream(device=dev) for _ in range(world)]
    gen = torch.Generator(device="cpu").manual_seed(11)
    ok, n_calls = True, 0
    for it in range(200):
        n = int(torch.randint(1, 16385, (1,), generator=gen).item())
        base = torch.randn(world, n, generator=gen, dtype=torch.float32)
        f64 = it % 3 == 2
        if f64:
            n = min(n, 8192)
            xs = [(base[r, :n].double() * 1.0000001).to(dev) for r in range(world)]
            want = base[0, :n].double() * 1.0000001
            for r in range(1, world):
                want = want + base[r, :n].double() * 1.0000001
        else:
            xs = [base[r].to(dev) for r in range(world)]
            want = base[0].clone()
            for r in range(1, world):
                want = want + base[r]  # rank order
        torch.cuda.current_stream(dev).synchronize()  # (the uploads ran on the default stream)
        order = [(it * 3 + k) % world for k in range(world)]  # the rank that enqueues first rotates: late and early arrivers on every slot
        for r in order:
            _lib.check(L.tma_comm_allreduce(comms[r], C.c_void_p(xs[r].data_ptr()), n, 1 if f64 else 0, C.c_void_p(streams[r].cuda_stream)))
        n_calls += 1
        if it % 10 == 0 or it == 199:  # mostly back to back without a host sync: the two-parity argument keeps consecutive exchanges apart
            for st in streams:
                st.synchronize()
            ok = ok and all(bool(torch.equal(x.cpu(), want)) for x in xs)
    st = []
    for h in comms:
        en, calls, bad, words = C.c_int(0), C.c_int64(0), C.c_int(0), C.c_int64(0)
        _lib.check(L.tma_comm_p2p_status(h, C.byref(en), C.byref(calls), C.byref(bad), C.byref(words)))
        st.append((en.value, calls.value, bad.value))
        _lib.check(L.tma_comm_destroy(h))
    out[str(world)] = {"ok": ok, "n": n_calls, "status": st}
print("RESULT " + json.dumps(out))
"""


@pytest.mark.timeout(400)
def test_peer_exchange_protocol_at_node_world_sizes_in_one_process():
    """The exchange at the world sizes a node runs at -- 4 and P2P_MAX_WORLD = 8 ranks -- on one GPU: `world` communicators in ONE process
    (tma_comm_p2p_attach_local: the inboxes wired directly), every rank on a stream of its own (GPU_MAX_HW_QUEUES = 16: a receiver spins on
    words another rank's sender stores, so no two ranks may share a hardware queue), 200 consecutive all-reduces of random lengths (f32 and
    f64) enqueued in a rotating rank order, most of them without a host synchronisation in between: the two-parity slots and the rank-ordered
    sums hold bit for bit on every rank, nothing times out.  (What one GPU cannot show is the xGMI transport itself.)"""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16", TMA_P2P_TIMEOUT_S="20", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", _NODE_WORLDS_PROGRAM, ROOT], capture_output=True, text=True, timeout=380, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    import json

    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for world in (4, 8):
        d = res[str(world)]
        assert d["ok"] and d["n"] == 200, d
        assert all(en == 1 and calls == 200 and bad == 0 for en, calls, bad in d["status"]), d


@pytest.mark.timeout(400)
def test_peer_exchange_receiver_gives_up_instead_of_spinning_for_ever():
    res = _run_p2p_raw("timeout")
    assert res[0]["first"] and res[1]["first"]
    assert res[0]["timed_out"] and 0.4 < res[0]["waited"] < 30.0 and "timed out" in res[0]["err"], res[0]


def _p2p_world1(q):
    """World size 1: the fused exchange (slab_reduce_kernel -> own inbox -> grad_pull_sumsq64_kernel) against the plain data-parallel chain."""
    os.environ.update({"HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    from three_mlagents_amd.harness import make_vector_env
    from three_mlagents_amd.ppo import PPO

    def run(p2p, fuse=True):
        for k in ("TMA_P2P", "TMA_P2P_NO_FUSE", "TMA_NATIVE_RCCL"):
            os.environ.pop(k, None)
        os.environ["TMA_DP_PATH"] = "1"
        os.environ["TMA_NATIVE_RCCL"] = "1"
        if p2p:
            os.environ["TMA_P2P"] = "1"
        env = make_vector_env("gridworld", n_envs=256, seed=5)
        m = PPO("MlpPolicy", env, n_steps=64, batch_size=2048, n_epochs=3, seed=5, policy_kwargs={"net_arch": [64, 64]})
        assert m._native_comm is not None and m._native_comm.p2p_enabled == p2p
        m._native_comm.timing(8)
        m.collect_rollouts()
        m.train()
        tim = m.dp_timing_collect()
        st = m._native_comm.p2p_status()
        out = (m.policy.params.cpu(), m.exp_avg.cpu(), m.exp_avg_sq.cpu(), st, tim["grad_allreduce_us"])
        env.close()
        return out

    a, b = run(True), run(False)
    same = all(bool(torch.equal(x, y)) for x, y in zip(a[:3], b[:3]))
    q.put((same, a[3], a[4]["path"], a[4]["calls_timed"], b[3]))


def _p2p_contest_world1(q):
    """TMA_P2P=auto at world size 1 with the RCCL side present: the start-up procedure a node runs (inbox, ticket, attach, exact-sum check,
    timing contest against ncclAllReduce, agreement) end to end, then a training step on whichever path won."""
    os.environ.update({"HSA_ENABLE_IPC_MODE_LEGACY": "0", "TMA_DP_PATH": "1", "TMA_NATIVE_RCCL": "1", "TMA_P2P": "auto"})
    from three_mlagents_amd.harness import make_vector_env
    from three_mlagents_amd.ppo import PPO

    env = make_vector_env("gridworld", n_envs=256, seed=5)
    m = PPO("MlpPolicy", env, n_steps=64, batch_size=2048, n_epochs=2, seed=5, policy_kwargs={"net_arch": [64, 64]})
    c = m._native_comm
    note, on, rccl = (c.p2p_note, c.p2p_enabled, c.has_rccl) if c is not None else ("", None, None)
    m.collect_rollouts()
    m.train()
    st = c.p2p_status() if c is not None else {}
    finite = bool(torch.isfinite(m.policy.params).all())
    env.close()
    q.put((c is not None, rccl, on, note, st, finite))


@pytest.mark.timeout(300)
def test_peer_exchange_start_up_contest_runs_end_to_end():
    if os.environ.get("TMA_NO_NATIVE_RCCL"):
        pytest.skip("TMA_NO_NATIVE_RCCL keeps every collective on the torch.distributed callback: no native communicator to carry the exchange")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_p2p_contest_world1, args=(q,))
    p.start()
    have, rccl, on, note, st, finite = q.get(timeout=240)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert have and rccl and finite and not st["timed_out"]
    # the contest ran and left its two figures; which side won at ONE rank (where RCCL has nothing to do) is not asserted
    assert note.startswith(("on:", "off:")) and "us per" in note and "RCCL's" in note, note
    assert st["enabled"] == on and (st["calls"] >= 2 + 45 if not on else st["calls"] >= 2 + 45 + 16)


@pytest.mark.timeout(300)
def test_fused_peer_exchange_at_world_size_one_changes_no_bit():
    if os.environ.get("TMA_NO_NATIVE_RCCL"):
        pytest.skip("TMA_NO_NATIVE_RCCL keeps every collective on the torch.distributed callback: no native communicator to carry the exchange")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_p2p_world1, args=(q,))
    p.start()
    same, st, path, timed, st_off = q.get(timeout=240)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert same and st["enabled"] and not st["timed_out"] and st["calls"] == 2 + 24 and "peer exchange" in path and timed == 8
    assert not st_off["enabled"] and st_off["calls"] == 0


def test_bench_gpus_2_fails_cleanly_on_a_one_gpu_box():
    if torch.cuda.device_count() >= 2:
        pytest.skip("multi-GPU box: `bench.py --gpus 2` would really run")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=280)
    assert r.returncode == 2 and "needs 2 visible GPUs" in r.stderr and r.stdout.strip() == ""


@pytest.mark.timeout(900)
@pytest.mark.parametrize("p2p,gpus", [(False, 2), (True, 2), (False, 8)])
def test_bench_two_ranks_end_to_end_on_one_gpu(p2p, gpus):
    """The whole `bench.py --gpus 2` rank program (barriers, max-over-ranks timing, sharded envs, advantage-sum and gradient all-reduces,
    rank-0-only roofline legs and JSON line) under torch.distributed.run with two ranks -- on this one-GPU box over gloo with both ranks on
    device 0 (test hooks TMA_DIST_BACKEND / TMA_BENCH_ONE_DEVICE); on a multi-GPU node the same program runs one rank per GPU over RCCL."""
    import json

    env = dict(os.environ, TMA_DIST_BACKEND="gloo", TMA_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if p2p and os.environ.get("TMA_NO_NATIVE_RCCL"):
        pytest.skip("TMA_NO_NATIVE_RCCL keeps every collective on the torch.distributed callback")
    env.pop("TMA_P2P", None)
    if p2p:  # the collectives through the peer exchange (the communicator's only path under gloo) instead of the torch.distributed callback
        env["TMA_P2P"] = "1"
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    # (gpus = 8: the driver's `--gpus 8` rank program, one JSON line with n_gpus 8 and a dp_timing object -- the first real 8-GPU run must not
    #  fail on plumbing)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "1", "--warmup", "1", "--n-envs", "512", "--n-steps", "64", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=860, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 prints ONE JSON line
    d = json.loads(lines[0])
    assert d["n_gpus"] == gpus and d["scaling"] == "weak" and d["config"]["envs_per_gpu"] == 512 and d["value"] > 0
    assert d["value"] == pytest.approx(gpus * 512 * 64 / (d["ms_per_step"] * 1e-3), rel=1e-6)  # whole-job env-steps of all ranks / max-over-ranks time
    assert "roofline" in d and "cpu_baseline" not in d and "extra_configs" not in d  # CPU baseline and extras are N = 1 legs
    # what the first real multi-GPU run will be read by: per-collective timings and every rank's own rollout / update split
    t = d["dp_timing"]
    assert t["backend"] == "gloo" and len(t["per_rank_rollout_ms"]) == len(t["per_rank_update_ms"]) == gpus
    assert t["grad_allreduces_per_iteration"] == 10 * 32 and t["adv_sums_allreduces_per_iteration"] == 10
    assert t["grad_allreduce"]["calls_timed"] == 64 and t["grad_allreduce"]["median_us"] > 0 and t["grad_allreduce"]["bytes"] == 9350 * 4
    if p2p:
        assert t["allreduce_path"] == "native peer exchange" and t["peer_exchange"].startswith("on"), t
    else:
        assert t["adv_sums_allreduce"]["calls_timed"] == 20 and t["adv_sums_allreduce"]["median_us"] > 0 and t["adv_sums_allreduce"]["bytes"] == 32 * 16
    assert all(x > 0 for x in t["per_rank_rollout_ms"] + t["per_rank_update_ms"])
