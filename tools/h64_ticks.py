#!/usr/bin/env python3
"""Per-phase cycle breakdown of the H = 64 gradient kernel's tile chain (diagnostic build libtma_hip_ticks.so, wave 0 of block pair 0), and
how the two waves of each SIMD of that block pair share the loop (TMA_H64_NO_PAIR_BALANCE=1: without the pair balance; TMA_H64_PAIR_PRIO=2 / 3
and TMA_H64_PAIR_LEAD=1: the variants of it that only this build has).  A second argument `loop` stops behind the tile loop's figures.
Run: make -C three-mlagents_amd/csrc libtma_hip_ticks.so && TMA_LIB_PATH=three-mlagents_amd/csrc/libtma_hip_ticks.so python tools/h64_ticks.py"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from three_mlagents_amd import _lib
from three_mlagents_amd.ppo import PPO
from three_mlagents_amd.harness import make_vector_env

B = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
env = make_vector_env("gridworld", n_envs=4096, seed=1)
m = PPO("MlpPolicy", env, n_steps=max(1, B // 4096), batch_size=B, n_epochs=1, seed=1, policy_kwargs={"net_arch": [64, 64]})
m.collect_rollouts()
mb = _lib.Minibatch(None, 1, 0, 0, B)
L = _lib.lib()
def grad():
    _lib.check(L.tma_ppo_minibatch_grad(_lib.ptr(m.policy.params), C.byref(m.policy.dims), C.byref(m._rollout_view), C.byref(mb), C.byref(m._hp),
                                        _lib.ptr(m.grad), _lib.ptr(m.workspace), m._stream()))
for _ in range(3):
    grad()
out = (C.c_ulonglong * 64)()  # [0..31]: the tile phases and launch sums of both nets; [32..63]: the launch edges (g_h64_edge_ticks)
L.tma_debug_h64_ticks.argtypes = [C.c_void_p, C.c_int]
L.tma_debug_h64_ticks(None, 1)
if hasattr(L, "tma_debug_h64_pair_ticks"):
    L.tma_debug_h64_pair_ticks.argtypes = [C.c_void_p, C.c_int]
    L.tma_debug_h64_pair_ticks(None, 1)
def edges(n):
    """The prologue split at its waits and barriers (cumulative, wave 0) and each wave's loop-end clock against wave 0's: block pair 0, per launch."""
    for net, o in (("pi", 32), ("vf", 48)):
        pro = [round(out[o + i] / n) for i in range(5)]
        ends = [round(C.c_longlong(out[o + 8 + w]).value / n) for w in range(8)]
        print("   ", net, "prologue, cycles since the kernel's start: first tile's records issued", pro[0], "| coefficient published (first barrier)", pro[2], "| layer-2 block updated (optimizer state consumed)", pro[1],
              "| image stores issued", pro[3], "| advantage statistics published", pro[4])
        print("   ", net, "loop end of waves 0..7 minus wave 0's:", ends, "-- waves 0-3 mean", round(sum(ends[:4]) / 4), "waves 4-7 mean", round(sum(ends[4:]) / 4), "latest", max(ends))
reps = 10
for _ in range(reps):
    grad()
L.tma_debug_h64_ticks(out, 0)
# the order of the small weight gradients in the headline kernel, from TMA_H64_SMALL_SERIAL as csrc/tma_h64.hip reads it: unset both folded,
# A = dW1 under dW2 alone, B = dW3 under the dh1 chain alone, anything else = each in a phase of its own
sw = os.environ.get("TMA_H64_SMALL_SERIAL")
w1_fold, w3_fold = sw is None or sw[:1] == "A", sw is None or sw[:1] == "B"
names = ["L1", "tanh1+st h1+L2", "tanh2+head+st h2", "loss+st dz3", "dh2" if w3_fold else "dh2+dW3", "dz2+st+dh1|dW3" if w3_fold else "dz2+st+dh1",
         "dW2 reads+dz1+st" if w1_fold else "dW2+dz1+st", "dW2|dW1" if w1_fold else "dW1", "", "", "", "", "", "", "", "loop top"]
tiles = max(1, reps * (B // 16) // (min(128, (B // 16 + 7) // 8) * 8))
for net, o in (("pi", 0), ("vf", 16)):
    v = [out[o + i] / tiles for i in range(16)]
    print(net, "cycles per tile:", {n: round(x) for n, x in zip(names, v) if n}, "sum", round(sum(v[:10]) + v[15]))
    loop_c, loop_rt, pro, epi = (out[o + i] / reps for i in (10, 11, 12, 13))
    # H64_TICK adds (clock at the stamp) - (clock after the PREVIOUS stamp's bookkeeping): what a stamp itself costs between its two clock
    # reads (lane 0's read-add-write of the global counter) belongs to no phase.  The phase sum is therefore SHORTER than the loop, and a
    # pipe-busy fraction must be taken over the loop time per tile (or from SQ counters), never over the sum.
    per_tile = out[o + 10] / tiles
    print("    loop per tile", round(per_tile), "cycles; the phase sum leaves out", round(per_tile - (sum(v[:10]) + v[15])), "cycles a tile spent inside the stamps")
    print("    of the epilogue,", round(out[o + 14] / reps), "cycles are the wait for the block's slowest wave")
    print("    per launch: loop", round(loop_c), "cycles =", round(loop_rt / 100, 1), "us (100 MHz counter) -> clock", round(loop_c / max(loop_rt, 1) * 0.1, 2),
          "GHz; prologue", round(pro), "cycles, epilogue", round(epi), "cycles")

def pairs(pt, n):
    """How the two waves of a SIMD (w and w + 4) of block pair 0 share their loop, per launch: (a) the loop clock at which the one that left
    first did, (b) its partner's completed tiles at that moment, (c) the partner's cycles per tile up to its last tile top with company,
    (d) its cycles per tile from its first tile top alone to its loop's end.  SIMD 0 hosts the stamped wave 0: read the other three."""
    for net, o in (("pi", 0), ("vf", 64)):
        w = [[pt[o + 8 * k + i] for i in range(8)] for k in range(8)]
        print("   ", net, "loop end of waves 0..7 since wave 0's loop start:", [round((C.c_longlong(w[k][7]).value + w[k][0]) / n) for k in range(8)],
              "tiles a wave and launch:", [round(w[k][6] / n, 2) for k in range(8)])
        for k in range(4):
            first, last = (k, k + 4) if w[k][0] + C.c_longlong(w[k][7]).value <= w[k + 4][0] + C.c_longlong(w[k + 4][7]).value else (k + 4, k)
            f, l = w[first], w[last]
            print("   ", net, "waves", (k, k + 4), "-- (a) wave", first, "left at", round(f[0] / n), "of its loop, (b) wave", last, "had completed", round(f[1] / n, 2),
                  "tiles, (c) wave", last, "with company:", round(l[2] / max(l[3], 1)), "cycles a tile over", round(l[3] / n, 2), "tiles, (d) alone:",
                  round(l[4] / max(l[5], 1)), "cycles a tile over", round(l[5] / n, 2), "tiles; it left at", round(l[0] / n),
                  "-- wave", first, "itself:", round(f[2] / max(f[3], 1)), "cycles a tile")
if hasattr(L, "tma_debug_h64_pair_ticks"):
    pt = (C.c_ulonglong * 128)()
    L.tma_debug_h64_pair_ticks(pt, 1)
    print("pair balance", "off (TMA_H64_NO_PAIR_BALANCE)" if os.environ.get("TMA_H64_NO_PAIR_BALANCE", "")[:1] == "1" else
          "on, priority %s%s" % (os.environ.get("TMA_H64_PAIR_PRIO", "1"), " beyond one tile's lead" if os.environ.get("TMA_H64_PAIR_LEAD") else ""))
    pairs(pt, reps)
if sys.argv[2:3] == ["loop"]:  # (python tools/h64_ticks.py 131072 loop: the tile loop alone)
    sys.exit(0)

# ---- the value blocks' tail phase (the next minibatch's advantage pre-pass, carried by the launch): two epochs of two minibatches of B rows
# through tma_ppo_train_epochs_local -- four gradient launches a call, three of them carrying a pre-pass
if hasattr(L, "tma_debug_h64_tail_ticks"):
    env.close()
    env = make_vector_env("gridworld", n_envs=4096, seed=1)
    m = PPO("MlpPolicy", env, n_steps=max(1, 2 * B // 4096), batch_size=B, n_epochs=2, seed=1, policy_kwargs={"net_arch": [64, 64]})
    m.collect_rollouts()
    L.tma_debug_h64_tail_ticks.argtypes = [C.c_void_p, C.c_int]
    tail = C.c_ulonglong(0)
    for switch in (None, "1"):
        os.environ.pop("TMA_NO_PREP_FOLD", None)
        if switch:
            os.environ["TMA_NO_PREP_FOLD"] = switch
        m.train()
        L.tma_debug_h64_ticks(None, 1)
        L.tma_debug_h64_tail_ticks(None, 1)
        for _ in range(reps):
            m.train()
        L.tma_debug_h64_ticks(out, 0)
        L.tma_debug_h64_tail_ticks(C.byref(tail), 0)
        n, carrying = reps * 4, reps * 3
        print("train(), pre-passes", "in launches of their own (TMA_NO_PREP_FOLD=1)" if switch else "carried by the gradient launches", "-- cycles per launch:")
        for net, o in (("pi", 0), ("vf", 16)):
            pro, loop_c, epi = (out[o + i] / n for i in (12, 10, 13))
            print("   ", net, "prologue", round(pro), "loop", round(loop_c), "epilogue", round(epi), "sum", round(pro + loop_c + epi),
                  "-- of the epilogue,", round(out[o + 14] / n), "the wait for the block's slowest wave")
        edges(n)
        if not switch:
            print("    vf: end of the loop -> end of the tail phase", round(tail.value / carrying), "cycles per carrying launch: the phase itself",
                  round(tail.value / carrying - out[16 + 13] / n))
    os.environ.pop("TMA_NO_PREP_FOLD", None)
