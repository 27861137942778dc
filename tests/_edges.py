"""The committed list of branch labels of tests/golden/{bicycle,brickbreak,glider}_edges.npz (tools/gen_golden.py `edges`) and what each label
promises about its rows.  `check_coverage` reads the FIXTURE only -- no oracle, no kernel -- so an edges file regenerated with a branch
missing, or with a row that no longer takes the branch its label names, fails on the CPU before anything is compared with it.

A label maps to (reward, terminated, truncated[, claim]); reward None means "the task's ordinary shaped reward", i.e. none of its
terminal constants.  `claim` names a check of the recorded state in CLAIMS below.  Every label has one row per action of the task, a
label ending in `_a<k>` one row with action k."""
import numpy as np

N_ACT = {"bicycle": 3, "brickbreak": 3, "glider": 5}
SDIM = {"bicycle": 10, "brickbreak": 46, "glider": 14}
STEPS_AT = {"bicycle": 9, "brickbreak": 5, "glider": 13}
LIMIT = {"bicycle": 2000, "brickbreak": 2000, "glider": 4000}
TERMINAL_REWARDS = {"bicycle": (-10.0, 50.0), "brickbreak": (-1.0, 10.0), "glider": (-50.0,)}

C, T_, L_ = (False, False), (True, False), (False, True)  # continues / terminated / truncated (the adapter never sets both)

EXPECT = {
    "bicycle": {
        "goal_inside": (50.0, *T_), "goal_outside": (None, *C),
        "fall_pos": (-10.0, *T_), "fall_neg": (-10.0, *T_), "upright_pos": (None, *C), "upright_neg": (None, *C),
        "goal_and_fall": (50.0, *T_), "goal_and_upright": (50.0, *T_), "fall_and_goal_outside": (-10.0, *T_),
        "delta_clip_hi": (None, *C, "delta_hi"), "delta_clip_lo": (None, *C, "delta_lo"),
        "delta_below_clip_hi": (None, *C, "delta_free"), "delta_above_clip_lo": (None, *C, "delta_free"),
        "delta_clip_hi_by_a2": (None, *C, "delta_hi"), "delta_clip_lo_by_a0": (None, *C, "delta_lo"),
        "delta_near_clip_hi_a1": (None, *C, "delta_free"), "delta_near_clip_lo_a1": (None, *C, "delta_free"),
        "steps1998_continue": (None, *C), "steps1998_fall": (-10.0, *T_), "steps1998_goal": (50.0, *T_),
        # at the limit the adapter reports a truncation, never a termination, and keeps the reward
        "steps1999_continue": (None, *L_), "steps1999_fall": (-10.0, *L_), "steps1999_goal": (50.0, *L_),
        "steps2000_continue": (None, *L_), "steps2000_fall": (-10.0, *L_), "steps2000_goal": (50.0, *L_),
        "on_goal_exact": (50.0, *T_, "dist_zero"), "on_goal_1e-9": (50.0, *T_, "dist_tiny"),
        # start states of multi-step replays: `pre_<x>` steps onto the one state of `any_<x>`, whose outcome is the same under every action
        "pre_goal_a1": (None, *C), "any_goal": (50.0, *T_), "pre_fall_a1": (None, *C), "any_fall": (-10.0, *T_),
        "pre_continue_a1": (None, *C), "any_continue": (None, *C),
    },
    "brickbreak": {
        "win_last_brick": (10.0, *T_, "no_bricks"), "win_and_lost": (10.0, *T_, "ball_below"), "win_no_bricks_midair": (10.0, *T_, "no_bricks"),
        "two_bricks_left_hit_one": (1.0, *C, "one_brick_gone"),
        "wall_left_on": (0.0, *C, "vx_flipped"), "wall_left_off": (0.0, *C, "vx_kept"),
        "wall_right_on": (0.0, *C, "vx_flipped"), "wall_right_off": (0.0, *C, "vx_kept"),
        "ceiling_on": (0.0, *C, "vy_flipped"), "ceiling_off": (0.0, *C, "vy_kept"),
        "paddle_band_on": (0.1, *C, "vy_flipped"), "paddle_band_off": (0.0, *C, "vy_kept"),
        "paddle_left_on": (0.1, *C, "vy_flipped"), "paddle_left_off": (0.0, *C, "vy_kept"),
        "paddle_right_on": (0.1, *C, "vy_flipped"), "paddle_right_off": (0.0, *C, "vy_kept"),
        "paddle_ball_rising": (0.0, *C, "vy_kept"), "paddle_ball_level": (0.0, *C, "vy_kept"),
        "lost_on": (0.0, *C), "lost_off": (-1.0, *T_, "ball_below"), "paddle_hit_and_lost": (-1.0, *T_, "vy_flipped"),
        "paddle_clip_lo": (0.0, *C, "paddle_4"), "paddle_clip_hi": (0.0, *C, "paddle_36"),
        "paddle_at_lo": (0.0, *C, "paddle_in_range"), "paddle_at_hi": (0.0, *C, "paddle_in_range"),
        "paddle_lands_on_lo_a0": (0.0, *C, "paddle_4"), "paddle_lands_on_hi_a2": (0.0, *C, "paddle_36"),
        "brick_bottom_on": (1.0, *C, "brick_0_3"), "brick_bottom_off": (0.0, *C, "bricks_kept"),
        "brick_top_on": (1.0, *C, "brick_4_3"), "brick_top_off": (0.0, *C, "bricks_kept"),
        "xedge_both": (1.0, *C, "brick_2_3"), "xedge_lower_gone": (1.0, *C, "brick_2_4"), "xedge_upper_gone": (1.0, *C, "brick_2_3"),
        "xedge_both_gone": (0.0, *C, "bricks_kept"),
        "yedge_both": (1.0, *C, "brick_1_3"), "yedge_lower_gone": (1.0, *C, "brick_2_3"), "yedge_upper_gone": (1.0, *C, "brick_1_3"),
        "corner_gone0": (1.0, *C, "brick_1_3"), "corner_gone1": (1.0, *C, "brick_1_4"), "corner_gone2": (1.0, *C, "brick_2_3"),
        "corner_gone3": (1.0, *C, "brick_2_4"), "corner_gone4": (0.0, *C, "bricks_kept"),
        "wall_left_and_brick": (1.0, *C, "brick_0_0_vx_flipped"), "wall_right_and_brick": (1.0, *C, "brick_4_7_vx_flipped"),
        "steps1998_continue": (0.0, *C), "steps1998_lost": (-1.0, *T_), "steps1998_brick": (1.0, *C, "brick_2_3"), "steps1998_win": (10.0, *T_),
        "steps1999_continue": (0.0, *L_), "steps1999_lost": (-1.0, *L_), "steps1999_brick": (1.0, *L_, "brick_2_3"), "steps1999_win": (10.0, *L_),
        "pre_win_a1": (0.0, *C), "any_win": (10.0, *T_, "no_bricks"), "pre_lost_a1": (0.0, *C), "any_lost": (-1.0, *T_, "ball_below"),
        "pre_continue_a1": (0.0, *C), "any_continue": (0.0, *C),
    },
    "glider": {
        "cruise": (None, *C, "wp_kept"),
        "wp0_reached": (None, *C, "wp_0_to_1"), "wp0_missed": (None, *C, "wp_kept"),
        "wp1_reached": (None, *C, "wp_1_to_0"), "wp1_missed": (None, *C, "wp_kept"),
        "corridor_pos_outside": (None, *C, "lateral"), "corridor_pos_inside": (None, *C), "corridor_pos_far": (None, *C, "lateral"),
        "corridor_neg_outside": (None, *C, "lateral"), "corridor_neg_inside": (None, *C), "corridor_neg_far": (None, *C, "lateral"),
        "alt_high_over": (None, *C, "high"), "alt_high_under": (None, *C), "alt_high_far": (None, *C, "high"),
        "alt_low_under": (None, *C, "low"), "alt_low_over": (None, *C), "no_crash": (None, *C, "low"),
        "crash": (-50.0, *T_), "stall_pos": (-50.0, *T_), "stall_neg": (-50.0, *T_), "too_far": (-50.0, *T_),
        "no_stall_pos": (None, *C), "no_stall_neg": (None, *C), "not_too_far": (None, *C),
        "crash_and_stall": (-50.0, *T_), "crash_and_too_far": (-50.0, *T_), "stall_and_too_far": (-50.0, *T_), "crash_stall_too_far": (-50.0, *T_),
        "vair_over_steep": (-50.0, *T_), "vair_under_steep": (None, *C), "vair_over_level": (None, *C), "vair_under_level": (None, *C),
        "vair_x_zero": (None, *C), "vair_x_tiny": (-50.0, *T_),
        "roll_clamp_hi": (None, *C, "roll_hi"), "roll_clamp_lo": (None, *C, "roll_lo"),
        "pitch_clamp_hi": (None, *C, "pitch_hi"), "pitch_clamp_lo": (None, *C, "pitch_lo"),
        "steps3998_cruise": (None, *C), "steps3998_crash": (-50.0, *T_), "steps3998_wp_reached": (None, *C, "wp_1_to_0"),
        "steps3999_cruise": (None, *L_), "steps3999_crash": (-50.0, *L_), "steps3999_wp_reached": (None, *L_, "wp_1_to_0"),
        "pre_crash_a0": (None, *C, "low"), "any_crash": (-50.0, *T_), "pre_cruise_a0": (None, *C), "any_cruise": (None, *C, "wp_kept"),
        "pre_wp_reached_a0": (None, *C, "wp_kept"), "any_wp_reached": (None, *C, "wp_1_to_0"),
    },
}


def _glider_reward(si, so, claim):
    """glider.py's shaped reward from the recorded post-state, with exactly the penalties the label claims (to 1e-9: the fixture's own
    value went through the same formula in another association)."""
    wp = np.array([[-160.0, 0.0, 70.0], [160.0, 0.0, 70.0]])[int(si[12])]
    vec, vel = wp - so[0:3], so[3:6]
    H = (np.dot(vel / (np.linalg.norm(vel) + 1e-8), vec / (np.linalg.norm(vec) + 1e-8)) + 1) / 2
    E = min(max(np.linalg.norm(vel) / 30.0, 0.0), 2.0)
    r = E * (H - E + 1)
    if claim == "lateral":
        r -= 2.0 * ((abs(so[1]) - 250.0) / 100.0) ** 2
    if claim == "high":
        r -= 2.0 * ((so[2] - 250.0) / 50.0) ** 2
    if claim == "low":
        r -= 0.5
    return r


def _brick(so, si, r, c, vx=None):
    gone = np.flatnonzero(si[6:46] != so[6:46])
    return gone.tolist() == [r * 8 + c] and so[4] == -si[4] and (vx is None or so[3] == -si[3])


CLAIMS = {
    "delta_hi": lambda si, so: so[5] == 0.95 * (np.pi / 6), "delta_lo": lambda si, so: so[5] == 0.95 * -(np.pi / 6),
    "delta_free": lambda si, so: abs(so[5]) < 0.95 * (np.pi / 6),
    "dist_zero": lambda si, so: so[8] == 0.0, "dist_tiny": lambda si, so: 0.0 < so[8] <= 1e-9,
    "no_bricks": lambda si, so: so[6:46].sum() == 0, "ball_below": lambda si, so: so[2] < 1.0,
    "one_brick_gone": lambda si, so: so[6:46].sum() == 1 and si[6:46].sum() == 2,
    "vx_flipped": lambda si, so: so[3] == -si[3] and so[4] == si[4], "vx_kept": lambda si, so: so[3] == si[3] and so[4] == si[4],
    "vy_flipped": lambda si, so: so[4] == -si[4] != 0, "vy_kept": lambda si, so: so[4] == si[4] and so[3] == si[3],
    "paddle_4": lambda si, so: so[0] == 4.0 and si[0] != 4.0, "paddle_36": lambda si, so: so[0] == 36.0 and si[0] != 36.0,
    "paddle_in_range": lambda si, so: 4.0 <= so[0] <= 36.0,
    "bricks_kept": lambda si, so: np.array_equal(si[6:46], so[6:46]) and so[4] == si[4],
    "brick_0_0_vx_flipped": lambda si, so: _brick(so, si, 0, 0, vx=True), "brick_4_7_vx_flipped": lambda si, so: _brick(so, si, 4, 7, vx=True),
    **{f"brick_{r}_{c}": (lambda si, so, r=r, c=c: _brick(so, si, r, c)) for r, c in ((0, 3), (4, 3), (1, 3), (1, 4), (2, 3), (2, 4))},
    "wp_kept": lambda si, so: so[12] == si[12], "wp_0_to_1": lambda si, so: (si[12], so[12]) == (0, 1),
    "wp_1_to_0": lambda si, so: (si[12], so[12]) == (1, 0),
    "roll_hi": lambda si, so: so[6] == np.pi / 2, "roll_lo": lambda si, so: so[6] == -np.pi / 2,
    "pitch_hi": lambda si, so: so[7] == np.pi / 4, "pitch_lo": lambda si, so: so[7] == -np.pi / 4,
}


def actions_of(task, label):
    tail = label.rsplit("_", 1)[-1]
    return [int(tail[1:])] if len(tail) == 2 and tail[0] == "a" and tail[1].isdigit() else list(range(N_ACT[task]))


def check_coverage(task, g):
    labels = g["labels"]
    assert set(labels.tolist()) == set(EXPECT[task]), sorted(set(labels.tolist()) ^ set(EXPECT[task]))
    assert g["state_in"].shape == g["state_out"].shape == (len(labels), SDIM[task])
    for label, (reward, term, trunc, *claim) in EXPECT[task].items():
        rows = np.flatnonzero(labels == label)
        assert g["action"][rows].tolist() == actions_of(task, label), (task, label, g["action"][rows])
        for i in rows:
            si, so, r = g["state_in"][i], g["state_out"][i], float(g["rew64"][i])
            ctx = (task, label, int(g["action"][i]), r)
            assert (bool(g["terminated"][i]), bool(g["truncated"][i])) == (term, trunc), ctx
            assert so[STEPS_AT[task]] == si[STEPS_AT[task]] + 1 and trunc == (so[STEPS_AT[task]] >= LIMIT[task]), ctx
            assert g["rew32"][i] == np.float32(r) and np.array_equal(g["obs32"][i], g["obs64"][i].astype(np.float32)), ctx
            if reward is not None:
                assert r == reward, ctx
            else:
                assert r not in TERMINAL_REWARDS[task] and abs(r) < 5.0, ctx
                if task == "glider":
                    want = _glider_reward(si, so, claim[0] if claim else None)
                    assert abs(r - want) <= 1e-9, (*ctx, want)
            if claim and claim[0] in CLAIMS:
                assert CLAIMS[claim[0]](si, so), (*ctx, claim[0])
        if label.startswith("any_"):  # one state under every action, and it is where the `pre_` row lands
            pre = np.flatnonzero(np.char.startswith(labels, "pre_" + label[4:] + "_a"))
            assert pre.size == 1 and all(np.array_equal(g["state_in"][i], g["state_out"][pre[0]]) for i in rows), (task, label)
    return len(labels)


def start_row(g, tag):
    """(state, action) of the `pre_<tag>_a<k>` row: after that one step every action leads to `any_<tag>`'s outcome (check_coverage)."""
    (i,) = np.flatnonzero(np.char.startswith(g["labels"], f"pre_{tag}_a"))
    return g["state_in"][i].copy(), int(g["action"][i])
