"""GPU: hsad_env_determinize_belief_worlds (BatchedHanabiEnv.determinize_belief_worlds) against tests/belief_world_ref.py -- the
restatement of the per-slot stratified uniforms -- and the references of tests/belief_head_ref.py under them.

The states and inputs are tests/belief_world_cases.py's: the three configurations of tests/test_env_belief_sample_gpu.py (70 games:
more than a wave, not a multiple of 64; 2 and 3 players; hands of 5, 4 and 2; every ninth viewer -1; some games finished).
tests/test_belief_world_cpu.py holds the float64 reference to at most 1 % `near` rows on the same states, inputs and world counts."""
import numpy as np
import pytest
import torch

from tests import belief_head_ref as R
from tests import belief_world_cases as WC
from tests import belief_world_ref as BW
from tests import determinize_ref as D
from tests import hand_belief_ref as HB
from tests.test_env_fork_gpu import make_env, same, snapshot

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
G = WC.G


def state(case):
    from tests.test_env_belief_sample_gpu import state as sample_state
    return sample_state(case)


def call(env, viewer, inp, W, **over):
    a = dict(inp, **over)
    out = env.determinize_belief_worlds(viewer, a["logits"].to(DEV), a["row"], a["group"], a["world"], W, a["seed"])
    env.check_errors()
    return out


def untouched(before, after, games, what):
    for g in games:
        for name in after:
            assert same(after[name][g], before[name][g]), "game %d %s but its %s changed" % (g, what, name)


def sample_and_check(env, viewer, live, inp, W):
    before = snapshot(env)
    status, logp, logp0 = call(env, viewer, inp, W)
    assert status.dtype == torch.int32 and logp.dtype == logp0.dtype == torch.float32 and status.shape == logp.shape == logp0.shape == (G,)
    status, logp, logp0 = status.cpu().numpy(), logp.cpu().numpy(), logp0.cpu().numpy()
    after = snapshot(env)
    dead = [g for g in range(G) if not live[g]]
    assert all(status[g] == 0 and logp[g] == 0.0 and logp0[g] == 0.0 for g in dead)
    untouched(before, after, dead, "was skipped")
    bel = env.hand_belief(viewer)
    assert bool((bel.total[torch.from_numpy(live).to(DEV)] >= 1).all()), "a sampled hand is not consistent with the card knowledge"
    return status, logp, logp0, after["state"].cpu().numpy(), after


@pytest.mark.parametrize("W", WC.WORLDS)
@pytest.mark.parametrize("case", WC.CASES, ids=WC.IDS)
def test_zero_logits_give_the_fp32_restatements_hand_and_state(case, W):
    env, viewer, key, alive, live, rows = state(case)
    P, H = env.P, env.H
    inp = WC.inputs(case, H, "direct", W)
    inp["logits"] = torch.zeros_like(inp["logits"])
    status, logp, logp0, a_rows, after = sample_and_check(env, viewer, live, inp, W)
    z = [0.0] * (25 * H)
    changed = 0
    for g in np.nonzero(live)[0]:
        p = int(viewer[g])
        pool, cms, hand = HB.pool_and_masks(rows[g], P, H, p)
        n = len(hand)
        want = BW.row_f32(z, pool, cms, n, inp["seed"], int(inp["group"][g]), W, int(inp["world"][g]))
        assert status[g] == 1 and not want["bad"]
        row = np.array(rows[g], copy=True)
        row[0:25] = want["q"]
        for i, c in enumerate(want["hand"]):
            row[D.HANDS + (p * H + i) * 6] = c
        assert np.array_equal(a_rows[g], row), "game %d: the state after determinize_belief_worlds differs from the restatement" % g
        assert np.float32(logp[g]).view(np.uint32) == np.float32(logp0[g]).view(np.uint32), "zero logits: logp and logp0 are the same sums"
        ref = R.row(z, pool, cms + [[0] * 25] * (H - n), want["hand"] + [-1] * (H - n))
        assert not ref["bad"] and abs(float(logp0[g]) + ref["nll0"]) <= ref["e_nll0"], (g, float(logp0[g]), ref["nll0"])
        changed += want["hand"] != hand
    assert changed >= 5
    # the rows of the resampled games are what the observe pass of a fork writes from the new state
    second = make_env(case[1], case[2], case[3], 0, G, 64, case[4] + 1)
    second.fork_from(env, np.arange(G, dtype=np.int32))
    sel = torch.from_numpy(live).to(DEV)
    forked = snapshot(second)
    for name in after:
        assert same(after[name][sel], forked[name][sel]), "%s of the resampled games is not what a fork of the result observes" % name
    second.close()
    env.close()


@pytest.mark.parametrize("W", WC.WORLDS)
@pytest.mark.parametrize("mode", WC.MODES)
@pytest.mark.parametrize("case", WC.CASES, ids=WC.IDS)
def test_random_logits_sample_consistent_hands_that_equal_the_reference(case, mode, W):
    env, viewer, key, alive, live, rows = state(case)
    P, H = env.P, env.H
    inp = WC.inputs(case, H, mode, W)
    status, logp, logp0, a_rows, _ = sample_and_check(env, viewer, live, inp, W)
    zs = inp["logits"].numpy()
    near = moved = 0
    for g in np.nonzero(live)[0]:
        p = int(viewer[g])
        pool, cms, hand = HB.pool_and_masks(rows[g], P, H, p)
        n = len(hand)
        z = [float(x) for x in zs[WC.row_of(inp, g)]]
        ref = BW.sample(z, pool, cms, inp["seed"], int(inp["group"][g]), W, int(inp["world"][g]))
        got = [int(a_rows[g][D.HANDS + (p * H + i) * 6]) for i in range(n)]
        assert status[g] == 1
        q = list(pool)
        for i, c in enumerate(got):      # consistent with the knowledge and the counts, whatever the draw
            assert cms[i][c] and q[c] > 0, (g, i, c)
            q[c] -= 1
        assert a_rows[g][0:25].tolist() == q, g
        other = np.array(a_rows[g], copy=True)
        other[0:25] = rows[g][0:25]
        for i in range(n):
            other[D.HANDS + (p * H + i) * 6] = rows[g][D.HANDS + (p * H + i) * 6]
        assert np.array_equal(other, rows[g]), "game %d: more than the hand and the deck counts changed" % g
        if ref["near"]:
            near += 1
            continue
        assert got == ref["cards"], (g, got, ref["cards"])
        assert abs(float(logp[g]) - ref["logp"]) <= ref["e_logp"], (g, float(logp[g]), ref["logp"], ref["e_logp"])
        # logp0: the same hand scored at zero logits (belief_head_ref.row's bound for nll0)
        r0 = R.row([0.0] * (25 * H), pool, cms + [[0] * 25] * (H - n), got + [-1] * (H - n))
        assert abs(float(logp0[g]) + r0["nll0"]) <= r0["e_nll0"], (g, float(logp0[g]), r0["nll0"], r0["e_nll0"])
        assert abs(ref["logp0"] + r0["nll0"]) <= 1e-9
        moved += got != hand
    assert near <= 0.01 * int(live.sum()), "%d of %d draws lie at a boundary: pick another seed" % (near, int(live.sum()))
    assert moved >= 5
    env.close()


def test_row_world_and_logits_out_of_range_leave_the_game_alone():
    case, W = WC.CASES[0], 8
    env, viewer, key, alive, live, rows = state(case)
    inp = WC.inputs(case, env.H, "rows7", W)
    lv = np.nonzero(live)[0]
    bad_row, bad_world = inp["row"].copy(), inp["world"].copy()
    bad_row[lv[0]], bad_row[lv[1]] = -1, 7
    bad_world[lv[2]], bad_world[lv[3]] = -1, W
    logits = inp["logits"].clone()
    nan_row = int(inp["row"][lv[4]])
    first_of_row = [int(g) for g in lv if inp["row"][g] == nan_row and g not in lv[:4]]
    logits[nan_row, 3] = float("nan")      # slot 0 is occupied in every live game
    before = snapshot(env)
    status, logp, logp0 = call(env, viewer, inp, W, row=bad_row, world=bad_world, logits=logits)
    status, logp, logp0 = status.cpu().numpy(), logp.cpu().numpy(), logp0.cpu().numpy()
    after = snapshot(env)
    alone = [int(g) for g in lv[:4]] + first_of_row
    assert len(first_of_row) >= 2
    assert all(status[g] == 0 and logp[g] == 0.0 and logp0[g] == 0.0 for g in alone)
    untouched(before, after, alone, "was to be left alone")
    rest = [int(g) for g in lv if int(g) not in alone]
    assert all(status[g] == 1 for g in rest) and len(rest) >= 20
    env.close()


def test_the_same_seed_group_and_world_give_the_same_world_in_every_slot_of_both_waves():
    case = WC.CASES[0]
    env, viewer, key, alive, live, rows = state(case)
    g0 = int(np.nonzero(live)[0][0])
    p = int(viewer[g0])
    dst = make_env(case[1], case[2], case[3], 0, G, 64, 1)
    dst.fork_from(env, np.full(G, g0, np.int32))
    m = np.arange(G) % 7      # seven (group, world) pairs, each in ten slots of both waves
    group, world = (m // 3 - 1).astype(np.int64), (m % 3).astype(np.int32)
    gen = torch.Generator().manual_seed(5)
    logits = (torch.randn(1, 25 * env.H, generator=gen) * 3.0).to(DEV)      # one row, read by every slot
    status, logp, logp0 = dst.determinize_belief_worlds(np.full(G, p, np.int32), logits, np.zeros(G, np.int32), group, world, 3, 99)
    dst.check_errors()
    assert bool((status == 1).all())
    st = dst.export_state().cpu().numpy()
    for j in range(7, G):
        assert np.array_equal(st[j], st[j % 7]), j
        assert torch.equal(dst.priv_s[j], dst.priv_s[j % 7])
        assert float(logp[j]) == float(logp[j % 7]) and float(logp0[j]) == float(logp0[j % 7])
    assert len({tuple(r) for r in st[:7].tolist()}) >= 3
    dst.close()
    env.close()


def fork_groups(case):
    """one live game of the case forked into 64 slots as 8 groups x 8 worlds (the 6 slots left over: world out of range)"""
    env, viewer, key, alive, live, rows = state(case)
    g0 = int(np.nonzero(live)[0][0])
    p = int(viewer[g0])
    dst = make_env(case[1], case[2], case[3], 0, G, 64, 1)
    dst.fork_from(env, np.full(G, g0, np.int32))
    j = np.arange(G)
    group, world = (j // 8 + 40).astype(np.int64), np.where(j < 64, j % 8, 8).astype(np.int32)
    gen = torch.Generator().manual_seed(17)
    z = torch.randn(1, 25 * env.H, generator=gen) * 3.0
    status, _, _ = dst.determinize_belief_worlds(np.full(G, p, np.int32), z.to(DEV), np.zeros(G, np.int32), group, world, 8, 4321)
    dst.check_errors()
    status = status.cpu().numpy()
    assert status[:64].all() and not status[64:].any()
    st = dst.export_state().cpu().numpy()
    pool, cms, hand = HB.pool_and_masks(rows[g0], env.P, env.H, p)
    first = D.HANDS + p * env.H * 6
    dst.close()
    env.close()
    return [float(x) for x in z[0]], pool, cms, st[:64, first].reshape(8, 8)


def test_slot_0_is_stratified_in_its_cumulative_counts_on_a_game_forked_as_8_groups_of_8_worlds():
    """what one point per part of [0, 1) gives (tests/test_belief_world_cpu.py): the worlds of a group with a type <= t in slot 0 number
    8 P_0[<= t] to within 1, plus the worlds the reference puts within the fp32 margin of that boundary, and the device's counts are
    the reference's up to those worlds"""
    z, pool, cms, slot0 = fork_groups(WC.CASES[0])
    for k in range(8):
        count, p, near = BW.slot0_counts(z, pool, cms, 4321, 40 + k, 8)
        got = [int((slot0[k] == t).sum()) for t in range(25)]
        assert sum(got) == 8
        cum_n, cum_p = 0, 0.0
        for t in range(25):
            cum_n, cum_p = cum_n + got[t], cum_p + p[t]
            assert abs(cum_n - 8 * cum_p) <= 1.0 + near[t] + 1e-9, (k, t, cum_n, 8 * cum_p, near[t])
            assert abs(got[t] - count[t]) <= near[t], (k, t, got[t], count[t], near[t])


def test_the_slot_0_count_property_on_a_game_forked_as_8_groups_of_8_worlds():
    """per group, the number of the 8 worlds that hold type t in slot 0 lies within 8 p_0[t] +- 1 (plus the float bound at a boundary):
    the jitter is one per (group, slot), so slot 0's 8 points are a lattice of spacing 1 / 8 and an interval of length p holds
    floor(8 p) or ceil(8 p) of them (tests/test_belief_world_cpu.py, test_slot_0_of_a_games_worlds_is_stratified)"""
    z, pool, cms, slot0 = fork_groups(WC.CASES[0])
    over = []
    for k in range(8):
        count, p, near = BW.slot0_counts(z, pool, cms, 4321, 40 + k, 8)
        for t in range(25):
            got = int((slot0[k] == t).sum())
            if p[t]:
                print("group %d type %d: %d worlds, 8 p = %.3f" % (k, t, got, 8 * p[t]))
            if abs(got - 8 * p[t]) > 1.0 + near[t] + 1e-9:
                over.append((k, t, got, round(8 * p[t], 3)))
    assert not over, over


def test_refused_calls_return_minus_one_and_leave_the_state_unchanged():
    env, viewer, key, alive, live, rows = state(WC.CASES[1])
    H, W = env.H, 8
    inp = WC.inputs(WC.CASES[1], H, "direct", W)
    z = inp["logits"].to(DEV)
    ldz = int(z.stride(0))
    v = torch.from_numpy(viewer).to(DEV)
    grp = torch.from_numpy(inp["group"]).to(DEV)
    wd = torch.from_numpy(inp["world"]).to(DEV)
    f = env.lib.hsad_env_determinize_belief_worlds
    ok = dict(viewer=v.data_ptr(), logits=z.data_ptr(), ldz=ldz, n_rows=G, row=None, group=grp.data_ptr(), world=wd.data_ptr(), W=W)

    def rc(**over):
        a = dict(ok, **over)
        return f(env.h, a["viewer"], a["logits"], a["ldz"], a["n_rows"], a["row"], a["group"], a["world"], a["W"], 1, None, None, None, None)
    for over in (dict(viewer=None), dict(logits=None), dict(group=None), dict(world=None), dict(ldz=25 * H - 1), dict(n_rows=0),
                 dict(n_rows=G - 1), dict(W=0), dict(W=(1 << 20) + 1)):
        assert rc(**over) == -1, over
    with pytest.raises(ValueError):
        env.determinize_belief_worlds(viewer, torch.zeros(G, 25 * H - 1, device=DEV), None, inp["group"], inp["world"], W, 1)
    with pytest.raises(ValueError):
        env.determinize_belief_worlds(viewer, torch.zeros(G - 1, 25 * H, device=DEV), None, inp["group"], inp["world"], W, 1)
    with pytest.raises(ValueError):
        env.determinize_belief_worlds(viewer, z, None, inp["group"], inp["world"], 0, 1)
    torch.cuda.synchronize()
    assert np.array_equal(env.export_state().cpu().numpy(), rows)
    # n_rows below G is fine with a row index
    status, _, _ = env.determinize_belief_worlds(viewer, z[:7], (np.arange(G) % 7).astype(np.int32), inp["group"], inp["world"], W, 1)
    assert int(status.sum()) == int(live.sum())
    env.close()
