"""GPU: hsad_env_hand_knowledge and hsad_env_determinize_belief (BatchedHanabiEnv.hand_knowledge / determinize_belief) against the
references of tests/hand_belief_ref.py and tests/belief_head_ref.py.

Envs of 70 games (more than a wave, not a multiple of 64) of 2 players with hands of 5 and 2 and of 3 players with hands of 4,
stepped a seeded number of random moves so that hints exist; viewer -1 in every ninth game, some games finished."""
import numpy as np
import pytest
import torch

from tests import belief_head_ref as R
from tests import determinize_ref as D
from tests import hand_belief_ref as HB
from tests import search_fixtures as SF
from tests.test_env_fork_gpu import make_env, same, snapshot

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
G = 70
# (id, config, sad, shuffle_color, env seed, policy seed, iterations, sampler seed)
CASES = [("full", "full", True, False, 9150, 17, 16, 2025), ("small", "small", True, False, 9350, 23, 7, 6),
         ("c3r4", "c3r4", False, True, 9550, 31, 20, 4243)]
IDS = [c[0] for c in CASES]


def state(case):
    _, config, sad, sc, seed, pseed, iters, _ = case
    env = make_env(config, sad, sc, 0, G, 64, seed)
    env.rollout_random(iters, pseed)
    viewer, key = SF.viewers_and_keys(G, env.P)
    q = env.query().cpu().numpy()
    alive = (q[:, 14] == 1) & (q[:, 0] == 0)
    live = alive & (viewer >= 0)
    assert live.sum() >= 20 and (~live).any()
    return env, viewer, key, alive, live, env.export_state().cpu().numpy()


def knowledge_of(row, P, H, p):
    pool, cms, hand = HB.pool_and_masks(row, P, H, p)
    return pool, cms, hand


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_knowledge_equals_the_restatement_and_only_reads(case):
    env, viewer, key, alive, live, rows = state(case)
    P, H = env.P, env.H
    before = snapshot(env)
    pool, compat, cards = env.hand_knowledge()
    env.check_errors()
    after = snapshot(env)
    for name in after:
        assert same(after[name], before[name]), "hand_knowledge changed %s" % name
    assert pool.dtype == torch.int64 and compat.dtype == cards.dtype == torch.int32
    assert pool.shape == (G, P) and compat.shape == cards.shape == (G, P, H)
    pool, compat, cards = pool.cpu().numpy(), compat.cpu().numpy(), cards.cpu().numpy()
    hinted = 0
    for g in range(G):
        for p in range(P):
            if not alive[g]:
                assert pool[g, p] == 0 and not compat[g, p].any() and (cards[g, p] == -1).all(), (g, p)
                continue
            pl, cms, hand = knowledge_of(rows[g], P, H, p)
            n = len(hand)
            assert R.unpack_pool(pool[g, p]) == pl, (g, p)
            assert [R.unpack_mask(m) for m in compat[g, p, :n]] == cms and not compat[g, p, n:].any(), (g, p)
            assert cards[g, p].tolist() == hand + [-1] * (H - n), (g, p)
            hinted += any(sum(cm) < sum(1 for t in range(25) if SF.FULL_DECK[case[1]][t]) for cm in cms)
    assert hinted >= 10, "the states hold no hints"
    env.close()


def sample_and_check(env, viewer, key, live, rows, logits, seed):
    """determinize_belief on a copy-free env -> (status, logp, rows after); checks what holds for any logits"""
    P, H = env.P, env.H
    before = snapshot(env)
    status, logp = env.determinize_belief(viewer, logits, key, seed)
    env.check_errors()
    assert status.dtype == torch.int32 and logp.dtype == torch.float32 and status.shape == logp.shape == (G,)
    status, logp = status.cpu().numpy(), logp.cpu().numpy()
    after = snapshot(env)
    a_rows = after["state"].cpu().numpy()
    for g in range(G):
        if not live[g]:
            assert status[g] == 0 and logp[g] == 0.0, g
            for name in after:
                assert same(after[name][g], before[name][g]), "game %d was skipped but its %s changed" % (g, name)
    bel = env.hand_belief(viewer)
    assert bool((bel.total[torch.from_numpy(live).to(DEV)] >= 1).all()), "a sampled hand is not consistent with the card knowledge"
    return status, logp, a_rows, after


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zero_logits_sample_the_exact_belief(case):
    env, viewer, key, alive, live, rows = state(case)
    P, H, seed = env.P, env.H, case[7]
    logits = torch.zeros(G, 25 * H + 3, dtype=torch.float32, device=DEV)
    status, logp, a_rows, after = sample_and_check(env, viewer, key, live, rows, logits, seed)
    z = [0.0] * (25 * H)
    changed = 0
    for g in np.nonzero(live)[0]:
        p = int(viewer[g])
        pool, cms, hand = knowledge_of(rows[g], P, H, p)
        n = len(hand)
        want = R.row_f32(z, pool, cms, None, R.draws(seed, int(key[g]), n), n)
        assert status[g] == 1 and not want["bad"]
        row = np.array(rows[g], copy=True)
        row[0:25] = want["q"]
        for i, c in enumerate(want["hand"]):
            row[D.HANDS + (p * H + i) * 6] = c
        assert np.array_equal(a_rows[g], row), "game %d: the state after determinize_belief differs from the restatement" % g
        changed += want["hand"] != hand
        ref = R.row(z, pool, cms + [[0] * 25] * (H - n), want["hand"] + [-1] * (H - n))
        assert not ref["bad"] and abs(float(logp[g]) + ref["nll0"]) <= ref["e_nll0"], (g, float(logp[g]), ref["nll0"])
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


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_logits_sample_consistent_hands_that_equal_the_reference(case):
    env, viewer, key, alive, live, rows = state(case)
    P, H, seed = env.P, env.H, case[7]
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.randn(G, 25 * H, generator=gen) * 3.0).to(DEV)
    status, logp, a_rows, _ = sample_and_check(env, viewer, key, live, rows, logits, seed)
    zs = logits.cpu().numpy()
    near, moved = 0, 0
    for g in np.nonzero(live)[0]:
        p = int(viewer[g])
        pool, cms, hand = knowledge_of(rows[g], P, H, p)
        n = len(hand)
        ref = R.sample([float(x) for x in zs[g]], pool, cms, R.draws(seed, int(key[g]), n))
        got = [int(a_rows[g][D.HANDS + (p * H + i) * 6]) for i in range(n)]
        assert status[g] == 1
        # consistent with the knowledge and the counts, whatever the draw: every card plausible for its slot, the deck the pool less the hand
        q = list(pool)
        for i, c in enumerate(got):
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
        moved += got != hand
    assert near <= 0.01 * int(live.sum()), "%d of %d draws lie at a boundary: pick another seed" % (near, int(live.sum()))
    assert moved >= 5
    env.close()


def test_the_same_seed_and_key_give_the_same_world_wherever_the_game_lies():
    case = CASES[0]
    env, viewer, key, alive, live, rows = state(case)
    g0 = int(np.nonzero(live)[0][0])
    p = int(viewer[g0])
    dst = make_env(case[1], case[2], case[3], 0, G, 64, 1)
    dst.fork_from(env, np.full(G, g0, np.int32))
    keys = (np.arange(G) % 7 - 2).astype(np.int64)      # seven worlds, each in ten slots of both waves
    gen = torch.Generator().manual_seed(5)
    z7 = torch.randn(7, 25 * env.H, generator=gen) * 3.0
    logits = z7[torch.from_numpy(np.arange(G) % 7)].contiguous().to(DEV)
    status, logp = dst.determinize_belief(np.full(G, p, np.int32), logits, keys, 99)
    dst.check_errors()
    assert bool((status == 1).all())
    st = dst.export_state().cpu().numpy()
    for j in range(7, G):
        assert np.array_equal(st[j], st[j % 7]), j
        assert torch.equal(dst.priv_s[j], dst.priv_s[j % 7]) and float(logp[j]) == float(logp[j % 7])
    assert len({tuple(r) for r in st[:7].tolist()}) >= 3
    dst.close()
    env.close()


def test_refusals():
    from hanabi_sad_amd import _lib
    env, viewer, key, alive, live, rows = state(CASES[1])
    H = env.H
    with pytest.raises(ValueError):
        env.determinize_belief(viewer, torch.zeros(G, 25 * H - 1, device=DEV), key, 1)
    with pytest.raises(ValueError):
        env.determinize_belief(viewer, torch.zeros(G - 1, 25 * H, device=DEV), key, 1)
    z = torch.zeros(G, 25 * H, device=DEV)
    v = torch.from_numpy(viewer).to(DEV)
    k = torch.from_numpy(key).to(DEV)
    lib = env.lib
    assert lib.hsad_env_determinize_belief(env.h, v.data_ptr(), None, 25 * H, k.data_ptr(), 1, None, None, None) == -1
    assert lib.hsad_env_determinize_belief(env.h, v.data_ptr(), z.data_ptr(), 25 * H - 1, k.data_ptr(), 1, None, None, None) == -1
    assert lib.hsad_env_determinize_belief(env.h, None, z.data_ptr(), 25 * H, k.data_ptr(), 1, None, None, None) == -1
    assert lib.hsad_env_hand_knowledge(env.h, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(env.export_state().cpu().numpy(), rows)
    # a non-finite logit on an occupied slot: the game is left alone
    z[:, 3] = float("nan")
    status, logp = env.determinize_belief(viewer, z, key, 1)
    assert int(status.sum()) == 0 and float(logp.abs().sum()) == 0.0
    assert np.array_equal(env.export_state().cpu().numpy(), rows)
    assert isinstance(_lib.HsadError("x"), Exception)
    env.close()
