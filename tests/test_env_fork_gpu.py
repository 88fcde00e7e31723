"""GPU: hsad_env_fork and hsad_env_determinize (BatchedHanabiEnv.fork_from / determinize).  A fork is the source game bit for bit --
state, generator, every bound output -- and then plays the same game; a determinised game is what the numpy restatement of the
sampler (tests/determinize_ref.py) makes of the exported state, observes like a state that was reached by play, and plays on without
breaking the rules.  Shapes: 65 and 33 games (two workgroups, the second partial, for 64- and 32-game workgroups)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import determinize_ref as R
from tests import search_fixtures as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_env(config, sad, sc, km, G, gpw, seed, **extra):
    from hanabi_sad_amd import BatchedHanabiEnv
    env = BatchedHanabiEnv(G, seed=seed, eps_list=SF.EPS, device=DEV, games_per_workgroup=gpw, **SF.env_kwargs(config, sad, sc, km), **extra)
    assert env.games_per_workgroup == gpw
    env.packed = km == 0
    if env.packed:   # packed outputs on wherever the library has them (not with the V0-belief rows of knowledge_mode 1)
        env.enable_packed((env.F + 63) // 64 * 64, keep_float32=True)
    return env


def outputs(env):
    out = {"priv_s": env.priv_s, "legal_move": env.legal_move, "own_hand": env.own_hand, "eps": env.eps, "reward": env.reward,
           "terminal": env.terminal}
    if env.packed:
        out.update(priv_bits=env.priv_bits, legal_bits=env.legal_bits, own_bits=env.own_bits, priv_s_bf16=env.priv_s_bf16)
    return out


def snapshot(env):
    snap = {k: v.clone() for k, v in outputs(env).items()}
    snap["state"] = env.export_state()
    return snap


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a, b)


def source_at(config, sad, sc, km, G, gpw, k, seed=8000):
    src = make_env(config, sad, sc, km, G, gpw, seed + k)
    src.reset()
    if k:
        src.rollout_random(k, 13)
    return src


def fork_index(G, salt):
    rng = np.random.RandomState(100 + salt)
    idx = rng.randint(0, G, size=G)
    idx[rng.rand(G) < 0.2] = -1
    idx[0], idx[1], idx[2], idx[G - 1] = -1, G - 1, G - 1, 3   # untouched, the last source game twice, the last slot
    idx[5] = 5
    return idx.astype(np.int32)


def conserved(rows, P, H, config):
    """per card type: deck + discards + hands + fireworks == the full deck"""
    rows = np.asarray(rows)
    total = rows[:, 0:25] + rows[:, 25:50]
    for c in range(5):
        for r in range(5):
            total[:, c * 5 + r] += (rows[:, 50 + c] > r)
    for s in range(P * H):
        card = rows[:, 80 + s * 6]
        for g in np.nonzero(card >= 0)[0]:
            total[g, card[g]] += 1
    return (total == np.asarray(SF.FULL_DECK[config])[None, :]).all(axis=1)


FORK_CASES = []
for _i, (_cfg, _sad, _sc) in enumerate((c, s, x) for c in ("full", "small", "c3r4") for s in (False, True) for x in (False, True)):
    _km = (_i + _i // 4) % 2
    _G, _gpw = ((65, 64), (33, 32))[(_i // 2 + _i // 4) % 2]
    FORK_CASES.append(pytest.param(_cfg, _sad, _sc, _km, _G, _gpw, id="%s-sad%d-sc%d-k%d-G%d" % (_cfg, _sad, _sc, _km, _G)))


@pytest.mark.parametrize("config,sad,sc,km,G,gpw", FORK_CASES)
def test_a_fork_is_the_source_game_bit_for_bit_and_plays_the_same_game(config, sad, sc, km, G, gpw):
    for k in (0, 1, 7, 30):
        src = source_at(config, sad, sc, km, G, gpw, k)
        dst = make_env(config, sad, sc, km, G, gpw, 777)
        dst.rollout_random(3, 5)   # some other position in every slot
        before = snapshot(dst)
        idx = fork_index(G, k)
        dst.fork_from(src, idx)
        dst.check_errors()
        sel = torch.from_numpy(idx >= 0).to(DEV)
        pick = torch.from_numpy(idx[idx >= 0].astype(np.int64)).to(DEV)
        s_snap, d_snap = snapshot(src), snapshot(dst)
        for name in d_snap:
            want = s_snap[name][pick]
            if name == "reward":
                want = torch.zeros_like(want)
            assert same(d_snap[name][sel], want), "k=%d: %s of the forked games differs from the source's" % (k, name)
            assert same(d_snap[name][~sel], before[name][~sel]), "k=%d: %s of an untouched game changed" % (k, name)
        (dh_d, n_d), (dh_s, n_s) = dst.deck_history(), src.deck_history()
        assert torch.equal(n_d[sel], n_s[pick]) and torch.equal(dh_d[sel], dh_s[pick])
        # the generator came along (seeds = NULL): both now play, and deal, the same game
        for it in range(20):
            src.reset()
            dst.reset()
            a, ga = src.policy_random(99)
            da, dga = dst.policy_random(99)
            assert torch.equal(da[5], a[5]), "the policy counter was not copied"   # slot 5 is game 5: same hash key
            da[sel], dga[sel] = a[pick], ga[pick]
            src.step(a, ga)
            dst.step(da, dga)
            for name, t in outputs(dst).items():
                assert same(t[sel], outputs(src)[name][pick]), "k=%d: %s differs %d steps after the fork" % (k, name, it + 1)
        assert torch.equal(dst.export_state()[sel], src.export_state()[pick])
        src.check_errors()
        dst.check_errors()
        src.close()
        dst.close()


def _mt19937_first_two(seed):
    x = [seed & 0xFFFFFFFF]
    for i in range(1, 624):
        x.append((1812433253 * (x[-1] ^ (x[-1] >> 30)) + i) & 0xFFFFFFFF)
    out = []
    for i in range(2):
        y = (x[i] & 0x80000000) | (x[i + 1] & 0x7FFFFFFF)
        v = x[i + 397] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        v ^= v >> 11
        v ^= (v << 7) & 0x9D2C5680
        v ^= (v << 15) & 0xEFC60000
        v ^= v >> 18
        out.append(v)
    return out


def _deal(deck_counts, seed):
    """the card the first deal of std::mt19937(seed) takes from this deck: first type whose cumulative count exceeds
    floor(S * D / 2^64), S = u1 + u2 * 2^32 (the env's discrete_distribution, away from its 2^-35 rounding corner)"""
    u1, u2 = _mt19937_first_two(seed)
    S, D = u1 + (u2 << 32), int(sum(deck_counts))
    need, run = (S * D >> 64) + 1, 0
    for t, n in enumerate(deck_counts):
        run += int(n)
        if run >= need:
            return t


@pytest.mark.parametrize("config,sc", [("full", False), ("c3r4", True)])
def test_a_fork_with_seeds_keeps_the_state_and_deals_from_the_new_generator(config, sc):
    """What "the same deal as a fresh env seeded alike" can mean: a fresh env has spent its generator's first draws on the opening
    deal from the full deck, the fork spends them on its next card from the deck it has.  Both are the same function of the same two
    raw outputs of std::mt19937(seed), restated here (_deal) and checked on both: the fresh env's first card and the fork's next one."""
    G, P, H = 33, SF.CONFIGS[config]["players"], SF.CONFIGS[config]["hand_size"]
    src = make_env(config, False, sc, 0, G, 32, 8100)
    src.reset()
    dst = make_env(config, False, sc, 0, G, 32, 555)
    idx = np.arange(G, dtype=np.int32)[::-1].copy()
    seeds = (4000 + np.arange(G) // 2).astype(np.int32)   # pairs of slots share a seed
    dst.fork_from(src, idx, seeds)
    s_state, d_state = src.export_state().cpu().numpy()[idx], dst.export_state().cpu().numpy()
    assert (d_state[:, 73] == 0).all() and (s_state[:, 73] > 0).all(), "draws consumed: 0 in the fork"
    d_state[:, 73] = s_state[:, 73]
    assert np.array_equal(d_state, s_state)
    for name in ("priv_s", "legal_move", "own_hand", "eps", "priv_bits"):
        assert same(outputs(dst)[name], outputs(src)[name][torch.from_numpy(idx.astype(np.int64)).to(DEV)]), name
    # everybody plays the first card: the next card is dealt to deck position P * H
    a = torch.full((G, P), dst.A - 1, dtype=torch.int64, device=DEV)
    a[:, 0] = H
    dst.step(a, a)
    dst.check_errors()
    dh, n = dst.deck_history()
    dh, n = dh.cpu().numpy(), n.cpu().numpy()
    assert (n == P * H + 1).all()
    fresh = make_env(config, False, sc, 0, G, 32, 4000)   # game g seeded 4000 + g
    fresh.reset()
    fdh = fresh.deck_history()[0].cpu().numpy()
    for j in range(G):
        assert dh[j, P * H] == _deal(s_state[j, 0:25], int(seeds[j])), "slot %d" % j
        assert fdh[j, 0] == _deal(SF.FULL_DECK[config], 4000 + j), "fresh game %d" % j
    assert len(set(dh[:, P * H])) > 1


def test_fork_refusals_and_the_out_of_range_index():
    from hanabi_sad_amd import _lib
    G = 33
    src = make_env("small", False, False, 0, G, 32, 8200)
    src.reset()
    idx = np.arange(G, dtype=np.int32)
    for other in (make_env("small", True, False, 0, G, 32, 1), make_env("small", False, True, 0, G, 32, 1),
                  make_env("small", False, False, 1, G, 32, 1), make_env("c3r4", False, False, 0, G, 32, 1),
                  make_env("small", False, False, 0, G, 32, 1, track_deck_history=True)):
        donor = src if other.config != src.config else make_env("small", False, False, 0, G, 32, 2, track_deck_history=False)
        with pytest.raises(_lib.HsadError):
            other.fork_from(donor, idx)
    with pytest.raises(_lib.HsadError, match="same env"):
        src.fork_from(src, idx)
    # sad: the greedy-action section can only come from the source's rows
    sad_src = make_env("small", True, False, 1, G, 32, 3)     # float32 rows only: accepted
    sad_src.reset()
    sad_dst = make_env("small", True, False, 1, G, 32, 4)
    sad_dst.fork_from(sad_src, idx)
    assert torch.equal(sad_dst.priv_s, sad_src.priv_s)
    bare = make_env("small", True, False, 0, G, 32, 5)
    bare.reset()
    L = bare.lib
    _lib.check(L.hsad_env_bind_packed(bare.h, None, None, None, bare.priv_s_bf16.data_ptr(), bare.priv_s_bf16.shape[-1], 0))   # bf16 rows only
    sad_dst0 = make_env("small", True, False, 0, G, 32, 6)
    with pytest.raises(_lib.HsadError, match="sad"):
        sad_dst0.fork_from(bare, idx)
    # an index outside the source is counted, and that game is left alone
    dst = make_env("small", False, False, 0, G, 32, 7)
    dst.rollout_random(2, 3)
    before = snapshot(dst)
    bad = idx.copy()
    bad[4], bad[32] = G, -7
    dst.fork_from(src, bad)
    n, g, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(L.hsad_env_error_count(dst.h, C.byref(n), C.byref(g), C.byref(c)))
    assert (n.value, c.value) == (2, 4) and g.value in (4, 32)
    after = snapshot(dst)
    keep = torch.tensor([4, 32], device=DEV)
    for name in after:
        assert same(after[name][keep], before[name][keep]), name
    assert torch.equal(after["state"][:4], src.export_state()[:4])
    dst.fork_from(src, bad)
    with pytest.raises(_lib.HsadError, match="fork source index"):
        dst.check_errors()


def _hint_bits(env, new_row, q, p, perm_q):
    """the colour / rank hint uids observer q (on turn) may give player p, from p's exported hand"""
    P, H, Cn, Rn = env.P, env.H, env.colors, env.ranks
    o = (p - q) % P
    uids = set()
    for card, _, _ in R.hand_of(new_row, P, H, p):
        uids.add(2 * H + (o - 1) * Cn + int(perm_q[card // 5]))
        uids.add(2 * H + (P - 1) * Cn + (o - 1) * Rn + card % 5)
    return uids


@pytest.mark.parametrize("case", SF.DET_CASES, ids=lambda c: c[0])
def test_determinize_matches_the_restatement_observes_consistently_and_plays_on(case):
    _, config, sad, sc, km, G, gpw, seed, pseed, iters, det_seed = case
    env = make_env(config, sad, sc, km, G, gpw, seed)
    P, H, F, A, Cn, Rn = env.P, env.H, env.F, env.A, env.colors, env.ranks
    env.rollout_random(iters, pseed)
    before = snapshot(env)
    q0 = env.query().cpu().numpy()
    viewer, key = SF.viewers_and_keys(G, P)
    tries = env.determinize(viewer, key, det_seed).cpu().numpy()
    env.check_errors()
    after = snapshot(env)
    b_rows, a_rows = before["state"].cpu().numpy(), after["state"].cpu().numpy()
    live = (q0[:, 14] == 1) & (q0[:, 0] == 0) & (viewer >= 0)
    assert live.any() and (~live).any()
    assert conserved(a_rows, P, H, config).all()
    b_priv, a_priv = before["priv_s"].cpu().numpy(), after["priv_s"].cpu().numpy()
    b_legal, a_legal = before["legal_move"].cpu().numpy(), after["legal_move"].cpu().numpy()
    CR = Cn * Rn
    n_changed = 0
    for g in range(G):
        if not live[g]:
            assert tries[g] == 0
            for name in after:
                assert same(after[name][g], before[name][g]), "game %d was skipped but its %s changed" % (g, name)
            continue
        p = int(viewer[g])
        want, want_tries = R.determinize_row(b_rows[g], P, H, p, int(key[g]), det_seed)
        assert tries[g] == want_tries and want_tries >= 1, g
        assert np.array_equal(a_rows[g], want), "game %d: state after determinize differs from the restatement" % g
        n_changed += int(not np.array_equal(a_rows[g], b_rows[g]))
        for card, cp, rp in R.hand_of(a_rows[g], P, H, p):
            assert (cp >> (card // 5)) & 1 and (rp >> (card % 5)) & 1, "game %d: a sampled card is outside its slot's knowledge" % g
        assert np.array_equal(a_priv[g, p], b_priv[g, p]), "game %d: the viewer's own observation changed" % g
        for name in ("eps", "terminal"):
            assert same(after[name][g], before[name][g])
        if km != 0:
            continue
        hand = R.hand_of(a_rows[g], P, H, p)
        for q in range(P):
            if q == p:
                continue
            perm_q = a_rows[g][80 + P * H * 6 + q * 5: 80 + P * H * 6 + q * 5 + 5]
            o = (p - q) % P
            lo, hi = o * H * CR, (o + 1) * H * CR
            row = a_priv[g, q]
            assert np.array_equal(np.delete(row, np.s_[lo:hi]), np.delete(b_priv[g, q], np.s_[lo:hi])), \
                "game %d observer %d: the row changed outside player %d's hand" % (g, q, p)
            onehot = np.zeros(H * CR, np.float32)
            for i, (card, _, _) in enumerate(hand):
                onehot[i * CR + int(perm_q[card // 5]) * Rn + card % 5] = 1.0
            assert np.array_equal(row[lo:hi], onehot), "game %d observer %d" % (g, q)
            if q == a_rows[g][57] and a_rows[g][55] > 0:   # on turn, with an information token: the hints the new hand allows
                o_lo = 2 * H + (o - 1) * Cn, 2 * H + (P - 1) * Cn + (o - 1) * Rn
                got = {u for u in list(range(o_lo[0], o_lo[0] + Cn)) + list(range(o_lo[1], o_lo[1] + Rn)) if a_legal[g, q, u] != 0}
                assert got == _hint_bits(env, a_rows[g], q, p, perm_q), "game %d observer %d: hint moves" % (g, q)
                rest = np.ones(A, bool)
                rest[o_lo[0]:o_lo[0] + Cn] = rest[o_lo[1]:o_lo[1] + Rn] = False
                assert np.array_equal(a_legal[g, q][rest], b_legal[g, q][rest])
    assert n_changed > 0
    if env.packed:   # the packed forms are the same rows
        bits = after["priv_bits"].cpu().numpy().astype(np.uint64)
        unpacked = ((bits[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(G, P, -1)[..., :F]
        assert np.array_equal(unpacked.astype(np.float32), a_priv)
        assert np.array_equal(after["priv_s_bf16"].float().cpu().numpy()[..., :F], a_priv)
    # the determinised games play on to their end: no contract error, cards conserved all the way
    for _ in range(40):
        env.playout_random(5, 71)
        assert conserved(env.export_state().cpu().numpy(), P, H, config).all()
        if bool((env.query()[:, 0] == 1).all()):
            break
    env.check_errors()
    assert bool((env.query()[:, 0] == 1).all())


def test_equal_keys_give_equal_worlds_in_different_slots():
    _, config, sad, sc, km, Gs, gpw, seed, pseed, iters, _ = SF.DET_CASES[0]
    G = len(SF.PAIR_KEYS)
    src = make_env(config, sad, sc, km, Gs, gpw, seed)
    src.rollout_random(iters, pseed)
    q = src.query().cpu().numpy()
    g0 = int(np.nonzero(q[:, 0] == 0)[0][0])     # the first live game
    dst = make_env(config, sad, sc, km, G, 32, 1)
    dst.fork_from(src, np.full(G, g0, np.int32))
    key = SF.PAIR_KEYS                            # pairs of slots share a key (negative ones too)
    tries = dst.determinize(np.full(G, q[g0, 1], np.int32), key, SF.PAIR_SEED).cpu().numpy()
    assert (tries >= 1).all()
    rows = dst.export_state().cpu().numpy()
    for j in range(0, G - 1, 2):
        assert np.array_equal(rows[j], rows[j + 1])
        assert torch.equal(dst.priv_s[j], dst.priv_s[j + 1]) and torch.equal(dst.priv_bits[j], dst.priv_bits[j + 1])
    assert len({rows[j].tobytes() for j in range(G)}) > 4, "different keys never gave different worlds"
