"""CPU tests of the variant restatement (tests/variant_oracle): the game with HLE's colors / ranks / max_information_tokens /
max_life_tokens passed at creation.

At the full game's 5 / 5 / 8 / 3 it must be the project's oracle bit for bit; for the HLE presets and mixed variants its
sizes follow the canonical encoder's section formula, and random episodes keep the game's invariants."""
import numpy as np
import pytest

from oracle.oracle import OracleEnv, policy_random
from tests.variant_oracle.variant_oracle import VariantEnv

EPS = [0.1 ** (1 + 7 * i / 79) for i in range(80)]

# the configurations of tests/test_oracle_env.py and tests/test_env_parity_gpu.py
FULL_CONFIGS = [
    dict(players=2, hand_size=5, sad=False, shuffle_color=False, knowledge_mode=0, bomb=0, max_len=80),
    dict(players=2, hand_size=5, sad=True, shuffle_color=True, knowledge_mode=0, bomb=1, max_len=80),
    dict(players=2, hand_size=5, sad=True, shuffle_color=False, knowledge_mode=1, bomb=0, max_len=12),
    dict(players=3, hand_size=5, sad=False, shuffle_color=True, knowledge_mode=1, bomb=0, max_len=-1),
    dict(players=5, hand_size=4, sad=True, shuffle_color=True, knowledge_mode=0, bomb=0, max_len=80),
    dict(players=4, hand_size=4, sad=False, shuffle_color=False, knowledge_mode=0, bomb=1, max_len=80),
    dict(players=5, hand_size=5, sad=True, shuffle_color=True, knowledge_mode=0, bomb=0, max_len=80),
]

# HLE's presets (Full-Minimal apart from its observation type) and mixed cases
PRESETS = {
    "full": dict(players=2, hand_size=5, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3),
    "small": dict(players=2, hand_size=2, colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1),
    "very_small": dict(players=2, hand_size=2, colors=1, ranks=5, max_information_tokens=3, max_life_tokens=1),
    "c3r4": dict(players=3, hand_size=4, colors=3, ranks=4, max_information_tokens=6, max_life_tokens=2),
    "r1": dict(players=2, hand_size=3, colors=4, ranks=1, max_information_tokens=2, max_life_tokens=3),
    "p4": dict(players=4, hand_size=3, colors=4, ranks=3, max_information_tokens=5, max_life_tokens=2),
    "r2": dict(players=2, hand_size=2, colors=3, ranks=2, max_information_tokens=1, max_life_tokens=1),
}


def instances(r, R):
    return 3 if r == 0 else (1 if r == R - 1 else 2)


def section_sizes(P, H, C, R, MI, ML, sad=False):
    deck = C * sum(instances(r, R) for r in range(R))
    lal = P + 4 + P + C + R + H + H + C * R + 2
    F = (P * H * C * R + P) + (deck - P * H + C * R + MI + ML) + deck + lal + P * H * (C * R + C + R)
    return F + (lal if sad else 0), 2 * H + (P - 1) * (C + R) + 1, deck


def _episodes(make, n_games, steps, pseed=5, check=None):
    envs = [make(seed) for seed in range(n_games)]
    for g, e in enumerate(envs):
        o = e.reset()
        for n in range(steps):
            if e.terminated():
                o = e.reset()
            a, ga = policy_random(o["legal_move"], pseed, g, n)
            o, r, t = e.step(a, ga)
            e.terminated()
            if check:
                check(e, o, r, t)
    return envs


@pytest.mark.parametrize("cfg", FULL_CONFIGS, ids=lambda c: "p%dh%d_sad%d_sc%d_k%d_b%d" % (
    c["players"], c["hand_size"], c["sad"], c["shuffle_color"], c["knowledge_mode"], c["bomb"]))
def test_full_game_equals_the_oracle_bit_for_bit(cfg):
    for seed in range(6):
        ref = OracleEnv(seed=seed, eps_list=EPS, **cfg)
        var = VariantEnv(seed=seed, eps_list=EPS, **cfg)
        assert (var.F, var.A, var.deck) == (ref.F, ref.A, 50)
        assert var.L.orc_env_hand_feature_size(var.h) == ref.L.orc_env_hand_feature_size(ref.h)
        for n in range(140):
            if ref.terminated():
                assert var.terminated()
                o_r, o_v = ref.reset(), var.reset()
                for k in o_r:
                    assert o_r[k].tobytes() == o_v[k].tobytes(), (seed, n, k)
            a, ga = policy_random(o_r["legal_move"], 3, seed, n)
            o_r, r_r, t_r = ref.step(a, ga)
            o_v, r_v, t_v = var.step(a, ga)
            for k in o_r:
                assert o_r[k].tobytes() == o_v[k].tobytes(), (seed, n, k)
            assert (r_r, t_r) == (r_v, t_v)
            ref.terminated(), var.terminated()
            assert np.array_equal(ref.export_state(), var.export_state()), (seed, n)
            assert ref.rng_draws() == var.rng_draws()
            assert ref.deck_history() == var.deck_history()


@pytest.mark.parametrize("sad", [False, True])
@pytest.mark.parametrize("name", sorted(PRESETS))
def test_sizes_follow_the_section_formula(name, sad):
    p = PRESETS[name]
    e = VariantEnv(sad=sad, **p)
    F, A, deck = section_sizes(p["players"], p["hand_size"], p["colors"], p["ranks"], p["max_information_tokens"],
                               p["max_life_tokens"], sad)
    assert (e.F, e.A, e.deck) == (F, A, deck)
    assert e.L.orc_env_hand_feature_size(e.h) == p["hand_size"] * p["colors"] * p["ranks"]
    if name == "full":
        assert (e.F, e.A) == ((838, 21) if sad else (783, 21))
    if name == "small":
        assert (e.F, e.A) == ((222, 12) if sad else (191, 12))


@pytest.mark.parametrize("shuffle_color", [False, True])
@pytest.mark.parametrize("name", sorted(PRESETS))
def test_invariants_over_random_episodes(name, shuffle_color):
    p = PRESETS[name]
    P, H, C, R, MI, ML = (p[k] for k in ("players", "hand_size", "colors", "ranks", "max_information_tokens",
                                         "max_life_tokens"))
    full = np.zeros(25, np.int64)
    for c in range(C):
        for r in range(R):
            full[c * 5 + r] = instances(r, R)
    A = 2 * H + (P - 1) * (C + R) + 1

    def check(e, o, r, t):
        st = e.export_state()
        deck, disc, fw = st[:25], st[25:50], st[50:55]
        info, life, cur = st[55], st[56], st[57]
        hands = np.zeros(25, np.int64)
        for slot in range(P * H):
            card = st[80 + slot * 6]
            if card >= 0:
                hands[card] += 1
                assert card % 5 < R and card // 5 < C
                assert st[80 + slot * 6 + 1] & ~((1 << C) - 1) == 0 and st[80 + slot * 6 + 2] & ~((1 << R) - 1) == 0
        played = np.zeros(25, np.int64)
        for c in range(5):
            played[c * 5: c * 5 + fw[c]] = 1
        assert np.array_equal(deck + disc + hands + played, full)          # card conservation
        assert (fw[C:] == 0).all() and (fw <= R).all() and fw.sum() <= C * R
        assert 0 <= info <= MI and 0 <= life <= ML and st[61] == deck.sum()
        assert 0 <= e.get("score") <= C * R
        lm = o["legal_move"]
        if cur >= 0 and not t:
            row = lm[cur]
            assert row[:H].any() == (info < MI)                                 # discards only below max_info
            if info == 0:
                assert not row[2 * H:A - 1].any()                               # no hints without a token
        base = 80 + P * H * 6
        perm, inv = st[base:base + 5 * P].reshape(P, 5), st[base + 5 * P:base + 10 * P].reshape(P, 5)
        for q in range(P):
            assert sorted(perm[q, :C]) == list(range(C)) and list(perm[q, C:]) == list(range(C, 5))
            assert all(inv[q, perm[q, c]] == c for c in range(5))
        if t:
            assert fw.sum() == C * R or life == 0 or st[59] <= 0 or e.get("num_step") == 80
    envs = _episodes(lambda s: VariantEnv(seed=s, eps_list=EPS, shuffle_color=shuffle_color, **p), 6, 200, check=check)
    assert all(e.rng_draws() > 0 for e in envs)


def test_colour_shuffle_relabels_the_observation_consistently():
    """with shuffle_color each observer sees colour c at the slot perm[observer][c]: the partner's hand block of a 2-colour
    game, read through the inverse permutation, is the partner's real hand"""
    p = PRESETS["small"]
    for seed in range(20):
        e = VariantEnv(seed=seed, shuffle_color=True, **p)
        o = e.reset()
        st = e.export_state()
        C, R, H = p["colors"], p["ranks"], p["hand_size"]
        base = 80 + 2 * H * 6
        for obs in range(2):
            perm = st[base + obs * 5: base + obs * 5 + 5]
            other = 1 - obs
            block = o["priv_s"][obs, H * C * R: 2 * H * C * R].reshape(H, C * R)
            for i in range(H):
                card = st[80 + (other * H + i) * 6]
                c, r = card // 5, card % 5
                assert block[i].sum() == 1 and block[i, perm[c] * R + r] == 1


@pytest.mark.parametrize("bad", [dict(colors=0), dict(colors=6), dict(ranks=0), dict(ranks=6),
                                 dict(max_information_tokens=0), dict(max_information_tokens=9),
                                 dict(max_life_tokens=0), dict(max_life_tokens=4),
                                 dict(colors=1, ranks=1, players=2, hand_size=2)])
def test_out_of_range_rules_are_refused(bad):
    kw = dict(players=2, hand_size=5)
    kw.update(bad)
    with pytest.raises(ValueError):
        VariantEnv(**kw)


def test_hanalearn_params_honour_rule_keys_and_refuse_unsupported_ones():
    from hanabi_sad_amd.hanalearn import game_rules
    assert game_rules({"players": "2"}) == dict(colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3)
    small = {"players": "2", "colors": "2", "ranks": "5", "hand_size": "2", "max_information_tokens": "3",
             "max_life_tokens": "1", "observation_type": "1", "random_start_player": "false", "seed": "3", "unknown": "x"}
    assert game_rules(small) == dict(colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1)
    for key, val in (("colors", "6"), ("colors", "0"), ("ranks", "7"), ("max_information_tokens", "9"),
                     ("max_life_tokens", "4"), ("observation_type", "2"), ("random_start_player", "true"),
                     ("random_start_player", "1")):
        with pytest.raises(ValueError, match=key):
            game_rules({"players": "2", key: val})
