"""CPU: the restatement of the hidden-hand sampler (tests/determinize_ref.py) is uniform over the hands the knowledge allows, handles
the pinned and the dead-end cases, and never gives up on the states (and with the seeds) the GPU tests determinise."""
import functools
import math

import numpy as np
import pytest

from tests import determinize_ref as R
from tests import search_fixtures as SF


def _t(c, r):
    return c * 5 + r


# 2 colours x 3 ranks (3, 2, 1 copies), 2 players with 2 cards: the other player holds c0r0 and c1r0, so the viewer's pool
# (deck + own hand) is the full deck less those two
TINY_POOL = [0] * 25
for _c in range(2):
    for _r, _n in enumerate((3, 2, 1)):
        TINY_POOL[_t(_c, _r)] = _n
TINY_POOL[_t(0, 0)] -= 1
TINY_POOL[_t(1, 0)] -= 1
# slot 0: either colour, rank 0 or 1; slot 1: colour 1, any rank -> 4 x 3 = 12 hands, all consistent
TINY_MASKS = [(0b11, 0b011), (0b10, 0b111)]


def test_accepted_hands_are_uniform_over_the_consistent_physical_cards():
    exact = R.exact_distribution(TINY_POOL, TINY_MASKS)
    assert len(exact) == 12 and abs(sum(exact.values()) - 1.0) < 1e-12
    # not flat: the hand (c1r0, c1r0) needs both remaining copies
    assert exact[(_t(1, 0), _t(1, 0))] < exact[(_t(0, 0), _t(1, 1))]
    N, seed = 20000, 20260101
    counts, tries_total = {}, 0
    for key in range(N):
        cards, q, tries = R.sample_hand(TINY_POOL, TINY_MASKS, key, seed)
        assert tries != -1, "the sampler gave up at key %d" % key
        assert sum(q) == sum(TINY_POOL) - 2 and min(q) >= 0
        counts[tuple(cards)] = counts.get(tuple(cards), 0) + 1
        tries_total += tries
    assert set(counts) <= set(exact)
    for hand, p in exact.items():
        n = counts.get(hand, 0)
        sd = math.sqrt(N * p * (1.0 - p))   # binomial(N, p)
        print("hand %s: %d drawn, %.1f expected, %.2f sd" % (hand, n, N * p, (n - N * p) / sd))
        assert abs(n - N * p) <= 5.0 * sd, (hand, n, N * p, sd)
    print("mean tries %.3f" % (tries_total / N))


def test_a_fully_pinned_hand_is_returned_unchanged():
    pool = list(TINY_POOL)
    masks = [(0b01, 0b010), (0b10, 0b100)]   # c0r1, c1r2
    for key in range(50):
        cards, q, tries = R.sample_hand(pool, masks, key, 3)
        assert cards == [_t(0, 1), _t(1, 2)] and tries == 1   # Z = Zmax in every slot: always accepted
        assert q[_t(0, 1)] == pool[_t(0, 1)] - 1 and q[_t(1, 2)] == pool[_t(1, 2)] - 1


def test_a_try_that_runs_out_of_cards_is_rejected():
    # both slots can only be c1r2, of which one copy exists: slot 1 always finds Z == 0, every try fails, the sampler gives up
    pool = [0] * 25
    pool[_t(1, 2)] = 1
    pool[_t(0, 0)] = 2
    assert R.sample_hand(pool, [(0b10, 0b100), (0b10, 0b100)], 9, 1) == (None, None, -1)
    # with an alternative for slot 0 only the tries that give slot 0 the single c1r2 fail; the accepted hand is the other one
    seen = set()
    for key in range(200):
        cards, q, tries = R.sample_hand(pool, [(0b11, 0b101), (0b10, 0b100)], key, 1)
        assert cards == [_t(0, 0), _t(1, 2)] and tries >= 1
        seen.add(tries)
    assert max(seen) > 1, "no try was ever rejected"


@functools.lru_cache(maxsize=None)
def _variant_oracle():
    from tests.variant_oracle import variant_oracle
    variant_oracle.build()
    return variant_oracle


def _oracle_rows(config, sad, sc, km, G, seed, pseed, iters):
    variant_oracle = _variant_oracle()
    vec = variant_oracle.VariantVecEnv(G, seed, eps_list=SF.EPS, **SF.env_kwargs(config, sad, sc, km))
    vec.rollout(iters, pseed)
    return [e.export_state() for e in vec.envs], [e.terminated() for e in vec.envs]


@pytest.mark.parametrize("case", SF.DET_CASES, ids=lambda c: c[0])
def test_the_sampler_never_gives_up_on_the_states_the_gpu_tests_determinise(case):
    _, config, sad, sc, km, G, _, seed, pseed, iters, det_seed = case
    P, H = SF.CONFIGS[config]["players"], SF.CONFIGS[config]["hand_size"]
    rows, term = _oracle_rows(config, sad, sc, km, G, seed, pseed, iters)
    viewer, key = SF.viewers_and_keys(G, P)
    live = changed = 0
    for g in range(G):
        if viewer[g] < 0 or term[g]:
            continue
        new, tries = R.determinize_row(rows[g], P, H, int(viewer[g]), int(key[g]), det_seed)
        assert tries >= 1, "game %d: the sampler gave up" % g
        live += 1
        changed += int(not np.array_equal(new, rows[g]))
    assert live > G // 2 and changed > 0


def test_the_sampler_never_gives_up_on_the_paired_keys():
    _, config, sad, sc, km, G, _, seed, pseed, iters, _ = SF.DET_CASES[0]
    P, H = SF.CONFIGS[config]["players"], SF.CONFIGS[config]["hand_size"]
    rows, term = _oracle_rows(config, sad, sc, km, G, seed, pseed, iters)
    g0 = term.index(False)
    worlds = {int(k): R.determinize_row(rows[g0], P, H, int(rows[g0][57]), int(k), SF.PAIR_SEED) for k in SF.PAIR_KEYS}
    assert all(t >= 1 for _, t in worlds.values())
    assert len({r.tobytes() for r, _ in worlds.values()}) > 4


def test_the_sampler_never_gives_up_in_the_search_test():
    from hanabi_sad_amd.search import world_key
    s = SF.SEARCH_ROOT
    P, H = SF.CONFIGS[s["config"]]["players"], SF.CONFIGS[s["config"]]["hand_size"]
    rows, term = _oracle_rows(s["config"], False, False, 0, s["G"], s["seed"], s["pseed"], s["iters"])
    assert sum(not t for t in term) >= 2, "the search test needs live roots"   # (a finished one as well: its values are NaN)
    for g in range(s["G"]):
        if term[g]:
            continue
        cur = int(rows[g][57])
        for w in range(s["worlds"]):
            assert R.determinize_row(rows[g], P, H, cur, world_key(g, w), s["search_seed"])[1] >= 1
