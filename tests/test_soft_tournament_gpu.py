"""GPU: tournaments whose network seats play their softmax policy (eval.play_seatings(temperature=, sample_seed=), eval.evaluate
(temperature=)).  Hanabi-Small rules (2 colours, hands of 2, 3 information tokens, 1 life), 64 deals, a pool of two small random nets
and the rule bot `piers`; seatings that put every member on both seats and next to every other."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
RULES = dict(colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1)
HAND, SAD, DEALS, SEED = 2, True, 64, 5100
SEATINGS = [(0, 1), (1, 0), (0, 2), (2, 1), (1, 1), (0, 0)]
NAMES = ["cold", "warm", "piers"]


@pytest.fixture(scope="module")
def pool():
    from hanabi_sad_amd.eval import env_dims
    from hanabi_sad_amd.rulebot import PRESETS
    from hanabi_sad_amd.selfplay import init_weights
    F, A = env_dims(2, HAND, SAD, **RULES)
    return [init_weights(F, 64, A, HAND, 11), init_weights(F, 64, A, HAND, 12), PRESETS["piers"]]


def play(pool, **kw):
    from hanabi_sad_amd.eval import play_seatings
    return play_seatings(pool, SEATINGS, DEALS, SEED, 0, SAD, device=DEV, hand_size=HAND, records=True, names=NAMES, bot_seed=3, **RULES, **kw)


def by_game(res):
    return sorted(res.records, key=lambda r: (r.meta["seating"], r.meta["game"]))


def same(x, y):
    return np.array_equal(x.scores, y.scores) and np.array_equal(x.totals, y.totals) and by_game(x) == by_game(y)


@pytest.fixture(scope="module")
def greedy(pool):
    return play(pool)


@pytest.fixture(scope="module")
def mixed(pool):
    return play(pool, temperature=[0, 1, 0], sample_seed=7)


def test_no_temperature_and_zero_are_the_greedy_tournament(pool, greedy):
    assert len(greedy.records) == len(SEATINGS) * DEALS
    for t in (None, 0, 0.0, [0, 0, 0]):
        assert same(play(pool, temperature=t, sample_seed=9), greedy), t


def test_only_the_warm_member_leaves_its_greedy_move(pool, greedy, mixed):
    left = {k: 0 for k in range(3)}
    for r in mixed.records:
        r.validate()
        seats = SEATINGS[r.meta["seating"]]
        assert r.meta["seats"] == [NAMES[k] for k in seats]
        for i, (a, g) in enumerate(zip(r.moves, r.greedy)):
            left[seats[i % 2]] += a != g
    print("moves that are not the greedy one, per member:", left)
    assert left[0] == 0 and left[1] > 0
    assert not np.array_equal(mixed.scores, greedy.scores)
    # the seating without the warm member plays its greedy games
    assert np.array_equal(mixed.scores[2], greedy.scores[2]) and np.array_equal(mixed.scores[5], greedy.scores[5])
    assert same(play(pool, temperature=[0, 1, 0], sample_seed=7), mixed), "the same call gives other games"


def test_a_deal_plays_the_same_in_every_chunking(pool, mixed):
    S = len(SEATINGS)
    for per in (S * 24, S * 10):          # `mixed` played one chunk of 64 deals; here 24 + 24 + 16 and 6 x 10 + 4
        assert same(play(pool, temperature=[0, 1, 0], sample_seed=7, games_per_launch=per), mixed), per


def test_the_sample_seed_changes_the_games(pool, mixed):
    other = play(pool, temperature=[0, 1, 0], sample_seed=8)
    assert by_game(other) != by_game(mixed)
    assert np.array_equal(other.scores[5], mixed.scores[5])


def test_evaluate_plays_the_one_member_tournament(pool):
    """evaluate keys its draws like play_seatings -- (sample_seed; deal seed, seat, move) -- so its games are the rows of the seating
    that puts the one net on every seat"""
    from hanabi_sad_amd.eval import evaluate, play_seatings
    kw = dict(device=DEV, hand_size=HAND, **RULES)
    one = play_seatings([pool[1]], [(0, 0)], DEALS, SEED, 0, SAD, temperature=1.0, sample_seed=7, **kw)
    mean, perfect, scores, _ = evaluate(pool[1], DEALS, SEED, 0, SAD, temperature=1.0, sample_seed=7, **kw)
    assert scores == one.scores[0].tolist()
    assert scores != evaluate(pool[1], DEALS, SEED, 0, SAD, **kw)[2]
