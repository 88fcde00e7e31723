"""CPU: the Python restatement of the exact hand belief (tests/hand_belief_ref.py: count by Moebius inversion over set partitions,
marginals, unrank, stratified rank) against brute-force enumeration of every hand, on 60 seeded random pools (counts between 0 and
the full deck's per type, 1 to 5 slots, random colour / rank masks).  These tests pass without the feature: they validate the
yardstick the header's harness (test_hand_count_cpu.py) and the GPU tests (test_hand_belief_gpu.py) are held to."""
import itertools
from collections import Counter

import pytest

from tests import determinize_ref as R
from tests import hand_belief_ref as B

CASES = 60
HIST_MAX = 3000


def enumerate_weights(pool, cms):
    """{hand tuple: number of assignments of physical cards} by walking every hand"""
    out = {}
    for hand in itertools.product(*[[t for t in range(25) if cm[t]] for cm in cms]):
        q, weight = list(pool), 1
        for t in hand:
            weight *= q[t]
            q[t] -= 1
        if weight > 0:
            out[hand] = weight
    return out


@pytest.fixture(scope="module")
def cases():
    out = []
    for c in range(CASES):
        k = B.seeded_case(c)
        k["weights"] = enumerate_weights(k["pool"], k["cms"])
        out.append(k)
    return out


def test_the_cases_cover_what_they_should(cases):
    assert {k["n"] for k in cases} == {1, 2, 3, 4, 5}
    totals = [sum(k["weights"].values()) for k in cases]
    assert any(t == 0 for t in totals) and any(0 < t <= HIST_MAX for t in totals) and any(t > HIST_MAX for t in totals)
    assert all(0 <= v <= B.FULL[t] for k in cases for t, v in enumerate(k["pool"]))


def test_count_equals_the_enumerated_weight_sum(cases):
    for c, k in enumerate(cases):
        assert B.total_of(k["pool"], k["cms"]) == sum(k["weights"].values()), c


def test_marginals_equal_the_enumerated_marginal_weights(cases):
    for c, k in enumerate(cases):
        want = [[0] * 25 for _ in range(k["n"])]
        for hand, w in k["weights"].items():
            for i, t in enumerate(hand):
                want[i][t] += w
        num = B.marginals(k["pool"], k["cms"])
        assert num == want, c
        N = sum(k["weights"].values())
        assert all(sum(row) == N for row in num), c
        tri = B.trinary(num, k["fireworks"])
        assert all(sum(row) == N for row in tri), c
        for i in range(k["n"]):
            assert tri[i][0] == sum(v for t, v in enumerate(want[i]) if t % 5 == k["fireworks"][t // 5]), c


def test_unrank_gives_every_hand_exactly_its_weight(cases):
    seen = 0
    for c, k in enumerate(cases):
        N = sum(k["weights"].values())
        if N > HIST_MAX:
            continue
        hist = Counter()
        for r in range(N):
            cards, q = B.unrank(k["pool"], k["cms"], r)
            hist[tuple(cards)] += 1
            left = list(k["pool"])
            for t in cards:
                left[t] -= 1
            assert q == left, (c, r)
            assert B.rank_of(k["pool"], k["cms"], cards) <= r, (c, r)
        for hand in k["weights"]:
            assert tuple(B.unrank(k["pool"], k["cms"], B.rank_of(k["pool"], k["cms"], list(hand)))[0]) == hand, c
        assert dict(hist) == k["weights"], c
        with pytest.raises(ValueError):
            B.unrank(k["pool"], k["cms"], N)
        seen += N > 0
    assert seen >= 30


def test_exact_distribution_is_the_same_weights(cases):
    for c, k in enumerate(cases[:20]):
        N = sum(k["weights"].values())
        if N == 0:
            continue
        dist = R.exact_distribution(k["pool"], k["masks"])
        assert {h: round(p * N) for h, p in dist.items()} == k["weights"], c


def test_stratified_rank_lies_in_its_stratum(cases):
    for c, k in enumerate(cases):
        N = sum(k["weights"].values())
        for W in (1, 2, k["W"], 16, 2 * N + 1, 1 << 20):
            ws = range(W) if W <= 64 else list(range(0, W, max(1, W // 37))) + [W - 1]
            for w in ws:
                lo, hi = B.stratum_bounds(N, w, W)
                for r in (B.rank_from_u64(N, w, W, 0), B.rank_from_u64(N, w, W, B.M64), B.rank_from_u64(N, w, W, k["u64"]),
                          B.stratified_rank(N, w, W, (c << 32) | w, 12345 + c)):
                    assert (lo <= r < hi) if hi > lo else r == lo, (c, W, w)
        # the strata tile [0, N)
        W = k["W"]
        assert B.stratum_bounds(N, 0, W)[0] == 0 and B.stratum_bounds(N, W - 1, W)[1] == N
        assert all(B.stratum_bounds(N, w, W)[1] == B.stratum_bounds(N, w + 1, W)[0] for w in range(W - 1))
