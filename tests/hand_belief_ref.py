"""Python-int restatement of the exact hand belief (include/hsad.h: hsad_env_hand_belief / hsad_env_determinize_exact), written from
its specification and independent of hanabi_sad_amd/csrc/hsad_hand_count.h: the count of the assignments of physical unseen cards to
the hand's slots that agree with the card knowledge, the per-slot marginals, the trinary marginals, the unranking map and the
stratified rank.  Pools are lists of 25 counts by card type colour * 5 + rank, compat lists are tests/determinize_ref.compat's;
rows are export_state rows (layout: tests/determinize_ref.py)."""
import functools
import itertools
from math import factorial

import numpy as np

from tests.determinize_ref import HANDS, M64, compat, hand_of, policy_hash

STREAM = 65   # the hash stream of the stratified rank (the rejection sampler's is 64)


def s_of(q, cms, B):
    """number of cards of q plausible for every slot of B (a tuple of slot numbers)"""
    return sum(q[t] for t in range(25) if all(cms[i][t] for i in B))


def count(q, cms, S):
    """C(S, q): injective assignments of physical cards of q to the slots S (a sorted tuple)"""
    return _count(tuple(q), tuple(tuple(cm) for cm in cms), tuple(S))


@functools.lru_cache(maxsize=1 << 16)
def _count(q, cms, S):
    if not S:
        return 1
    first, rest = S[0], S[1:]
    total = 0
    for k in range(len(rest) + 1):
        for extra in itertools.combinations(rest, k):
            B = (first,) + extra
            left = tuple(i for i in rest if i not in extra)
            total += (-1) ** (len(B) - 1) * factorial(len(B) - 1) * s_of(q, cms, B) * _count(q, cms, left)
    return total


def less_one(q, t):
    q = list(q)
    q[t] -= 1
    return q


def total_of(pool, cms):
    return count(pool, cms, tuple(range(len(cms))))


def marginals(pool, cms):
    """num[i][t] = pool[t] compat_i[t] C(all \\ {i}, pool - e_t)"""
    n = len(cms)
    num = [[0] * 25 for _ in range(n)]
    for i in range(n):
        others = tuple(j for j in range(n) if j != i)
        for t in range(25):
            if pool[t] and cms[i][t]:
                num[i][t] = pool[t] * count(less_one(pool, t), cms, others)
    return num


def trinary(num, fireworks):
    """tri[i] = [playable, rank below the firework, rank above it] (the classes of EncodeOwnHandTrinary)"""
    tri = [[0, 0, 0] for _ in num]
    for i, row in enumerate(num):
        for t, v in enumerate(row):
            r, fw = t % 5, fireworks[t // 5]
            tri[i][0 if r == fw else (1 if r < fw else 2)] += v
    return tri


def unrank(pool, cms, r):
    """-> (cards in slot order, the pool that is left); r in [0, N)"""
    n = len(cms)
    q = list(pool)
    cards = []
    for i in range(n):
        later = tuple(range(i + 1, n))
        for t in range(25):
            if q[t] * cms[i][t] == 0:
                continue
            c = count(less_one(q, t), cms, later)
            w = q[t] * c
            if r < w:
                cards.append(t)
                q[t] -= 1
                r %= c
                break
            r -= w
        else:
            raise ValueError("rank outside [0, N)")
    return cards, q


def rank_of(pool, cms, hand):
    """the lowest of the ranks that unrank to `hand`: per slot, the ranks taken by the lower types"""
    q, r, n = list(pool), 0, len(hand)
    for i, card in enumerate(hand):
        later = tuple(range(i + 1, n))
        r += sum(q[t] * count(less_one(q, t), cms, later) for t in range(card) if q[t] * cms[i][t])
        q[card] -= 1
    return r


def stratum_bounds(N, w, W):
    return (w * N) // W, ((w + 1) * N) // W


def rank_from_u64(N, w, W, u64):
    lo, hi = stratum_bounds(N, w, W)
    return lo if hi == lo else lo + ((u64 * (hi - lo)) >> 64)


def stratified_rank(N, w, W, key, seed):
    u64 = (policy_hash(seed, key & M64, 0, STREAM) << 32) | policy_hash(seed, key & M64, 1, STREAM)
    return rank_from_u64(N, w, W, u64)


# ---- on export_state rows ---------------------------------------------------------------------------------------------------------
def pool_and_masks(row, P, H, p):
    """-> (pool, [compat list per occupied slot], the hand's cards)"""
    hand = hand_of(row, P, H, p)
    pool = [int(row[t]) for t in range(25)]
    for card, _, _ in hand:
        pool[card] += 1
    return pool, [compat(cp, rp) for _, cp, rp in hand], [card for card, _, _ in hand]


def belief_row(row, P, H, p):
    """-> (N, counts [H][25], trinary [H][3]) of player p's hand; empty slots are zero"""
    pool, cms, _ = pool_and_masks(row, P, H, p)
    num = marginals(pool, cms)
    tri = trinary(num, [int(row[50 + c]) for c in range(5)])
    pad = H - len(cms)
    return total_of(pool, cms), num + [[0] * 25] * pad, tri + [[0, 0, 0]] * pad


def determinize_exact_row(row, P, H, p, r):
    """-> the export_state row with player p's hand unranked from r"""
    row = np.array(row, dtype=np.int32, copy=True)
    pool, cms, _ = pool_and_masks(row, P, H, p)
    cards, q = unrank(pool, cms, r)
    row[0:25] = q
    for i, card in enumerate(cards):
        row[HANDS + (p * H + i) * 6] = card
    return row


# ---- seeded cases shared with tests/hand_count/hand_count_main.cc (the formula: tests/test_hand_count_cpu.py) ------------------------
FULL = [3 if t % 5 == 0 else (1 if t % 5 == 4 else 2) for t in range(25)]


class Gen:
    def __init__(self, c):
        self.x = ((c + 1) * 0x9E3779B97F4A7C15) & M64

    def raw(self):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & M64
        return self.x

    def next(self):
        return self.raw() >> 33


def seeded_case(c):
    """-> dict(n, pool, masks [(colour mask, rank mask)], cms, fireworks, W, u64)"""
    g = Gen(c)
    n = 1 + g.next() % 5
    pool = [g.next() % (FULL[t] + 1) for t in range(25)]
    masks = []
    for _ in range(n):
        cp = 1 + g.next() % 31
        rp = 1 + g.next() % 31
        masks.append((cp, rp))
    fireworks = [g.next() % 6 for _ in range(5)]
    W = 1 + g.next() % 40
    return dict(n=n, pool=pool, masks=masks, cms=[compat(cp, rp) for cp, rp in masks], fireworks=fireworks, W=W, u64=g.raw())
