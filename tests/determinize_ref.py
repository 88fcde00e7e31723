"""numpy / Python-int restatement of hsad_env_determinize (include/hsad.h), written from its specification and independent of the
kernel: the counter-based hash (mix64 / policy_hash), the slot-wise proposal from the shrinking pool and the acceptance test.  Works on
rows of export_state (layout: hanabi_sad_amd/csrc/hsad_env.hip export_state_kernel): words 0..24 deck counts by card type
colour * 5 + rank, 80 + (p * H + i) * 6 + {0 card or -1, 1 colour-plausible mask, 2 rank-plausible mask} per hand slot."""
import itertools

import numpy as np

M64 = (1 << 64) - 1
MAX_TRIES = 32
HANDS = 80   # first hand word of an export_state row


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def policy_hash(seed, game, counter, stream):
    k = mix64((seed & M64) ^ mix64(((game & M64) * 0xD1342543DE82EF95 + stream) & M64))
    return mix64((k + counter) & M64) >> 32


def compat(cp, rp):
    """compat[t] for t = colour * 5 + rank"""
    return [((cp >> (t // 5)) & 1) & ((rp >> (t % 5)) & 1) for t in range(25)]


def sample_hand(pool, masks, key, seed):
    """pool: 25 counts (deck + the viewer's hand); masks: [(colour mask, rank mask)] per slot.
    -> (cards, q, tries) on acceptance, (None, None, -1) after MAX_TRIES failed tries"""
    cms = [compat(cp, rp) for cp, rp in masks]
    zmax = 1
    for cm in cms:
        zmax *= sum(pool[t] * cm[t] for t in range(25))
    for t_ in range(MAX_TRIES):
        q = list(pool)
        zprod, cards, ok = 1, [], True
        for i, cm in enumerate(cms):
            Z = sum(q[t] * cm[t] for t in range(25))
            if Z == 0:
                ok = False
                break
            h = policy_hash(seed, key, t_ * 8 + i, 64)
            k = (h * Z) >> 32
            run, card = 0, -1
            for t in range(25):
                run += q[t] * cm[t]
                if run > k:
                    card = t
                    break
            q[card] -= 1
            zprod *= Z
            cards.append(card)
        if not ok:
            continue
        u = policy_hash(seed, key, t_ * 8 + 7, 64)
        assert u * zmax < 1 << 61 and zprod << 32 < 1 << 61
        if u * zmax < zprod << 32:
            return cards, q, t_ + 1
    return None, None, -1


def hand_of(row, P, H, p):
    """[(card, colour mask, rank mask)] of player p's occupied slots"""
    out = []
    for i in range(H):
        s = HANDS + (p * H + i) * 6
        if row[s] >= 0:
            out.append((int(row[s]), int(row[s + 1]), int(row[s + 2])))
    return out


def determinize_row(row, P, H, p, key, seed):
    """-> (new export_state row, tries) for a live game with viewer p"""
    row = np.array(row, dtype=np.int32, copy=True)
    hand = hand_of(row, P, H, p)
    pool = [int(row[t]) for t in range(25)]
    for card, _, _ in hand:
        pool[card] += 1
    cards, q, tries = sample_hand(pool, [(cp, rp) for _, cp, rp in hand], key, seed)
    if cards is not None:
        row[0:25] = q
        for i, card in enumerate(cards):
            row[HANDS + (p * H + i) * 6] = card
    return row, tries


def exact_distribution(pool, masks):
    """{hand tuple: probability}: uniform over assignments of physical cards = weight prod of the falling counts"""
    cms = [compat(cp, rp) for cp, rp in masks]
    w = {}
    for hand in itertools.product(*[[t for t in range(25) if cm[t]] for cm in cms]):
        q, weight = list(pool), 1
        for t in hand:
            weight *= q[t]
            q[t] -= 1
        if weight > 0:
            w[hand] = weight
    total = sum(w.values())
    return {h: v / total for h, v in w.items()}
