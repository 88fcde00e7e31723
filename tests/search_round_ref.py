"""Plain-Python restatement of hsad_search_round (include/hsad.h), of search.round_world_order and of the round loop of
PolicySearch.search(rounds=...), written from their specification with Python ints only -- the yardstick of
tests/test_search_rounds_cpu.py / tests/test_search_rounds_gpu.py.  Also the seeded generator of the synthetic score tables both use."""
import random

ABSENT = 0xFF


def round_world_order(worlds):
    """the world indices sorted by the bit-reversed value of the index over (worlds - 1).bit_length() bits"""
    bits = (worlds - 1).bit_length() if worlds > 1 else 0

    def rev(w):
        r = 0
        for b in range(bits):
            r |= ((w >> b) & 1) << (bits - 1 - b)
        return r
    return sorted(range(worlds), key=rev)


def raw_sums(row):
    present = [int(s) for s in row if int(s) != ABSENT]
    return sum(present), len(present)


def paired_sums(row, ref):
    """(D, Q, n) = (sum d, sum d^2, count) over the worlds present in both rows, d = s - s_ref"""
    d = [int(s) - int(r) for s, r in zip(row, ref) if int(s) != ABSENT and int(r) != ABSENT]
    return sum(d), sum(x * x for x in d), len(d)


def prunes(D, Q, n, z2_num, z2_den, min_n):
    """the rule: n >= min_n, D < 0 and D^2 n z2_den > z2_num (n Q - D^2)"""
    return n >= min_n and D < 0 and D * D * n * z2_den > z2_num * (n * Q - D * D)


def search_round_ref(scores, first_pair, bp_pair, z2_num, z2_den, min_n, alive):
    """scores: n_pair rows of `worlds` ints (0xFF = absent); first_pair: n_game + 1 ascending pair indices; bp_pair: n_game pair indices;
    alive: n_pair ints.  -> dict(alive, leader, raw, paired_ref, paired_bp) of Python lists; the inputs are not written"""
    n_pair = len(scores)
    raw = [raw_sums(r) for r in scores]
    out_alive = [int(a) for a in alive]
    leader, paired_ref, paired_bp = [], [None] * n_pair, [None] * n_pair
    for k in range(len(first_pair) - 1):
        p0, p1, bp = first_pair[k], first_pair[k + 1], bp_pair[k]
        best = None
        for p in range(p0, p1):
            if alive[p] and raw[p][1] > 0 and (best is None or raw[p][0] * raw[best][1] > raw[best][0] * raw[p][1]):
                best = p                                       # strictly larger mean only: ties stay with the lowest index
        lead = bp if best is None else best
        leader.append(lead)
        for p in range(p0, p1):
            paired_ref[p] = paired_sums(scores[p], scores[lead])
            paired_bp[p] = paired_sums(scores[p], scores[bp])
            if alive[p] and p != lead and p != bp and prunes(*paired_ref[p], z2_num, z2_den, min_n):
                out_alive[p] = 0
    return dict(alive=out_alive, leader=leader, raw=[list(r) for r in raw], paired_ref=[list(x) for x in paired_ref],
                paired_bp=[list(x) for x in paired_bp])


def rounds_ref(flat, first_pair, bp_pair, rounds, z2_num, z2_den, min_n):
    """the round loop replayed over the table `flat` of a flat search (n_pair rows of sum(rounds) scores; 0xFF where the flat search
    counted nothing, e.g. worlds that consistent_only masks): round r uncovers the next rounds[r] worlds of round_world_order for
    every pair still alive whose game has more than one alive pair, then search_round_ref decides.
    -> dict(played: the table as uncovered (0xFF elsewhere), pruned_round, paired_bp, jobs: entries uncovered per round)"""
    n_pair, worlds = len(flat), sum(rounds)
    order = round_world_order(worlds)
    played = [[ABSENT] * worlds for _ in range(n_pair)]
    alive, pruned_round, jobs, off = [1] * n_pair, [-1] * n_pair, [], 0
    res = None
    for r, n_w in enumerate(rounds):
        ws, off = order[off:off + n_w], off + n_w
        count = 0
        for k in range(len(first_pair) - 1):
            mine = [p for p in range(first_pair[k], first_pair[k + 1]) if alive[p]]
            if r > 0 and len(mine) < 2:
                continue
            for p in mine:
                for w in ws:
                    played[p][w] = int(flat[p][w])
                count += len(ws)
        jobs.append(count)
        if count == 0:
            break
        res = search_round_ref(played, first_pair, bp_pair, z2_num, z2_den, min_n, alive)
        for p in range(n_pair):
            if alive[p] and not res["alive"][p]:
                pruned_round[p] = r
        alive = res["alive"]
    return dict(played=played, pruned_round=pruned_round, paired_bp=res["paired_bp"], jobs=jobs)


# ---------------------------------------------------------------------------------------------------------
# the synthetic tables
# ---------------------------------------------------------------------------------------------------------
GAME_PAIRS = (1, 2, 5, 21, 48, 3, 7)
WORLD_COUNTS = (1, 5, 64, 65, 130)
EQUALITY_ROWS = ((-3, -3, 1, 1), 1, 1), ((-4, -4, 0, 0), 4, 1)      # (d, z2_num, z2_den): D^2 n z2_den == z2_num (n Q - D^2)


def synthetic_table(worlds, seed=0):
    """-> dict(scores [n_pair][worlds], first_pair, bp_pair, alive): 7 games of GAME_PAIRS pairs.  Every pair has its own level (so
    that paired differences have a clear sign for some and not for others) plus a world effect shared by the game (common random
    numbers) plus noise; about 10 % of the entries are absent.  Planted: an all-absent row (game 3, its 3rd pair), a tie for the
    leader (game 4: pairs 40 and 45 share the best mean, with unequal counts; both lie past the 32 pairs whose raw sums the kernel keeps
    in LDS), dead pairs (alive = 0) among them one that would lead (game 3) and the only pair of game 0, and
    -- for worlds >= 5 -- the two equality rows in game 6 against a leader whose row is all present."""
    rng = random.Random(1000 * worlds + seed)
    first_pair, scores, alive, bp_pair = [0], [], [], []
    for k, n in enumerate(GAME_PAIRS):
        p0 = first_pair[-1]
        world_effect = [rng.randint(0, 8) for _ in range(worlds)]
        level = [rng.choice((2, 6, 9, 10, 10, 11, 11, 12)) for _ in range(n)]
        for i in range(n):
            row = [min(25, max(0, level[i] + world_effect[w] + rng.randint(-2, 2))) for w in range(worlds)]
            scores.append([ABSENT if rng.random() < 0.10 else s for s in row])
            alive.append(1)
        first_pair.append(p0 + n)
        bp_pair.append(p0 + rng.randrange(n))
    g3, g4, g6 = first_pair[3], first_pair[4], first_pair[6]
    alive[0] = 0                                        # game 0: no alive pair, so its leader is the blueprint's pair
    scores[g3 + 2] = [ABSENT] * worlds
    scores[g3 + 7] = [25] * worlds                      # would lead game 3 by far, but is dead
    alive[g3 + 7] = 0
    alive[g3 + 11] = 0
    if bp_pair[3] in (g3 + 2, g3 + 7, g3 + 11):
        bp_pair[3] = g3
    scores[g4 + 40], scores[g4 + 45] = [24] * worlds, [24] * worlds       # above every other level
    if worlds > 1:
        scores[g4 + 40][0] = ABSENT                      # equal means with unequal counts: the tie shows only by cross-multiplication
    if bp_pair[4] in (g4 + 40, g4 + 45):
        bp_pair[4] = g4
    if worlds >= 5:
        lead = [23 + (w % 2) for w in range(worlds)]    # all present, above every other level
        scores[g6] = lead
        for i, (d, _, _) in enumerate(EQUALITY_ROWS):
            row = [ABSENT] * worlds
            for w, dv in enumerate(d):
                row[w] = lead[w] + dv
            scores[g6 + 1 + i] = row
        bp_pair[6] = g6 + 3
    return dict(scores=scores, first_pair=first_pair, bp_pair=bp_pair, alive=alive)
