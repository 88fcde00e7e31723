"""CPU: the yardstick of the search in rounds (tests/search_round_ref.py) held to exact rational arithmetic, the conditions the
synthetic score tables must meet (asserted from the reference alone, so that the GPU test of hsad_search_round compares something),
search.round_world_order, search.choose_action_paired and the argument checks of the round loop."""
import ctypes as C
import itertools
import os
import re
from fractions import Fraction

import pytest
import torch

from tests import search_round_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z2 = ((0, 1), (1, 1), (4, 1))


def exact_prunes(d, z2, min_n):
    """mean + z sem < 0 in rationals, squared on the side where both are non-negative: mean = D / n, sem^2 = var / n with the population
    variance; for mean < 0:  mean + z sem < 0  <=>  z sem < -mean  <=>  z^2 sem^2 < mean^2"""
    n = len(d)
    if n < min_n or n == 0:
        return False
    mean = Fraction(sum(d), n)
    var = Fraction(sum(x * x for x in d), n) - mean * mean
    return mean < 0 and z2 * var / n < mean * mean


def test_the_rule_equals_exact_rationals_on_small_exhaustive_inputs():
    checked = pruned = 0
    for n in range(1, 6):
        for d in itertools.combinations_with_replacement(range(-4, 3), n):      # the sums do not depend on the order
            D, Q = sum(d), sum(x * x for x in d)
            for num, den in Z2 + ((1, 4), (9, 4)):
                want = exact_prunes(d, Fraction(num, den), 2)
                assert R.prunes(D, Q, n, num, den, 2) == want, (d, num, den)
                checked += 1
                pruned += want
    assert checked == 5 * 791 and 0 < pruned < checked          # 791 multisets of 1..5 values out of 7


def test_the_two_equality_cases_are_not_pruned():
    for d, num, den in R.EQUALITY_ROWS:
        D, Q, n = sum(d), sum(x * x for x in d), len(d)
        assert D < 0 and D * D * n * den == num * (n * Q - D * D)
        assert not R.prunes(D, Q, n, num, den, 2) and not exact_prunes(d, Fraction(num, den), 2)
        assert R.prunes(D - 1, Q - 2 * d[-1] + 1, n, num, den, 2)              # one point lower in its last world: pruned
    assert R.prunes(-1, 1, 1, 0, 1, 1) and not R.prunes(-1, 1, 1, 0, 1, 2)     # min_n
    assert not R.prunes(0, 4, 4, 0, 1, 2)                                       # D = 0 is never pruned


def test_paired_sums_and_leader_on_a_hand_written_table():
    A = R.ABSENT
    scores = [[3, 5, A, 7],        # game 0: mean 5
              [6, A, 6, 6],        # mean 6: the leader
              [9, 9, 9, 9],        # dead
              [A, A, A, A],
              [12, 0, 6, A]]       # mean 6 too: the tie goes to pair 1
    res = R.search_round_ref(scores, [0, 5], [0], 0, 1, 2, [1, 1, 0, 1, 1])
    assert res["leader"] == [1] and res["raw"] == [[15, 3], [18, 3], [36, 4], [0, 0], [18, 3]]
    assert res["paired_ref"] == [[-2, 10, 2], [0, 0, 3], [9, 27, 3], [0, 0, 0], [6, 36, 2]]
    assert res["paired_bp"] == [[0, 0, 3], [2, 10, 2], [12, 56, 3], [0, 0, 0], [4, 106, 2]]
    assert res["alive"] == [1, 1, 0, 1, 1]           # pair 0 is the blueprint's: never pruned, whatever its D
    res = R.search_round_ref(scores, [0, 5], [4], 0, 1, 2, [1, 1, 0, 1, 1])
    assert res["alive"] == [0, 1, 0, 1, 1]
    res = R.search_round_ref(scores, [0, 5], [4], 0, 1, 2, [0, 0, 0, 1, 0])      # no alive pair with an entry: the blueprint's leads
    assert res["leader"] == [4] and res["alive"] == [0, 0, 0, 1, 0]


@pytest.mark.parametrize("worlds", R.WORLD_COUNTS)
def test_the_synthetic_tables_meet_their_conditions(worlds):
    t = R.synthetic_table(worlds)
    fp, bp = t["first_pair"], t["bp_pair"]
    assert [b - a for a, b in zip(fp, fp[1:])] == list(R.GAME_PAIRS) and len(t["scores"]) == sum(R.GAME_PAIRS)
    cells = [s for row in t["scores"] for s in row]
    assert all(0 <= s <= 25 or s == R.ABSENT for s in cells)
    if worlds >= 64:
        assert 0.05 < sum(s == R.ABSENT for s in cells) / len(cells) < 0.15
    g3, g4, g6 = fp[3], fp[4], fp[6]
    for num, den in Z2:
        res = R.search_round_ref(t["scores"], fp, bp, num, den, 2, t["alive"])
        was = sum(t["alive"])
        gone = was - sum(res["alive"])
        others = [p for k in range(7) for p in range(fp[k], fp[k + 1]) if t["alive"][p] and p != res["leader"][k] and p != bp[k]]
        kept = [p for p in others if res["alive"][p]]
        print("worlds %d z^2 %d/%d: %d of %d alive pairs pruned, %d other pairs kept" % (worlds, num, den, gone, was, len(kept)))
        assert res["leader"][0] == bp[0] == 0 and res["raw"][g3 + 2] == [0, 0]
        assert res["leader"][3] != g3 + 7 and res["alive"][g3 + 7] == 0 and res["alive"][g3 + 11] == 0       # dead pairs stay dead
        assert res["leader"][4] == g4 + 40                                      # the tie: the lower index leads
        if worlds > 1:
            a, b = res["raw"][g4 + 40], res["raw"][g4 + 45]
            assert a[1] != b[1] and a[0] * b[1] == b[0] * a[1]
        if worlds == 1:
            assert gone == 0                                                   # min_n = 2
            continue
        assert gone >= 1 and len(kept) >= 1
        assert all(res["alive"][p] == t["alive"][p] for p in bp)               # the blueprint's pair is never pruned
        assert res["leader"][6] == g6
        for i, (d, e_num, e_den) in enumerate(R.EQUALITY_ROWS):
            D, Q, n = res["paired_ref"][g6 + 1 + i]
            assert (D, Q, n) == (sum(d), sum(x * x for x in d), len(d))
            assert bool(res["alive"][g6 + 1 + i]) == (not exact_prunes(d, Fraction(num, den), 2))
            if (num, den) == (e_num, e_den):
                assert res["alive"][g6 + 1 + i] == 1                           # equality does not prune


def test_rounds_ref_uncovers_a_flat_table_round_by_round():
    t = R.synthetic_table(8, seed=1)
    flat = [[0 if s == R.ABSENT else s for s in row] for row in t["scores"]]      # every entry present: "played" shows as != 0xFF
    fp, rounds = t["first_pair"], (2, 2, 4)
    out = R.rounds_ref(flat, fp, t["bp_pair"], rounds, 4, 1, 2)
    order, upto = R.round_world_order(8), (2, 4, 8)
    n_played = 0
    for p, row in enumerate(out["played"]):
        got = [w for w in range(8) if row[w] != R.ABSENT]
        assert len(got) in upto and sorted(order[:len(got)]) == got                # a prefix of the world order, whole rounds
        assert all(row[w] == flat[p][w] for w in got)
        r = out["pruned_round"][p]
        if r >= 0:
            assert len(got) == upto[r]                                             # dropped after round r: nothing later
        n_played += len(got)
    assert len(out["played"][0]) == 8 and sum(s != R.ABSENT for s in out["played"][0]) == 2     # game 0 has one pair: round 0 only
    assert sum(out["jobs"]) == n_played < 8 * len(flat) and out["jobs"][0] == 2 * len(flat)
    assert min(out["pruned_round"]) == -1 and len(set(out["pruned_round"])) >= 3
    assert all(out["pruned_round"][b] == -1 for b in t["bp_pair"])
    assert out["paired_bp"] == R.search_round_ref(out["played"], fp, t["bp_pair"], 4, 1, 2, [1] * len(flat))["paired_bp"]


# ---------------------------------------------------------------------------------------------------------
# search.py: the world order, the choice, the argument checks, the entry points
# ---------------------------------------------------------------------------------------------------------
def test_round_world_order():
    from hanabi_sad_amd.search import round_world_order
    assert round_world_order(8) == [0, 4, 2, 6, 1, 5, 3, 7] and round_world_order(6) == [0, 4, 2, 1, 5, 3]
    for worlds in list(range(1, 40)) + [64, 100, 130, 4096]:
        order = round_world_order(worlds)
        assert order == R.round_world_order(worlds) and sorted(order) == list(range(worlds)) and order[0] == 0
    for worlds in (8, 64, 4096):       # every power-of-two prefix is evenly spread: the multiples of worlds / m
        for m in (1, 2, 4, 8):
            assert sorted(round_world_order(worlds)[:m]) == list(range(0, worlds, worlds // m))
    for worlds in (6, 100, 130):       # other counts: a prefix of m = 2^j holds one world of every block of 2^bits / m indices that has any
        bits = (worlds - 1).bit_length()
        for j in range(bits):
            block = (1 << bits) >> j
            first = sorted(w for w in range(0, worlds, block))
            assert sorted(round_world_order(worlds)[:len(first)]) == first


def _sv(paired, pruned, blueprint):
    from hanabi_sad_amd.search import SearchValues
    paired = torch.tensor(paired, dtype=torch.int64)
    totals = torch.zeros(paired.shape[0], paired.shape[1], 3, dtype=torch.int64)
    return SearchValues(totals, torch.tensor(blueprint), None, paired=paired, pruned_round=torch.tensor(pruned, dtype=torch.int32),
                        world_scores=torch.zeros(paired.shape[0], paired.shape[1], 1, dtype=torch.uint8))


def test_choose_action_paired():
    from hanabi_sad_amd.search import SearchValues, choose_action_paired
    none = [0, 0, 0]
    #          action 0 (blueprint)  1: +0.5 +/- 0.25   2: +0.5, tie     3: +2.0 but pruned  4: never played
    game = [[0, 0, 8], [4, 6, 8], [4, 4, 8], [16, 40, 8], none]
    sv = _sv([game, game, [[0, 0, 8], [-8, 8, 8], none, none, none], game], [[-1, -1, -1, 0, -1]] * 4, [0, 0, 0, -1])
    assert sv.paired_mean.dtype == torch.float32 and sv.paired_sem.dtype == torch.float32
    assert sv.paired_mean[0].tolist()[:4] == [0.0, 0.5, 0.5, 2.0] and bool(torch.isnan(sv.paired_mean[0, 4]))
    assert sv.paired_sem[0, 0] == 0.0 and abs(float(sv.paired_sem[0, 1]) - (6 / 8 - 0.25) ** 0.5 / 8 ** 0.5) < 1e-7
    # the best candidate is action 1 (lowest uid of the tie; the pruned action 3 never wins); game 2 has no gain; -1 passes through
    assert choose_action_paired(sv).tolist() == [1, 1, 0, -1]
    assert choose_action_paired(sv, threshold=0.5).tolist() == [0, 0, 0, -1]            # the gain must EXCEED the threshold
    assert choose_action_paired(sv, threshold=0.49).tolist() == [1, 1, 0, -1]
    sem1 = float(sv.paired_sem[0, 1])
    assert choose_action_paired(sv, z=0.5 / sem1 * 0.99).tolist() == [1, 1, 0, -1]     # the z test on the best action's own sem
    assert choose_action_paired(sv, z=0.5 / sem1 * 1.01).tolist() == [0, 0, 0, -1]
    assert choose_action_paired(sv, threshold=float("inf")).tolist() == [0, 0, 0, -1]
    flat = SearchValues(torch.zeros(1, 5, 3, dtype=torch.int64), torch.tensor([0]))
    assert flat.paired is None and flat.paired_mean is None and flat.paired_sem is None and flat.pruned_round is None and flat.world_scores is None
    with pytest.raises(ValueError):
        choose_action_paired(flat)


def test_round_arguments_are_checked():
    from hanabi_sad_amd.search import _check_rounds
    assert _check_rounds((2, 2, 4), 8, 2.0, 2) == ((2, 2, 4), 4, 1)
    assert _check_rounds([8], 8, 0.5, 2) == ((8,), 1, 4) and _check_rounds((8,), 8, 0, 1) == ((8,), 0, 1)
    assert _check_rounds((4096,), 4096, 128.0, 2) == ((4096,), 16384, 1)
    num, den = _check_rounds((8,), 8, 1.96, 2)[1:]
    assert 1 <= den <= 1024 and abs(num / den - 1.96 ** 2) < 1e-3
    for rounds, worlds, z, min_n in (((2, 2), 8, 2.0, 2), ((), 0, 2.0, 2), ((8, 0), 8, 2.0, 2), ((-1, 9), 8, 2.0, 2), (8, 8, 2.0, 2),
                                     ((4097,), 4097, 2.0, 2), ((8,), 8, 129.0, 2), ((8,), 8, -1.0, 2), ((8,), 8, 2.0, 0)):
        with pytest.raises(ValueError):
            _check_rounds(rounds, worlds, z, min_n)


DECLARED = {
    "hsad_search_world_scores": "int hsad_search_world_scores(const hsad_env* env, const int32_t* pair, const int32_t* world, int n_pair, "
                                "int worlds, uint8_t* scores, void* stream);",
    "hsad_search_round": "int hsad_search_round(const uint8_t* scores, int n_pair, int worlds, const int32_t* first_pair, int n_game, "
                         "const int32_t* bp_pair, int z2_num, int z2_den, int min_n, uint8_t* alive, int32_t* leader_out, int64_t* raw_out, "
                         "int64_t* paired_ref_out, int64_t* paired_bp_out, void* stream);",
}


def test_header_ctypes_table_and_callers_carry_the_entry_points():
    import inspect
    from hanabi_sad_amd import _lib, eval_model, search
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hsad.h")).read(), flags=re.S)
    for name, want in DECLARED.items():
        found = re.findall(r"\bint\s+%s\s*\([^;]*\);" % name, txt)
        assert len(found) == 1 and re.sub(r"\s+", " ", found[0]) == want, name
        restype, argtypes = _lib.SIGNATURES[name]
        args = want[want.index("(") + 1:want.rindex(")")].split(", ")
        assert restype is C.c_int and argtypes == [C.c_void_p if "*" in a else C.c_int for a in args], name
    for fn in (search.PolicySearch.search, search.policy_action_values):
        p = inspect.signature(fn).parameters
        assert (p["rounds"].default, p["prune_z"].default, p["min_n"].default) == (None, 2.0, 2)
    p = inspect.signature(search.play_with_search).parameters
    assert (p["rounds"].default, p["prune_z"].default, p["deviate_z"].default) == (None, 2.0, 0.0)
    args = eval_model.parse_args(["--search_worlds", "32", "--search_rounds", "8,8,16", "--search_prune_z", "1.5", "--search_deviate_z", "1"])
    assert args.search_rounds == (8, 8, 16) and args.search_prune_z == 1.5 and args.search_deviate_z == 1.0
    args = eval_model.parse_args([])
    assert args.search_rounds is None and args.search_prune_z == 2.0 and args.search_deviate_z == 0.0
