"""Behaviour counters without a device: the reference classifier (tests/behaviour_ref.py) on hand-written positions with the expected
increments written here, csrc/hsad_behaviour.h compiled alone under the sanitizers against that reference on every move of games
the reference bots play against each other, and the coverage those games must reach.  The kernel and the path up to the commands
are held to the same reference in test_behaviour_gpu.py.  Everything is integer logic: every comparison is exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from hanabi_sad_amd import position as pos
from hanabi_sad_amd.position import Card, Position
from tests import behaviour_cases as bc
from tests import behaviour_ref as bref
from tests.search_fixtures import CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, C3R4 = CONFIGS["full"], CONFIGS["c3r4"]

# full game, 2 players: discard slot i = i, play = 5 + i, colour hint = 10 + colour, rank hint = 15 + rank, noop = 20
# c3r4, 3 players: discard = i, play = 4 + i, colour hint = 8 + 3 (o - 1) + colour, rank hint = 14 + 4 (o - 1) + rank, noop = 22
OWN = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1)]          # seat 0: knows nothing, holds nothing playable on empty fireworks
PARTNER = [(3, 3), (3, 4), (4, 3), (4, 4), (2, 3)]      # seat 1: nothing playable, nothing dead, no colour 0 or 1, no rank 0..2
PARTNER_B = [(4, 0), (3, 4), (4, 3), (4, 4), (2, 3)]    # ... without the (3, 3)
PARTNER_C = [(2, 0), (2, 3), (4, 3), (4, 4), (3, 3)]    # two cards of colour 2, one of them playable on empty fireworks


def exactly(c, r):
    return Card(c, r, colours=1 << c, ranks=1 << r, hinted_colour=c, hinted_rank=r)


def swap(hand, i, card):
    return hand[:i] + [card] + hand[i + 1:]


def full2(own=OWN, partner=PARTNER, **kw):
    return Position(FULL, [list(own), list(partner)], **kw)


def vec(info, **kw):
    """the expected increments: MOVES = 1, INFO_SUM = info, and the counters named"""
    out = [0] * bref.NSTAT
    out[bref.MOVES], out[bref.INFO_SUM] = 1, info
    for k, v in kw.items():
        out[bref.NAMES.index(k)] = v
    return out


NOTHING = [0] * bref.NSTAT
HANDS3 = [[(1, 0), (1, 2), (2, 2), (2, 3)], [(0, 2), (0, 3), (1, 1), (2, 1)], [(1, 3), (2, 1), (0, 2), (0, 1)]]
SHUFFLED = [[2, 0, 1, 3, 4], [0, 1, 2, 3, 4]]            # seat 0 names the colours 0, 1, 2 as 2, 0, 1


def cases():
    """[(what, position, uid, expected 13 increments)]"""
    out = []

    def case(what, P_, uid, want):
        out.append((what, P_, uid, want))

    # ---- plays ----
    # slot 2 is known to be (1, 0), playable on empty fireworks: play_i == n_i
    case("good play, certain", full2(swap(OWN, 2, exactly(1, 0))), 7, vec(8, PLAY_OK=1, PLAY_CERTAIN=1))
    case("good play, not certain", full2(swap(OWN, 2, (1, 0))), 7, vec(8, PLAY_OK=1))
    case("misplay at life 2", full2(life=2, info=5), 5, vec(5, PLAY_FAIL=1))
    case("misplay at life 1", full2(life=1, info=5), 5, vec(5, PLAY_FAIL=1, LAST_LIFE=1))
    # the other (0, 1) is discarded and firework 0 still needs it
    case("misplay of the last copy of a needed card", full2(discards=[(0, 1)]), 5, vec(8, PLAY_FAIL=1, LAST_COPY_LOST=1))
    # ---- discards ----
    # firework 0 at 1, slot 1 known to be (0, 0)
    case("certain-dead discard", full2(swap(OWN, 1, exactly(0, 0)), fireworks=[1, 0, 0, 0, 0], info=7), 1,
         vec(7, DISCARD=1, DISCARD_CERTAIN_DEAD=1))
    case("discard of the last copy of a needed card", full2(discards=[(0, 1)], info=7), 0, vec(7, DISCARD=1, LAST_COPY_LOST=1))
    # both (3, 2) are gone, so (3, 3) is dead; one (3, 3) is discarded and slot 0 holds the other (its holder knows nothing of it)
    case("discard of the last copy of a dead card", full2(swap(OWN, 0, (3, 3)), PARTNER_B, discards=[(3, 2), (3, 2), (3, 3)], info=5), 0,
         vec(5, DISCARD=1))
    # ... and when the holder knows the card, the blocked colour makes the discard certain-dead
    case("discard of a card dead by a fully discarded lower rank",
         full2(swap(OWN, 0, exactly(3, 3)), PARTNER_B, discards=[(3, 2), (3, 2)], info=5), 0, vec(5, DISCARD=1, DISCARD_CERTAIN_DEAD=1))
    # ---- hints ----
    case("colour hint touching two cards, one playable", full2(OWN, PARTNER_C), 12, vec(8, HINT_COLOUR=1, HINT_CARDS=2, HINT_PLAYABLE=1))
    case("rank hint touching none playable", full2(info=4), 18, vec(4, HINT_RANK=1, HINT_CARDS=3))
    # 3 players, seat 1 on turn: offset 1 is seat 2, offset 2 is seat 0; firework 0 at 1, so seat 0's (1, 0) is playable
    case("3 players, colour hint at offset 2", Position(C3R4, HANDS3, fireworks=[1, 0, 0], mover=1), 12,
         vec(6, HINT_COLOUR=1, HINT_CARDS=2, HINT_PLAYABLE=1))
    case("3 players, the same colour at offset 1", Position(C3R4, HANDS3, fireworks=[1, 0, 0], mover=1), 9, vec(6, HINT_COLOUR=1, HINT_CARDS=1))
    case("3 players, rank hint at offset 2", Position(C3R4, HANDS3, fireworks=[1, 0, 0], mover=1), 20, vec(6, HINT_RANK=1, HINT_CARDS=2))
    # the uid says colour 1, the actor's permutation sends colour 2 there: the partner's two cards of colour 2
    case("shuffle_color: the uid's colour is not the cards'", full2(OWN, PARTNER_C, perms=SHUFFLED), 11,
         vec(8, HINT_COLOUR=1, HINT_CARDS=2, HINT_PLAYABLE=1))
    # ---- nothing counted ----
    case("shuffle_color: the uid that names colour 0, which the partner does not hold", full2(OWN, PARTNER_C, perms=SHUFFLED), 12, NOTHING)
    case("the noop", full2(), 20, NOTHING)
    case("a uid past the noop", full2(), 21, NOTHING)
    case("a negative uid", full2(), -1, NOTHING)
    case("a hint touching no card", full2(), 10, NOTHING)
    return out


CASES = cases()


@pytest.mark.parametrize("what,P_,uid,want", CASES, ids=[c[0] for c in CASES])
def test_hand_written_positions(what, P_, uid, want):
    shuffled = any(row != [0, 1, 2, 3, 4] for row in P_.perms)
    assert pos.validate(P_.to_record(), P_.rules, dict(shuffle_color=shuffled)) == 0, "the test's own position is not one"
    before = repr(P_)
    assert bref.classify(P_, uid) == want
    assert repr(P_) == before


def last_round():
    """the last round on an empty deck: the mover holds four cards, slot 4 is empty"""
    own, partner = OWN[:4], PARTNER
    left = pos.full_deck(FULL)
    for c, r in own + partner:
        left[c * 5 + r] -= 1
    return Position(FULL, [own, partner], discards=left, deck=[0] * 25, turns_to_play=1, info=3)


def test_an_empty_slot_counts_nothing():
    P_ = last_round()
    assert pos.validate(P_.to_record(), FULL) == 0
    assert bref.classify(P_, 4) == NOTHING and bref.classify(P_, 9) == NOTHING
    assert bref.classify(P_, 3)[bref.DISCARD] == 1 and bref.classify(P_, 8)[bref.PLAY_FAIL] == 1


def test_games_reach_every_counter():
    """over the games the header is compared on, the reference's own sums have every counter >= 1, and both hint kinds occur under
    shuffle_color"""
    sums = {k: np.sum([e[3] for e in entries], axis=0) for k, entries in bc.games().items()}
    assert sorted(sums) == sorted((c, s) for c in ("full", "c3r4", "small") for s in (False, True))
    total = np.sum(list(sums.values()), axis=0)
    assert total.shape == (bref.NSTAT,) and int(total.min()) >= 1, dict(zip(bref.NAMES, total.tolist()))
    for (config, sc), s in sums.items():
        if sc:
            assert s[bref.HINT_COLOUR] >= 1 and s[bref.HINT_RANK] >= 1, (config, s.tolist())


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("behaviour") / "behaviour_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hanabi_sad_amd", "csrc"), os.path.join(ROOT, "tests", "behaviour", "behaviour_main.cc"),
                           "-o", exe])
    return exe


def run_harness(exe, rules, shuffle_color, entries):
    """entries: [(record, uid)] -> [(seat, the 13 increments)]"""
    head = "%d %d %d %d %d %d %d %d\n" % (rules["players"], rules["hand_size"], rules["colors"], rules["ranks"],
                                          rules["max_information_tokens"], rules["max_life_tokens"], int(shuffle_color), len(entries))
    text = head + "".join(" ".join(str(int(v)) for v in r) + " %d\n" % uid for r, uid in entries)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = [[int(x) for x in l.split()] for l in out.stdout.splitlines()]
    assert all(len(l) == 1 + bref.NSTAT for l in lines)
    return [(l[0], l[1:]) for l in lines]


@pytest.mark.parametrize("config,sc", [(c, s) for c, s, _ in bc.GAMES],
                         ids=["%s%s" % (c, "-shuffle" if s else "") for c, s, _ in bc.GAMES])
def test_header_agrees_with_the_reference_under_sanitizers(harness, config, sc):
    """csrc/hsad_behaviour.h, compiled alone with the address and undefined-behaviour sanitizers, counts every move of the reference
    bots' games as the reference does, line for line"""
    entries = bc.games()[(config, sc)]
    got = run_harness(harness, CONFIGS[config], sc, [e[:2] for e in entries])
    want = [(e[2], e[3]) for e in entries]
    assert len(got) == len(want)
    assert got == want, (config, sc, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])


def test_header_agrees_on_the_hand_written_positions(harness):
    for what, P_, uid, want in CASES:
        shuffled = any(row != [0, 1, 2, 3, 4] for row in P_.perms)
        assert run_harness(harness, P_.rules, shuffled, [(P_.to_record(), uid)]) == [(P_.mover, want)], what
    P_ = last_round()
    assert run_harness(harness, FULL, False, [(P_.to_record(), uid) for uid in (4, 9, 3, 8)]) == [(0, bref.classify(P_, uid)) for uid in (4, 9, 3, 8)]


# ---- the host side of the counters: rates, table, flags (no device) ---------------------------------------------------------------------
def test_behaviour_stats_rates_and_table_round_trip():
    from hanabi_sad_amd.eval import BEHAVIOUR_RATES, BehaviourStats, format_behaviour_table, parse_behaviour_table
    sums = [np.sum([e[3] for e in entries], axis=0) for _, entries in sorted(bc.games().items())]
    counts = np.zeros((4, 2, bref.NSTAT), np.int64)
    counts[:3] = np.array(sums, np.int64).reshape(3, 2, bref.NSTAT)           # the last pairing made no move at all
    st = BehaviourStats(counts.reshape(2, 2, 2, bref.NSTAT))
    assert tuple(st.names) == bref.NAMES and st.counts.dtype == np.int64
    row = st.row(0, 1, 0)
    c = dict(zip(bref.NAMES, counts[1, 0].tolist()))
    assert {k: row[k] for k in bref.NAMES} == c
    plays, hints = c["PLAY_OK"] + c["PLAY_FAIL"], c["HINT_COLOUR"] + c["HINT_RANK"]
    assert plays + hints + c["DISCARD"] == c["MOVES"]
    want = dict(hint_share=hints / c["MOVES"], play_share=plays / c["MOVES"], discard_share=c["DISCARD"] / c["MOVES"],
                colour_hint_share=c["HINT_COLOUR"] / hints, certain_play_share=c["PLAY_CERTAIN"] / plays, misplay_rate=c["PLAY_FAIL"] / plays,
                safe_discard_share=c["DISCARD_CERTAIN_DEAD"] / c["DISCARD"], playable_hint_share=c["HINT_PLAYABLE"] / hints,
                cards_per_hint=c["HINT_CARDS"] / hints, mean_info=c["INFO_SUM"] / c["MOVES"])
    assert sorted(want) == sorted(BEHAVIOUR_RATES) and {k: row[k] for k in want} == want
    for r in BEHAVIOUR_RATES:
        a = getattr(st, r)
        assert a.shape == (2, 2, 2) and a.dtype == np.float64 and np.isnan(a[1, 1]).all() and not np.isnan(a[:1]).any()
    text = format_behaviour_table(["M0", "piers"], st)
    assert len(text.splitlines()) == 3 + 2 * 2 * 2
    names, back = parse_behaviour_table("a score table\n\n" + text + "\n")
    assert names == ["M0", "piers"] and back.dtype == np.int64 and np.array_equal(back, st.counts)


def test_command_flags():
    from hanabi_sad_amd import eval_model, selfplay
    with pytest.raises(SystemExit, match="--behaviour needs --cross_play"):
        eval_model.main(["--paper", "op", "--method", "sad", "--idx1", "0", "--idx2", "3", "--behaviour"])
    assert eval_model.parse_args(["--cross_play", "--behaviour"]).behaviour and not eval_model.parse_args(["--cross_play"]).behaviour
    assert selfplay.parse_args([]).partner_behaviour == 0
    assert selfplay.parse_args(["--partner", "piers", "--partner_behaviour", "1"]).partner_behaviour == 1
