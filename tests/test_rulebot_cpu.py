"""Rule-list bots without a device: the reference (tests/rulebot_ref.py) on hand-written positions with the expected uid written here,
csrc/hsad_rulebot.h compiled alone under the sanitizers against that reference on games the reference bots play themselves, the
coverage those games must reach, and the header's refusals.  The device kernels are held to the same reference in
test_rulebot_gpu.py."""
import collections
import os
import shutil
import subprocess

import pytest

from hanabi_sad_amd import position as pos
from hanabi_sad_amd import rulebot
from hanabi_sad_amd.position import Card, Position
from tests import rulebot_cases as rc
from tests import rulebot_ref as ref
from tests.determinize_ref import policy_hash
from tests.search_fixtures import CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, C3R4 = CONFIGS["full"], CONFIGS["c3r4"]
SEED, KEY, COUNTER = 77, 123456789, 5

# full game, 2 players: discard slot i = i, play = 5 + i, colour hint = 10 + colour, rank hint = 15 + rank, noop = 20
# c3r4, 3 players: discard = i, play = 4 + i, colour hint = 8 + 3 (o - 1) + colour, rank hint = 14 + 4 (o - 1) + rank, noop = 22
OWN = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1)]          # seat 0: knows nothing, holds nothing playable on empty fireworks
PARTNER = [(3, 3), (3, 4), (4, 3), (4, 4), (2, 3)]      # seat 1: nothing playable, nothing dead


def rank_known(c, r):
    return Card(c, r, ranks=1 << r, hinted_rank=r)


def exactly(c, r):
    return Card(c, r, colours=1 << c, ranks=1 << r, hinted_colour=c, hinted_rank=r)


def swap(hand, i, card):
    return hand[:i] + [card] + hand[i + 1:]


def full2(own=OWN, partner=PARTNER, **kw):
    return Position(FULL, [list(own), list(partner)], **kw)


def endgame2(own, partner, **kw):
    """the full game on an empty deck: every card that is in no hand is discarded"""
    left = pos.full_deck(FULL)
    for c, r in [(x.colour, x.rank) if isinstance(x, Card) else x for x in list(own) + list(partner)]:
        left[c * 5 + r] -= 1
    return Position(FULL, [list(own), list(partner)], discards=left, deck=[0] * 25, **kw)


def hash_pick(uids, p, j):
    return uids[policy_hash(SEED, KEY, COUNTER, 128 + 16 * p + j) % len(uids)]


def cases():
    """[(what, position, seat, rule list, expected uid, index of the deciding rule or -1)]"""
    out = []

    def case(what, P_, bot, uid, fired, p=0):
        out.append((what, P_, p, bot, uid, fired))

    # 1 PLAY_CERTAIN: slot 2 is known to be a 1, and every 1 is playable on empty fireworks
    one_known = swap(OWN, 2, rank_known(1, 0))
    case("PLAY_CERTAIN fires", full2(one_known), [(1, 0)], 7, 0)
    # ... with the colour-1 firework at 1 the slot may be the dead (1, 0): nothing fires, info is full, lowest legal = play slot 0
    case("PLAY_CERTAIN stopped", full2(one_known, fireworks=[0, 1, 0, 0, 0]), [(1, 0)], 5, -1)

    # 2 PLAY_PROBABLE: firework 0 at 1, slot 3 known rank 0: pool holds 2 + 4 * 3 = 14 ones, 12 playable: 85 %
    probable = swap(OWN, 3, rank_known(1, 0))
    case("PLAY_PROBABLE fires", full2(probable, fireworks=[1, 0, 0, 0, 0]), [(2, 85)], 8, 0)
    case("PLAY_PROBABLE below k", full2(probable, fireworks=[1, 0, 0, 0, 0]), [(2, 86)], 5, -1)
    case("PLAY_PROBABLE needs life > 1", full2(probable, fireworks=[1, 0, 0, 0, 0], life=1), [(2, 50)], 5, -1)
    # a tie between slots 1 and 3 (both known rank 0): the lowest slot
    tie = swap(swap(OWN, 1, rank_known(2, 0)), 3, rank_known(1, 0))
    case("PLAY_PROBABLE tie", full2(tie, fireworks=[1, 0, 0, 0, 0]), [(2, 50)], 6, 0)

    # 3 PLAY_PROBABLE_ENDGAME: empty deck, the pool is the own hand; slot 4 is known to be the playable (0, 0)
    end_own = swap(OWN, 4, exactly(0, 0))
    case("PLAY_PROBABLE_ENDGAME fires", endgame2(end_own, PARTNER), [(3, 0)], 9, 0)
    case("PLAY_PROBABLE_ENDGAME needs an empty deck", full2(end_own), [(3, 0)], 5, -1)

    # 4 HINT_PLAYABLE: firework 1 at 1; the partner's slot 0 is publicly known (2, 0): skipped; slot 2 = (1, 1) is playable
    hp = swap(swap(PARTNER, 0, exactly(2, 0)), 2, (1, 1))
    case("HINT_PLAYABLE fires", full2(OWN[:2] + [(0, 3), (1, 3), (2, 1)], hp, fireworks=[0, 1, 0, 0, 0]), [(4, 0)], 16, 0)
    case("HINT_PLAYABLE needs a token", full2(OWN[:2] + [(0, 3), (1, 3), (2, 1)], hp, fireworks=[0, 1, 0, 0, 0], info=0), [(4, 0)], 0, -1)
    # the colour hint under a permutation: the rank of (1, 0) is known, firework 0 is at 1 so "a 1" is not known playable;
    # the actor's permutation sends colour 1 to 0
    cp = swap(PARTNER, 2, rank_known(1, 0))
    case("HINT_PLAYABLE colour hint, permuted", full2(OWN, cp, fireworks=[1, 0, 0, 0, 0], perms=[[2, 0, 1, 3, 4], [0, 1, 2, 3, 4]]),
         [(4, 0)], 10, 0)

    # 5 / 6: firework 0 at 1, both (3, 2) discarded: the partner's (0, 0) is dead, its (3, 3) is dead by the blocked colour
    blocked = [(0, 0), (3, 3), (2, 2), (4, 4), (2, 3)]
    bk = dict(fireworks=[1, 0, 0, 0, 0], discards=[(3, 2), (3, 2)], info=6)
    case("HINT_USEFUL fires", full2(OWN, blocked, **bk), [(5, 0)], 17, 0)
    case("HINT_USEFUL needs a token", full2(OWN, blocked, **dict(bk, info=0)), [(5, 0)], 0, -1)
    case("HINT_DEAD fires", full2(OWN, blocked, **bk), [(6, 0)], 15, 0)
    case("HINT_DEAD blocked colour", full2(OWN, blocked[1:] + [(4, 3)], **bk), [(6, 0)], 18, 0)
    case("HINT_DEAD needs a token", full2(OWN, blocked, **dict(bk, info=0)), [(6, 0)], 0, -1)

    # 7 HINT_RANDOM: the partner holds colours 2, 3, 4 and ranks 3, 4
    case("HINT_RANDOM fires", full2(), [(1, 0), (7, 0)], hash_pick([12, 13, 14, 18, 19], 0, 1), 1)
    case("HINT_RANDOM needs a token", full2(info=0), [(7, 0)], 0, -1)

    # 8 DISCARD_CERTAIN_DEAD: firework 0 at 1, slot 1 known to be (0, 0)
    dead_own = swap(OWN, 1, exactly(0, 0))
    case("DISCARD_CERTAIN_DEAD fires", full2(dead_own, fireworks=[1, 0, 0, 0, 0], info=7), [(8, 0)], 1, 0)
    case("DISCARD_CERTAIN_DEAD needs room for a token", full2(dead_own, fireworks=[1, 0, 0, 0, 0]), [(8, 0)], 5, -1)

    # 9 DISCARD_PROBABLE_DEAD: firework 0 at 1, slot 2 known rank 0: 2 of the 14 ones in the pool are dead: 14.3 %
    pd = swap(OWN, 2, rank_known(1, 0))
    case("DISCARD_PROBABLE_DEAD fires", full2(pd, fireworks=[1, 0, 0, 0, 0], info=7), [(9, 14)], 2, 0)
    case("DISCARD_PROBABLE_DEAD below k", full2(pd, fireworks=[1, 0, 0, 0, 0], info=7), [(9, 15)], 0, -1)
    case("DISCARD_PROBABLE_DEAD needs room for a token", full2(pd, fireworks=[1, 0, 0, 0, 0]), [(9, 0)], 5, -1)

    # 10 / 11 / 12
    hinted = swap(OWN, 0, Card(0, 1, colours=1, hinted_colour=0))
    case("DISCARD_UNHINTED_OLDEST fires", full2(hinted, info=7), [(10, 0)], 1, 0)
    case("DISCARD_UNHINTED_OLDEST needs room for a token", full2(hinted), [(10, 0)], 5, -1)
    case("DISCARD_OLDEST fires", full2(hinted, info=7), [(11, 0)], 0, 0)
    case("DISCARD_OLDEST needs room for a token", full2(hinted), [(11, 0)], 5, -1)
    case("DISCARD_RANDOM fires", full2(info=3), [(12, 0)], hash_pick([0, 1, 2, 3, 4], 0, 0), 0)
    case("DISCARD_RANDOM needs room for a token", full2(), [(12, 0)], 5, -1)

    # 13, and the seat that is not on turn
    case("LEGAL_RANDOM fires", full2(info=3), [(13, 0)], hash_pick([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 18, 19], 0, 0), 0)
    case("not on turn: the noop", full2(info=3), [(13, 0)], 20, -1, p=1)
    # nothing fires: the lowest legal bit (a discard when there is room for a token)
    case("nothing fires", full2(info=3), [(1, 0), (8, 0)], 0, -1)

    # 3 players, seat 1 on turn: offset 1 is seat 2, offset 2 is seat 0.  Firework 0 at 1: seat 0's (1, 0) in slot 0 and seat 2's
    # (0, 1) in slot 3 are playable; the scan meets seat 2 first
    hands3 = [[(1, 0), (1, 2), (2, 2), (2, 3)], [(0, 2), (0, 3), (1, 1), (2, 1)], [(1, 3), (2, 1), (0, 2), (0, 1)]]
    case("scan order, 3 players", Position(C3R4, hands3, fireworks=[1, 0, 0], mover=1), [(4, 0)], 15, 0, p=1)
    hands3b = [hands3[0], hands3[1], [(1, 3), (2, 1), (0, 2), (1, 1)]]
    case("scan order, second offset", Position(C3R4, hands3b, fireworks=[1, 0, 0], mover=1), [(4, 0)], 18, 0, p=1)
    return out


CASES = cases()


@pytest.mark.parametrize("what,P_,p,bot,uid,fired", CASES, ids=[c[0] for c in CASES])
def test_hand_written_positions(what, P_, p, bot, uid, fired):
    shuffled = any(row != [0, 1, 2, 3, 4] for row in P_.perms)
    assert pos.validate(P_.to_record(), P_.rules, dict(shuffle_color=shuffled)) == 0, "the test's own position is not one"
    assert ref.act(P_, p, bot, SEED, KEY, COUNTER) == (uid, fired)


def test_every_code_has_a_firing_and_a_stopped_case():
    fires = collections.Counter(bot[fired][0] for _, _, _, bot, _, fired in CASES if fired >= 0)
    stopped = collections.Counter(bot[-1][0] for _, _, _, bot, _, fired in CASES if fired < 0)
    assert sorted(fires) == list(range(1, 14))
    assert sorted(stopped) == list(range(1, 14))   # (LEGAL_RANDOM has no guard: its case is the seat that is not on turn)


def test_presets_are_the_specified_lists():
    assert {k: v.rules for k, v in rulebot.PRESETS.items()} == ref.PRESETS
    assert len(rulebot.PRESETS["piers"].rules) == rulebot.MAX_RULES


@pytest.mark.parametrize("preset", sorted(ref.PRESETS))
def test_games_cover_every_rule(preset):
    """in the games the header and the kernels are compared on, every rule of the preset decides at least 5 times"""
    n = collections.Counter(e[5] for entries in rc.games_of(preset).values() for e in entries)
    assert all(n[j] >= 5 for j in range(len(ref.PRESETS[preset]))), sorted(n.items())


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("rulebot") / "rulebot_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hanabi_sad_amd", "csrc"), os.path.join(ROOT, "tests", "rulebot", "rulebot_main.cc"),
                           "-o", exe])
    return exe


def run_harness(exe, rules, shuffle_color, bot, seed, entries):
    """entries: [(record, key, counter)] -> (what rb_rules_invalid says, [(seat, uid, deciding rule)])"""
    head = "%d %d %d %d %d %d %d %d %d %d\n" % (rules["players"], rules["hand_size"], rules["colors"], rules["ranks"],
                                                rules["max_information_tokens"], rules["max_life_tokens"], int(shuffle_color), len(bot),
                                                seed, len(entries))
    text = head + " ".join("%d %d" % ck for ck in bot) + "\n"
    text += "".join(" ".join(str(int(v)) for v in r) + " %d %d\n" % (k, c) for r, k, c in entries)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = [int(x) for x in out.stdout.split()]
    return got[0], [tuple(got[1 + 3 * i:4 + 3 * i]) for i in range((len(got) - 1) // 3)]


@pytest.mark.parametrize("preset", sorted(ref.PRESETS))
def test_header_agrees_with_the_reference_under_sanitizers(harness, preset):
    """csrc/hsad_rulebot.h, compiled alone with the address and undefined-behaviour sanitizers, answers every position of the
    reference bots' own games as the reference does: seat, uid and the rule that decided"""
    for (config, sc), entries in rc.games_of(preset).items():
        bad, got = run_harness(harness, CONFIGS[config], sc, ref.PRESETS[preset], rc.POLICY_SEED, [e[:3] for e in entries])
        want = [e[3:] for e in entries]
        assert bad == 0
        assert got == want, (config, sc, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])


def test_header_agrees_on_the_hand_written_positions(harness):
    for what, P_, p, bot, uid, fired in CASES:
        if p != P_.mover:
            continue
        shuffled = any(row != [0, 1, 2, 3, 4] for row in P_.perms)
        bad, got = run_harness(harness, P_.rules, shuffled, bot, SEED,
                               [(P_.to_record(), KEY, COUNTER)])
        assert bad == 0 and got == [(p, uid, fired)], what


@pytest.mark.parametrize("bot,why", [([], 1), ([(1, 0)] * 9, 1), ([(0, 0)], 2), ([(14, 0)], 2), ([(1, 0), (-3, 0)], 2),
                                     ([(2, 101)], 3), ([(9, -1)], 3), ([(1, 5)], 3), ([(13, 1)], 3)])
def test_header_refuses_what_is_no_rule_list(harness, bot, why):
    """1 = the number of rules, 2 = an unknown code, 3 = k out of range (the C ABI's refusals themselves need an env: they are in
    test_rulebot_gpu.py)"""
    bad, got = run_harness(harness, FULL, False, bot, 0, [])
    assert bad == why and got == []
