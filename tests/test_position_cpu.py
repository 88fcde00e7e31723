"""CPU: hanabi_sad_amd/position.py.  `validate` is held to an engine written independently of it (the CPU oracle: every position
a real game passes through is valid, every final one is exactly `terminal`), each rule of the specification is shown to bite
alone, and `Position` round-trips through the canonical record.  The same tables drive the device checks in
test_env_position_gpu.py, where hsad_env_import_state's status words are held to `validate`."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from hanabi_sad_amd import position as pos
from tests import position_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(pc.RULESETS))
@pytest.mark.parametrize("shuffle_color", [False, True])
def test_validate_accepts_every_position_of_real_games(name, shuffle_color):
    rules = pc.RULESETS[name]
    n_live = n_done = 0
    ends = set()
    for k, max_len in enumerate((80, 80, 80, 80, 80, 80, 2)):   # the last game is cut short by max_len
        flags = dict(max_len=max_len, shuffle_color=shuffle_color)
        for rec, finished in pc.oracle_game(name, 4100 + 17 * k, 7 + k, shuffle_color=shuffle_color, max_len=max_len):
            got = pos.validate(rec, rules, flags)
            want = pos.TERMINAL if finished else 0
            assert got == want, "%s game %d step %d: %s" % (name, k, rec[60], pos.explain(got ^ want))
            n_live += not finished
            n_done += finished
            if finished:
                ends.add("len" if rec[60] == max_len else "life" if rec[56] < 1 else "turns" if rec[59] < 1 else "won")
    assert n_done == 7 and n_live > 7
    assert "len" in ends and len(ends) >= 2, ends    # more than one way to end was seen, truncation among them


@pytest.mark.parametrize("name", sorted(pc.RULESETS))
@pytest.mark.parametrize("shuffle_color", [False, True])
def test_one_flag_per_corruption(name, shuffle_color):
    rules = pc.RULESETS[name]
    flags = dict(max_len=pc.MAX_LEN, shuffle_color=shuffle_color)
    assert pos.validate(pc.opening(rules).to_record(), rules, flags) == 0
    assert pos.validate(pc.endgame(rules).to_record(), rules, flags) == 0
    seen = 0
    for what, rec, want in pc.corruptions(rules, shuffle_color):
        got = pos.validate(rec, rules, flags)
        assert got == want, "%s / %s: got %s, want %s" % (name, what, pos.explain(got), pos.explain(want))
        seen |= want
    assert seen == (pos.CONSERVATION | pos.BOARD | pos.HANDS | pos.KNOWLEDGE | pos.LASTMOVE | pos.STEP | pos.PERM | pos.TERMINAL |
                    pos.FIELD)


def test_corruptions_of_played_positions():
    """the same single-field changes on positions of a real game (knowledge narrowed by hints, discards, a last move)"""
    rules = pc.RULESETS["full"]
    flags = dict(max_len=80, shuffle_color=False)
    game = pc.oracle_game("full", 4242, 3)
    live = [rec for rec, finished in game if not finished]
    assert len(live) > 8
    for rec in live[3::4]:
        r = rec.copy()
        r[80 + 2] = 0   # seat 0's first card could be of no rank
        assert pos.validate(r, rules, flags) == pos.KNOWLEDGE
        r = rec.copy()
        r[58] = r[57]
        assert pos.validate(r, rules, flags) == pos.BOARD
        r = rec.copy()
        r[61] -= 1
        assert pos.validate(r, rules, flags) == pos.CONSERVATION


def hand_written():
    full, small, c3 = pc.RULESETS["full"], pc.RULESETS["small"], pc.RULESETS["c3r4"]
    C = pos.Card
    yield pos.Position(full, [[(0, 0), (0, 1), (1, 1), (2, 2), (4, 4)],
                              [C(0, 0, colours=0b00001, hinted_colour=0), C(3, 1, colours=0b11110), C(1, 0, ranks=0b00001, hinted_rank=0),
                               (2, 0), (3, 3)]],
                       fireworks=[1, 0, 0, 0, 0], discards=[(4, 0), (4, 0)], info=5, life=2, mover=1, num_step=9,
                       last_move=dict(type="hint_colour", player=0, target_offset=1, value=0, reveal_mask=0b00001), last_score=17)
    yield pos.Position(small, [[(0, 4)], [(1, 3), (1, 4)]], fireworks=[4, 3], info=0, life=1,
                       discards=[(0, 0), (0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 0), (1, 1), (1, 2), (1, 3)], deck="rest",
                       mover=1, turns_to_play=1, num_step=30,
                       last_move=dict(type="play", player=0, card_index=1, colour=0, rank=3, scored=1))
    yield pc.opening(c3, perms=[[1, 2, 0, 3, 4], [0, 1, 2, 3, 4], [2, 1, 0, 3, 4]])
    yield pc.endgame(pc.RULESETS["p5h4"], turns_to_play=3, mover=2, short=(0, 1))


def test_position_round_trips_through_the_record():
    n = 0
    for p in hand_written():
        rec = p.to_record()
        assert rec.dtype == np.int32 and rec.shape == (pos.state_words(p.rules),)
        q = pos.from_record(rec, p.rules)
        assert q == p, "%r\n!=\n%r" % (q, p)
        assert np.array_equal(q.to_record(), rec)
        n += 1
    assert n == 4


def test_hand_written_positions_are_valid():
    shuffle = [False, False, True, False]
    for p, sc in zip(hand_written(), shuffle):
        got = pos.validate(p.to_record(), p.rules, dict(max_len=80, shuffle_color=sc))
        assert got == 0, (p, pos.explain(got))
    # the shuffled one is no position of an env that does not shuffle
    p = list(hand_written())[2]
    assert pos.validate(p.to_record(), p.rules, dict(max_len=80, shuffle_color=False)) == pos.PERM


def test_explain_names_every_flag():
    bits = [1 << k for k in range(14)]
    texts = [pos.explain(b) for b in bits]
    assert all(len(t) == 1 for t in texts) and len({t[0] for t in texts}) == 14
    assert pos.explain(0) == []
    assert pos.explain(pos.BOARD | pos.PERM) == texts[1] + texts[6]
    assert pos.explain(1 << 20)[0].startswith("unknown")
    assert pos.explain(-1)[0].startswith("not taken")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_header_agrees_with_validate_under_sanitizers(tmp_path):
    """csrc/hsad_position.h -- the decoder and position_valid the kernels run -- compiled alone with the address and undefined-
    behaviour sanitizers into a stand-alone program (tests/position/position_main.cc) that reads records and prints flags: line
    for line what validate says, over the corruption tables and the positions of played games of every rule set."""
    exe = str(tmp_path / "position_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hanabi_sad_amd", "csrc"), os.path.join(ROOT, "tests", "position", "position_main.cc"),
                           "-o", exe])
    for name, rules in sorted(pc.RULESETS.items()):
        for sc in (False, True):
            recs = [r for _, r, _ in pc.corruptions(rules, sc)] + [pc.opening(rules).to_record(), pc.endgame(rules).to_record()]
            recs += [r for r, _ in pc.oracle_game(name, 977, 5, shuffle_color=sc)]
            want = [pos.validate(r, rules, dict(max_len=pc.MAX_LEN, shuffle_color=sc)) for r in recs]
            head = "%d %d %d %d %d %d %d %d %d\n" % (rules["players"], rules["hand_size"], rules["colors"], rules["ranks"],
                                                     rules["max_information_tokens"], rules["max_life_tokens"], pc.MAX_LEN, int(sc), len(recs))
            text = head + "".join(" ".join(str(int(v)) for v in r) + "\n" for r in recs)
            out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr[-2000:]
            got = [int(x) for x in out.stdout.split()]
            assert got == want, (name, sc, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])
