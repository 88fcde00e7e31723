"""Game records without a device: csrc/hsad_game_record.h compiled alone under the sanitizers against the Python restatement
(tests/game_record_ref.py) and the reference classifier (tests/behaviour_ref.py); the pure-Python replay of
hanabi_sad_amd/game_record.py against the CPU oracle, position by position; bytes, JSON and files both ways; what validate()
refuses.  The kernels are held to the same references in test_game_record_gpu.py.  Integer logic only: every comparison is exact."""
import itertools
import os
import shutil
import subprocess

import pytest

from hanabi_sad_amd import game_record as gr
from hanabi_sad_amd import position as pos
from tests import behaviour_ref as bref
from tests import game_record_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (rule set, env seed, policy): random play loses its lives, the bots reach the end of the deck
GAMES = [(name, seed, policy) for name in rref.RULESETS for seed, policy in ((8101, "random"), (8102, "piers"), (8103, "cautious"))]
IDS = ["%s-%d-%s" % g for g in GAMES]


def record_of(game, meta=None):
    """the GameRecord of an oracle game: the oracle's moves, its deck history, the reference classifier's flags, its final position"""
    rules, states = game["rules"], game["states"]
    flags = [rref.flags_of(bref.classify_record(states[k], rules, uid)[1]) for k, uid in enumerate(game["moves"])]
    last = states[-1]
    return gr.GameRecord(dict(rules, bomb=0), game["deck"], game["moves"], game["greedy"], flags, score=int(last[74]), lives=int(last[56]),
                         info=int(last[55]), end=rref.end_reason(rules, last, True), meta=meta)


# ---- the header under the sanitizers -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("game_record") / "record_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hanabi_sad_amd", "csrc"),
                           os.path.join(ROOT, "tests", "game_record", "record_main.cc"), "-o", exe])
    return exe


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = [[int(x) for x in l.split()] for l in out.stdout.splitlines()]
    assert len(got) == len(lines)
    return got


def test_capacity_formula_for_every_rule_set(harness):
    assert rref.capacity(rref.RULESETS["full"]) == 95
    names = sorted(rref.ALL_RULESETS)
    got = ask(harness, ["cap %d %d %d %d %d" % (r["players"], r["hand_size"], rref.deck_size(r), r["max_information_tokens"], r["colors"])
                        for r in (rref.ALL_RULESETS[n] for n in names)])
    for n, (L, ok, nbytes) in zip(names, got):
        r = rref.ALL_RULESETS[n]
        assert (L, ok, nbytes) == (rref.capacity(r), 1, rref.record_bytes(r)), n
        assert (gr.capacity(r), gr.record_bytes(r), gr.deck_size(r)) == (L, nbytes, rref.deck_size(r)), n
    # a log is refused above 255 moves: the env counts steps in eight bits
    assert ask(harness, ["cap 2 1 60 120 5", "cap 2 1 60 133 5", "layout 95"]) == [[243, 1, 68 + 3 * 243], [256, 0, 68 + 3 * 256],
                                                                                  [16, 68, 68 + 3 * 95]]


def test_no_oracle_game_needs_more_than_the_capacity():
    for name, seed, policy in GAMES:
        g = rref.oracle_game(name, seed, policy)
        assert 0 < len(g["moves"]) <= rref.capacity(g["rules"]), (name, seed, policy)


def test_header_packs_and_unpacks(harness):
    heads = [[1, 2, 5, 5, 5, 8, 3, 0, 61, 50, 25, 3, 8, 3, 95], [1, 4, 4, 5, 5, 8, 3, 1, 0, 16, 0, 3, 8, 0, 86],
             [1, 2, 3, 3, 4, 5, 2, 0, 255, 52, 12, 0, 0, 2, 255]]
    for h, row in zip(heads, ask(harness, ["hdr " + " ".join(map(str, h)) for h in heads])):
        assert row[:16] == h + [0] and row[16:] == h
        rules = dict(zip(gr.RULE_KEYS, h[1:8]))
        if h[14] == rref.capacity(rules):      # the Python reader takes the same sixteen bytes apart the same way
            body = bytes(row[:16]) + bytes(52 + 3 * h[14])
            rec = gr.GameRecord.from_bytes(body)
            assert (rec.rules, rec.n_moves, len(rec.deck), rec.score, rec.lives, rec.info, rec.end) == (rules, h[8], h[9], *h[10:14])


def test_colour_mapping_both_directions(harness):
    cases = []
    for name, perm in (("full", [2, 0, 1, 4, 3]), ("full", [0, 1, 2, 3, 4]), ("p4h4", [4, 3, 2, 1, 0]), ("c3r4h3", [1, 2, 0, 3, 4])):
        r = rref.RULESETS[name]
        A = 2 * r["hand_size"] + (r["players"] - 1) * (r["colors"] + r["ranks"]) + 1
        cases += [(r, perm, uid) for uid in range(A)]
    got = ask(harness, ["col %d %d %d %s %d" % (r["players"], r["hand_size"], r["colors"], " ".join(map(str, perm)), uid)
                        for r, perm, uid in cases])
    for (r, perm, uid), (to_true, from_true) in zip(cases, got):
        assert to_true == rref.uid_to_true(r, uid, perm) and from_true == rref.uid_from_true(r, uid, perm), (r, perm, uid)
        assert rref.uid_to_true(r, from_true, perm) == uid and rref.uid_from_true(r, to_true, perm) == uid
    assert any(a != uid for (_, _, uid), (a, _) in zip(cases, got))


def test_flag_byte_on_every_move_of_the_oracle_games(harness):
    incs = [[0] * bref.NSTAT]
    for name, seed, policy in GAMES:
        g = rref.oracle_game(name, seed, policy)
        incs += [bref.classify_record(g["states"][k], g["rules"], uid)[1] for k, uid in enumerate(g["moves"])]
    want = [rref.flags_of(i) for i in incs]
    assert [row[0] for row in ask(harness, ["flag " + " ".join(map(str, i)) for i in incs])] == want
    seen = 0
    for f in want:
        seen |= f
    assert seen == 255, "the games must raise every flag at least once (seen 0x%02x)" % seen
    assert [n for n in gr.FLAG_NAMES] == ["counted", "play_fail", "play_uncertain", "last_copy_lost", "last_life", "hint_not_playable",
                                          "discard_uncertain", "no_info"]
    assert [gr.FLAGS[n] for n in gr.FLAG_NAMES] == [rref.COUNTED, rref.PLAY_FAIL, rref.PLAY_UNCERTAIN, rref.LAST_COPY_LOST, rref.LAST_LIFE,
                                                    rref.HINT_NOT_PLAYABLE, rref.DISCARD_UNCERTAIN, rref.NO_INFO]


def test_filter_predicate(harness):
    filters = [dict(score_min=0, score_max=255, max_lives=255, moves_min=0, moves_max=255, end_mask=0, seat_mask=0, flag_mask=0),
               dict(score_min=3, score_max=10, max_lives=1, moves_min=10, moves_max=40, end_mask=1 << rref.END_LIVES, seat_mask=0, flag_mask=0),
               dict(score_min=0, score_max=255, max_lives=255, moves_min=0, moves_max=255, end_mask=0, seat_mask=2, flag_mask=rref.LAST_LIFE)]
    keys = list(filters[0])
    cases = list(itertools.product(filters, (2, 3, 11), (0, 1, 2), (9, 10, 41), range(4), (0, 1)))
    got = ask(harness, ["filter %s %d %d %d %d %d" % (" ".join(str(f[k]) for k in keys), score, lives, n, end, hit)
                        for f, score, lives, n, end, hit in cases])
    for (f, score, lives, n, end, hit), (passed,) in zip(cases, got):
        flags = [0] * n
        if hit and n > 1:
            flags[1] = f["flag_mask"] or 1       # a move of seat 1
        want = rref.filter_pass(f, 2, score, lives, end, flags) if (hit and n > 1) or not hit else None
        if want is not None:
            assert bool(passed) == want, (f, score, lives, n, end, hit)
            rec = gr.GameRecord(dict(rref.RULESETS["full"], bomb=0), [], [0] * n, None, flags, score, lives, 0, end)
            assert gr.GameFilter(**f).matches(rec) == want


# ---- the pure-Python replay against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed,policy", GAMES, ids=IDS)
def test_position_at_every_move_equals_the_oracle(name, seed, policy):
    game = rref.oracle_game(name, seed, policy)
    rec = record_of(game)
    assert rec.validate() is rec
    for k, state in enumerate(game["states"]):
        assert rec.position(k) == pos.from_record(state, game["rules"]), (name, seed, policy, k)
    last = game["states"][-1]
    assert rec.position(rec.n_moves).last_score == int(last[74]) == rec.score
    # the result fields follow from the deal and the moves alone
    assert gr.GameRecord.from_game(rec.rules, rec.deck, rec.moves, rec.greedy, rec.flags) == rec
    with pytest.raises(ValueError):
        rec.position(rec.n_moves + 1)


def test_the_sample_ends_by_lives_and_by_the_deck():
    ends = {(policy, record_of(rref.oracle_game(name, seed, policy)).end) for name, seed, policy in GAMES}
    assert {e for _, e in ends} >= {rref.END_LIVES, rref.END_DECK}, ends


# ---- bytes, JSON, files ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed,policy", GAMES, ids=IDS)
def test_bytes_and_json_round_trip(name, seed, policy):
    game = rref.oracle_game(name, seed, policy)
    rec = record_of(game, meta={"deal_seed": seed, "seats": [policy] * game["rules"]["players"], "seating": 0})
    data = rec.to_bytes()
    last = game["states"][-1]
    assert data == rref.pack(game["rules"], 0, game["deck"], game["moves"], game["greedy"], rec.flags, int(last[74]), int(last[56]),
                             int(last[55]), rec.end)
    assert len(data) == gr.record_bytes(rec.rules)
    back = gr.GameRecord.from_bytes(data, meta=rec.meta)
    assert back == rec and back.to_bytes() == data
    assert gr.GameRecord.from_json(rec.to_json()) == rec and gr.GameRecord.from_json(rec.to_json()).to_json() == rec.to_json()


def test_save_and_load(tmp_path):
    recs = [record_of(rref.oracle_game(*g), meta={"deal_seed": g[1], "seats": [g[2]] * rref.RULESETS[g[0]]["players"]}) for g in GAMES]
    path = str(tmp_path / "games.jsonl")
    gr.save(path, recs)
    assert len(open(path).read().splitlines()) == len(recs)
    assert gr.load(path) == recs
    gr.save(path, [])
    assert gr.load(path) == []


def test_from_bytes_refusals():
    data = bytearray(record_of(rref.oracle_game(*GAMES[0])).to_bytes())
    for edit in (lambda d: d.__setitem__(0, 2), lambda d: d.__setitem__(14, 94), lambda d: d.__setitem__(8, 96), lambda d: d.__setitem__(9, 53),
                 lambda d: d.__setitem__(2, 4), lambda d: d.pop()):
        bad = bytearray(data)
        edit(bad)
        with pytest.raises(ValueError):
            gr.GameRecord.from_bytes(bytes(bad))
    with pytest.raises(ValueError):
        gr.GameRecord.from_bytes(b"\x01\x02")


# ---- validate ---------------------------------------------------------------------------------------------------------------------------
def edited(rec, **kw):
    d = dict(rules=rec.rules, deck=rec.deck, moves=rec.moves, greedy=rec.greedy, flags=rec.flags, score=rec.score, lives=rec.lives,
             info=rec.info, end=rec.end)
    d.update(kw)
    return gr.GameRecord(**d)


@pytest.mark.parametrize("name,seed,policy", [GAMES[1], GAMES[5], GAMES[6]], ids=[IDS[1], IDS[5], IDS[6]])
def test_validate_refusals(name, seed, policy):
    rec = record_of(rref.oracle_game(name, seed, policy))
    n = rec.n_moves
    rec.validate()
    with pytest.raises(ValueError, match="deck"):                       # a truncated deck: a later move needs a card it no longer lists
        edited(rec, deck=rec.deck[:-1]).validate()
    with pytest.raises(ValueError, match="deck"):                       # ... and one too short for the first deal
        edited(rec, deck=rec.deck[:3]).validate()
    if len(rec.deck) < gr.deck_size(rec.rules):                         # a card nobody was dealt
        with pytest.raises(ValueError, match="deck lists"):
            edited(rec, deck=rec.deck + [0]).validate()
    else:                                                               # the whole deck dealt: a fourth copy of a card type
        with pytest.raises(ValueError, match="does not hold"):
            edited(rec, deck=rec.deck[:-1] + [rec.deck[0] if rec.deck[0] != rec.deck[-1] else rec.deck[1]]).validate()
    # an illegal move: a hint as the first move names a rank no card of the target hand has, or a discard with all tokens in stock
    with pytest.raises(ValueError, match="illegal"):
        edited(rec, moves=[0] + rec.moves[1:]).validate()
    k = next(i for i, u in enumerate(rec.moves) if gr.decode_move(rec.rules, u)[0] in ("play", "discard"))
    with pytest.raises(ValueError, match="illegal"):                    # a uid that is no move at all
        edited(rec, moves=rec.moves[:k] + [gr.num_actions(rec.rules) - 1] + rec.moves[k + 1:]).validate()
    with pytest.raises(ValueError, match="n_moves is wrong|the deck lists"):   # a wrong n_moves: the last move is missing
        edited(rec, moves=rec.moves[:n - 1], greedy=rec.greedy[:n - 1], flags=rec.flags[:n - 1]).validate()
    with pytest.raises(ValueError):                                     # ... or a move after the end
        edited(rec, moves=rec.moves + [rec.moves[-1]], greedy=rec.greedy + [0], flags=rec.flags + [0]).validate()
    with pytest.raises(ValueError, match="greedy"):
        edited(rec, greedy=rec.greedy[:-1]).validate()
    with pytest.raises(ValueError, match="result"):
        edited(rec, score=rec.score + 1).validate()
    with pytest.raises(ValueError, match="ends by"):
        edited(rec, end=rref.END_PERFECT if rec.end != rref.END_PERFECT else rref.END_DECK).validate()


# ---- describe and the command line ------------------------------------------------------------------------------------------------------
def test_describe_and_command_line(tmp_path, capsys):
    game = rref.oracle_game("full", 8101, "random")
    rec = record_of(game, meta={"deal_seed": 8101, "seats": ["random", "random"]})
    text = rec.describe()
    lines = text.splitlines()
    assert len(lines) == 2 + 2 + rec.n_moves + 1
    assert lines[-1] == "result: score %d, %d lives, %d tokens, ended by %s" % (rec.score, rec.lives, rec.info, gr.END_NAMES[rec.end])
    for k in range(rec.n_moves):
        after = game["states"][k + 1]
        assert lines[4 + k].startswith("%3d  seat %d (random) " % (k, game["seats"][k]))
        assert lines[4 + k].endswith("| score %d lives %d tokens %d deck %d" % (sum(after[50:55]), after[56], after[55], after[61]))
        for n in gr.flag_names(rec.flags[k] & ~1):
            assert n in lines[4 + k]
    assert sum("MISFIRE" in l for l in lines) == rref.RULESETS["full"]["max_life_tokens"] - rec.lives
    path = str(tmp_path / "g.jsonl")
    gr.save(path, [rec, rec])
    assert gr.main([path, "--game", "1"]) == 0
    assert capsys.readouterr().out == "== game 1 ==\n" + text + "\n"
    assert gr.main([path, "--game", "0", "--at", "3"]) == 0
    assert capsys.readouterr().out == "== game 0 ==\n" + repr(rec.position(3)) + "\n"
    with pytest.raises(SystemExit):
        gr.main([path, "--game", "2"])


def test_command_flags():
    from hanabi_sad_amd import eval_model
    args = eval_model.parse_args(["--cross_play", "--save_games", "g.jsonl", "--save_games_where", "score<=10,flag=last_life,seat=1"])
    assert args.save_games == "g.jsonl" and args.save_games_where == "score<=10,flag=last_life,seat=1"
    assert eval_model.parse_args(["--cross_play"]).save_games is None
    with pytest.raises(SystemExit, match="--save_games_where needs --save_games"):
        eval_model.main(["--paper", "op", "--method", "sad", "--idx1", "0", "--idx2", "3", "--save_games_where", "score<=10"])
    with pytest.raises(SystemExit, match="--save_games_where: flag=nothing"):
        eval_model.main(["--paper", "op", "--method", "sad", "--idx1", "0", "--idx2", "3", "--save_games", "g.jsonl",
                         "--save_games_where", "flag=nothing"])


def test_filter_parse():
    f = gr.GameFilter.parse("score<=10,flag=last_life,seat=1")
    assert f == gr.GameFilter(score_max=10, flag_mask=rref.LAST_LIFE, seat_mask=2)
    f = gr.GameFilter.parse("score>=3, moves=40, lives<=1, end=lives, end=deck, flag=play_fail, flag=no_info")
    assert f == gr.GameFilter(score_min=3, moves_min=40, moves_max=40, max_lives=1, end_mask=(1 << rref.END_LIVES) | (1 << rref.END_DECK),
                              flag_mask=rref.PLAY_FAIL | rref.NO_INFO)
    assert gr.GameFilter.parse("") == gr.GameFilter()
    for bad in ("score<10", "flag=nothing", "end=tired", "seat", "colour=3"):
        with pytest.raises(ValueError):
            gr.GameFilter.parse(bad)
