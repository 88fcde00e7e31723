"""Game records on the device: the log (append), the way out of it (select, gather), the replay (hsad_env_playout_logged) and the
recording tournament, at the three kernel shapes -- <2,5,false> (standard 2-player game, with shuffle_color), <0,0,false> (4 players,
hands of 4) and <0,0,true> (the variant colors=3, ranks=4, hand_size=3).  G = 130: two waves and two lanes of a third, so the padded
wave and the compaction across a wave boundary are exercised.  The games are played by the random-legal policy and by the rule-bot
presets piers and cautious; the references are the classifier of tests/behaviour_ref.py, the restatement tests/game_record_ref.py and
the env's own move-by-move path (rewind_scripted + step).  Integer equalities throughout."""
import ctypes as C

import numpy as np
import pytest
import torch

from hanabi_sad_amd import _lib
from hanabi_sad_amd import game_record as gr
from tests import behaviour_ref as bref
from tests import game_record_ref as rref

pytestmark = pytest.mark.gpu

G = 130
# (rule set, shuffle_color, env seed, policy seed).  Random play loses its lives, the bots reach the end of the deck (the CPU
# restatement, test_game_record_cpu.test_the_sample_ends_by_lives_and_by_the_deck); test_condition asserts it of the device's games.
SHAPES = {"full-shuffle": ("full", True, 8300, 31), "p4h4": ("p4h4", False, 8400, 37), "c3r4h3": ("c3r4h3", False, 8500, 41)}


def make_env(shape):
    from hanabi_sad_amd import BatchedHanabiEnv
    name, shuffle, seed, _ = SHAPES[shape]
    return BatchedHanabiEnv(G, seed=seed, eps_list=[0.0], max_len=-1, sad=False, shuffle_color=shuffle, bomb=0, **rref.RULESETS[name])


def drain(env):
    n, g, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(env.lib.hsad_env_error_count(env.h, C.byref(n), C.byref(g), C.byref(c)))
    return n.value, g.value, c.value


def perms_of(state, rules):
    base = 80 + rules["players"] * rules["hand_size"] * 6
    return [[int(v) for v in state[base + 5 * p:base + 5 * p + 5]] for p in range(rules["players"])]


class Sample:
    """130 games played to their end with the recorder on, and what the host collected on the way"""


_SAMPLES = {}


def sample(shape):
    if shape in _SAMPLES:
        return _SAMPLES[shape]
    from hanabi_sad_amd.rulebot import PRESETS
    name, shuffle, seed, pseed = SHAPES[shape]
    rules = rref.RULESETS[name]
    P, A = rules["players"], rref.ref.num_actions(rules)
    s = Sample()
    s.rules, s.env = rules, make_env(shape)
    env = s.env
    s.rec = gr.GameRecorder(env)
    env.reset()
    # games 0..43 random, 44..86 piers on every seat, 87..129 cautious
    seat_bot = np.full((G, P), -1, np.int32)
    seat_bot[44:87], seat_bot[87:] = 0, 1
    seat_bot = torch.from_numpy(seat_bot).to(env.device)
    moves, greedy, flags = [[] for _ in range(G)], [[] for _ in range(G)], [[] for _ in range(G)]
    for _ in range(rref.capacity(rules) + 1):
        states = env.export_state().cpu().numpy()
        term = env.query()[:, 0].cpu().numpy() == 1
        if term.all():
            break
        env.policy_random(pseed)
        env.policy_rule([PRESETS["piers"], PRESETS["cautious"]], seat_bot, seed=pseed)
        live = torch.from_numpy(~term).to(env.device).unsqueeze(1)
        a = torch.where(live, env.a, torch.full_like(env.a, A - 1)).contiguous()
        ga = torch.where(live, env.greedy_a, torch.full_like(env.a, A - 1)).contiguous()
        s.rec.append(a, ga)
        ah, gh = a.cpu().numpy(), ga.cpu().numpy()
        for g in np.nonzero(~term)[0]:
            st = states[g]
            cur, k = int(st[57]), int(st[60])
            assert k == len(moves[g])
            perm = perms_of(st, rules)[cur]
            moves[g].append(rref.uid_to_true(rules, int(ah[g, cur]), perm))
            greedy[g].append(rref.uid_to_true(rules, int(gh[g, cur]), perm))
            flags[g].append(rref.flags_of(bref.classify_record(st, rules, int(ah[g, cur]))[1]))
        env.step(a, ga)
    drain(env)   # finished games were handed the noop
    torch.cuda.synchronize()
    s.moves, s.greedy, s.flags = moves, greedy, flags
    s.final = env.export_state().cpu().numpy()
    s.query = env.query().cpu().numpy()
    dh, cnt = env.deck_history()
    s.deck = [dh[g, :int(cnt[g])].cpu().numpy().tolist() for g in range(G)]
    s.records = s.rec.collect()
    _SAMPLES[shape] = s
    return s


def host_fields(s, g):
    """(score, lives, info, end) of game g from the env's final position"""
    st = s.final[g]
    return int(st[74]), int(st[56]), int(st[55]), rref.end_reason(s.rules, st, bool(s.query[g, 0]))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_condition(shape):
    s = sample(shape)
    assert s.query[:, 0].all(), "every game of the sample is played to its end"
    ends = [host_fields(s, g)[3] for g in range(G)]
    assert rref.END_LIVES in ends and rref.END_DECK in ends, ends
    assert s.rec.overflow_count() == 0
    assert s.rec.capacity == rref.capacity(s.rules) and s.rec.record_bytes == rref.record_bytes(s.rules)
    assert max(len(m) for m in s.moves) <= s.rec.capacity


@pytest.mark.parametrize("shape", list(SHAPES))
def test_recorder_planes_deck_and_result(shape):
    s = sample(shape)
    assert [r.meta["game"] for r in s.records] == list(range(G))
    if SHAPES[shape][1]:
        assert any(p != [0, 1, 2, 3, 4] for g in range(G) for p in perms_of(s.final[g], s.rules)), "shuffle_color must permute"
    for g, r in enumerate(s.records):
        assert r.moves == s.moves[g] and r.greedy == s.greedy[g] and r.flags == s.flags[g], g
        assert r.deck == s.deck[g], g
        assert (r.score, r.lives, r.info, r.end) == host_fields(s, g), g
        assert r.rules == dict(s.rules, bomb=0)
        r.validate()
    assert any(r.moves != r.greedy for r in s.records[:44]), "the random policy's greedy stream differs from its moves somewhere"
    # byte for byte what the restatement packs
    data = s.rec.gather(torch.arange(G, dtype=torch.int32)).cpu().numpy()
    for g in (0, 63, 64, 129):
        f = host_fields(s, g)
        assert data[g].tobytes() == rref.pack(s.rules, 0, s.deck[g], s.moves[g], s.greedy[g], s.flags[g], *f)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_finished_games_stop_growing(shape):
    s = sample(shape)
    env = s.env
    before = s.rec.gather(torch.arange(G, dtype=torch.int32)).cpu()
    a = torch.zeros_like(env.a)          # uid 0 for every seat: a move any live game would log
    s.rec.append(a, a)
    s.rec.append(a, None)
    assert torch.equal(s.rec.gather(torch.arange(G, dtype=torch.int32)).cpu(), before)
    assert s.rec.overflow_count() == 0


def test_a_running_game_is_not_selected_and_noops_are_not_logged():
    env = make_env("p4h4")
    rec = gr.GameRecorder(env)
    assert rec.collect() == []                         # never started
    env.reset()
    noop = torch.full_like(env.a, env.A - 1)
    rec.append(noop, noop)
    rec.append(torch.full_like(env.a, env.A), None)    # outside [0, A)
    rec.append(torch.full_like(env.a, -1), None)
    assert rec.collect() == [] and rec.select().numel() == 0
    data = rec.gather(torch.tensor([0, 129, -1, G], dtype=torch.int32)).cpu().numpy()
    assert not data[2:].any()
    for row in data[:2]:
        r = gr.GameRecord.from_bytes(row.tobytes())
        assert (r.n_moves, len(r.deck), r.end, r.lives) == (0, 16, rref.END_UNFINISHED, 3)
    env.policy_random(3)
    rec.append(env.a, env.greedy_a)
    r = gr.GameRecord.from_bytes(rec.gather(torch.tensor([5], dtype=torch.int32)).cpu().numpy()[0].tobytes())
    assert r.n_moves == 1
    rec.clear()
    r = gr.GameRecord.from_bytes(rec.gather(torch.tensor([5], dtype=torch.int32)).cpu().numpy()[0].tobytes())
    assert r.n_moves == 0
    rec.close()
    env.close()


def test_log_needs_the_deck_history():
    from hanabi_sad_amd import BatchedHanabiEnv
    env = BatchedHanabiEnv(4, track_deck_history=False)
    with pytest.raises(_lib.HsadError, match="deck history"):
        gr.GameRecorder(env)
    env.close()


# ---- select / gather ----------------------------------------------------------------------------------------------------------------
def filters(s):
    scores = sorted(r.score for r in s.records)
    lens = sorted(r.n_moves for r in s.records)
    P = s.rules["players"]
    return {
        "all": gr.GameFilter(),
        "none": gr.GameFilter(score_min=200),
        "score range": gr.GameFilter(score_min=scores[G // 3], score_max=scores[2 * G // 3]),
        "lives": gr.GameFilter(max_lives=0),
        "moves": gr.GameFilter(moves_min=lens[G // 4], moves_max=lens[3 * G // 4]),
        "end lives": gr.GameFilter(end_mask=1 << rref.END_LIVES),
        "end deck or perfect": gr.GameFilter(end_mask=(1 << rref.END_DECK) | (1 << rref.END_PERFECT)),
        "seat 1 spends the last life": gr.GameFilter(seat_mask=2, flag_mask=rref.LAST_LIFE),
        "last seat loses a last copy": gr.GameFilter(seat_mask=1 << (P - 1), flag_mask=rref.LAST_COPY_LOST),
        "anyone, two flags": gr.GameFilter(flag_mask=rref.PLAY_FAIL | rref.NO_INFO),
        "everything at once": gr.GameFilter(score_min=1, max_lives=2, moves_min=5, end_mask=1 << rref.END_DECK, seat_mask=1,
                                            flag_mask=rref.HINT_NOT_PLAYABLE | rref.DISCARD_UNCERTAIN),
    }


@pytest.mark.parametrize("shape", list(SHAPES))
def test_select_and_gather_equal_a_host_filter(shape):
    s = sample(shape)
    P = s.rules["players"]
    full = s.rec.gather(torch.arange(G, dtype=torch.int32)).cpu().numpy()
    sizes = {}
    for what, f in filters(s).items():
        want = [g for g in range(G) if rref.filter_pass(vars(f), P, *host_fields(s, g)[:2], host_fields(s, g)[3], s.flags[g])]
        idx = s.rec.select(f)
        assert idx.dtype == torch.int32 and idx.cpu().numpy().tolist() == want, what
        got = s.rec.gather(idx).cpu().numpy()
        assert got.shape == (len(want), s.rec.record_bytes) and np.array_equal(got, full[want]), what
        again = s.rec.select(f)
        assert torch.equal(again, idx) and np.array_equal(s.rec.gather(again).cpu().numpy(), got), what     # the same bits run to run
        assert [r.meta["game"] for r in s.rec.collect(f)] == want
        assert all(f.matches(s.records[g]) == (g in want) for g in range(G)), what
        sizes[what] = len(want)
    assert sizes["all"] == G and sizes["none"] == 0
    assert 0 < sizes["end lives"] < G and 0 < sizes["score range"] < G and sizes["anyone, two flags"] > 0, sizes
    assert s.rec.select(None).cpu().numpy().tolist() == list(range(G))
    # the take byte: every third game, on top of a filter and alone; a wave boundary (63 | 64) inside the kept run
    take = torch.tensor([g % 3 == 0 or g in (63, 64) for g in range(G)])
    assert s.rec.select(None, take).cpu().numpy().tolist() == [g for g in range(G) if take[g]]
    f = filters(s)["end lives"]
    assert s.rec.select(f, take).cpu().numpy().tolist() == [g for g in range(G) if take[g] and s.records[g].end == rref.END_LIVES]
    assert s.rec.select(None, torch.zeros(G, dtype=torch.bool)).numel() == 0


# ---- replay -------------------------------------------------------------------------------------------------------------------------
ROWS = ("priv_s", "legal_move", "own_hand", "eps", "terminal")


def rows_of(env):
    return {k: getattr(env, k).cpu().numpy().copy() for k in ROWS}


def packed(records):
    return np.frombuffer(b"".join(r.to_bytes() for r in records), dtype=np.uint8).reshape(len(records), -1)


def move_by_move(shape, records, src, stop, prestep=None):
    """the existing path: rewind_scripted with the records' decks, then step with the logged moves forced (a game at its stop is
    handed the noop, which the step refuses and leaves alone) -> (export_state, rows).  prestep: the policy seed of one random
    step made before the rewind, as the env under test made it"""
    rules = rref.RULESETS[SHAPES[shape][0]]
    P, A = rules["players"], rref.ref.num_actions(rules)
    env = make_env(shape)
    env.reset()
    if prestep is not None:
        env.policy_random(prestep)
        env.step(env.a, env.greedy_a)
    script, count = np.zeros((G, 52), np.uint8), np.zeros(G, np.int32)
    for g in range(G):
        if src[g] >= 0:
            d = records[src[g]].deck
            script[g, :len(d)], count[g] = d, len(d)
    env.rewind_scripted(torch.from_numpy(script), torch.from_numpy(count))
    perms = [perms_of(st, rules) for st in env.export_state().cpu().numpy()]
    for t in range(int(max(stop))):
        a = np.full((G, P), A - 1, np.int64)
        ga = a.copy()
        for g in range(G):
            if src[g] >= 0 and t < min(stop[g], records[src[g]].n_moves):
                r = records[src[g]]
                a[g, t % P] = rref.uid_from_true(rules, r.moves[t], perms[g][t % P])
                ga[g, t % P] = rref.uid_from_true(rules, r.greedy[t], perms[g][t % P])
        env.step(torch.from_numpy(a).to(env.device), torch.from_numpy(ga).to(env.device))
    drain(env)
    out = env.export_state().cpu().numpy(), rows_of(env)
    env.close()
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_replay_to_full_length_reproduces_the_original(shape):
    """Word for word, with one word set aside: word 73 counts the generator draws, which a position does not hold (import_state
    ignores it) -- the original game drew its deals from the generator, the replay takes them from the record and draws nothing."""
    s = sample(shape)
    env = make_env(shape)
    env.reset()
    status = env.playout_logged(packed(s.records), torch.arange(G, dtype=torch.int32))
    env.check_errors()
    assert status.cpu().numpy().tolist() == [r.n_moves for r in s.records]
    got = env.export_state().cpu().numpy()
    keep = np.arange(got.shape[1]) != 73
    assert np.array_equal(got[:, keep], s.final[:, keep])
    assert np.array_equal(env.query().cpu().numpy()[:, :13], s.query[:, :13])
    dh, cnt = env.deck_history()
    assert [dh[g, :int(cnt[g])].cpu().numpy().tolist() for g in range(G)] == s.deck
    assert bool(env.terminal.all()) and not env.reward.any()
    # the rows are those of the original env after its last step (sad = 0: nothing but the position is in them)
    for k in ("priv_s", "legal_move", "own_hand", "eps"):
        assert torch.equal(getattr(env, k), getattr(s.env, k)), k
    # the pure-Python replay agrees with the device about the final position
    for g in (0, 50, 64, 100, 129):
        r = s.records[g]
        assert r.position(r.n_moves, perms=perms_of(got[g], s.rules)) == gr.pos.from_record(got[g], s.rules), g
    env.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_replay_to_any_move_equals_the_move_by_move_path(shape):
    s = sample(shape)
    # game j replays record (j * 7) % G, so that a lane's record is not its own game; a different stop in every lane, 0 and
    # n_moves (and past it) included; every 13th game is left alone
    src = np.array([-1 if j % 13 == 5 else (j * 7) % G for j in range(G)], np.int32)
    n = np.array([s.records[i].n_moves if i >= 0 else 0 for i in src])
    stop = np.array([(0, n[j], n[j] + 3, (j * 5) % (n[j] + 1), n[j] - 1)[j % 5] for j in range(G)], np.int32)
    env = make_env(shape)
    env.reset()
    env.policy_random(9)
    env.step(env.a, env.greedy_a)          # a started env somewhere else than its first deal
    before_state, before_rows = env.export_state().cpu().numpy(), rows_of(env)
    status = env.playout_logged(packed(s.records), torch.from_numpy(src), torch.from_numpy(stop)).cpu().numpy()
    env.check_errors()
    played = np.minimum(stop, n)
    assert status[src >= 0].tolist() == played[src >= 0].tolist() and (status[src < 0] == -1).all()
    assert len(set(played[src >= 0].tolist())) > 20
    got_state, got_rows = env.export_state().cpu().numpy(), rows_of(env)
    want_state, want_rows = move_by_move(shape, s.records, src, stop, prestep=9)
    on = src >= 0
    assert np.array_equal(got_state[on], want_state[on])
    for k in ROWS:
        assert np.array_equal(got_rows[k][on], want_rows[k][on]), k
    assert not env.reward.cpu().numpy()[on].any()
    # -1 slots are untouched: state, rows and reward
    assert (~on).sum() == 10 and np.array_equal(got_state[~on], before_state[~on])
    for k in ROWS:
        assert np.array_equal(got_rows[k][~on], before_rows[k][~on]), k
    # the step path goes on from there: the env holds the record's deck as its script
    live = np.nonzero(on & (played < n))[0]
    assert len(live) > 10
    P, A = s.rules["players"], env.A
    a = np.full((G, P), A - 1, np.int64)
    perms = [perms_of(st, s.rules) for st in got_state]
    for j in live:
        t = int(played[j])
        a[j, t % P] = rref.uid_from_true(s.rules, s.records[src[j]].moves[t], perms[j][t % P])
    env.step(torch.from_numpy(a).to(env.device), torch.from_numpy(a).to(env.device))
    drain(env)
    after = env.export_state().cpu().numpy()
    for j in live[:12]:
        r = s.records[src[j]]
        assert r.position(int(played[j]) + 1, perms=perms[j]) == gr.pos.from_record(after[j], s.rules), j
    env.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_replay_refusals(shape):
    s = sample(shape)
    rules, A = s.rules, rref.ref.num_actions(s.rules)
    recs = [gr.GameRecord.from_bytes(r.to_bytes()) for r in s.records[:G]]
    # game 3: move 0 becomes a discard with every token in stock; game 70: move 4 becomes the noop uid; game 129: its greedy move 2
    # becomes a uid that is no move, which matters with sad only -- here the replay goes through
    recs[3].moves[0] = 0
    k70 = min(4, recs[70].n_moves - 1)
    recs[70].moves[k70] = A - 1
    recs[129].greedy[min(2, recs[129].n_moves - 1)] = A - 1
    # game 9: a deck the rules cannot deal (a fourth copy of its first card)
    recs[9].deck[1:4] = [recs[9].deck[0]] * 3
    env = make_env(shape)
    env.reset()
    before = env.export_state().cpu().numpy()
    status = env.playout_logged(packed(recs), torch.arange(G, dtype=torch.int32)).cpu().numpy()
    n_err, first, code = drain(env)
    assert n_err == 3 and (first, code) in ((3, 8), (70, 8), (9, 5))
    assert status[3] == 0 and status[70] == k70 and status[9] == -2 and status[129] == recs[129].n_moves
    want = [r.n_moves for r in recs]
    assert [int(v) for g, v in enumerate(status) if g not in (3, 9, 70)] == [v for g, v in enumerate(want) if g not in (3, 9, 70)]
    got = env.export_state().cpu().numpy()
    assert np.array_equal(got[9], before[9])               # left alone
    src = np.full(G, -1, np.int32)
    src[3], src[70] = 3, 70
    stop = np.zeros(G, np.int32)
    stop[70] = k70
    ref_state, ref_rows = move_by_move(shape, s.records, src, stop)
    rows = rows_of(env)
    for g in (3, 70):
        assert np.array_equal(got[g], ref_state[g]), g
        for k in ROWS:
            assert np.array_equal(rows[k][g], ref_rows[k][g]), (g, k)
    with pytest.raises(_lib.HsadError, match="illegal logged move"):
        env.playout_logged(packed(recs), torch.from_numpy(src))
        env.check_errors()
    drain(env)
    # rules that differ are refused on the host, before the launch
    state = env.export_state().cpu().numpy()
    for offset, value in ((0, 2), (2, rules["hand_size"] - 1), (5, rules["max_information_tokens"] - 1), (7, 1), (8, 255)):
        bad = packed(s.records[:2]).copy()
        bad[1, offset] = value
        with pytest.raises(_lib.HsadError, match="record 1"):
            env.playout_logged(bad, torch.zeros(G, dtype=torch.int32))
    assert np.array_equal(env.export_state().cpu().numpy(), state) and drain(env)[0] == 0
    st = env.playout_logged(packed(s.records[:2]), torch.full((G,), 2, dtype=torch.int32)).cpu().numpy()   # index 2 of 2 records
    assert (st == -3).all() and drain(env)[2] == 4
    env.close()


def test_replay_helper_builds_its_env():
    s = sample("c3r4h3")
    recs = s.records[40:48]
    stop = [0, 1, 2, 3, 4, 5, 6, 7]
    env = gr.replay(recs, stop=stop)
    assert env.G == 8 and env.replay_status.cpu().numpy().tolist() == [min(k, r.n_moves) for k, r in zip(stop, recs)]
    state = env.export_state().cpu().numpy()
    for j, r in enumerate(recs):
        assert r.position(min(stop[j], r.n_moves)) == gr.pos.from_record(state[j], s.rules), j
    env.close()
    with pytest.raises(ValueError, match="different rules"):
        gr.replay([recs[0], sample("p4h4").records[0]])


# ---- the recording tournament ---------------------------------------------------------------------------------------------------------
def test_tournament_records():
    from hanabi_sad_amd.eval import BEHAVIOUR_NAMES, play_seatings
    from hanabi_sad_amd.rulebot import PRESETS
    pool, seatings, n, seed = [PRESETS["piers"], PRESETS["cautious"]], [(0, 1), (1, 0)], 65, 8600
    res = play_seatings(pool, seatings, n, seed, 0, False, records=True, behaviour=True, bot_seed=3)
    assert len(res.records) == 2 * n
    flag_sums = np.zeros((2, 2, 8), np.int64)
    for r in res.records:
        m = r.meta
        assert m["seats"] == [pool[k].name for k in seatings[m["seating"]]] and m["deal_seed"] == seed + m["game"]
        assert r.score == res.scores[m["seating"], m["game"]]
        assert r.n_moves == res.behaviour.game_moves[m["seating"], m["game"]]
        r.validate()
        for k, f in enumerate(r.flags):
            flag_sums[m["seating"], k % 2] += [(f >> b) & 1 for b in range(8)]
    assert sorted((r.meta["seating"], r.meta["game"]) for r in res.records) == [(s, d) for s in range(2) for d in range(n)]
    c = {name: res.behaviour.counts[..., i] for i, name in enumerate(BEHAVIOUR_NAMES)}
    hints = c["HINT_COLOUR"] + c["HINT_RANK"]
    want = [c["MOVES"], c["PLAY_FAIL"], c["PLAY_OK"] + c["PLAY_FAIL"] - c["PLAY_CERTAIN"], c["LAST_COPY_LOST"], c["LAST_LIFE"],
            hints - c["HINT_PLAYABLE"], c["DISCARD"] - c["DISCARD_CERTAIN_DEAD"]]
    for b, w in enumerate(want):
        assert np.array_equal(flag_sums[..., b], w), gr.FLAG_NAMES[b]
    assert flag_sums[..., 0].sum() > 0 and flag_sums[..., 5].sum() > 0
    # a filter on the device keeps what the host filter keeps
    where = gr.GameFilter(score_max=int(np.median(res.scores)), seat_mask=2, flag_mask=gr.FLAGS["hint_not_playable"])
    some = play_seatings(pool, seatings, n, seed, 0, False, records=where, bot_seed=3)
    assert [r for r in res.records if where.matches(r)] == some.records and 0 < len(some.records) < 2 * n
    # the device's final position of a recorded deal: replay it and compare with the record's own rules
    env = gr.replay(res.records[:G])
    state = env.export_state().cpu().numpy()
    for j in (0, 64, 129):
        r = res.records[j]
        assert r.position(r.n_moves) == gr.pos.from_record(state[j], r.rules), j
        assert int(state[j][74]) == r.score
    env.close()
    # recording changes nothing: the same scores and counters without it
    plain = play_seatings(pool, seatings, n, seed, 0, False, behaviour=True, bot_seed=3)
    assert plain.records is None and np.array_equal(plain.scores, res.scores) and np.array_equal(plain.totals, res.totals)
    assert np.array_equal(plain.behaviour.counts, res.behaviour.counts)
    assert np.array_equal(plain.behaviour.game_moves, res.behaviour.game_moves)
