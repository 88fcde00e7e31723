"""GPU: the behaviour counters of a tournament.  hsad_seating_behaviour is held to the plain-Python classifier
(tests/behaviour_ref.py) step by step on games the rule bots play to the end, then followed up through play_seatings / cross_play,
the C ABI's refusals and the two commands.  Integer counters: every comparison is exact."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from hanabi_sad_amd import _lib, rulebot
from hanabi_sad_amd import position as pos
from tests import behaviour_ref as bref
from tests import search_fixtures as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZOO = os.path.join("tests", "golden", "op_zoo")
NSTAT = bref.NSTAT
BOTS = ("piers", "flawed", "random")
INVALID = -1            # HSAD_ERR_INVALID

# (id, config, shuffle_color, seatings S, games per seating n): n no multiple of 64 with S > 1; 3 players; the permuted colour
# hints; a seating that crosses a 256-game workgroup
CASES = [("full-3x11", "full", False, 3, 11), ("c3r4-2x5", "c3r4", False, 2, 5), ("full-shuffle-2x7", "full", True, 2, 7),
         ("small-2x300", "small", False, 2, 300)]


def make_env(rules, sc, seed, G):
    from hanabi_sad_amd import BatchedHanabiEnv
    return BatchedHanabiEnv(G, seed=seed, eps_list=(0.0,), sad=False, bomb=0, shuffle_color=sc, max_len=-1, device=DEV,
                            track_deck_history=False, **rules)


def behaviour(env, n, a, counts):
    return env.lib.hsad_seating_behaviour(env.h, n, a.data_ptr() if a is not None else None,
                                          counts.data_ptr() if counts is not None else None, env._stream())


def errors(env):
    n, g, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    env.lib.hsad_env_error_count(env.h, C.byref(n), C.byref(g), C.byref(c))
    return n.value, c.value


# ---- 3: the kernel is the reference, step by step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,config,sc,S,n", CASES, ids=[c[0] for c in CASES])
def test_kernel_is_the_reference_after_every_step(name, config, sc, S, n):
    rules = SF.CONFIGS[config]
    G, P = S * n, rules["players"]
    env = make_env(rules, sc, 8800, G)
    env.reset()
    bots = [rulebot.PRESETS[b] for b in BOTS]
    seats = torch.tensor([[(g // n + p) % len(BOTS) for p in range(P)] for g in range(G)], dtype=torch.int32)   # seating-major
    key = torch.arange(G, dtype=torch.int64) * 1000003 + 17
    counts = torch.zeros(S, P, NSTAT, dtype=torch.int64, device=DEV)
    want = np.zeros((S, P, NSTAT), np.int64)
    live_steps = 0
    for t in range(200):
        live = env.terminal == 0
        if not bool(live.any()):
            break
        sb = seats.clone()
        sb[~live.cpu()] = -1            # a finished game gets no bot (it keeps its counter) ...
        env.a.fill_(env.A - 1)
        env.greedy_a.fill_(env.A - 1)
        a, ga = env.policy_rule(bots, sb, seed=4242, key=key)
        rec = env.export_state().cpu().numpy()
        probe = a.clone()
        probe[~live] = rules["hand_size"]     # ... and the kernel a real uid in its rows: a game that is not live adds nothing
        moves = probe.cpu().numpy()
        for g in np.nonzero(live.cpu().numpy())[0]:
            P_ = pos.from_record(rec[g], rules)
            want[g // n, P_.mover] += bref.classify(P_, moves[g, P_.mover])
            live_steps += 1
        _lib.check(behaviour(env, n, probe, counts))
        env.step(a, ga)
        got = counts.cpu().numpy()
        assert np.array_equal(got, want), (name, "step %d" % t, np.argwhere(got != want)[:5].tolist())
    assert not bool((env.terminal == 0).any()), "the games did not end"
    assert errors(env)[1] in (0, 3)
    q = env.query().cpu().numpy().astype(np.int64)
    assert int(want[:, :, bref.MOVES].sum()) == live_steps == int(q[:, 6].sum())
    assert np.array_equal(want[:, :, bref.PLAY_OK].sum(axis=1), q[:, 5].reshape(S, n).sum(axis=1))     # bomb = 0: a point per good play
    assert int(want[:, :, bref.MOVES].min()) >= 1
    env.close()


# ---- 4: through play_seatings ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    from hanabi_sad_amd.checkpoint import load_op_model
    from hanabi_sad_amd.eval import env_dims
    nets = [load_op_model("sad", i, None, DEV, root=os.path.join(ROOT, ZOO), precision="bf16")[0] for i in (0, 3)]
    sad = getattr(nets[0].online, "F", None) == env_dims(2, 5, sad=True)[0]
    return nets + [rulebot.PRESETS["piers"]], sad


def test_play_seatings_counts_without_changing_the_games(pool):
    from hanabi_sad_amd.eval import BehaviourStats, cross_play, play_seatings
    agents, sad = pool
    n, K = 8, 3
    seatings = [(i, j) for i in range(K) for j in range(K)]
    plain = play_seatings(agents, seatings, n, 1, 0, sad, device=DEV)
    res = play_seatings(agents, seatings, n, 1, 0, sad, device=DEV, behaviour=True)
    assert plain.behaviour is None and isinstance(res.behaviour, BehaviourStats)
    assert np.array_equal(res.scores, plain.scores) and np.array_equal(res.totals, plain.totals)
    c = res.behaviour.counts
    assert c.shape == (K * K, 2, NSTAT) and c.dtype == np.int64 and tuple(res.behaviour.names) == bref.NAMES
    again = play_seatings(agents, seatings, n, 1, 0, sad, device=DEV, behaviour=True)
    chunked = play_seatings(agents, seatings, n, 1, 0, sad, device=DEV, behaviour=True, games_per_launch=16)   # one deal per chunk
    assert np.array_equal(again.behaviour.counts, c) and np.array_equal(chunked.behaviour.counts, c)
    assert np.array_equal(chunked.scores, plain.scores)
    # the invariants: a seating's MOVES are its games' moves, and with bomb = 0 its good plays are its points
    assert np.array_equal(c[:, :, bref.MOVES].sum(axis=1), res.behaviour.game_moves.sum(axis=1))
    assert np.array_equal(chunked.behaviour.game_moves, res.behaviour.game_moves) and int(res.behaviour.game_moves.min()) >= 1
    assert np.array_equal(c[:, :, bref.PLAY_OK].sum(axis=1), res.scores.sum(axis=1))
    # a model with itself: the seats alternate, so their move counts differ by at most one per game
    for k in range(K):
        s = k * K + k
        assert abs(int(c[s, 0, bref.MOVES]) - int(c[s, 1, bref.MOVES])) <= n
    # the derived rates are those counters
    row = res.behaviour.row(1, 0)
    hints = row["HINT_COLOUR"] + row["HINT_RANK"]
    assert row["MOVES"] == int(c[1, 0, 0]) and row["hint_share"] == hints / row["MOVES"]
    assert res.behaviour.hint_share.shape == (K * K, 2) and res.behaviour.mean_info.dtype == np.float64
    xp = cross_play(agents, n, 1, 0, sad, device=DEV, behaviour=True)
    assert xp.behaviour.counts.shape == (K, K, 2, NSTAT) and np.array_equal(xp.behaviour.counts.reshape(K * K, 2, NSTAT), c)
    assert cross_play(agents[1:], n, 1, 0, sad, device=DEV).behaviour is None


# ---- 5: the refusals of the C ABI -------------------------------------------------------------------------------------------------------
def test_the_abi_refuses_before_any_launch():
    env = make_env(SF.CONFIGS["full"], False, 8900, 12)
    env.reset()
    env.policy_rule(rulebot.PRESETS["piers"])
    counts = torch.full((3, 2, NSTAT), 7, dtype=torch.int64, device=DEV)
    for what, rc in (("null a", behaviour(env, 4, None, counts)), ("null counts", behaviour(env, 4, env.a, None)),
                     ("games_per_seating 0", behaviour(env, 0, env.a, counts)), ("games_per_seating -3", behaviour(env, -3, env.a, counts)),
                     ("not dividing G", behaviour(env, 5, env.a, counts)),
                     ("null env", env.lib.hsad_seating_behaviour(None, 4, env.a.data_ptr(), counts.data_ptr(), env._stream()))):
        assert rc == INVALID, what
    torch.cuda.synchronize()
    assert bool((counts == 7).all()), "a refused call wrote counters"
    # ... and the call it does take accumulates on top of what is there
    _lib.check(behaviour(env, 4, env.a, counts))
    got = counts.cpu().numpy() - 7
    assert int(got[:, :, bref.MOVES].sum()) == 12 and int(got[:, 1].sum()) == 0      # seat 0 opens every game
    env.close()


# ---- 6: the commands --------------------------------------------------------------------------------------------------------------------------
def test_eval_model_command_prints_a_behaviour_table_that_reads_back(pool):
    from hanabi_sad_amd.eval import cross_play, parse_behaviour_table, parse_cross_play_table
    cmd = [sys.executable, "-m", "hanabi_sad_amd.eval_model", "--paper", "op", "--method", "sad", "--root", ZOO, "--device", DEV,
           "--idx", "0", "3", "--cross_play", "--bots", "piers", "--behaviour", "--num_game", "4"]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)   # a fresh child process
    assert out.returncode == 0, out.stderr[-2000:]
    agents, sad = pool
    xp = cross_play(agents, 4, 1, 0, sad, device=DEV, behaviour=True)
    _, names, mean, _ = parse_cross_play_table(out.stdout[out.stdout.index("self-play & cross-play of SAD"):])
    assert names == ["M0", "M3", "piers"]
    assert np.array_equal(mean, np.array([[float("%.2f" % v) for v in r] for r in xp.mean]))
    bnames, counts = parse_behaviour_table(out.stdout)
    assert bnames == names and counts.dtype == np.int64
    assert np.array_equal(counts, xp.behaviour.counts)
    # without --behaviour the output is the matrix alone
    plain = subprocess.run([c for c in cmd if c != "--behaviour"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert plain.returncode == 0 and "behaviour" not in plain.stdout
    assert out.stdout.startswith(plain.stdout.rstrip("\n"))


def test_eval_model_command_refuses_behaviour_without_cross_play():
    cmd = [sys.executable, "-m", "hanabi_sad_amd.eval_model", "--paper", "op", "--method", "sad", "--root", ZOO, "--device", DEV,
           "--idx1", "0", "--idx2", "3", "--behaviour", "--num_game", "4"]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode != 0 and "--behaviour needs --cross_play" in out.stderr


def test_selfplay_prints_both_behaviour_lines_under_a_partner_line(capsys):
    from hanabi_sad_amd import selfplay
    from hanabi_sad_amd.eval import BEHAVIOUR_RATES
    selfplay.main(["--num_game", "128", "--partner", "piers", "--partner_behaviour", "1", "--num_update", "3", "--burn_in_frames", "64",
                   "--replay_buffer_size", "512", "--batchsize", "32", "--colors", "2", "--hand_size", "2", "--max_life_tokens", "1"])
    lines = capsys.readouterr().out.splitlines()
    at = [i for i, l in enumerate(lines) if re.match(r"partner piers: score \S+ \(", l)]
    assert at, lines[-20:]
    for i in at:
        for who, line in (("learner", lines[i + 1]), ("partner", lines[i + 2])):
            head = "partner piers behaviour %s: " % who
            assert line.startswith(head), line
            words = line[len(head):].split()
            assert tuple(words[0::2]) == BEHAVIOUR_RATES
            rates = [float(v) for v in words[1::2]]
            assert len(rates) == len(BEHAVIOUR_RATES) and all(v >= 0.0 for v in rates if v == v)      # (nan: no such move was made)
