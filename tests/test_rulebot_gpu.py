"""GPU: the rule-list bots on the device.  policy_rule is held to the plain-Python reference (tests/rulebot_ref.py) on every position
of games the bots play to the end; playout_rule to the loop policy_rule -> step on a twin env, bit for bit; then the seating
semantics of seat_bot, the search and tournament entry points built on the two, the C ABI's refusals, and one comparison of
playing strength against the random policy.  Everything is integer logic: every check is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hanabi_sad_amd import rulebot
from tests import rulebot_ref as ref
from tests import search_fixtures as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 65   # one full wave and one lane of a second

FULL = SF.CONFIGS["full"]
# (id, rules, shuffle_color): P=2/H=5 runs the specialised kernels, P=3/H=5 the generic ones, `small` the variant ones
CASES = [("p2h5", FULL, False), ("p2h5-shuffle", FULL, True), ("p3h5", dict(FULL, players=3), False), ("small", SF.CONFIGS["small"], False)]
IDS = [c[0] for c in CASES]


def make_env(rules, sc, seed, n=G, max_len=80):
    from hanabi_sad_amd import BatchedHanabiEnv
    return BatchedHanabiEnv(n, seed=seed, eps_list=(0.0,), sad=False, shuffle_color=sc, max_len=max_len, device=DEV,
                            track_deck_history=False, **rules)


def errors(env):
    n, g, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    env.lib.hsad_env_error_count(env.h, C.byref(n), C.byref(g), C.byref(c))
    return n.value, c.value


def keys_of(n=G):
    return torch.arange(n, dtype=torch.int64) * 1000003 + 17


def step_live(env, bots, seats, seed, key, live):
    """one policy_rule -> step for the live games: the finished ones are given no bot (so they keep their counter) and the noop,
    which the step refuses and leaves alone (error code 3, drained by the caller)"""
    sb = torch.tensor(seats, dtype=torch.int32).view(1, -1).repeat(env.G, 1)
    sb[~live.cpu()] = -1
    env.a.fill_(env.A - 1)
    env.greedy_a.fill_(env.A - 1)
    a, ga = env.policy_rule(bots, sb, seed=seed, key=key)
    env.step(a, ga)


# ---- 1: policy_rule is the reference, position by position ------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", sorted(rulebot.PRESETS))
@pytest.mark.parametrize("name,rules,sc", CASES, ids=IDS)
def test_policy_rule_is_the_reference_on_every_position_of_its_games(name, rules, sc, preset):
    bot, seed = rulebot.PRESETS[preset], 4242
    env = make_env(rules, sc, 8100)
    env.reset()
    key = keys_of()
    fired = set()
    for t in range(81):
        live = env.terminal == 0
        if not bool(live.any()):
            break
        rec = env.export_state().cpu().numpy()
        step_live(env, bot, [0] * env.P, seed, key, live)
        a, ga = env.a.cpu().numpy(), env.greedy_a.cpu().numpy()
        assert np.array_equal(a, ga)
        for g in np.nonzero(live.cpu().numpy())[0]:
            p, uid, j = ref.act_record(rec[g], rules, ref.PRESETS[preset], seed, int(key[g]), t)
            want = [env.A - 1] * env.P
            want[p] = uid
            assert a[g].tolist() == want, (name, preset, "step %d game %d: rule %d" % (t, g, j))
            fired.add(j)
    assert not bool((env.terminal == 0).any()), "the games did not end"
    assert errors(env)[1] in (0, 3)
    assert len(fired - {-1}) >= min(2, len(bot.rules))
    env.close()


# ---- 2: playout_rule is policy_rule -> step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [False, True], ids=["index", "keyed"])
@pytest.mark.parametrize("name,rules,sc", CASES, ids=IDS)
def test_playout_rule_is_the_loop_over_policy_rule_and_step(name, rules, sc, keyed):
    bots = [rulebot.PRESETS["piers"], rulebot.PRESETS["flawed"]]
    seats = [p % 2 for p in range(rules["players"])]
    seed, key = 99, (keys_of() if keyed else None)
    env, twin = make_env(rules, sc, 8200), make_env(rules, sc, 8200)
    env.reset()
    twin.reset()

    def same_state(what):
        assert torch.equal(env.snapshot(), twin.snapshot()), "%s: the snapshots differ (state, generator or policy counter)" % what
        assert torch.equal(env.query(), twin.query()) and torch.equal(env.terminal, twin.terminal), what

    same_state("after the reset")
    # three iterations in one launch, the moves of the last one included
    for _ in range(3):
        live = twin.terminal == 0
        step_live(twin, bots, seats, seed, key, live)
    env.playout_rule(3, bots, seats, seed=seed, key=key)
    same_state("after 3 iterations")
    assert bool(live.any())
    assert torch.equal(env.a[live], twin.a[live]) and torch.equal(env.greedy_a[live], twin.greedy_a[live])
    # to the end: one launch against the loop
    for _ in range(80):
        live = twin.terminal == 0
        if not bool(live.any()):
            break
        step_live(twin, bots, seats, seed, key, live)
    env.playout_rule(100, bots, seats, seed=seed, key=key)
    same_state("at the end")
    assert bool((env.terminal == 1).all()) and bool((env.query()[:, 0] == 1).all())
    assert errors(env) == (0, 0) and errors(twin)[1] in (0, 3)
    # finished games are not touched by further iterations: state, counter, and their rows of a / greedy_a
    snap, q = env.snapshot(), env.query()
    env.a.fill_(-5)
    env.greedy_a.fill_(-6)
    env.playout_rule(10, bots, seats, seed=seed, key=key)
    assert torch.equal(env.snapshot(), snap) and torch.equal(env.query(), q)
    assert bool((env.a == -5).all()) and bool((env.greedy_a == -6).all()) and errors(env) == (0, 0)
    env.close()
    twin.close()


# ---- 3: seat_bot ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rules,sc", CASES, ids=IDS)
def test_seat_bot_picks_the_list_and_minus_one_keeps_the_row(name, rules, sc):
    names = ["cautious", "random"]
    bots = [rulebot.PRESETS[n] for n in names]
    env = make_env(rules, sc, 8300)
    P = env.P
    env.reset()
    env.playout_rule(4, bots[1], seed=1)              # some way into the games; every game has now had 4 policy calls
    live = (env.terminal == 0).cpu().numpy()
    sb = np.array([[(g + p) % 2 for p in range(P)] for g in range(G)], np.int32)
    sb[::5, 1] = -1                                   # a row left alone
    sb[3::7] = -1                                     # whole games left alone: they keep their counter
    sb[2, 0] = 2                                      # no such bot: the row is left alone and the error counted
    sb[4, P - 1] = -2
    rec = env.export_state().cpu().numpy()
    before = env.snapshot()
    env.a.fill_(-7)
    env.greedy_a.fill_(-9)
    seed, key = 31, keys_of()
    env.policy_rule(bots, sb, seed=seed, key=key)
    a, ga = env.a.cpu().numpy(), env.greedy_a.cpu().numpy()
    for g in range(G):
        for p in range(P):
            if sb[g, p] not in (0, 1):
                assert (a[g, p], ga[g, p]) == (-7, -9), (g, p)
            elif live[g]:
                seat, uid, _ = ref.act_record(rec[g], rules, ref.PRESETS[names[sb[g, p]]], seed, int(key[g]), 4)
                assert a[g, p] == ga[g, p] == (uid if p == seat else env.A - 1), (g, p)
    assert errors(env) == (2, 7)
    # the counter advanced in exactly the games that have a bot; nothing else of any game changed
    after = env.snapshot()
    changed = (before != after).any(dim=1).cpu().numpy()
    assert np.array_equal(changed, (sb != -1).any(axis=1))
    env.policy_rule(bots, np.full((G, P), -1, np.int32))
    assert torch.equal(env.snapshot(), after)
    env.close()


# ---- 4: the search plays its worlds out with a bot ----------------------------------------------------------------------------------------
def test_mc_action_values_with_a_bot_equal_the_loop_over_the_primitives():
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.search import mc_action_values, world_key, world_seed
    s = SF.SEARCH_ROOT
    bot = rulebot.PRESETS["flawed"]
    root = BatchedHanabiEnv(s["G"], seed=s["seed"], eps_list=SF.EPS, device=DEV, **SF.env_kwargs(s["config"], False, False, 0))
    root.rollout_random(s["iters"], s["pseed"])
    before = root.export_state()
    got = {cap: mc_action_values(root, s["worlds"], s["search_seed"], capacity=cap, playout=bot) for cap in (64, 96)}
    assert torch.equal(root.export_state(), before), "the search changed its root"

    def same(a, b):
        return a.dtype == b.dtype == torch.float32 and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))

    assert same(got[64], got[96])
    assert not same(got[64], mc_action_values(root, s["worlds"], s["search_seed"], capacity=64)), "the bot plays the random playout's games"
    with pytest.raises(ValueError):
        mc_action_values(root, s["worlds"], s["search_seed"], playout="cautious")
    one = BatchedHanabiEnv(1, seed=0, eps_list=(0.0,), device=DEV, track_deck_history=False, **root.config)
    q, legal = root.query().cpu().numpy(), root.legal_move.cpu().numpy()
    want = np.full((root.G, root.A), np.nan, np.float32)
    for g in range(root.G):
        if q[g, 0] == 1:
            continue
        p = int(q[g, 1])
        for a in np.nonzero(legal[g, p])[0]:
            total = 0
            for w in range(s["worlds"]):
                one.fork_from(root, [g], [world_seed(s["search_seed"], g, w)])
                assert int(one.determinize([p], [world_key(g, w)], s["search_seed"])[0]) >= 1
                act = torch.full((1, root.P), root.A - 1, dtype=torch.int64, device=DEV)
                act[0, p] = int(a)
                one.step(act, act)
                one.playout_rule(80, bot, seed=s["search_seed"], key=[world_key(g, w)])
                qq = one.query()[0].cpu().numpy()
                assert qq[0] == 1
                total += int(qq[2])
            want[g, a] = np.float32(total) / np.float32(s["worlds"])
    one.check_errors()
    assert same(got[64], torch.from_numpy(want).to(DEV))
    one.close()
    root.close()


# ---- 5: bots in the tournament --------------------------------------------------------------------------------------------------------------
def test_play_seatings_seats_bots_next_to_nets():
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.eval import cross_play, env_dims, play_seatings
    from hanabi_sad_amd.selfplay import init_weights
    n, seed, bot_seed = 24, 8500, 7
    piers, flawed = rulebot.PRESETS["piers"], rulebot.PRESETS["flawed"]
    # all bots: the scores of playout_rule on the same deals, with the hash keyed by the deal's seed
    res = play_seatings([piers, flawed], [(0, 0), (0, 1), (1, 0)], n, seed, 0, False, device=DEV, bot_seed=bot_seed)
    assert res.scores.shape == (3, n)
    for s_, seats in enumerate([(0, 0), (0, 1), (1, 0)]):
        env = make_env(FULL, False, seed, n=n, max_len=-1)
        env.reset()
        env.playout_rule(200, [piers, flawed], seats, seed=bot_seed, key=torch.arange(n) + seed)
        assert bool((env.terminal == 1).all())
        assert res.scores[s_].tolist() == env.query()[:, 5].cpu().tolist(), seats
        env.close()
    assert res.scores.max() > 0
    chunked = play_seatings([piers, flawed], [(0, 0), (0, 1), (1, 0)], n, seed, 0, False, device=DEV, bot_seed=bot_seed, games_per_launch=3 * 10)
    assert np.array_equal(chunked.scores, res.scores)
    # a bot next to a small random-weights net: the mixed seatings finish, the net-only seating is what it is without bots
    F, A = env_dims(2, 5, False)
    net = CNet(init_weights(F, 64, A, 5, 3), DEV)
    agent = CompositeAgent(net, net, 1, 0.99)
    mixed = play_seatings([agent, piers], [(0, 0), (0, 1), (1, 0), (1, 1)], n, seed, 0, False, device=DEV, bot_seed=bot_seed)
    assert int(mixed.totals[:, 3].min()) == n, "a seating did not finish its games"
    alone = play_seatings([agent], [(0, 0)], n, seed, 0, False, device=DEV)
    assert np.array_equal(mixed.scores[0], alone.scores[0])
    assert np.array_equal(mixed.scores[3], res.scores[0])
    xp = cross_play([agent, piers], n, seed, 0, False, device=DEV, bot_seed=bot_seed)
    assert np.array_equal(xp.scores.reshape(4, n), mixed.scores)


def test_eval_model_command_appends_the_bots_to_the_matrix():
    from hanabi_sad_amd.checkpoint import load_op_model
    from hanabi_sad_amd.eval import cross_play, parse_cross_play_table
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    zoo = os.path.join("tests", "golden", "op_zoo")
    cmd = [sys.executable, "-m", "hanabi_sad_amd.eval_model", "--paper", "op", "--method", "sad", "--root", zoo, "--num_game", "8",
           "--device", DEV, "--idx", "0", "--cross_play", "--bots", "cautious", "piers"]
    out = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)   # a fresh child process
    assert out.returncode == 0, out.stderr[-2000:]
    _, names, mean, _ = parse_cross_play_table(out.stdout[out.stdout.index("self-play & cross-play of SAD"):])
    assert names == ["M0", "cautious", "piers"]
    pool = [load_op_model("sad", 0, None, DEV, root=os.path.join(root, zoo), precision="bf16")[0], rulebot.PRESETS["cautious"], rulebot.PRESETS["piers"]]
    xp = cross_play(pool, 8, 1, 0, False, device=DEV)
    assert np.array_equal(mean, np.array([[float("%.2f" % v) for v in r] for r in xp.mean]))
    assert mean[1, 1] > 0


# ---- 6: the refusals of the C ABI ---------------------------------------------------------------------------------------------------------------
def test_the_abi_refuses_what_is_no_bot():
    from hanabi_sad_amd._lib import HsadError
    env = make_env(FULL, False, 8600, n=4)
    env.reset()
    before = env.snapshot()
    ok = rulebot.PRESETS["cautious"]
    bad_lists = [rulebot.RuleBot([]), rulebot.RuleBot([1] * 9), rulebot.RuleBot([0]), rulebot.RuleBot([14]), rulebot.RuleBot([(2, 101)]),
                 rulebot.RuleBot([(9, -1)]), rulebot.RuleBot([(1, 5)])]
    for bad in bad_lists:
        for call in (lambda: env.policy_rule([ok, bad]), lambda: env.playout_rule(5, [ok, bad])):
            with pytest.raises(HsadError, match="bot 1"):
                call()
    for bots in ([], [ok] * 9):
        for call in (lambda: env.policy_rule(bots), lambda: env.playout_rule(5, bots, seats=[0, 0])):
            with pytest.raises(HsadError, match="n_bot"):
                call()
    for seats in ([0, 1], [-1, 0]):
        with pytest.raises(HsadError, match="seat"):
            env.playout_rule(5, [ok], seats=seats)
    assert torch.equal(env.snapshot(), before) and errors(env) == (0, 0)
    env.close()


# ---- 7: a bot that plays Hanabi scores more than noise --------------------------------------------------------------------------------------------
def test_cautious_scores_more_than_the_random_policy_on_the_same_deals():
    n = 1024
    a, b = make_env(FULL, False, 8700, n=n, max_len=-1), make_env(FULL, False, 8700, n=n, max_len=-1)
    a.reset()
    b.reset()
    assert torch.equal(a.export_state(), b.export_state())
    a.playout_rule(200, rulebot.PRESETS["cautious"], seed=1)
    b.playout_random(200, 1)
    qa, qb = a.query(), b.query()
    assert bool((qa[:, 0] == 1).all()) and bool((qb[:, 0] == 1).all())
    bot, rnd = float(qa[:, 5].double().mean()), float(qb[:, 5].double().mean())
    print("mean score over %d deals: cautious %.3f, random %.3f" % (n, bot, rnd))
    assert bot > rnd
    a.close()
    b.close()
