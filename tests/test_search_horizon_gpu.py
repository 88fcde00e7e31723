"""GPU: depth-limited blueprint-policy search (search.PolicySearch / policy_action_values / play_with_search with depth=D,
hsad_search_horizon_stats of csrc/hsad_search.hip, eval_model --search_depth).

The kernel is held to the numpy restatement tests/search_horizon_ref.py on an env that holds live, finished and never-started games;
the search to a test-local loop over the primitives -- fork_from / determinize, `h[:, rows]` indexing, agent.act, env.step, then
act(with_q=True), query() and the restatement -- with the jobs in REVERSED slot order.  A row's result depends on no other row of a
batch and every batch here stays under the 1,024-row switch of the act kernels, so totals, cut, values and the blueprint's move must
agree bit for bit.  With a depth no game outlasts, the search is the full search in 1/256 points."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import search_fixtures as SF
from tests import search_horizon_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZOO = os.path.join(os.path.dirname(__file__), "golden", "op_zoo")
DEV = "cuda:0"
Q_TERM, Q_STARTED = 0, 14
INVALID = -1            # HSAD_ERR_INVALID
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------
# 1. hsad_search_horizon_stats against the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(2, 0), (3, 1)], ids=["2p", "3p_bomb"])
def mixed_env(request):
    """96 games: 80 forked from an env in the middle of random play (some of them finished), 16 never started"""
    from hanabi_sad_amd import BatchedHanabiEnv
    P, bomb = request.param
    kw = dict(players=P, bomb=bomb, eps_list=[0.0], max_len=-1, sad=True, device=DEV, track_deck_history=False)
    played = BatchedHanabiEnv(96, seed=3, **kw)
    played.reset()
    for it in range(200):
        done = played.query()[:, Q_TERM] == 1
        if int(done.sum()) >= 12:
            break
        a, g = played.policy_random(1234)
        noop = torch.full_like(a, played.A - 1)
        played.step(torch.where(done.unsqueeze(1), noop, a).contiguous(), torch.where(done.unsqueeze(1), noop, g).contiguous())
    env = BatchedHanabiEnv(96, seed=5, **kw)
    idx = torch.arange(96, dtype=torch.int32)
    idx[80:] = -1
    env.fork_from(played, idx)
    q = env.query().cpu().numpy()
    started, term = q[:, Q_STARTED] == 1, q[:, Q_TERM] == 1
    live, finished = started & ~term, started & term
    assert live.sum() >= 8 and finished.sum() >= 8 and (~started).sum() == 16
    played.close()
    return env, q, live, finished


@pytest.mark.parametrize("mode", [R.MOVER, R.TEAM], ids=["mover", "team"])
def test_horizon_stats_against_the_restatement(mixed_env, mode):
    from hanabi_sad_amd import _lib
    env, q, live, finished = mixed_env
    lib, st = env.lib, env._stream()
    G, P, n_job, worlds = env.G, env.P, 7, env.G + 3
    rng = np.random.default_rng(11 + mode)
    q_rows = (rng.standard_normal((G, P)) * 6).astype(f32)
    q_rows[rng.random((G, P)) < 0.2] *= f32(0.001953125 * 300)      # more values near the grid of 1/512
    lv = np.nonzero(live)[0]
    plant = [f32("nan"), f32("inf"), f32("-inf"), f32(1e9), f32(-1e9), f32(64.001953125), f32(2.501953125), f32(-0.998046875)]
    for g, x in zip(lv, plant):
        q_rows[g, :] = 0
        q_rows[g, q[g, 6] % P] = x                                   # the mover's row: both modes see it
    if len(lv) > len(plant):
        q_rows[lv[len(plant)], :2] = (f32("inf"), f32("-inf"))       # team: inf - inf = NaN; mover: one of the two
    # uneven world counts per job; -1 and values >= n_job skip the slot
    jobs = [np.repeat(np.arange(-1, n_job + 2), [9, 30, 1, 12, 5, 0, 17, 8, 6, 8]).astype(np.int32),
            rng.integers(-1, n_job + 1, size=G).astype(np.int32)]
    rng.shuffle(jobs[0])
    for job in jobs:
        job[lv[:len(plant) + 1]] = rng.integers(0, n_job, size=len(lv[:len(plant) + 1]))     # the planted games are counted
    assert all(len(j) == G for j in jobs)
    world = np.arange(G, dtype=np.int32) + 1                         # one (job, world) per slot: nothing is stored twice in a call
    fin = np.nonzero(finished)[0]
    world[fin[0]], world[lv[-1]] = -1, worlds                        # no such world: counted, not stored
    perfect = 25
    v, counted, cut, bad = R.from_query(q, q_rows, mode, perfect)
    qd, wd = torch.from_numpy(q_rows.reshape(-1)).to(DEV), torch.from_numpy(world).to(DEV)
    before = [qd.clone(), env.export_state().clone()]
    stats = torch.zeros(n_job, 3, dtype=torch.int64, device=DEV)
    cuts = torch.zeros(n_job, dtype=torch.int64, device=DEV)
    nonf = torch.zeros(1, dtype=torch.int64, device=DEV)
    table = torch.full((n_job, worlds), -1, dtype=torch.int16, device=DEV)
    stats2, cuts2, nonf2 = torch.zeros_like(stats), torch.zeros_like(cuts), torch.zeros_like(nonf)
    want = None
    for k, job in enumerate(jobs):
        jd = torch.from_numpy(job).to(DEV)
        _lib.check(lib.hsad_search_horizon_stats(env.h, jd.data_ptr(), n_job, qd.data_ptr(), mode, stats.data_ptr(), cuts.data_ptr(),
                                                 nonf.data_ptr(), wd.data_ptr(), worlds, table.data_ptr(), st))
        want = R.job_reduce(v, counted, cut, bad, job, n_job, world, worlds, want)
        assert np.array_equal(stats.cpu().numpy(), want[0]), k        # the second call adds to the first
        assert np.array_equal(cuts.cpu().numpy(), want[1]) and np.array_equal(nonf.cpu().numpy(), want[2]), k
        assert np.array_equal(table.view(torch.uint16).cpu().numpy(), want[3]), k
        # without the table: the same sums
        _lib.check(lib.hsad_search_horizon_stats(env.h, jd.data_ptr(), n_job, qd.data_ptr(), mode, stats2.data_ptr(), cuts2.data_ptr(),
                                                 nonf2.data_ptr(), None, 0, None, st))
        assert torch.equal(stats2, stats) and torch.equal(cuts2, cuts) and torch.equal(nonf2, nonf)
    assert torch.equal(qd.view(torch.int32), before[0].view(torch.int32)) and torch.equal(env.export_state(), before[1])
    # every class of slot occurred
    valid = (jobs[0] >= 0) & (jobs[0] < n_job)
    assert (valid & finished).sum() > 0 and (valid & cut).sum() > 0 and (valid & bad).sum() >= 2 and (~valid).sum() > 0
    assert (valid & ~counted).sum() > 0 and want[2][0] >= 4 and (want[3] != R.NOT_PLAYED).sum() > 40
    assert 0 < want[1].sum() < want[0][:, 2].sum() and (want[0][:, 0] % 256 != 0).any()
    live_v = v[cut & ~bad]
    assert (live_v % 256 != 0).any() and live_v.min() >= 0 and live_v.max() <= perfect * 256
    # the refusals
    jd = torch.from_numpy(jobs[0]).to(DEV)
    good = [env.h, jd.data_ptr(), n_job, qd.data_ptr(), mode, stats.data_ptr(), cuts.data_ptr(), nonf.data_ptr(), wd.data_ptr(), worlds,
            table.data_ptr(), st]
    keep = [stats.clone(), cuts.clone(), nonf.clone(), table.clone()]
    for pos, bad_arg in ((2, 0), (2, -3), (4, 2), (4, -1), (1, None), (3, None), (5, None), (6, None), (7, None), (8, None), (9, 0), (9, -1)):
        args = list(good)
        args[pos] = bad_arg
        assert lib.hsad_search_horizon_stats(*args) == INVALID, (pos, bad_arg)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(keep, (stats, cuts, nonf, table)))


# ------------------------------------------------------------------------------------------------------------------
# 2. the search equals the loop over the primitives
# ------------------------------------------------------------------------------------------------------------------
WORLDS, SEED = 4, 21


def _agent(kind):
    from hanabi_sad_amd.eval import _acting_agent
    if kind == "3p":
        from hanabi_sad_amd.composite import CNet, CompositeAgent
        from hanabi_sad_amd.eval import env_dims
        from hanabi_sad_amd.selfplay import init_weights
        F, A = env_dims(3, 5, False)
        net = CNet(init_weights(F, 64, A, 5, 1), DEV)
        return CompositeAgent(net, net, 1, 0.99), 3
    from hanabi_sad_amd.checkpoint import load_op_model
    return _acting_agent(load_op_model("sad", 0, None, DEV, root=ZOO, precision=kind)[0], kind, DEV), 2


def _obs(env):
    N = env.G * env.P
    return {"priv_s": env.priv_s.view(N, env.F), "legal_move": env.legal_move.view(N, env.A), "eps": torch.zeros(N, device=DEV)}


def _act_q(agent, obs, hid):
    if "defer_target" in inspect.signature(agent.act).parameters:
        return agent.act(obs, hid, with_q=True, defer_target=True)[0]
    return agent.act(obs, hid, with_q=True)[0]


def _make_root(agent, P, moves):
    """3 games after `moves` lock-step greedy moves -> (env, the agent's state entering the next step)"""
    from hanabi_sad_amd import BatchedHanabiEnv
    env = BatchedHanabiEnv(3, players=P, seed=17, bomb=0, eps_list=[0.0], max_len=-1, sad=False, device=DEV, track_deck_history=False)
    env.reset()
    hid = agent.get_h0(3 * P)
    for _ in range(moves):
        reply, hid = agent.act(_obs(env), hid)
        env.step(reply["a"].view(3, P).contiguous(), reply["greedy_a"].view(3, P).contiguous())
    env.check_errors()
    assert bool((env.query()[:, Q_TERM] == 0).all())
    return env, {"h0": hid["h0"], "c0": hid["c0"]}


def _yardstick(root, agent, hid, worlds, seed, depth, mode, cap=64):
    """the depth-limited search with none of the search kernels, jobs in reversed slot order -> (values float32 [G, A], totals int64
    [G, A, 3], cut int64 [G, A], blueprint int64 [G], non-finite Q count) as numpy"""
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.search import search_jobs, world_key, world_seed
    G, P, A = root.G, root.P, root.A
    perfect = root.config.get("colors", 5) * root.config.get("ranks", 5)
    pairs, cur = search_jobs(root)
    jobs = [(int(g), int(a), w) for g, a in pairs for w in range(worlds)]
    senv = BatchedHanabiEnv(cap, seed=0, eps_list=(0.0,), device=DEV, track_deck_history=False, **root.config)
    senv.reset()
    totals, cuts, nonfinite = np.zeros((G, A, 3), dtype=np.int64), np.zeros((G, A), dtype=np.int64), 0
    blueprint = np.full(G, -1, dtype=np.int64)
    L, H = hid["h0"].shape[0], hid["h0"].shape[2]
    noop = torch.full((cap, P), A - 1, dtype=torch.int64, device=DEV)
    for c0 in range(0, len(jobs), cap):
        chunk = jobs[c0:c0 + cap]
        slots = [cap - 1 - i for i in range(len(chunk))]
        src, seeds = np.full(cap, -1, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        key, player = np.zeros(cap, dtype=np.int64), np.full(cap, -1, dtype=np.int32)
        for s, (g, a, w) in zip(slots, chunk):
            src[s], seeds[s], key[s], player[s] = g, world_seed(seed, g, w), world_key(g, w), cur[g]
        senv.fork_from(root, torch.from_numpy(src), torch.from_numpy(seeds))
        senv.determinize(torch.from_numpy(player), torch.from_numpy(key), seed)
        dst_rows = torch.tensor([s * P + p for s in slots for p in range(P)], device=DEV)
        src_rows = torch.tensor([g * P + p for (g, a, w) in chunk for p in range(P)], device=DEV)
        h, c = torch.zeros(L, cap * P, H, device=DEV), torch.zeros(L, cap * P, H, device=DEV)
        h[:, dst_rows], c[:, dst_rows] = hid["h0"][:, src_rows], hid["c0"][:, src_rows]
        hd = {"h0": h, "c0": c}
        for t in range(depth + 1):
            live = senv.query()[:, Q_TERM] == 0
            reply, hd = agent.act(_obs(senv), hd)
            a_all, g_all = reply["a"].view(cap, P).clone(), reply["greedy_a"].view(cap, P)
            if t == 0:
                for s, (g, a, w) in zip(slots, chunk):
                    if w == 0 and blueprint[g] < 0:
                        blueprint[g] = int(g_all[s, cur[g]])
                    a_all[s, cur[g]] = a
            senv.step(torch.where(live.unsqueeze(1), a_all, noop).contiguous(), torch.where(live.unsqueeze(1), g_all, noop).contiguous())
        q_rows = _act_q(agent, _obs(senv), hd)["q_online_a"].cpu().numpy().reshape(cap, P)
        v, counted, cut, bad = R.from_query(senv.query().cpu().numpy(), q_rows, mode, perfect)
        for s, (g, a, w) in zip(slots, chunk):
            assert counted[s]
            totals[g, a] += (v[s], v[s] * v[s], 1)
            cuts[g, a] += int(cut[s])
            nonfinite += int(bad[s])
    senv.close()
    values = np.full((G, A), np.nan, dtype=np.float32)
    n = totals[..., 2]
    values[n > 0] = (totals[..., 0][n > 0].astype(np.float64) / n[n > 0].astype(np.float64) / 256).astype(np.float32)
    return values, totals, cuts, blueprint, nonfinite


def _same(x, y):
    x, y = torch.as_tensor(x), torch.as_tensor(y).to(x.device)
    return x.dtype == y.dtype and torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0))


@pytest.fixture(scope="module", params=[("bf16", "mover"), ("3p", "team")], ids=["sad-bf16-mover", "3p-team"])
def rooted(request):
    kind, horizon_value = request.param
    agent, P = _agent(kind)
    root, hid = _make_root(agent, P, 5 if P == 2 else 4)
    return agent, root, hid, horizon_value


@pytest.mark.parametrize("depth", [0, 2])
def test_depth_limited_search_equals_the_loop_over_the_primitives(rooted, depth):
    from hanabi_sad_amd.search import policy_action_values
    agent, root, hid, horizon_value = rooted
    before = [root.export_state().clone(), root.priv_s.clone(), hid["h0"].clone(), hid["c0"].clone()]
    counter = getattr(agent, "counter", None)
    sv = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64, depth=depth, horizon_value=horizon_value, keep_world_values=True)
    if counter is not None:
        # depth + 1 moves per chunk and nothing for the valuing act
        n_jobs = int(sv.totals[..., 2].sum())
        assert agent.counter - counter == (depth + 1) * ((n_jobs + 63) // 64)
    mode = {"mover": R.MOVER, "team": R.TEAM}[horizon_value]
    values, totals, cuts, blueprint, nonfinite = _yardstick(root, agent, hid, WORLDS, SEED, depth, mode)
    jobs = int(totals[..., 2].sum())
    assert jobs > 96 and jobs % 64 != 0                                # several chunks and a short last one
    assert sv.scale == 256 and sv.nonfinite == nonfinite == 0
    assert np.array_equal(sv.totals.cpu().numpy(), totals)
    assert np.array_equal(sv.cut.cpu().numpy(), cuts)
    assert np.array_equal(sv.blueprint_a.cpu().numpy(), blueprint)
    assert _same(sv.values, torch.from_numpy(values))
    for x, y in zip(before, [root.export_state(), root.priv_s, hid["h0"], hid["c0"]]):
        assert torch.equal(x, y)
    # the table holds every world's own value: its rows add up to the totals
    wv = sv.world_values.cpu().numpy().astype(np.int64)
    played = wv != R.NOT_PLAYED
    assert sv.world_values.dtype == torch.uint16 and wv.shape == (root.G, root.A, WORLDS)
    assert np.array_equal(played.sum(-1), totals[..., 2]) and np.array_equal((wv * played).sum(-1), totals[..., 0])
    assert np.array_equal((wv * wv * played).sum(-1), totals[..., 1])
    # the capacity changes nothing
    again = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=96, depth=depth, horizon_value=horizon_value)
    assert torch.equal(again.totals, sv.totals) and torch.equal(again.cut, sv.cut) and _same(again.values, sv.values) and again.world_values is None
    assert (totals[..., 0] % 256 != 0).any(), "no world was valued with a Q"
    finished = jobs - int(cuts.sum())
    print("depth %d, %s: %d jobs, %d cut at the horizon, %d finished" % (depth, horizon_value, jobs, int(cuts.sum()), finished))
    if depth == 0:
        assert int(cuts.sum()) > 0
    if horizon_value == "mover" and depth == 2:       # the zoo fixture's games are short: both kinds of world occur here
        assert int(cuts.sum()) > 0 and finished > 0


# ------------------------------------------------------------------------------------------------------------------
# 3. a depth no game outlasts is the full search
# ------------------------------------------------------------------------------------------------------------------
def test_full_depth_is_the_full_search():
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.search import PolicySearch, policy_action_values
    from hanabi_sad_amd.selfplay import init_weights
    s = SF.SEARCH_ROOT
    root = BatchedHanabiEnv(s["G"], seed=s["seed"], eps_list=SF.EPS, device=DEV, **SF.env_kwargs(s["config"], False, False, 0))
    root.rollout_random(s["iters"], s["pseed"])
    net = CNet(init_weights(root.F, 64, root.A, SF.CONFIGS[s["config"]]["hand_size"], 5), DEV)
    agent = CompositeAgent(net, net, 1, 0.99)
    hid = agent.get_h0(root.G * root.P)
    hid = {"h0": hid["h0"], "c0": hid["c0"]}
    full = policy_action_values(root, agent, hid, s["worlds"], s["search_seed"], capacity=64, keep_world_values=True)
    # 20 cards, 4 of them dealt: at most 16 + 2 card moves (the deck, then one last turn each), and 3 + 18 hints (every discard
    # returns a token at most): no game of this variant lasts more than 39 moves
    ps = PolicySearch(root, agent, 64, depth=40, horizon_value="team")
    try:
        deep = ps.search(root, hid, s["worlds"], s["search_seed"], keep_world_values=True)
        chunks = (int(deep.totals[..., 2].sum()) + 63) // 64
        assert ps.acts == 42 * chunks and ps.iterations == 41 * chunks and ps.open_games == []      # D + 2 acts, no word read back
    finally:
        ps.close()
    assert int(full.totals[..., 2].sum()) > 64 and int(full.totals[..., 0].sum()) > 0
    assert deep.scale == 256 and full.scale == 1 and full.cut is None and int(deep.cut.sum()) == 0 and deep.nonfinite == 0
    mul = torch.tensor([256, 65536, 1], dtype=torch.int64, device=deep.totals.device)
    assert torch.equal(deep.totals, full.totals * mul)
    assert _same(deep.values, full.values) and torch.equal(deep.blueprint_a, full.blueprint_a)
    wf, wd = full.world_values.cpu().numpy().astype(np.int64), deep.world_values.cpu().numpy().astype(np.int64)
    assert np.array_equal(wf == R.NOT_PLAYED, wd == R.NOT_PLAYED) and np.array_equal(np.where(wf == R.NOT_PLAYED, 0, wf * 256), np.where(wd == R.NOT_PLAYED, 0, wd))
    # depth=None is the search it has always been
    plain = policy_action_values(root, agent, hid, s["worlds"], s["search_seed"], capacity=64)
    assert torch.equal(plain.totals, full.totals) and _same(plain.values, full.values) and plain.world_values is None
    root.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. play_with_search      5. the command
# ------------------------------------------------------------------------------------------------------------------
def test_play_with_search_at_a_depth_repeats_and_writes_the_depth_down():
    from hanabi_sad_amd.eval import env_dims
    from hanabi_sad_amd.search import play_with_search
    from hanabi_sad_amd.selfplay import init_weights
    rules = {k: v for k, v in SF.CONFIGS["small"].items() if k not in ("players", "hand_size")}
    F, A = env_dims(2, 2, True, **rules)
    W = init_weights(F, 64, A, 2, 3)
    kw = dict(worlds=4, search_seed=77, num_player=2, hand_size=2, device=DEV, depth=2, horizon_value="team", **rules)
    one = play_with_search(W, 8, 301, 0, True, **kw)
    two = play_with_search(W, 8, 301, 0, True, records=True, **kw)
    assert one.scores == two.scores and torch.equal(one.deviations, two.deviations) and len(one.trace) == len(two.trace)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(one.trace, two.trace))
    assert (one.worlds_played, one.worlds_cut, one.nonfinite) == (two.worlds_played, two.worlds_cut, two.nonfinite)
    assert 0 < one.worlds_cut < one.worlds_played and one.cut_share == one.worlds_cut / one.worlds_played and one.nonfinite == 0
    assert one.records is None and len(two.records) == 8
    for k, r in enumerate(two.records):
        assert r.meta["depth"] == 2 and r.meta["horizon_value"] == "team" and r.meta["worlds"] == 4 and r.meta["game"] == k
    for v in two.search_values:
        assert (v[np.isfinite(v)] >= 0).all() and (v[np.isfinite(v)] <= 10).all()
    plain = play_with_search(W, 8, 301, 0, True, worlds=4, search_seed=77, num_player=2, hand_size=2, device=DEV, records=True, **rules)
    assert plain.cut_share is None and plain.worlds_cut is None and "depth" not in plain.records[0].meta
    print("depth 2: scores", one.scores, "cut share %.3f" % one.cut_share, "; full search: scores", plain.scores)


def test_eval_model_command_prints_the_cut_share():
    cmd = [sys.executable, "-m", "hanabi_sad_amd.eval_model", "--paper", "op", "--method", "sad", "--root", os.path.join("tests", "golden", "op_zoo"),
           "--num_game", "4", "--device", DEV, "--idx", "0", "--search_worlds", "2", "--search_depth", "1"]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)     # a fresh child process
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len([l for l in lines if re.match(r"blueprint: \S+ \+/- \S+ ; perfect:  \S+$", l)]) == 1
    found = [re.match(r"blueprint \+ search \(2 worlds\): (\S+) \+/- (\S+) ; perfect:  (\S+) ; deviations per game: (\S+) ; depth 1 \(mover\): "
                      r"(\S+) of the worlds cut at the horizon$", l) for l in lines]
    found = [m for m in found if m]
    assert len(found) == 1
    mean, sem, perfect, dev, share = (float(x) for x in found[0].groups())
    assert 0.0 <= mean <= 25.0 and sem >= 0.0 and 0.0 <= perfect <= 1.0 and dev >= 0.0 and 0.0 < share <= 1.0
