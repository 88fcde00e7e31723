"""GPU: blueprint-policy search (search.PolicySearch / policy_action_values / play_with_search, the glue kernels of
csrc/hsad_search.hip and eval_model --search_worlds).

The kernels are held to torch indexing; the search to a test-local loop over what the code base could do before -- fork_from /
determinize, `h[:, rows]` indexing, agent.act, torch.where, env.step, query() -- with the jobs in REVERSED slot order.  A row's
result depends on no other row of a batch and every batch here stays under the 1,024-row switch of the act kernels, so values,
totals and the blueprint's move must agree bit for bit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZOO = os.path.join(os.path.dirname(__file__), "golden", "op_zoo")
DEV = "cuda:0"
Q_TERM, Q_CUR, Q_SCORE, Q_STARTED = 0, 1, 2, 14
INVALID = -1            # HSAD_ERR_INVALID


# ------------------------------------------------------------------------------------------------------------------
# 1. hsad_search_fork_state against torch.index_select
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,G_src,G_dst", [(2, 7, 96), (3, 5, 5)])
def test_fork_state_against_index_select(P, G_src, G_dst):
    from hanabi_sad_amd import _lib
    lib = _lib.load_library()
    L, H = 2, 64
    gen = torch.Generator().manual_seed(10 * P + G_dst)
    h_src = torch.randn(L, G_src * P, H, generator=gen).to(DEV)
    c_src = torch.randn(L, G_src * P, H, generator=gen).to(DEV)
    idx = torch.randint(0, G_src, (G_dst,), generator=gen).to(torch.int32)
    idx[:5] = torch.tensor([-1, 3, 3, G_src, -7], dtype=torch.int32)        # skip, a repeated source, two values out of range
    idx = idx.to(DEV)
    h_keep, c_keep = h_src.clone(), c_src.clone()
    valid = ((idx >= 0) & (idx < G_src))
    rows = (idx.long().clamp(0, G_src - 1).unsqueeze(1) * P + torch.arange(P, device=DEV)).reshape(-1)
    keep = ~valid.repeat_interleave(P).view(1, -1, 1)
    want_h = torch.where(keep, torch.full_like(h_src[:, :1, :1], 7.0), torch.index_select(h_src, 1, rows))
    want_c = torch.where(keep, torch.full_like(h_src[:, :1, :1], 7.0), torch.index_select(c_src, 1, rows))
    want_16 = torch.where(keep, torch.full_like(h_src[:, :1, :1], 7.0).to(torch.bfloat16), torch.index_select(h_src, 1, rows).to(torch.bfloat16))
    st = torch.cuda.current_stream().cuda_stream
    for with16 in (True, False):
        h = torch.full((L, G_dst * P, H), 7.0, device=DEV)
        c = torch.full((L, G_dst * P, H), 7.0, device=DEV)
        h16 = torch.full((L, G_dst * P, H), 7.0, device=DEV, dtype=torch.bfloat16)
        _lib.check(lib.hsad_search_fork_state(idx.data_ptr(), G_dst, G_src, P, L, H, h_src.data_ptr(), c_src.data_ptr(), h.data_ptr(),
                                              c.data_ptr(), h16.data_ptr() if with16 else None, st))
        assert torch.equal(h.view(torch.int32), want_h.view(torch.int32))
        assert torch.equal(c.view(torch.int32), want_c.view(torch.int32))
        if with16:
            assert torch.equal(h16.view(torch.int16), want_16.view(torch.int16))
        else:
            assert bool((h16 == 7.0).all())
    assert int(valid.sum()) >= 2 and int((~valid).sum()) >= 3
    assert torch.equal(h_src, h_keep) and torch.equal(c_src, c_keep)
    # the refusals
    args = (h_src.data_ptr(), c_src.data_ptr(), h.data_ptr(), c.data_ptr(), None, st)
    assert lib.hsad_search_fork_state(idx.data_ptr(), G_dst, G_src, P, L, 62, *args) == INVALID
    assert lib.hsad_search_fork_state(idx.data_ptr(), 0, G_src, P, L, H, *args) == INVALID
    assert lib.hsad_search_fork_state(idx.data_ptr(), G_dst, G_src, P, -1, H, *args) == INVALID


def test_fork_state_rows_of_four_values():
    """H % 8 != 0: the 16-byte path of the fp32 rows with 8-byte bf16 stores"""
    from hanabi_sad_amd import _lib
    lib = _lib.load_library()
    L, H, P, G_src, G_dst = 1, 12, 2, 3, 300
    gen = torch.Generator().manual_seed(3)
    h_src, c_src = torch.randn(L, G_src * P, H, generator=gen).to(DEV), torch.randn(L, G_src * P, H, generator=gen).to(DEV)
    idx = torch.randint(0, G_src, (G_dst,), generator=gen).to(torch.int32).to(DEV)
    rows = (idx.long().unsqueeze(1) * P + torch.arange(P, device=DEV)).reshape(-1)
    h, c = torch.zeros(L, G_dst * P, H, device=DEV), torch.zeros(L, G_dst * P, H, device=DEV)
    h16 = torch.zeros(L, G_dst * P, H, device=DEV, dtype=torch.bfloat16)
    _lib.check(lib.hsad_search_fork_state(idx.data_ptr(), G_dst, G_src, P, L, H, h_src.data_ptr(), c_src.data_ptr(), h.data_ptr(), c.data_ptr(),
                                          h16.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert torch.equal(h, h_src[:, rows]) and torch.equal(c, c_src[:, rows])
    assert torch.equal(h16.view(torch.int16), h_src[:, rows].to(torch.bfloat16).view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------
# 2 / 3. hsad_search_actions against torch.where, hsad_search_job_stats against numpy on query()
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


def test_search_actions_against_where(mixed_env):
    from hanabi_sad_amd import _lib
    env, q, live_np, _ = mixed_env
    lib, st = env.lib, env._stream()
    G, P, A = env.G, env.P, env.A
    gen = torch.Generator().manual_seed(7)
    a_src = torch.randint(0, A - 1, (G * P,), generator=gen).to(DEV)
    g_src = torch.randint(0, A - 1, (G * P,), generator=gen).to(DEV)
    player = torch.randint(0, P, (G,), generator=gen).to(torch.int32)
    live_ids = np.nonzero(live_np)[0]
    player[int(live_ids[0])], player[int(live_ids[1])] = -1, P                        # a player outside [0, P): no override
    override = torch.randint(0, A - 1, (G,), generator=gen) + 100                     # told apart from every a_src value
    override[torch.rand(G, generator=gen) < 0.4] = -1
    override[int(live_ids[0])], override[int(live_ids[1])] = 105, 106
    player, override = player.to(DEV), override.to(DEV)
    live = torch.from_numpy(live_np).to(DEV).unsqueeze(1)
    noop = torch.full((G, P), A - 1, dtype=torch.int64, device=DEV)
    seat = torch.arange(P, device=DEV).unsqueeze(0) == player.unsqueeze(1)
    forced = seat & (override >= 0).unsqueeze(1)
    want_masked = torch.where(live, a_src.view(G, P), noop)
    want_a = torch.where(live, torch.where(forced, override.unsqueeze(1).expand(G, P), a_src.view(G, P)), noop)
    want_g = torch.where(live, g_src.view(G, P), noop)
    hit = (forced & live).any(0)
    assert bool(hit.all()), "overrides must land on every seat"
    assert bool(((override < 0) & live.squeeze(1)).any()) and int((want_a != want_masked).sum()) == int((forced & live).sum())

    def run(pl, ov):
        a = torch.full((G, P), -5, dtype=torch.int64, device=DEV)
        g = torch.full((G, P), -5, dtype=torch.int64, device=DEV)
        _lib.check(lib.hsad_search_actions(env.h, a_src.data_ptr(), g_src.data_ptr(), None if pl is None else pl.data_ptr(),
                                           None if ov is None else ov.data_ptr(), a.data_ptr(), g.data_ptr(), st))
        return a, g
    a, g = run(player, override)
    assert torch.equal(a, want_a) and torch.equal(g, want_g)
    for pl in (player, None):                                   # override == NULL: masking only
        a, g = run(pl, None)
        assert torch.equal(a, want_masked) and torch.equal(g, want_g)
    assert lib.hsad_search_actions(env.h, a_src.data_ptr(), g_src.data_ptr(), None, override.data_ptr(), a.data_ptr(), g.data_ptr(), st) == INVALID


def test_job_stats_against_numpy_on_query(mixed_env):
    from hanabi_sad_amd import _lib
    env, q, _, finished = mixed_env
    lib, st = env.lib, env._stream()
    G, n_job = env.G, 7
    rng = np.random.default_rng(11)
    # uneven world counts per job; -1 and values >= n_job skip the slot
    jobs = [np.repeat(np.arange(-1, n_job + 2), [9, 30, 1, 12, 5, 0, 17, 8, 6, 8]).astype(np.int32),
            rng.integers(-1, n_job + 1, size=G).astype(np.int32)]
    rng.shuffle(jobs[0])
    assert all(len(j) == G for j in jobs)
    stats = torch.zeros(n_job, 3, dtype=torch.int64, device=DEV)
    want = np.zeros((n_job, 3), dtype=np.int64)
    score = q[:, Q_SCORE].astype(np.int64)
    for k, job in enumerate(jobs):
        jd = torch.from_numpy(job).to(DEV)
        _lib.check(lib.hsad_search_job_stats(env.h, jd.data_ptr(), n_job, stats.data_ptr(), st))
        for g in range(G):
            if finished[g] and 0 <= job[g] < n_job:
                want[job[g]] += (score[g], score[g] * score[g], 1)
        assert np.array_equal(stats.cpu().numpy(), want), k        # the second call adds to the first
    assert want[:, 2].sum() > 0 and len(set(want[:, 2].tolist())) > 2
    if env.config["bomb"] == 0:
        assert want[:, 0].sum() > 0
    assert lib.hsad_search_job_stats(env.h, jd.data_ptr(), 0, stats.data_ptr(), st) == INVALID


# ------------------------------------------------------------------------------------------------------------------
# 4 / 5. policy_action_values equals the loop over the existing primitives; invariance and layout
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
    return env, {"h0": hid["h0"], "c0": hid["c0"]}


def _yardstick(root, agent, hid, worlds, seed, cap=64):
    """the search with none of the new kernels, jobs in reversed slot order -> (values float32 [G, A], totals int64 [G, A, 3],
    blueprint int64 [G]) as numpy"""
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.search import search_jobs, world_key, world_seed
    G, P, A = root.G, root.P, root.A
    pairs, cur = search_jobs(root)
    jobs = [(int(g), int(a), w) for g, a in pairs for w in range(worlds)]
    senv = BatchedHanabiEnv(cap, seed=0, eps_list=(0.0,), device=DEV, track_deck_history=False, **root.config)
    senv.reset()
    totals = np.zeros((G, A, 3), dtype=np.int64)
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
        sl = torch.tensor(slots, device=DEV)
        for t in range(200):
            live = senv.query()[:, Q_TERM] == 0
            if not bool(live[sl].any()):
                break
            reply, hd = agent.act(_obs(senv), hd)
            a_all, g_all = reply["a"].view(cap, P).clone(), reply["greedy_a"].view(cap, P)
            if t == 0:
                for s, (g, a, w) in zip(slots, chunk):
                    if w == 0 and blueprint[g] < 0:
                        blueprint[g] = int(g_all[s, cur[g]])
                    a_all[s, cur[g]] = a
            senv.step(torch.where(live.unsqueeze(1), a_all, noop).contiguous(), torch.where(live.unsqueeze(1), g_all, noop).contiguous())
        else:
            raise AssertionError("yardstick games did not finish")
        score = senv.query()[:, Q_SCORE].cpu().numpy().astype(np.int64)
        for s, (g, a, w) in zip(slots, chunk):
            totals[g, a] += (score[s], score[s] * score[s], 1)
    senv.close()
    values = np.full((G, A), np.nan, dtype=np.float32)
    n = totals[..., 2]
    values[n > 0] = totals[..., 0][n > 0].astype(np.float32) / n[n > 0].astype(np.float32)
    return values, totals, blueprint


@pytest.fixture(scope="module", params=["bf16", "fp32", "3p"])
def searched(request):
    """agent, root, hid, snapshots of what the search may only read, and policy_action_values at capacity 64"""
    from hanabi_sad_amd.search import policy_action_values
    agent, P = _agent(request.param)
    root, hid = _make_root(agent, P, 5 if P == 2 else 4)
    before = [root.export_state().clone(), root.priv_s.clone(), root.legal_move.clone(), hid["h0"].clone(), hid["c0"].clone()]
    sv = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64)
    return agent, root, hid, before, sv


def _same(x, y):
    x, y = torch.as_tensor(x), torch.as_tensor(y).to(x.device)
    return x.dtype == y.dtype and torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0))


def test_policy_action_values_equal_the_loop_over_the_primitives(searched):
    agent, root, hid, before, sv = searched
    values, totals, blueprint = _yardstick(root, agent, hid, WORLDS, SEED)
    jobs = int(totals[..., 2].sum())
    assert jobs > 96 and (jobs % 64 != 0 or jobs % 96 != 0)        # several chunks, and a short last one at capacity 64 or 96
    assert np.array_equal(sv.totals.cpu().numpy(), totals)
    assert _same(sv.values, torch.from_numpy(values))
    assert np.array_equal(sv.blueprint_a.cpu().numpy(), blueprint)
    print("scores summed over the jobs:", int(totals[..., 0].sum()), "jobs:", int(totals[..., 2].sum()))


def test_search_invariance_and_layout(searched):
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.search import policy_action_values
    agent, root, hid, before, sv = searched
    G, P, A = root.G, root.P, root.A
    # the root and the carried state were only read
    after = [root.export_state(), root.priv_s, root.legal_move, hid["h0"], hid["c0"]]
    for name, x, y in zip(("state", "priv_s", "legal_move", "h0", "c0"), before, after):
        assert torch.equal(x, y), name
    # capacity and repeats
    for cap in (96, 64):
        again = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=cap)
        assert torch.equal(again.totals, sv.totals) and _same(again.values, sv.values) and torch.equal(again.blueprint_a, sv.blueprint_a), cap
        assert _same(again.sem, sv.sem)
    other = policy_action_values(root, agent, hid, WORLDS, SEED + 1, capacity=96)
    assert not torch.equal(other.totals, sv.totals)
    assert torch.equal(other.blueprint_a, sv.blueprint_a)
    # layout
    q = root.query()
    cur = q[:, Q_CUR].long()
    assert bool((q[:, Q_TERM] == 0).all())
    legal = root.legal_move[torch.arange(G, device=DEV), cur] != 0
    assert torch.equal(~torch.isnan(sv.values), legal) and torch.equal(~torch.isnan(sv.sem), legal)
    assert torch.equal(sv.totals[..., 2], legal.long() * WORLDS)
    assert sv.values.dtype == torch.float32 and sv.values.device == root.priv_s.device and sv.totals.shape == (G, A, 3)
    reply, _ = agent.act(_obs(root), hid)
    assert torch.equal(sv.blueprint_a, reply["greedy_a"].view(G, P)[torch.arange(G, device=DEV), cur])
    # who searches: a seat (lock-step roots: everyone or no one is on turn), a mask
    seat = int(cur[0])
    on = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64, searcher=seat)
    assert torch.equal(on.totals, sv.totals) and torch.equal(on.blueprint_a, sv.blueprint_a)
    off = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64, searcher=(seat + 1) % P)
    assert bool(torch.isnan(off.values).all()) and bool((off.blueprint_a == -1).all()) and int(off.totals.sum()) == 0
    part = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64, searcher=torch.tensor([1, 0, 1]))
    assert torch.equal(part.totals[[0, 2]], sv.totals[[0, 2]]) and int(part.totals[1].sum()) == 0
    assert part.blueprint_a.tolist() == [int(sv.blueprint_a[0]), -1, int(sv.blueprint_a[2])]
    assert bool(torch.isnan(part.values[1]).all()) and _same(part.values[[0, 2]], sv.values[[0, 2]])
    # a game that is not live: the same root with a fourth, never started game
    wide = BatchedHanabiEnv(4, seed=0, eps_list=(0.0,), device=DEV, track_deck_history=False, **root.config)
    wide.fork_from(root, torch.tensor([0, 1, 2, -1], dtype=torch.int32))
    L, H = hid["h0"].shape[0], hid["h0"].shape[2]
    pad = torch.full((L, P, H), 0.25, device=DEV)
    hid4 = {"h0": torch.cat([hid["h0"], pad], 1), "c0": torch.cat([hid["c0"], pad], 1)}
    sv4 = policy_action_values(wide, agent, hid4, WORLDS, SEED, capacity=64)
    assert torch.equal(sv4.totals[:3], sv.totals) and int(sv4.totals[3].sum()) == 0 and bool(torch.isnan(sv4.values[3]).all())
    assert sv4.blueprint_a.tolist() == sv.blueprint_a.tolist() + [-1]
    wide.close()
    # games that do not end in time are an error, not a silent result
    with pytest.raises(RuntimeError):
        policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64, max_steps=3)


# ------------------------------------------------------------------------------------------------------------------
# 6. play_with_search      7. the command
# ------------------------------------------------------------------------------------------------------------------
def test_play_with_search_without_deviation_is_evaluate():
    from hanabi_sad_amd.eval import evaluate
    from hanabi_sad_amd.search import play_with_search
    agent, _ = _agent("bf16")
    mean, perfect, scores, num_perfect = evaluate(agent, 8, 11, 0, False, device=DEV)
    assert max(scores) > 0
    plain = play_with_search(agent, 8, 11, 0, False, worlds=0, device=DEV)
    assert plain.scores == scores and plain.mean == mean and plain.perfect == perfect and plain.num_perfect == num_perfect
    assert plain.trace == [] and plain.deviations.tolist() == [0] * 8
    never = play_with_search(agent, 8, 11, 0, False, worlds=2, threshold=float("inf"), capacity=256, device=DEV)
    assert never.scores == scores and never.deviations.tolist() == [0] * 8
    assert len(never.trace) > 0 and all(torch.equal(ch, bp) for ch, bp in never.trace)
    assert any(bool((bp >= 0).any()) for _, bp in never.trace)


def test_play_with_search_repeats_and_counts_its_deviations():
    from hanabi_sad_amd.search import play_with_search
    agent, _ = _agent("bf16")
    kw = dict(worlds=4, threshold=0.05, search_seed=3, capacity=256, device=DEV)
    one = play_with_search(agent, 3, 11, 0, False, **kw)
    two = play_with_search(agent, 3, 11, 0, False, **kw)
    assert one.scores == two.scores and torch.equal(one.deviations, two.deviations)
    assert len(one.trace) == len(two.trace) and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(one.trace, two.trace))
    assert all(0 <= s <= 25 for s in one.scores) and one.mean == float(np.mean(one.scores))
    count = sum(((ch >= 0) & (ch != bp)).long() for ch, bp in one.trace)
    assert one.deviations.dtype == torch.int64 and torch.equal(one.deviations, count)
    # one searching seat: the other seat's turns carry no search
    seat0 = play_with_search(agent, 3, 11, 0, False, searcher=0, **kw)
    searched_moves = [t for t, (ch, _) in enumerate(seat0.trace) if bool((ch >= 0).any())]
    assert len(searched_moves) > 1 and len({t % 2 for t in searched_moves}) == 1        # the seats alternate in the 2-player game
    print("scores", one.scores, "deviations", one.deviations.tolist(), "seat 0 only", seat0.scores, seat0.deviations.tolist())


def test_eval_model_command_prints_blueprint_and_search_lines():
    from hanabi_sad_amd.search import play_with_search
    agent, _ = _agent("bf16")
    cmd = [sys.executable, "-m", "hanabi_sad_amd.eval_model", "--paper", "op", "--method", "sad", "--root", os.path.join("tests", "golden", "op_zoo"),
           "--num_game", "4", "--device", DEV, "--idx", "0", "--search_worlds", "2"]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)     # a fresh child process
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    base = play_with_search(agent, 4, 1, 0, False, worlds=0, device=DEV)
    assert [l for l in lines if l.startswith("blueprint:")] == ["blueprint: %f +/- %f ; perfect:  %s" % (base.mean, base.sem, base.perfect)]
    found = [re.match(r"blueprint \+ search \(2 worlds\): (\S+) \+/- (\S+) ; perfect:  (\S+) ; deviations per game: (\S+)$", l) for l in lines]
    found = [m for m in found if m]
    assert len(found) == 1
    mean, sem, perfect, dev = (float(x) for x in found[0].groups())
    assert 0.0 <= mean <= 25.0 and sem >= 0.0 and 0.0 <= perfect <= 1.0 and dev >= 0.0
