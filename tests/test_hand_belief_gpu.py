"""GPU: hsad_env_hand_belief and hsad_env_determinize_exact (BatchedHanabiEnv.hand_belief / determinize_exact) against the Python
restatement (tests/hand_belief_ref.py, itself held to brute-force enumeration by test_hand_belief_cpu.py), and the
sampler="stratified" path of the search on top of them.  Every comparison is an integer or bit equality.

States: tests/search_fixtures.DET_CASES made with rollout_random, 33 and 65 games (two workgroups of the one-thread-per-game
kernels' observe pass, the second partial; 33 / 65 workgroups of the belief kernel), viewer -1 in every ninth game."""
from collections import Counter

import numpy as np
import pytest
import torch

from tests import determinize_ref as R
from tests import hand_belief_ref as B
from tests import search_fixtures as SF
from tests.test_env_fork_gpu import make_env, same, snapshot

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"
CASE_IDS = [c[0] for c in SF.DET_CASES]
_REF = {}


def det_state(case):
    """-> (env after the case's rollout, viewer, key, live mask, export_state rows)"""
    _, config, sad, sc, km, G, gpw, seed, pseed, iters, _ = case
    env = make_env(config, sad, sc, km, G, gpw, seed)
    env.rollout_random(iters, pseed)
    viewer, key = SF.viewers_and_keys(G, env.P)
    q = env.query().cpu().numpy()
    live = (q[:, 14] == 1) & (q[:, 0] == 0) & (viewer >= 0)
    assert live.any() and (~live).any()
    return env, viewer, key, live, env.export_state().cpu().numpy()


def reference(case, rows, viewer, live, P, H):
    """{game: (N, counts, trinary)} of the case's live games, computed once per case"""
    if case[0] not in _REF:
        _REF[case[0]] = ({g: B.belief_row(rows[g], P, H, int(viewer[g])) for g in np.nonzero(live)[0]}, rows.copy())
    ref, ref_rows = _REF[case[0]]
    assert np.array_equal(rows, ref_rows), "the case's state is not the one the reference was computed on"
    return ref


# ------------------------------------------------------------------------------------------------------------------
# 1. belief parity
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SF.DET_CASES, ids=CASE_IDS)
def test_hand_belief_equals_the_restatement_and_only_reads(case):
    env, viewer, key, live, rows = det_state(case)
    G, P, H = env.G, env.P, env.H
    before = snapshot(env)
    bel = env.hand_belief(viewer)
    env.check_errors()
    after = snapshot(env)
    for name in after:
        assert same(after[name], before[name]), "hand_belief changed %s" % name
    assert bel.total.dtype == bel.counts.dtype == bel.trinary.dtype == torch.int64
    assert bel.total.shape == (G,) and bel.counts.shape == (G, H, 25) and bel.trinary.shape == (G, H, 3)
    total, counts, tri = bel.total.cpu().numpy(), bel.counts.cpu().numpy(), bel.trinary.cpu().numpy()
    ref = reference(case, rows, viewer, live, P, H)
    for g in range(G):
        if not live[g]:
            assert total[g] == 0 and not counts[g].any() and not tri[g].any(), "game %d is skipped" % g
            continue
        N, num, t3 = ref[g]
        assert N >= 1 and int(total[g]) == N, g
        assert counts[g].tolist() == num, g
        assert tri[g].tolist() == t3, g
        for i, (card, _, _) in enumerate(R.hand_of(rows[g], P, H, int(viewer[g]))):
            assert counts[g, i, card] > 0, "game %d slot %d: the true card has no weight" % (g, i)
    assert len({int(total[g]) for g in np.nonzero(live)[0]}) > 3
    probs, tprobs = bel.probs(), bel.trinary_probs()
    assert probs.dtype == tprobs.dtype == torch.float64
    occupied = torch.from_numpy(np.stack([[len(R.hand_of(rows[g], P, H, int(viewer[g]))) > i if live[g] else False for i in range(H)]
                                          for g in range(G)])).to(DEV)
    one = occupied.to(torch.float64)
    assert torch.allclose(probs.sum(dim=2), one, rtol=0, atol=1e-12) and torch.allclose(tprobs.sum(dim=2), one, rtol=0, atol=1e-12)
    assert torch.equal(probs[~torch.from_numpy(live).to(DEV)], torch.zeros_like(probs[~torch.from_numpy(live).to(DEV)]))
    env.close()


def test_hand_belief_needs_no_observation_rows():
    """a sad = 1 env whose float32 and bit rows are not bound (bf16 rows only): the belief reads the state planes alone, while
    determinize_exact is refused like determinize -- it has no row to keep the SAD section from"""
    from hanabi_sad_amd import _lib
    case = SF.DET_CASES[2]                                  # small-sad-k1
    _, config, sad, sc, km, G, gpw, seed, pseed, iters, det_seed = case
    assert sad
    env = make_env(config, sad, sc, 0, G, gpw, seed)        # knowledge_mode 0: the packed outputs exist
    env.rollout_random(iters, pseed)
    viewer, key = SF.viewers_and_keys(G, env.P)
    _lib.check(env.lib.hsad_env_bind_packed(env.h, None, None, None, env.priv_s_bf16.data_ptr(), env.priv_s_bf16.shape[-1], 0))
    rows = env.export_state().cpu().numpy()
    q = env.query().cpu().numpy()
    live = (q[:, 14] == 1) & (q[:, 0] == 0) & (viewer >= 0)
    bel = env.hand_belief(viewer)
    assert np.array_equal(env.export_state().cpu().numpy(), rows)
    n_live = 0
    for g in range(G):
        if live[g]:
            N, num, t3 = B.belief_row(rows[g], env.P, env.H, int(viewer[g]))
            assert (int(bel.total[g]), bel.counts[g].tolist(), bel.trinary[g].tolist()) == (N, num, t3), g
            n_live += 1
        else:
            assert int(bel.total[g]) == 0 and not bool(bel.counts[g].any()) and not bool(bel.trinary[g].any())
    assert n_live > 8
    with pytest.raises(_lib.HsadError, match="sad"):
        env.determinize_exact(viewer, key, det_seed)
    env.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. sampler parity
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SF.DET_CASES, ids=CASE_IDS)
def test_determinize_exact_equals_the_restatement_and_observes_like_a_fork(case):
    _, config, sad, sc, km, G, gpw, seed, pseed, iters, det_seed = case
    env, viewer, key, live, rows = det_state(case)
    P, H = env.P, env.H
    ref = reference(case, rows, viewer, live, P, H)
    before = snapshot(env)
    rank = env.determinize_exact(viewer, key, det_seed)
    env.check_errors()
    assert rank.dtype == torch.int64 and rank.shape == (G,)
    rank = rank.cpu().numpy()
    after = snapshot(env)
    a_rows = after["state"].cpu().numpy()
    n_changed = 0
    for g in range(G):
        if not live[g]:
            assert rank[g] == -1, g
            for name in after:
                assert same(after[name][g], before[name][g]), "game %d was skipped but its %s changed" % (g, name)
            continue
        N = ref[g][0]
        want_rank = B.stratified_rank(N, 0, 1, int(key[g]), det_seed)
        assert 0 <= want_rank < N and int(rank[g]) == want_rank, g
        want = B.determinize_exact_row(rows[g], P, H, int(viewer[g]), want_rank)
        assert np.array_equal(a_rows[g], want), "game %d: state after determinize_exact differs from the restatement" % g
        n_changed += int(not np.array_equal(a_rows[g], rows[g]))
    assert n_changed > 0
    # the rows of the resampled games are what the observe pass of a fork writes from the new state
    second = make_env(config, sad, sc, km, G, gpw, seed + 1)
    second.fork_from(env, np.arange(G, dtype=np.int32))
    sel = torch.from_numpy(live).to(DEV)
    forked = snapshot(second)
    for name in after:
        assert same(after[name][sel], forked[name][sel]), "%s of the resampled games is not what a fork of the result observes" % name
    second.close()
    env.close()


def test_determinize_exact_refuses_a_strata_count_out_of_range():
    from hanabi_sad_amd import _lib
    env, viewer, key, live, rows = det_state(SF.DET_CASES[3])
    for n_strata in (0, -3, (1 << 20) + 1):
        with pytest.raises(_lib.HsadError, match="n_strata"):
            env.determinize_exact(viewer, key, 1, n_strata=n_strata)
    assert np.array_equal(env.export_state().cpu().numpy(), rows)
    env.close()


# ------------------------------------------------------------------------------------------------------------------
# 3 / 4. every rank of one small belief; strata
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_game():
    """the first live game of small-sc-k0: hand size 2, 20 cards -> N <= 380"""
    case = SF.DET_CASES[3]
    assert case[0] == "small-sc-k0"
    _, config, sad, sc, km, Gs, gpw, seed, pseed, iters, _ = case
    src = make_env(config, sad, sc, km, Gs, gpw, seed)
    src.rollout_random(iters, pseed)
    q = src.query().cpu().numpy()
    g0 = int(np.nonzero((q[:, 0] == 0) & (q[:, 14] == 1))[0][0])
    p = int(q[g0, 1])
    row = src.export_state().cpu().numpy()[g0]
    pool, cms, hand = B.pool_and_masks(row, src.P, src.H, p)
    masks = [(cp, rp) for _, cp, rp in R.hand_of(row, src.P, src.H, p)]
    N = B.total_of(pool, cms)
    assert 2 <= N <= 380 and len(hand) == 2
    yield dict(src=src, g0=g0, p=p, row=row, pool=pool, cms=cms, masks=masks, N=N, cfg=(config, sad, sc, km))
    src.close()


def forks_of(s, n):
    dst = make_env(*s["cfg"], n, 32, 1)
    dst.fork_from(s["src"], np.full(n, s["g0"], np.int32))
    return dst


def hands_of(rows, s):
    P, H = s["src"].P, s["src"].H
    return [tuple(card for card, _, _ in R.hand_of(r, P, H, s["p"])) for r in rows]


def test_every_rank_gives_every_hand_exactly_its_weight(small_game):
    s, N = small_game, small_game["N"]
    dst = forks_of(s, N + 2)
    base = snapshot(dst)
    rank_in = np.concatenate([np.arange(N), [N, -1]]).astype(np.int64)
    out = dst.determinize_exact(np.full(N + 2, s["p"], np.int32), np.zeros(N + 2, np.int64), 0, rank=rank_in).cpu().numpy()
    dst.check_errors()
    assert out.tolist() == list(range(N)) + [-1, -1]
    after = snapshot(dst)
    for name in after:
        assert same(after[name][N:], base[name][N:]), "a rank outside [0, N) changed %s" % name
    rows = after["state"].cpu().numpy()
    hist = Counter(hands_of(rows[:N], s))
    dist = R.exact_distribution(s["pool"], s["masks"])
    assert dict(hist) == {h: int(round(p * N)) for h, p in dist.items()}
    assert sum(hist.values()) == N and all(abs(p * N - round(p * N)) < 1e-6 for p in dist.values())
    for r in range(N):
        assert np.array_equal(rows[r], B.determinize_exact_row(s["row"], s["src"].P, s["src"].H, s["p"], r)), r
    dst.close()


def test_strata_cover_the_belief_and_equal_keys_give_equal_worlds(small_game):
    s, N = small_game, small_game["N"]
    seed, W = 4711, 16
    # 32 slots: slot j and slot j + 16 share (key, seed, stratum)
    n = 2 * W
    stratum = (np.arange(n) % W).astype(np.int32)
    key = (7 - (np.arange(n) % W) // 4).astype(np.int64)          # a few keys, a negative one among them
    dst = forks_of(s, n)
    out = dst.determinize_exact(np.full(n, s["p"], np.int32), key, seed, stratum=stratum, n_strata=W).cpu().numpy()
    rows = dst.export_state().cpu().numpy()
    for j in range(n):
        lo, hi = B.stratum_bounds(N, int(stratum[j]), W)
        assert (lo <= out[j] < hi) if hi > lo else out[j] == lo, j
        assert int(out[j]) == B.stratified_rank(N, int(stratum[j]), W, int(key[j]), seed), j
        assert np.array_equal(rows[j], B.determinize_exact_row(s["row"], s["src"].P, s["src"].H, s["p"], int(out[j]))), j
    for j in range(W):
        assert out[j] == out[j + W] and np.array_equal(rows[j], rows[j + W])
        assert torch.equal(dst.priv_s[j], dst.priv_s[j + W]) and torch.equal(dst.priv_bits[j], dst.priv_bits[j + W])
    if N >= W:      # no stratum is empty: the 16 worlds are 16 different ranks
        assert len(set(out.tolist())) == W
    dst.close()
    # W = 2 N: every second stratum is empty; two more slots name a stratum outside [0, W)
    W = 2 * N
    n = W + 2
    stratum = np.concatenate([np.arange(W), [W, -1]]).astype(np.int32)
    key = (np.arange(n) * 1000003 + 5).astype(np.int64)
    dst = forks_of(s, n)
    base = dst.export_state().cpu().numpy()
    out = dst.determinize_exact(np.full(n, s["p"], np.int32), key, seed, stratum=stratum, n_strata=W).cpu().numpy()
    rows = dst.export_state().cpu().numpy()
    empty = 0
    for j in range(W):
        lo, hi = B.stratum_bounds(N, j, W)
        empty += hi == lo
        assert (lo <= out[j] < hi) if hi > lo else out[j] == lo, j
        assert int(out[j]) == B.stratified_rank(N, j, W, int(key[j]), seed), j
    assert empty == N and sorted(set(out[:W].tolist())) == list(range(N))
    assert out[W:].tolist() == [-1, -1] and np.array_equal(rows[W:], base[W:])
    dst.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. the search with sampler="stratified"
# ------------------------------------------------------------------------------------------------------------------
def _same_values(a, b):
    return a.dtype == b.dtype == torch.float32 and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_mc_action_values_stratified_equals_the_loop_and_ignores_the_chunking():
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.search import mc_action_values, world_key, world_seed
    s = SF.SEARCH_ROOT
    root = BatchedHanabiEnv(s["G"], seed=s["seed"], eps_list=SF.EPS, device=DEV, **SF.env_kwargs(s["config"], False, False, 0))
    root.rollout_random(s["iters"], s["pseed"])
    before = root.export_state()
    got = {cap: mc_action_values(root, s["worlds"], s["search_seed"], capacity=cap, sampler="stratified") for cap in (64, 96)}
    assert torch.equal(root.export_state(), before)
    assert _same_values(got[64], got[96])
    plain = mc_action_values(root, s["worlds"], s["search_seed"], capacity=64)
    assert _same_values(plain, mc_action_values(root, s["worlds"], s["search_seed"], capacity=64, sampler="rejection"))
    with pytest.raises(ValueError):
        mc_action_values(root, s["worlds"], s["search_seed"], capacity=64, sampler="exact")
    one = BatchedHanabiEnv(1, seed=0, eps_list=(0.0,), device=DEV, track_deck_history=False, **root.config)
    q = root.query().cpu().numpy()
    legal = root.legal_move.cpu().numpy()
    rows = before.cpu().numpy()
    want = np.full((root.G, root.A), np.nan, np.float32)
    for g in range(root.G):
        if q[g, 0] == 1:
            continue
        p = int(q[g, 1])
        pool, cms, _ = B.pool_and_masks(rows[g], root.P, root.H, p)
        N = B.total_of(pool, cms)
        for a in np.nonzero(legal[g, p])[0]:
            total = 0
            for w in range(s["worlds"]):
                one.fork_from(root, [g], [world_seed(s["search_seed"], g, w)])
                r = int(one.determinize_exact([p], [world_key(g, w)], s["search_seed"], stratum=[w], n_strata=s["worlds"])[0])
                assert r == B.stratified_rank(N, w, s["worlds"], world_key(g, w), s["search_seed"])
                act = torch.full((1, root.P), root.A - 1, dtype=torch.int64, device=DEV)
                act[0, p] = int(a)
                one.step(act, act)
                one.playout_random(80, s["search_seed"], key=[world_key(g, w)])
                qq = one.query()[0].cpu().numpy()
                assert qq[0] == 1
                total += int(qq[2])
            want[g, a] = np.float32(total) / np.float32(s["worlds"])
    one.check_errors()
    assert _same_values(got[64], torch.from_numpy(want).to(DEV))
    one.close()
    root.close()


def test_policy_action_values_stratified_ignores_the_chunking():
    from hanabi_sad_amd.search import PolicySearch, policy_action_values
    from tests.test_policy_search_gpu import SEED, WORLDS, _agent, _make_root
    agent, P = _agent("3p")
    root, hid = _make_root(agent, P, 4)
    before = root.export_state().clone()
    got = {cap: policy_action_values(root, agent, hid, WORLDS, SEED, capacity=cap, sampler="stratified") for cap in (64, 96)}
    assert torch.equal(got[64].totals, got[96].totals) and torch.equal(got[64].blueprint_a, got[96].blueprint_a)
    assert torch.equal(got[64].values.view(torch.int32), got[96].values.view(torch.int32))
    assert torch.equal(got[64].sem.view(torch.int32), got[96].sem.view(torch.int32))
    assert int(got[64].totals[..., 2].sum()) > 96 and torch.equal(root.export_state(), before)
    plain = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64)
    named = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64, sampler="rejection")
    assert torch.equal(plain.totals, named.totals) and torch.equal(plain.values.view(torch.int32), named.values.view(torch.int32))
    assert torch.equal(plain.blueprint_a, named.blueprint_a) and torch.equal(plain.blueprint_a, got[64].blueprint_a)
    ps, ps_named = PolicySearch(root, agent, 64), PolicySearch(root, agent, 64, sampler="rejection")
    try:
        assert torch.equal(ps.search(root, hid, WORLDS, SEED).totals, plain.totals)
        assert torch.equal(ps_named.search(root, hid, WORLDS, SEED).totals, plain.totals)
    finally:
        ps.close()
        ps_named.close()
    with pytest.raises(ValueError):
        PolicySearch(root, agent, 64, sampler="exact")
    root.close()


def test_play_with_search_takes_the_sampler():
    """Hanabi-Small with a random 64-unit net: games of a few moves"""
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.search import play_with_search
    from hanabi_sad_amd.selfplay import init_weights
    rules = SF.CONFIGS["small"]
    probe = BatchedHanabiEnv(1, seed=0, eps_list=(0.0,), device=DEV, **SF.env_kwargs("small", False, False, 0))
    net = CNet(init_weights(probe.F, 64, probe.A, probe.H, 1), DEV)
    probe.close()
    agent = CompositeAgent(net, net, 1, 0.99)
    kw = dict(worlds=4, threshold=0.05, search_seed=3, capacity=64, device=DEV, num_player=rules["players"], hand_size=rules["hand_size"],
              colors=rules["colors"], ranks=rules["ranks"], max_information_tokens=rules["max_information_tokens"],
              max_life_tokens=rules["max_life_tokens"])

    def equal(x, y):
        return x.scores == y.scores and torch.equal(x.deviations, y.deviations) and len(x.trace) == len(y.trace) and \
            all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(x.trace, y.trace))
    plain = play_with_search(agent, 3, 11, 0, False, **kw)
    assert equal(plain, play_with_search(agent, 3, 11, 0, False, sampler="rejection", **kw))
    strat = play_with_search(agent, 3, 11, 0, False, sampler="stratified", **kw)
    assert equal(strat, play_with_search(agent, 3, 11, 0, False, sampler="stratified", **kw))
    assert len(strat.trace) > 0 and all(0 <= x <= 10 for x in strat.scores)
    with pytest.raises(ValueError):
        play_with_search(agent, 3, 11, 0, False, sampler="exact", **kw)


# ------------------------------------------------------------------------------------------------------------------
# 6. the replay stage with the stratified sampler
# ------------------------------------------------------------------------------------------------------------------
def test_replay_with_the_stratified_sampler_holds_the_same_worlds_and_the_true_hand_never_mismatches():
    from hanabi_sad_amd.search import PolicySearch, world_key, world_seed
    from tests import test_search_replay_gpu as T
    h = T.play_root("2p", 1, 0, 7)
    G, WORLDS, SEED = T.G, T.WORLDS, T.SEED
    P, H, n = h.P, h.H, T.G * T.WORLDS
    cur = h.q[:, T.Q_CUR].astype(np.int64)
    live = h.q[:, T.Q_TERM] == 0                     # a root game that has ended is not searched
    assert live.sum() >= 4
    g_of, w_of = np.arange(n) // WORLDS, np.arange(n) % WORLDS
    ok = torch.from_numpy(live[g_of]).to(DEV)
    src, viewer = T.i32(np.where(live[g_of], g_of, -1)), T.i32(np.where(live[g_of], cur[g_of], -1))
    seeds = np.asarray([world_seed(SEED, int(a), int(b)) for a, b in zip(g_of, w_of)], dtype=np.int32)
    key = torch.as_tensor(np.asarray([world_key(int(a), int(b)) for a, b in zip(g_of, w_of)], dtype=np.int64), device=DEV)
    # fork + determinize_exact: what every replayed world must hold
    want_env = T.new_env(h, n=n, seed=41, track=False)
    want_env.fork_from(h.root, src, T.i32(seeds))
    ranks = want_env.determinize_exact(viewer, key, SEED, stratum=T.i32(w_of), n_strata=WORLDS)
    assert bool((ranks[ok] >= 0).all()) and bool((ranks[~ok] == -1).all())
    ps = PolicySearch(h.root, h.agent, capacity=64, replay=True, sampler="stratified")
    try:
        games = np.nonzero(live)[0]
        k = len(games) * WORLDS
        mism = ps._replay(h.root, h.log, games, cur, WORLDS, SEED, seeds.reshape(G, WORLDS))
        assert mism.shape == (k,) and k <= 64
        got = ps.worlds_env[0].env.export_state()[:k].clone()
        want = want_env.export_state()[ok].clone()
        got[:, T.W_DRAWS] = 0
        want[:, T.W_DRAWS] = 0
        assert torch.equal(got, want), "a replayed world does not hold the cards of fork + determinize_exact"
        sv = ps.search(h.root, h.hid, WORLDS, SEED, log=h.log)
        assert torch.equal(sv.mismatch[torch.from_numpy(games).to(DEV)].view(-1), mism)
    finally:
        ps.close()
    # one world per live game is given the true hand through rank_in: it is the root itself, and replays without a mismatch
    rows = h.root.export_state().cpu().numpy()
    true_rank = np.full(G, -1, dtype=np.int64)
    for g in games:
        pool, cms, hand = B.pool_and_masks(rows[g], P, H, int(cur[g]))
        true_rank[g] = B.rank_of(pool, cms, hand)
        assert B.unrank(pool, cms, int(true_rank[g]))[0] == hand
    env = T.new_env(h, n=G, seed=43, track=False)
    idx, seat = T.i32(np.where(live, np.arange(G), -1)), T.i32(np.where(live, cur, -1))
    env.fork_from(h.root, idx, T.i32(np.arange(G) + 1))
    out = env.determinize_exact(seat, torch.zeros(G, dtype=torch.int64), 0, rank=true_rank)
    assert out.cpu().numpy().tolist() == true_rank.tolist()
    sel = torch.from_numpy(live).to(DEV)
    assert torch.equal(T.state_but_draws(env)[sel], T.state_but_draws(h.root)[sel])
    dh52 = torch.nn.functional.pad(h.dh, (0, 2)).contiguous()
    script = torch.zeros(G, 52, dtype=torch.uint8, device=DEV)
    count = torch.zeros(G, dtype=torch.int32, device=DEV)
    T._lib().check(env.lib.hsad_search_world_script(env.h, idx.data_ptr(), seat.data_ptr(), dh52.data_ptr(), h.cnt.data_ptr(), G,
                                                    h.log.a.data_ptr(), h.n_moves, script.data_ptr(), count.data_ptr(), env._stream()))
    env.rewind_scripted(script, count)
    assert torch.equal(count > 0, sel)
    ht, ct, mt, bt = T.replay_with_agent(h, env, idx, seat)
    assert int(mt.abs().sum()) == 0 and int(bt.sum()) == 0, "the true hand's world mismatches"
    r = (torch.arange(G, device=DEV)[sel].unsqueeze(1) * P + torch.arange(P, device=DEV)).flatten()
    assert torch.equal(ht[:, r], h.hid["h0"][:, r]) and torch.equal(ct[:, r], h.hid["c0"][:, r])
    T.drain(env)
    env.close()
    want_env.close()
    h.root.close()
    h.root0.close()
