"""GPU: the replay stage of blueprint-policy search -- hsad_env_rewind_scripted (BatchedHanabiEnv.rewind_scripted),
hsad_search_world_script, hsad_search_replay_actions, PolicySearch(replay=True) -- all held to bit equalities.

Roots: 8 games played with hsad_env_policy_random for 1, 7 or 20 moves (Hanabi-Small also until a deck has run out and a game has
ended; there the policy's plays are withheld while the deck holds cards, see play_root), an R2D2 agent of 64 hidden units acting alongside: its greedy action is what the root shows (greedy_a) and what the log
keeps, its h / c the state the root carries.  4 worlds per game; every act call has fewer than 1,024 rows (one acting regime)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import search_fixtures as SF
from tests import world_script_ref as W

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"
G, WORLDS, SEED = 8, 4, 2718
Q_TERM, Q_CUR, Q_DECK = 0, 1, 7      # include/hsad.h: hsad_env_query words
W_DRAWS, W_LAST_SCORE = 73, 74       # hsad_env_export_state: the generator's draw count, the score of the game before
RULES = {"2p": dict(players=2, hand_size=5), "3p": dict(players=3, hand_size=5), "small": SF.CONFIGS["small"]}

CASES = [(r, s, 0, n) for r in ("2p", "3p", "small") for s in (0, 1) for n in (1, 7, 20)]
CASES += [("small", 0, 0, "end"), ("small", 1, 0, "end"), ("2p", 0, 1, 7)]


def _lib():
    from hanabi_sad_amd import _lib as L
    return L


def new_env(h, n=G, seed=3, track=True):
    from hanabi_sad_amd import BatchedHanabiEnv
    return BatchedHanabiEnv(n, seed=seed, bomb=0, eps_list=[0.0], max_len=-1, sad=bool(h.sad), shuffle_color=bool(h.sc), device=DEV,
                            track_deck_history=track, **RULES[h.rules])


def obs_of(env):
    N = env.G * env.P
    return {"priv_s": env.priv_s.view(N, env.F), "legal_move": env.legal_move.view(N, env.A), "eps": torch.zeros(N, device=DEV)}


def rows_of(env):
    return {k: getattr(env, k).clone() for k in ("priv_s", "legal_move", "own_hand", "reward", "terminal")}


def drain(env):
    n, g, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib().check(env.lib.hsad_env_error_count(env.h, C.byref(n), C.byref(g), C.byref(c)))
    return n.value, c.value


def state_but_draws(env):
    s = env.export_state().clone()
    s[:, W_DRAWS] = 0
    return s


def i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32, device=DEV)


class Hist:
    pass


def play_root(rules, sad, sc, stop):
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.search import GameLog
    from hanabi_sad_amd.selfplay import init_weights
    L = _lib()
    h = Hist()
    h.rules, h.sad, h.sc = rules, sad, sc
    h.root = root = new_env(h, seed=4100 + 7 * len(rules) + sad)
    root.reset()
    h.P, h.H = root.P, root.H
    net = CNet(init_weights(root.F, 64, root.A, root.H, 1), DEV)
    h.agent = agent = CompositeAgent(net, net, 1, 0.99)
    h.root0 = new_env(h, seed=5)                     # the root as reset left it
    h.root0.fork_from(root, i32(np.arange(G)))
    hid = agent.get_h0(G * root.P)
    h.log = log = GameLog(G, root.P, DEV)
    h.rows = [rows_of(root)]
    t = 0
    while True:
        q = root.query().cpu().numpy()
        if stop == "end":
            if (q[:, Q_DECK] == 0).any() and (q[:, Q_TERM] == 1).any():
                break
            assert t < 80, "no Hanabi-Small game ran its deck out and none ended"
        elif t == stop:
            break
        reply, new_hid = agent.act(obs_of(root), hid)
        a, _ = root.policy_random(77)
        if stop == "end":
            # uniform random play loses Hanabi-Small's one life long before 16 cards are drawn: while a deck holds cards, a play the
            # policy picked is replaced by the mover's lowest legal move that is no play (a discard, else a hint)
            H, pick, legal = root.H, a.cpu().clone(), root.legal_move.cpu()
            for gi in range(G):
                p = int(q[gi, Q_CUR])
                if q[gi, Q_TERM] == 0 and q[gi, Q_DECK] > 0 and H <= int(pick[gi, p]) < 2 * H:
                    other = [u for u in range(root.A - 1) if legal[gi, p, u] != 0 and not H <= u < 2 * H]
                    if other:
                        pick[gi, p] = other[0]
            a.copy_(pick)
        g = reply["greedy_a"].contiguous()
        # finished games get the noop (the existing masking kernel); a aliases the env's own action rows, as its contract allows
        L.check(root.lib.hsad_search_actions(root.h, a.data_ptr(), g.data_ptr(), None, None, root.a.data_ptr(), root.greedy_a.data_ptr(),
                                             root._stream()))
        log.append(root.a, root.greedy_a)
        root.step(root.a, root.greedy_a)
        log.observed(root)
        h.rows.append(rows_of(root))
        hid = new_hid
        t += 1
    h.n_moves = t
    h.hid = {"h0": hid["h0"].contiguous(), "c0": hid["c0"].contiguous()}
    h.n_err, h.err_code = drain(root)       # "step on a finished game" notes of the games that ended on the way
    assert h.n_err == 0 or h.err_code == 3
    h.dh, h.cnt = root.deck_history()
    h.q = root.query().cpu().numpy()
    return h


@pytest.fixture(scope="module", params=CASES, ids=["%s-sad%d-sc%d-n%s" % c for c in CASES])
def hist(request):
    h = play_root(*request.param)
    yield h
    if getattr(h, "sampled", None) is not None:
        h.sampled[0].close()
    h.root.close()
    h.root0.close()


def same_rows(a, b, names=("priv_s", "legal_move", "own_hand", "reward", "terminal")):
    return [k for k in names if not (a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]))]


# ------------------------------------------------------------------------------------------------------------------
# 1. identity replay
# ------------------------------------------------------------------------------------------------------------------
def test_identity_replay_retraces_the_root_move_by_move(hist):
    h = hist
    f = new_env(h, seed=999)
    f.reset()
    f.rollout_random(3, 5)                                      # some other position, another generator
    f.reset()
    f.fork_from(h.root, i32(np.arange(G)), i32(np.arange(G) + 1000))
    f.rewind_scripted(h.dh, h.cnt)
    assert same_rows(rows_of(f), h.rows[0]) == [], "the rows after the rewind are not the rows after the root's reset"
    for t in range(h.n_moves):
        f.step(h.log.a[t].contiguous(), h.log.greedy_a[t].contiguous())
        assert same_rows(rows_of(f), h.rows[t + 1]) == [], "move %d" % t
    assert torch.equal(state_but_draws(f), state_but_draws(h.root))
    assert int(f.export_state()[:, W_DRAWS].max()) == 0         # every deal came from the script: no draw since the reseeded fork
    n, code = drain(f)
    assert (n, code if n else 0) == (h.n_err, h.err_code if h.n_err else 0)      # nothing but the root's own "finished game" notes
    dh, cnt = f.deck_history()
    assert torch.equal(cnt, h.cnt) and torch.equal(dh, h.dh)
    f.close()


def test_past_the_script_the_next_deal_comes_from_the_generator(hist):
    h = hist
    idx, seeds = i32(np.arange(G)), i32(np.arange(G) + 2000)
    ref = new_env(h, seed=11)
    ref.fork_from(h.root0, idx, seeds)                          # the root's first deal, generator `seeds`, never scripted
    f = new_env(h, seed=12)
    f.fork_from(h.root, idx, seeds)
    f.rewind_scripted(h.dh, torch.full((G,), h.P * h.H, dtype=torch.int32))     # the script ends with the initial hands

    def state(env):     # a rewind keeps the last score, as a reset does: a root game that has ended carries its score
        s = env.export_state().clone()
        s[:, W_LAST_SCORE] = 0
        return s
    assert torch.equal(state(f), state(ref)) and same_rows(rows_of(f), rows_of(ref)) == []
    deck0 = ref.query()[:, Q_DECK].clone()
    for t in range(6):
        a, ga = ref.policy_random(5)
        a, ga = a.clone(), ga.clone()
        ref.step(a, ga)
        f.step(a, ga)
        assert torch.equal(state(f), state(ref)), "move %d" % t          # the draw count included
        assert same_rows(rows_of(f), rows_of(ref)) == [], "move %d" % t
    assert bool((ref.query()[:, Q_DECK] < deck0).any())         # cards were dealt
    ref.close()
    f.close()


# ------------------------------------------------------------------------------------------------------------------
# 2 / 3. world scripts against the restatement; the determinised replay arrives at fork + determinize
# ------------------------------------------------------------------------------------------------------------------
def world_lists(h):
    from hanabi_sad_amd.search import world_key, world_seed
    n = G * WORLDS
    g = np.arange(n) // WORLDS
    w = np.arange(n) % WORLDS
    src = g.astype(np.int32)
    viewer = ((g + w) % h.P).astype(np.int32)
    src[5], src[9], viewer[13] = -1, 99, -1                     # untouched, out of range, no viewer
    seeds = np.asarray([world_seed(SEED, int(a), int(b)) for a, b in zip(g, w)], dtype=np.int32)
    key = np.asarray([world_key(int(a), int(b)) for a, b in zip(g, w)], dtype=np.int64)
    return src, viewer, seeds, key


def forked_worlds(h, src, viewer, seeds, key):
    env = new_env(h, n=G * WORLDS, seed=21, track=False)
    env.fork_from(h.root, i32(src), i32(seeds))
    assert drain(env) == (1, 4)                                 # slot 9
    env.determinize(i32(viewer), torch.from_numpy(key).to(DEV), SEED)
    return env


def test_world_script_and_determinised_replay(hist):
    h, L = hist, _lib()
    P, H, n = h.P, h.H, G * WORLDS
    src, viewer, seeds, key = world_lists(h)
    env = forked_worlds(h, src, viewer, seeds, key)
    src_d, viewer_d = i32(src), i32(viewer)
    dh52 = torch.nn.functional.pad(h.dh, (0, 2)).contiguous()
    script = torch.full((n, 52), 77, dtype=torch.uint8, device=DEV)
    count = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    la, lg = h.log.a, h.log.greedy_a
    L.check(env.lib.hsad_search_world_script(env.h, src_d.data_ptr(), viewer_d.data_ptr(), dh52.data_ptr(), h.cnt.data_ptr(), G, la.data_ptr(),
                                             h.n_moves, script.data_ptr(), count.data_ptr(), env._stream()))
    # --- 2. against the plain-Python restatement
    state = env.export_state().cpu().numpy()
    dh, cnt, moves = h.dh.cpu().numpy(), h.cnt.cpu().numpy(), la.cpu().numpy()
    got_s, got_c = script.cpu().numpy(), count.cpu().numpy()
    for j in range(n):
        s, v = int(src[j]), int(viewer[j])
        if not 0 <= s < G:
            want = ([0] * 52, 0)
        else:
            hand = [int(state[j, 80 + (v * H + i) * 6]) for i in range(H)] if v >= 0 else []
            hand = [c for c in hand if c >= 0]
            want = W.world_script_ref(dh[s], int(cnt[s]), [int(moves[t, s, t % P]) for t in range(h.n_moves)], v, hand, P, H)
        assert (got_s[j].tolist(), int(got_c[j])) == want, "slot %d" % j
    assert got_c[5] == 0 and got_c[9] == 0 and got_c[13] == 0 and (np.delete(got_c, [5, 9, 13]) > 0).all()
    # --- 3. rewind + teacher-forced replay == fork + determinize
    want_env = forked_worlds(h, src, viewer, seeds, key)
    env.rewind_scripted(script, count)
    live_src = torch.where(count > 0, src_d, torch.full_like(src_d, -1))
    mismatch = torch.zeros(n, dtype=torch.int32, device=DEV)
    nothing = torch.zeros(n * P, dtype=torch.int64, device=DEV)
    expected_notes = 0
    for t in range(h.n_moves):
        done = env.query()[:, Q_TERM] == 1
        # finished and never started slots are handed the noop ("step on a finished game"), and so is slot 13, whose live game
        # has no script ("illegal move", the game untouched).  A logged greedy action that is no legal move in a world is
        # replaced by the kernel: no note
        expected_notes += int(done.sum()) + int((~done & (count <= 0)).sum())
        L.check(env.lib.hsad_search_replay_actions(env.h, live_src.data_ptr(), viewer_d.data_ptr(), la[t].data_ptr(), lg[t].data_ptr(), G,
                                                   nothing.data_ptr(), env.a.data_ptr(), env.greedy_a.data_ptr(), mismatch.data_ptr(),
                                                   env._stream()))
        env.step(env.a, env.greedy_a)
        env.observe_sad(live_src, h.log.sad[t])
    n_err, code = drain(env)
    assert n_err == expected_notes                                      # no illegal move in a replayed world, no refused script
    ok = torch.from_numpy(got_c > 0).to(DEV)
    assert torch.equal(state_but_draws(env)[ok], state_but_draws(want_env)[ok])
    assert same_rows({k: v[ok] for k, v in rows_of(env).items()}, {k: v[ok] for k, v in rows_of(want_env).items()},
                     names=("legal_move", "own_hand", "terminal")) == []
    # slot 13 (no viewer) stayed the plain fork, slot 5 was never started
    assert torch.equal(env.export_state()[13], want_env.export_state()[13]) and int(env.query()[5, 14]) == 0
    env.close()
    want_env.close()


def test_a_script_the_deck_cannot_deal_is_refused(hist):
    h = hist
    f = new_env(h, seed=31, track=False)
    f.fork_from(h.root, i32(np.arange(G)))
    before = f.export_state().clone()
    bad = torch.nn.functional.pad(h.dh, (0, 2)).clone()
    count = torch.full((G,), h.P * h.H, dtype=torch.int32, device=DEV)
    bad[0, 0:4] = 4                     # four copies of a rank-5 card
    bad[1, 1] = 25                      # no card type
    count[2] = h.P * h.H - 1            # not even the hands
    count[3] = 51
    count[4] = 0                        # left alone, no error
    f.rewind_scripted(bad, count)
    assert drain(f) == (4, 5)
    after = f.export_state()
    assert torch.equal(after[:5], before[:5])
    assert bool((after[5:, 60] == 0).all())          # the others were rewound: step 0
    f.close()


# ------------------------------------------------------------------------------------------------------------------
# 4 / 5. the replayed LSTM states and the mismatch count
# ------------------------------------------------------------------------------------------------------------------
def replay_with_agent(h, env, src, viewer):
    """teacher-forced replay of env's slots from zero state -> (h, c, mismatch, count of differing partner replies in torch)"""
    L, P = _lib(), h.P
    n = env.G
    hid = h.agent.get_h0(n * P)
    mismatch = torch.zeros(n, dtype=torch.int32, device=DEV)
    by_torch = torch.zeros(n, dtype=torch.int64, device=DEV)
    src_l, viewer_l = src.long().clamp(min=0), viewer.long()
    slot = torch.arange(n, device=DEV)
    for t in range(h.n_moves):
        reply, hid = h.agent.act(obs_of(env), hid)
        g = reply["greedy_a"].contiguous()
        live = (env.query()[:, Q_TERM] == 0) & (src >= 0)
        mover = t % P
        shown = h.log.greedy_a[t][src_l, mover]
        by_torch += (live & (viewer_l != mover) & (g.view(n, P)[slot, mover] != shown)).long()
        L.check(env.lib.hsad_search_replay_actions(env.h, src.data_ptr(), viewer.data_ptr(), h.log.a[t].data_ptr(), h.log.greedy_a[t].data_ptr(),
                                                   G, g.data_ptr(), env.a.data_ptr(), env.greedy_a.data_ptr(), mismatch.data_ptr(), env._stream()))
        env.step(env.a, env.greedy_a)
        env.observe_sad(src, h.log.sad[t])        # every seat is shown what the root's rows showed (a no-op with sad = 0)
    return hid["h0"], hid["c0"], mismatch, by_torch


def sampled_worlds(h):
    """the worlds PolicySearch samples (the player on turn views, finished root games are not searched), replayed once per history"""
    if getattr(h, "sampled", None) is not None:
        return h.sampled
    from hanabi_sad_amd.search import world_key, world_seed
    L, n = _lib(), G * WORLDS
    cur = h.q[:, Q_CUR].astype(np.int64)
    live = h.q[:, Q_TERM] == 0
    g_of = np.arange(n) // WORLDS
    w_of = np.arange(n) % WORLDS
    src = i32(np.where(live[g_of], g_of, -1))
    viewer = i32(np.where(live[g_of], cur[g_of], -1))
    seeds = i32([world_seed(SEED, int(a), int(b)) for a, b in zip(g_of, w_of)])
    key = torch.as_tensor(np.asarray([world_key(int(a), int(b)) for a, b in zip(g_of, w_of)], dtype=np.int64), device=DEV)
    env = new_env(h, n=n, seed=41, track=False)
    env.fork_from(h.root, src, seeds)
    env.determinize(viewer, key, SEED)
    dh52 = torch.nn.functional.pad(h.dh, (0, 2)).contiguous()
    script = torch.zeros(n, 52, dtype=torch.uint8, device=DEV)
    count = torch.zeros(n, dtype=torch.int32, device=DEV)
    L.check(env.lib.hsad_search_world_script(env.h, src.data_ptr(), viewer.data_ptr(), dh52.data_ptr(), h.cnt.data_ptr(), G,
                                             h.log.a.data_ptr() if h.n_moves else None, h.n_moves, script.data_ptr(), count.data_ptr(),
                                             env._stream()))
    env.rewind_scripted(script, count)
    hw, cw, mism, by_torch = replay_with_agent(h, env, src, viewer)
    n_err, code = drain(env)
    assert n_err == 0 or code == 3          # nothing but finished and never started slots
    h.sampled = (env, src, viewer, seeds, hw, cw, mism, by_torch, cur, live, torch.from_numpy(live[g_of]).to(DEV))
    return h.sampled


def test_the_searchers_own_rows_are_the_roots_in_every_world(hist):
    """Check 4 of the issue, sampled worlds: after the replay the h / c rows of the viewer's seat equal the rows the root carries.

    The searcher's observations do not depend on its own hand -- once the replay shows the greedy-action section as it was seen.
    With sad = 1 that section is computed from the true cards (the card of a greedy play or discard that was not the move made, the
    slots a partner's greedy hint would touch), so a replay that recomputed it from a world's resampled hand gave the viewer another
    observation in most worlds after 7 moves (12 of 20 and 4 of 4 with 2 players, 16 of 28 and 15 of 16 with 3, 7 of 8 on
    Hanabi-Small, measured on an MI355X before GameLog.sad / hsad_env_observe_sad existed)."""
    h = hist
    env, src, viewer, seeds, hw, cw, mism, by_torch, cur, live, ok = sampled_worlds(h)
    P, n = h.P, G * WORLDS
    slots = torch.arange(n, device=DEV)[ok]
    rows_w = slots * P + viewer.long()[ok]
    rows_r = src.long()[ok] * P + viewer.long()[ok]
    same_h = (hw[:, rows_w] == h.hid["h0"][:, rows_r]).all(dim=2).all(dim=0)
    same_c = (cw[:, rows_w] == h.hid["c0"][:, rows_r]).all(dim=2).all(dim=0)
    differ = int((~(same_h & same_c)).sum())
    print("worlds whose viewer rows differ from the root's: %d of %d" % (differ, len(slots)))
    assert differ == 0


def test_replayed_states_and_mismatch_counts(hist):
    from hanabi_sad_amd.search import PolicySearch
    h = hist
    env, src, viewer, seeds, hw, cw, mism, by_torch, cur, live, ok = sampled_worlds(h)
    P, n = h.P, G * WORLDS
    # --- 5. the kernel's count is the count of differing partner replies
    assert torch.equal(mism.long(), by_torch)
    print("mismatch per world:", mism.view(G, WORLDS).tolist())
    # --- the true world, forced with the unmodified history: every seat's state is the root's, nothing mismatches
    true_env = new_env(h, n=G, seed=43, track=False)
    idx = i32(np.where(live, np.arange(G), -1))
    true_env.fork_from(h.root, idx, i32(np.arange(G) + 1))
    true_env.rewind_scripted(h.dh, torch.where(idx >= 0, h.cnt, torch.zeros_like(h.cnt)))
    ht, ct, mt, bt = replay_with_agent(h, true_env, idx, i32(np.where(live, cur, -1)))
    rows = (torch.arange(G, device=DEV)[idx >= 0].unsqueeze(1) * P + torch.arange(P, device=DEV)).flatten()
    assert torch.equal(ht[:, rows], h.hid["h0"][:, rows]) and torch.equal(ct[:, rows], h.hid["c0"][:, rows])
    assert int(mt.abs().sum()) == 0 and int(bt.sum()) == 0
    # --- PolicySearch(replay=True) replays the same worlds: its mismatch table and its rebuilt states are these
    ps = PolicySearch(h.root, h.agent, capacity=64, replay=True)
    try:
        games = np.nonzero(live)[0]
        got = ps._replay(h.root, h.log, games, cur, WORLDS, SEED, seeds.cpu().numpy().reshape(G, WORLDS))
        assert torch.equal(got.view(len(games), WORLDS), mism.view(G, WORLDS)[torch.from_numpy(games).to(DEV)])
        k = len(games) * WORLDS
        assert k <= 64
        if k:       # (every root game may have ended)
            assert torch.equal(ps.worlds_env[0].h[:, :k * P], hw.view(hw.shape[0], n, P, -1)[:, ok].reshape(hw.shape[0], k * P, -1))
            assert torch.equal(ps.worlds_env[0].env.export_state()[:k], env.export_state()[ok])
    finally:
        ps.close()
    true_env.close()


# ------------------------------------------------------------------------------------------------------------------
# 5 / 6. the search on top: a loop over the existing primitives from the replayed worlds, consistent_only, capacity
# ------------------------------------------------------------------------------------------------------------------
def per_world_scores(h, seed):
    """every (game, legal action, world) job played out greedily from the replayed world, one job after the other in slots of a
    64-slot env, in REVERSED slot order, with torch indexing for the state rows -> ({(g, a, w): score}, mismatch [G, WORLDS])"""
    from hanabi_sad_amd.search import search_jobs, world_key, world_seed
    L, P, A = _lib(), h.P, h.root.A
    pairs, cur = search_jobs(h.root)
    n = G * WORLDS
    g_of, w_of = np.arange(n) // WORLDS, np.arange(n) % WORLDS
    live = h.q[:, Q_TERM] == 0
    src = i32(np.where(live[g_of], g_of, -1))
    viewer = i32(np.where(live[g_of], cur[g_of], -1))
    seeds_np = np.asarray([world_seed(seed, int(a), int(b)) for a, b in zip(g_of, w_of)], dtype=np.int32)
    key = torch.as_tensor(np.asarray([world_key(int(a), int(b)) for a, b in zip(g_of, w_of)], dtype=np.int64), device=DEV)
    wenv = new_env(h, n=n, seed=51, track=False)
    wenv.fork_from(h.root, src, i32(seeds_np))
    wenv.determinize(viewer, key, seed)
    dh52 = torch.nn.functional.pad(h.dh, (0, 2)).contiguous()
    script = torch.zeros(n, 52, dtype=torch.uint8, device=DEV)
    count = torch.zeros(n, dtype=torch.int32, device=DEV)
    L.check(wenv.lib.hsad_search_world_script(wenv.h, src.data_ptr(), viewer.data_ptr(), dh52.data_ptr(), h.cnt.data_ptr(), G,
                                              h.log.a.data_ptr() if h.n_moves else None, h.n_moves, script.data_ptr(), count.data_ptr(),
                                              wenv._stream()))
    wenv.rewind_scripted(script, count)
    hw, cw, mism, _ = replay_with_agent(h, wenv, src, viewer)
    drain(wenv)
    cap = 64
    senv = new_env(h, n=cap, seed=52, track=False)
    senv.reset()
    jobs = [(int(g), int(a), w) for g, a in pairs for w in range(WORLDS)]
    noop = torch.full((cap, P), A - 1, dtype=torch.int64, device=DEV)
    scores, blueprint = {}, {}
    for c0 in range(0, len(jobs), cap):
        chunk = jobs[c0:c0 + cap]
        slots = [cap - 1 - i for i in range(len(chunk))]
        idx, sd = np.full(cap, -1, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        for s, (g, a, w) in zip(slots, chunk):
            idx[s], sd[s] = g * WORLDS + w, seeds_np[g * WORLDS + w]
        senv.fork_from(wenv, i32(idx), i32(sd))
        dst_rows = torch.tensor([s * P + p for s in slots for p in range(P)], device=DEV)
        src_rows = torch.tensor([(g * WORLDS + w) * P + p for (g, a, w) in chunk for p in range(P)], device=DEV)
        hh, cc = torch.zeros(hw.shape[0], cap * P, hw.shape[2], device=DEV), torch.zeros(hw.shape[0], cap * P, hw.shape[2], device=DEV)
        hh[:, dst_rows], cc[:, dst_rows] = hw[:, src_rows], cw[:, src_rows]
        hd = {"h0": hh, "c0": cc}
        sl = torch.tensor(slots, device=DEV)
        for t in range(200):
            alive = senv.query()[:, Q_TERM] == 0
            if not bool(alive[sl].any()):
                break
            reply, hd = h.agent.act(obs_of(senv), hd)
            a_all, g_all = reply["a"].view(cap, P).clone(), reply["greedy_a"].view(cap, P)
            if t == 0:
                for s, (g, a, w) in zip(slots, chunk):
                    if w == 0:
                        blueprint.setdefault(g, int(g_all[s, cur[g]]))
                    a_all[s, cur[g]] = a
            senv.step(torch.where(alive.unsqueeze(1), a_all, noop).contiguous(), torch.where(alive.unsqueeze(1), g_all, noop).contiguous())
        else:
            raise AssertionError("the games of the loop did not finish")
        sc = senv.query()[:, 2].cpu().numpy()
        for s, job in zip(slots, chunk):
            scores[job] = int(sc[s])
    wenv.close()
    senv.close()
    return scores, blueprint, mism.view(G, WORLDS).cpu().numpy()


def totals_of(scores, keep, A):
    t = np.zeros((G, A, 3), dtype=np.int64)
    for (g, a, w), s in scores.items():
        if keep[g, w]:
            t[g, a] += (s, s * s, 1)
    return t


@pytest.fixture(scope="module", params=[("2p", 0, 0, 7), ("small", 1, 0, 3)], ids=["2p-sad0-n7", "small-sad1-n3"])
def searched(request):
    h = play_root(*request.param)
    yield h, per_world_scores(h, SEED)
    h.root.close()
    h.root0.close()


def test_replay_search_equals_the_loop_and_ignores_capacity(searched):
    from hanabi_sad_amd.search import policy_action_values
    h, (scores, blueprint, mism) = searched
    A = h.root.A
    before = [h.root.export_state().clone(), h.root.priv_s.clone(), h.hid["h0"].clone(), h.log.a.clone()]
    want = totals_of(scores, np.ones((G, WORLDS), dtype=bool), A)
    assert want[..., 2].sum() > 64                   # more than one chunk at capacity 64
    res = {}
    for cap in (64, 96):
        sv = res[cap] = policy_action_values(h.root, h.agent, h.hid, WORLDS, SEED, capacity=cap, replay=True, log=h.log)
        assert np.array_equal(sv.totals.cpu().numpy(), want), cap
        assert np.array_equal(sv.mismatch.cpu().numpy(), mism) and sv.mismatch.dtype == torch.int32, cap
        assert sv.blueprint_a.tolist() == [blueprint.get(g, -1) for g in range(G)], cap
    assert torch.equal(res[64].values.nan_to_num(-1.0), res[96].values.nan_to_num(-1.0))
    after = [h.root.export_state(), h.root.priv_s, h.hid["h0"], h.log.a]
    assert all(torch.equal(x, y) for x, y in zip(before, after))          # root, carried state and log were only read
    # without the replay the values are those of the carried-state search: another result on these roots, and no mismatch table
    plain = policy_action_values(h.root, h.agent, h.hid, WORLDS, SEED, capacity=64)
    assert plain.mismatch is None
    assert torch.equal(plain.totals[..., 2], res[64].totals[..., 2]) and torch.equal(plain.blueprint_a, res[64].blueprint_a)
    print("totals differ from the carried-state search:", not torch.equal(plain.totals, res[64].totals), "; mismatch", mism.tolist())
    with pytest.raises(ValueError):
        policy_action_values(h.root, h.agent, h.hid, WORLDS, SEED, capacity=64, replay=True)       # no log
    with pytest.raises(ValueError):
        policy_action_values(h.root, h.agent, h.hid, WORLDS, SEED, capacity=64, consistent_only=True)


def test_consistent_only_sums_the_worlds_the_mask_keeps(searched):
    from hanabi_sad_amd.search import policy_action_values
    h, (scores, blueprint, mism) = searched
    keep = mism == 0
    keep[~keep.any(axis=1)] = True                  # no consistent world: all of them
    want = totals_of(scores, keep, h.root.A)
    sv = policy_action_values(h.root, h.agent, h.hid, WORLDS, SEED, capacity=64, replay=True, log=h.log, consistent_only=True)
    assert np.array_equal(sv.totals.cpu().numpy(), want)
    assert np.array_equal(sv.mismatch.cpu().numpy(), mism)
    n = sv.totals[..., 2].cpu().numpy()
    legal = n > 0
    assert (n[legal] == np.broadcast_to(keep.sum(axis=1)[:, None], n.shape)[legal]).all()
    print("worlds kept per game:", keep.sum(axis=1).tolist())


# ------------------------------------------------------------------------------------------------------------------
# 6. replay off is the path that was there before
# ------------------------------------------------------------------------------------------------------------------
def test_replay_off_is_the_loop_over_the_old_primitives():
    from hanabi_sad_amd.search import PolicySearch, choose_action, move_seed, play_with_search
    from tests.test_policy_search_gpu import _agent, _make_root, _yardstick
    agent, P = _agent("bf16")
    root, hid = _make_root(agent, P, 5)
    values, totals, blueprint = _yardstick(root, agent, hid, 4, 21)
    ps = PolicySearch(root, agent, capacity=64, replay=False)
    sv = ps.search(root, hid, 4, 21)
    ps.close()
    assert np.array_equal(sv.totals.cpu().numpy(), totals) and np.array_equal(sv.blueprint_a.cpu().numpy(), blueprint)
    assert torch.equal(sv.values.nan_to_num(-1.0), torch.from_numpy(values).to(DEV).nan_to_num(-1.0)) and sv.mismatch is None
    root.close()
    # play_with_search(replay_history=False): its first move is what the old loop gives on the freshly reset root
    root0, hid0 = _make_root(agent, P, 0)
    v0, _, bp0 = _yardstick(root0, agent, hid0, 2, move_seed(3, 0))
    want = choose_action(torch.from_numpy(v0), torch.from_numpy(bp0), 0.05)
    root0.close()
    kw = dict(worlds=2, threshold=0.05, search_seed=3, capacity=64, device=DEV, max_steps=200)
    off = play_with_search(agent, 3, 17, 0, False, replay_history=False, **kw)
    assert torch.equal(off.trace[0][0], want) and torch.equal(off.trace[0][1], torch.from_numpy(bp0))
    same = play_with_search(agent, 3, 17, 0, False, **kw)
    assert off.scores == same.scores and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(off.trace, same.trace))


def test_play_with_search_with_replay_runs_and_repeats():
    from hanabi_sad_amd.eval import evaluate
    from hanabi_sad_amd.search import play_with_search
    from tests.test_policy_search_gpu import _agent
    agent, _ = _agent("bf16")
    kw = dict(worlds=2, search_seed=3, capacity=64, device=DEV, searcher=0, replay_history=True)
    _, _, scores, _ = evaluate(agent, 2, 11, 0, False, device=DEV)
    never = play_with_search(agent, 2, 11, 0, False, threshold=float("inf"), consistent_only=True, **kw)
    assert never.scores == scores and never.deviations.tolist() == [0, 0]
    one = play_with_search(agent, 2, 11, 0, False, threshold=0.05, **kw)
    two = play_with_search(agent, 2, 11, 0, False, threshold=0.05, **kw)
    assert one.scores == two.scores and all(torch.equal(a[0], b[0]) for a, b in zip(one.trace, two.trace))
    assert all(0 <= s <= 25 for s in one.scores)
    print("with replay:", one.scores, one.deviations.tolist())


# ------------------------------------------------------------------------------------------------------------------
# 7. envs without a script
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules,sad", [("2p", 0), ("3p", 1), ("small", 0)])
def test_an_env_without_a_script_steps_and_rolls_out_as_ever(rules, sad):
    h = Hist()
    h.rules, h.sad, h.sc = rules, sad, 0
    a_env, b_env, c_env, d_env = (new_env(h, seed=77) for _ in range(4))
    # rollout_random is reset + policy + step, 30 times
    a_env.reset()
    a_env.rollout_random(30, 9)
    d_env.reset()
    for _ in range(30):
        d_env.reset()
        d_env.step(*d_env.policy_random(9))
    assert torch.equal(a_env.export_state(), d_env.export_state()) and same_rows(rows_of(a_env), rows_of(d_env)) == []
    # an env that was handed a script for no game runs the scripted step and deals every card from its generator
    b_env.reset()
    c_env.reset()
    c_env.rewind_scripted(torch.zeros(G, 52, dtype=torch.uint8), torch.zeros(G, dtype=torch.int32))
    assert torch.equal(b_env.export_state(), c_env.export_state()) and same_rows(rows_of(b_env), rows_of(c_env)) == []
    for t in range(30):
        a, ga = b_env.policy_random(9)
        b_env.step(a, ga)
        c_env.step(a.clone(), ga.clone())
        assert torch.equal(b_env.export_state(), c_env.export_state()), "move %d" % t
        assert same_rows(rows_of(b_env), rows_of(c_env)) == [], "move %d" % t
    with pytest.raises(_lib().HsadError):
        c_env.rollout_random(1, 9)              # refused while the env holds a script
    c_env.reset()
    c_env.rollout_random(1, 9)                  # reset cleared it
    for e in (a_env, b_env, c_env, d_env):
        e.close()


def test_reset_after_a_script_returns_the_env_to_generator_deals(hist):
    h = hist
    f = new_env(h, seed=61)
    f.fork_from(h.root, i32(np.arange(G)), i32(np.arange(G) + 3000))
    f.rewind_scripted(h.dh, h.cnt)
    f.step(h.log.a[0].contiguous(), h.log.greedy_a[0].contiguous())
    f.reset()                                   # restarts what has ended already, and clears the script of every game
    ref = new_env(h, seed=62)
    ref.fork_from(f, i32(np.arange(G)))         # same state, same generator, never scripted
    for t in range(8):
        a, ga = ref.policy_random(5)
        a, ga = a.clone(), ga.clone()
        ref.step(a, ga)
        f.step(a, ga)
        assert torch.equal(f.export_state(), ref.export_state()), "move %d" % t
    if h.n_moves >= 7:                          # the script would have dealt the root's cards: the generator deals others
        dh, cnt = f.deck_history()
        m = torch.minimum(cnt, h.cnt)
        col = torch.arange(50, device=DEV).unsqueeze(0)
        span = (col >= h.P * h.H) & (col < m.unsqueeze(1))
        assert bool(span.any()) and bool(((dh != h.dh) & span).any())
    drain(f)
    f.close()
    ref.close()
