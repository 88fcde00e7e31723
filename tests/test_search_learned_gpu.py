"""GPU: blueprint-policy search with sampler="learned" -- the worlds' hands drawn from a belief head's logits for the root act's
state (search.PolicySearch, belief.BeliefSampler, env.determinize_belief_worlds) -- on the small search root of
tests/search_fixtures.py with a random net, and on a played small root (tests/test_search_replay_gpu.play_root) for the replay
stage.  Everything is held to bit equalities; what the hands are is tests/test_env_belief_worlds_gpu.py's matter."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import belief_head_ref as R
from tests import determinize_ref as D
from tests import search_fixtures as SF

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S = SF.SEARCH_ROOT
WORLDS, SEED = S["worlds"], S["search_seed"]
Q_TERM, Q_CUR = 0, 1


def _same(x, y):
    x, y = torch.as_tensor(x), torch.as_tensor(y).to(x.device)
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                                      y.view(torch.int32) if y.dtype == torch.float32 else y)


def head_state(H, hand_size, seed=None, bias=None):
    """a head's state dict: zero (the exact belief), or seeded random weights; bias: {column: value}"""
    w, b = torch.zeros(25 * hand_size, H), torch.zeros(25 * hand_size)
    if seed is not None:
        gen = torch.Generator().manual_seed(seed)
        w, b = torch.randn(25 * hand_size, H, generator=gen) * 0.5, torch.randn(25 * hand_size, generator=gen) * 2.0
    for k, v in (bias or {}).items():
        b[k] = v
    return {"belief.weight": w, "belief.bias": b, "hand_size": hand_size, "H": H}


class Setup:
    pass


@pytest.fixture(scope="module")
def su():
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.search import policy_action_values
    from hanabi_sad_amd.selfplay import init_weights
    s = Setup()
    s.root = root = BatchedHanabiEnv(S["G"], seed=S["seed"], eps_list=SF.EPS, device=DEV, **SF.env_kwargs(S["config"], False, False, 0))
    root.rollout_random(S["iters"], S["pseed"])
    net = CNet(init_weights(root.F, 64, root.A, root.H, 1), DEV)
    s.agent = CompositeAgent(net, net, 1, 0.99)
    z = s.agent.get_h0(root.G * root.P)
    gen = torch.Generator().manual_seed(9)
    s.hid = {"h0": (torch.randn(z["h0"].shape, generator=gen) * 0.3).to(DEV), "c0": (torch.randn(z["c0"].shape, generator=gen) * 0.3).to(DEV)}
    s.head = head_state(64, root.H, seed=21)
    s.before = [root.export_state().clone(), root.priv_s.clone(), s.hid["h0"].clone(), s.hid["c0"].clone()]
    s.sv = policy_action_values(root, s.agent, s.hid, WORLDS, SEED, capacity=64, sampler="learned", belief=s.head)
    yield s
    root.close()


def test_learned_search_is_bit_identical_at_capacity_64_and_96_and_only_reads(su):
    from hanabi_sad_amd.belief import BeliefSampler
    from hanabi_sad_amd.search import policy_action_values
    sv = su.sv
    G, A = su.root.G, su.root.A
    for name, x, y in zip(("state", "priv_s", "h0", "c0"), su.before, [su.root.export_state(), su.root.priv_s, su.hid["h0"], su.hid["c0"]]):
        assert torch.equal(x, y), name
    q = su.root.query().cpu().numpy()
    live = q[:, Q_TERM] == 0
    assert live.sum() >= 2
    assert sv.belief_logp.shape == sv.belief_logp0.shape == (G, WORLDS) and sv.belief_logp.dtype == torch.float32
    lp = sv.belief_logp.cpu().numpy()
    assert np.isfinite(lp[live]).all() and (lp[live] <= 0).all() and np.isnan(lp[~live]).all()
    assert int(sv.totals[..., 2].sum()) > 96      # several chunks at either capacity, a short last one
    again = policy_action_values(su.root, su.agent, su.hid, WORLDS, SEED, capacity=96, sampler="learned", belief=BeliefSampler(su.head, DEV))
    for name in ("totals", "values", "sem", "blueprint_a", "belief_logp", "belief_logp0"):
        assert _same(getattr(again, name), getattr(sv, name)), name
    # the state after the root act, handed in: the same search
    N = G * su.root.P
    obs = {"priv_s": su.root.priv_s.view(N, su.root.F), "legal_move": su.root.legal_move.view(N, A), "eps": torch.zeros(N, device=DEV)}
    counter = su.agent.counter
    _, nxt = su.agent.act(obs, su.hid)
    su.agent.counter = counter
    given = policy_action_values(su.root, su.agent, su.hid, WORLDS, SEED, capacity=64, sampler="learned", belief=su.head, hid_next=nxt)
    assert _same(given.totals, sv.totals) and _same(given.belief_logp, sv.belief_logp)
    other = policy_action_values(su.root, su.agent, su.hid, WORLDS, SEED + 1, capacity=96, sampler="learned", belief=su.head)
    assert not _same(other.belief_logp, sv.belief_logp)


def test_belief_logp_is_single_valued_per_game_and_world(su, monkeypatch):
    """every slot that holds world w of game g -- one per action, in whatever chunk -- reports the same log-probabilities"""
    from hanabi_sad_amd import search
    seen = []
    inner = search._sample_hands

    def spy(env, sampler, viewer, key, seed, world, worlds, belief=None):
        got = inner(env, sampler, viewer, key, seed, world, worlds, belief)
        seen.append((belief[1].cpu().numpy(), world.cpu().numpy(), [t.cpu().numpy() for t in got]))
        return got
    monkeypatch.setattr(search, "_sample_hands", spy)
    sv = search.policy_action_values(su.root, su.agent, su.hid, WORLDS, SEED, capacity=64, sampler="learned", belief=su.head)
    table, slots = {}, 0
    for src, world, (status, logp, logp0) in seen:
        for j in range(len(src)):
            if src[j] < 0:
                assert status[j] == 0 and logp[j] == 0.0
                continue
            assert status[j] == 1
            table.setdefault((int(src[j]), int(world[j])), set()).add((logp[j].tobytes(), logp0[j].tobytes()))
            slots += 1
    assert len(seen) >= 2 and slots > len(table) and all(len(v) == 1 for v in table.values())
    lp, lp0 = sv.belief_logp.cpu().numpy(), sv.belief_logp0.cpu().numpy()
    for (g, w), v in table.items():
        assert (lp[g, w].tobytes(), lp0[g, w].tobytes()) in v


def forked_worlds(su, head, n_worlds=WORLDS):
    """the first live root game forked into n_worlds slots, determinised under `head` as the search does it -> (exported states,
    logp, logp0, the root game's row, the searcher)"""
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.belief import BeliefSampler
    root, agent = su.root, su.agent
    q = root.query().cpu().numpy()
    g0 = int(np.nonzero(q[:, Q_TERM] == 0)[0][0])
    p = int(q[g0, Q_CUR])
    N = root.G * root.P
    obs = {"priv_s": root.priv_s.view(N, root.F), "legal_move": root.legal_move.view(N, root.A), "eps": torch.zeros(N, device=DEV)}
    counter = agent.counter
    _, nxt = agent.act(obs, su.hid)
    agent.counter = counter
    logits = BeliefSampler(head, DEV).logits(nxt["h0"][-1].contiguous(), torch.from_numpy(q[:, Q_CUR].astype(np.int32)).to(DEV))
    env = BatchedHanabiEnv(n_worlds, seed=0, eps_list=(0.0,), device=DEV, track_deck_history=False, **root.config)
    env.fork_from(root, np.full(n_worlds, g0, np.int32))
    status, logp, logp0 = env.determinize_belief_worlds(np.full(n_worlds, p, np.int32), logits, np.full(n_worlds, g0, np.int32),
                                                        np.full(n_worlds, g0 << 32, np.int64), np.arange(n_worlds, dtype=np.int32), n_worlds, SEED)
    env.check_errors()
    assert bool((status == 1).all())
    st = env.export_state().cpu().numpy()
    env.close()
    return st, logp, logp0, root.export_state().cpu().numpy()[g0], g0, p


def test_a_zero_head_gives_equal_logp_bits_and_a_biased_head_moves_slot_0(su):
    from hanabi_sad_amd.search import policy_action_values
    from tests import hand_belief_ref as HB
    root = su.root
    zero = policy_action_values(root, su.agent, su.hid, WORLDS, SEED, capacity=64, sampler="learned", belief=head_state(64, root.H))
    assert _same(zero.belief_logp, zero.belief_logp0)
    live = ~torch.isnan(zero.belief_logp)
    assert bool(live.any())
    # the search's table is what the primitive gives on a fork of the root under the same head
    st, logp, logp0, row0, g0, p = forked_worlds(su, head_state(64, root.H))
    assert _same(zero.belief_logp[g0], logp) and _same(zero.belief_logp0[g0], logp0)
    st, logp, logp0, _, _, _ = forked_worlds(su, su.head)
    assert _same(su.sv.belief_logp[g0], logp) and _same(su.sv.belief_logp0[g0], logp0)
    # +30 on one type of slot 0: that type in slot 0 of every world -- it is feasible, being one the exact belief can draw
    pool, cms, hand = HB.pool_and_masks(row0, root.P, root.H, p)
    w0 = [t for t, w in enumerate(R.weights(list(pool), cms, 0)) if w]
    assert len(w0) >= 2
    first = D.HANDS + p * root.H * 6
    zero_slot0 = forked_worlds(su, head_state(64, root.H))[0][:, first]
    t = [x for x in w0 if x != np.bincount(zero_slot0, minlength=25).argmax()][0]      # not the type the exact belief draws most often
    pushed = head_state(64, root.H, bias={t: 30.0})
    st, logp, logp0, _, _, _ = forked_worlds(su, pushed)
    assert (st[:, first] == t).all(), (t, st[:, first])
    assert not (zero_slot0 == t).all()
    sv = policy_action_values(root, su.agent, su.hid, WORLDS, SEED, capacity=64, sampler="learned", belief=pushed)
    assert _same(sv.belief_logp[g0], logp) and not _same(sv.belief_logp, zero.belief_logp)
    assert not _same(sv.totals, zero.totals) or not _same(sv.values, zero.values), "the head has no effect on the values"


def test_other_samplers_and_no_worlds_are_untouched_by_the_new_arguments(su):
    from hanabi_sad_amd.search import PolicySearch, policy_action_values
    for sampler in ("rejection", "stratified"):
        old = policy_action_values(su.root, su.agent, su.hid, WORLDS, SEED, 64, 200, None, False, None, False, sampler)      # the call as it was
        ps = PolicySearch(su.root, su.agent, 64, sampler=sampler, belief=None)
        try:
            new = ps.search(su.root, su.hid, WORLDS, SEED, hid_next=None)
        finally:
            ps.close()
        for name in ("totals", "values", "sem", "blueprint_a"):
            assert _same(getattr(new, name), getattr(old, name)), (sampler, name)
        assert old.belief_logp is None and old.belief_logp0 is None and new.belief_logp is None
        assert not _same(old.totals, su.sv.totals)
        if sampler == "rejection":      # ... and what the loop over the primitives gives, which knows nothing of any sampler argument
            from tests.test_policy_search_gpu import _yardstick
            values, totals, blueprint = _yardstick(su.root, su.agent, su.hid, WORLDS, SEED)
            assert np.array_equal(old.totals.cpu().numpy(), totals) and np.array_equal(old.blueprint_a.cpu().numpy(), blueprint)
    none = policy_action_values(su.root, su.agent, su.hid, 0, SEED, capacity=64, sampler="learned", belief=su.head)
    plain = policy_action_values(su.root, su.agent, su.hid, 0, SEED, capacity=64)
    assert _same(none.totals, plain.totals) and _same(none.blueprint_a, plain.blueprint_a) and bool(torch.isnan(none.values).all())


def test_replay_holds_the_act_chunks_worlds_and_the_true_hand_world_never_mismatches():
    from hanabi_sad_amd.belief import BeliefSampler
    from hanabi_sad_amd.search import PolicySearch, policy_action_values, world_seed
    from tests import hand_belief_ref as HB
    from tests import test_search_replay_gpu as T
    h = T.play_root("small", 0, 0, 7)
    G, W, SD, P, H = T.G, T.WORLDS, T.SEED, h.P, h.H
    cur = h.q[:, T.Q_CUR].astype(np.int64)
    live = h.q[:, T.Q_TERM] == 0
    games = np.nonzero(live)[0]
    assert len(games) >= 2 and len(games) * W <= 64
    head = head_state(64, H, seed=33)
    flat = policy_action_values(h.root, h.agent, h.hid, W, SD, capacity=64, sampler="learned", belief=head)
    ps = PolicySearch(h.root, h.agent, capacity=64, replay=True, sampler="learned", belief=head)
    try:
        sv = ps.search(h.root, h.hid, W, SD, log=h.log)
        worlds_state = ps.worlds_env[0].env.export_state()[:len(games) * W].clone()
    finally:
        ps.close()
    # the same worlds as the act chunks of the search without replay: their log-probabilities, bit for bit
    assert _same(sv.belief_logp, flat.belief_logp) and _same(sv.belief_logp0, flat.belief_logp0)
    # ... and the cards of fork + determinize_belief_worlds under the logits of the root act's state
    N = G * P
    counter = h.agent.counter
    _, nxt = h.agent.act(T.obs_of(h.root), h.hid)
    h.agent.counter = counter
    logits = BeliefSampler(head, DEV).logits(nxt["h0"][-1].contiguous(), T.i32(cur))
    n = len(games) * W
    g_of, w_of = games[np.arange(n) // W], np.arange(n) % W
    want_env = T.new_env(h, n=n, seed=41, track=False)
    seeds = np.asarray([world_seed(SD, int(a), int(b)) for a, b in zip(g_of, w_of)], dtype=np.int32)
    want_env.fork_from(h.root, T.i32(g_of), T.i32(seeds))
    status, logp, _ = want_env.determinize_belief_worlds(T.i32(cur[g_of]), logits, T.i32(g_of), torch.from_numpy(g_of.astype(np.int64) << 32),
                                                         T.i32(w_of), W, SD)
    assert bool((status == 1).all())
    want = want_env.export_state().clone()
    worlds_state[:, T.W_DRAWS] = 0
    want[:, T.W_DRAWS] = 0
    assert torch.equal(worlds_state, want), "a replayed world does not hold the cards of fork + determinize_belief_worlds"
    assert _same(sv.belief_logp[torch.from_numpy(games).to(DEV)].view(-1), logp)
    want_env.close()
    # a head that puts +30 on the true cards of one game's searcher: every world of that game is the true world, and replays clean
    rows = h.root.export_state().cpu().numpy()
    g1 = int(games[0])
    pool, cms, hand = HB.pool_and_masks(rows[g1], P, H, int(cur[g1]))
    true_head = head_state(64, H, bias={i * 25 + c: 30.0 for i, c in enumerate(hand)})
    tv = policy_action_values(h.root, h.agent, h.hid, W, SD, capacity=64, replay=True, log=h.log, sampler="learned", belief=true_head)
    assert tv.mismatch[g1].tolist() == [0] * W, "the true hand's world mismatches"
    assert bool((tv.belief_logp[g1] > -1e-3).all())
    h.root.close()
    h.root0.close()


SMALL = dict(num_player=2, hand_size=2, colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1)


def test_play_with_search_learned_repeats_exactly_and_no_worlds_ignores_the_belief(su):
    from hanabi_sad_amd.search import play_with_search
    kw = dict(worlds=4, threshold=0.05, search_seed=3, capacity=128, device=DEV, sampler="learned", belief=su.head, **SMALL)
    one = play_with_search(su.agent, 3, 11, 0, False, **kw)
    two = play_with_search(su.agent, 3, 11, 0, False, **kw)
    assert one.scores == two.scores and torch.equal(one.deviations, two.deviations)
    assert len(one.trace) == len(two.trace) > 0 and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(one.trace, two.trace))
    none = play_with_search(su.agent, 3, 11, 0, False, **dict(kw, worlds=0))
    plain = play_with_search(su.agent, 3, 11, 0, False, worlds=0, device=DEV, **SMALL)
    assert none.scores == plain.scores and none.trace == [] and none.deviations.tolist() == [0, 0, 0]
    print("scores", one.scores, "deviations", one.deviations.tolist())


def test_eval_model_command_with_the_learned_sampler_runs_end_to_end(tmp_path):
    path = str(tmp_path / "belief.pthw")
    from hanabi_sad_amd.checkpoint import load_op_model
    zoo = os.path.join("tests", "golden", "op_zoo")
    agent = load_op_model("sad", 0, None, DEV, root=os.path.join(ROOT, zoo), precision="bf16")[0]
    torch.save(head_state(int(agent.online.H), 5, seed=4), path)
    cmd = [sys.executable, "-m", "hanabi_sad_amd.eval_model", "--paper", "op", "--method", "sad", "--root", zoo, "--num_game", "2", "--device", DEV,
           "--idx", "0", "--search_worlds", "2", "--search_sampler", "learned", "--search_belief", path]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)     # a fresh child process
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len([l for l in lines if re.match(r"blueprint: \S+ \+/- \S+ ; perfect:  \S+$", l)]) == 1
    found = [m for m in (re.match(r"blueprint \+ search \(2 worlds\): (\S+) \+/- (\S+) ; perfect:  (\S+) ; deviations per game: (\S+)$", l)
                         for l in lines) if m]
    assert len(found) == 1
    mean, sem, perfect, dev = (float(x) for x in found[0].groups())
    assert 0.0 <= mean <= 25.0 and sem >= 0.0 and 0.0 <= perfect <= 1.0 and dev >= 0.0
