"""GPU: the search in rounds -- hsad_search_world_scores, hsad_search_round (csrc/hsad_search.hip) and PolicySearch.search(rounds=...),
play_with_search(rounds=...), eval_model --search_rounds.

The kernels are held to numpy on query() and to the Python-int restatement of tests/search_round_ref.py, bit for bit.  The search is
held to the FLAT search: a (game, action, world) job is the same job wherever and whenever it runs, so the table of per-world scores
of a one-round search reproduces the flat totals, and a search in rounds (2, 2, 4) must show exactly what the reference's round loop
uncovers of that table.  Every act call has fewer than 1,024 rows (one acting regime).

PRUNE_Z: the largest of {2, 1, 0.5, 0} at which the reference, replayed over the flat tables, drops at least one action in every
fixture -- decided by the flat tables, asserted below (the figures stand at PRUNE_Z)."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import search_round_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
Q_TERM, Q_SCORE, Q_STARTED = 0, 2, 14
INVALID = -1            # HSAD_ERR_INVALID
WORLDS, ROUNDS, SEED = 8, (2, 2, 4), 21
# PRUNE_Z = 2 already drops an action in every fixture.  What the reference's round loop gave over the flat tables of an MI355X run
# (worlds = 8, rounds (2, 2, 4); actions dropped, jobs per round / jobs of the flat search):
#   bf16 and fp32 zoo agent, rejection   13 of 34 dropped   jobs  68 + 52 + 104 of 272      (z = 1: 20 dropped, 68 + 30 + 56)
#   bf16 and fp32 zoo agent, stratified  17 of 34           jobs  68 + 50 +  76 of 272
#   3 players, rejection                 45 of 60           jobs 120 + 92 + 124 of 480      (scores 0..1: most differences are exact)
#   3 players, stratified                46 of 60           jobs 120 + 86 + 116 of 480
#   Hanabi-Small, sad = 1, replay, consistent_only   6 of 17   jobs 34 + 30 + 60 of 136     (the same at z = 1, 0.5 and 0)
PRUNE_Z = 2.0
Z2 = Fraction(PRUNE_Z * PRUNE_Z).limit_denominator(1024)


# ------------------------------------------------------------------------------------------------------------------
# 1. hsad_search_world_scores against numpy on query()
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_env():
    """96 games: 80 forked from an env in the middle of random play (some of them finished), 16 never started"""
    from hanabi_sad_amd import BatchedHanabiEnv
    kw = dict(players=2, bomb=0, eps_list=[0.0], max_len=-1, sad=True, device=DEV, track_deck_history=False)
    played = BatchedHanabiEnv(96, seed=3, **kw)
    played.reset()
    for it in range(200):
        done = played.query()[:, Q_TERM] == 1
        if int(done.sum()) >= 24:
            break
        a, g = played.policy_random(1234)
        noop = torch.full_like(a, played.A - 1)
        played.step(torch.where(done.unsqueeze(1), noop, a).contiguous(), torch.where(done.unsqueeze(1), noop, g).contiguous())
    env = BatchedHanabiEnv(96, seed=5, **kw)
    idx = torch.arange(96, dtype=torch.int32)
    idx[80:] = -1
    env.fork_from(played, idx)
    q = env.query().cpu().numpy()
    played.close()
    yield env, q
    env.close()


def test_world_scores_against_numpy_on_query(mixed_env):
    from hanabi_sad_amd import _lib
    env, q = mixed_env
    lib, st = env.lib, env._stream()
    G, n_pair, worlds = env.G, 9, 13
    started, term = q[:, Q_STARTED] == 1, q[:, Q_TERM] == 1
    finished = started & term
    assert finished.sum() >= 16 and (started & ~term).sum() >= 8 and (~started).sum() == 16
    score = q[:, Q_SCORE].astype(np.int64)
    assert score[finished].max() > 0 and score.max() <= 25
    # every (pair, world) at most once: a random injection of the slots into the table, then the cases that store nothing
    rng = np.random.default_rng(5)
    cell = rng.permutation(n_pair * worlds)[:G]
    pair, world = (cell // worlds).astype(np.int32), (cell % worlds).astype(np.int32)
    fin = np.nonzero(finished)[0]
    pair[fin[0]], pair[fin[1]], world[fin[2]], world[fin[3]] = -1, n_pair, worlds, -1        # finished games that name no entry
    first = np.arange(G) % 2 == 0                   # the first call takes the even slots, the second the odd ones
    table = torch.full((n_pair, worlds), 0xFF, dtype=torch.uint8, device=DEV)
    guard = torch.full((n_pair * worlds + 64,), 0xFF, dtype=torch.uint8, device=DEV)       # the table inside a larger buffer: nothing lands outside
    want = np.full((n_pair, worlds), 0xFF, dtype=np.uint8)
    for k, mask in enumerate((first, ~first)):
        pd = torch.from_numpy(np.where(mask, pair, -1).astype(np.int32)).to(DEV)
        wd = torch.from_numpy(world).to(DEV)
        _lib.check(lib.hsad_search_world_scores(env.h, pd.data_ptr(), wd.data_ptr(), n_pair, worlds, table.data_ptr(), st))
        _lib.check(lib.hsad_search_world_scores(env.h, pd.data_ptr(), wd.data_ptr(), n_pair, worlds, guard[32:].data_ptr(), st))
        stored = 0
        for g in range(G):
            if mask[g] and finished[g] and 0 <= pair[g] < n_pair and 0 <= world[g] < worlds:
                want[pair[g], world[g]] = score[g]
                stored += 1
        assert stored >= 4
        assert np.array_equal(table.cpu().numpy(), want), k        # the second call only adds entries
    got = guard.cpu().numpy()
    assert (got[:32] == 0xFF).all() and (got[32 + n_pair * worlds:] == 0xFF).all() and np.array_equal(got[32:32 + n_pair * worlds].reshape(n_pair, worlds), want)
    assert (want != 0xFF).sum() == (finished & (pair >= 0) & (pair < n_pair) & (world >= 0) & (world < worlds)).sum() < finished.sum()
    assert lib.hsad_search_world_scores(env.h, pd.data_ptr(), wd.data_ptr(), 0, worlds, table.data_ptr(), st) == INVALID
    assert lib.hsad_search_world_scores(env.h, pd.data_ptr(), wd.data_ptr(), n_pair, 0, table.data_ptr(), st) == INVALID
    assert lib.hsad_search_world_scores(env.h, None, wd.data_ptr(), n_pair, worlds, table.data_ptr(), st) == INVALID


# ------------------------------------------------------------------------------------------------------------------
# 2. hsad_search_round against the Python-int reference
# ------------------------------------------------------------------------------------------------------------------
def _round(lib, t, num, den, min_n=2, worlds=None):
    scores = torch.tensor(t["scores"], dtype=torch.uint8, device=DEV).contiguous()
    n_pair, w = scores.shape
    first = torch.tensor(t["first_pair"], dtype=torch.int32, device=DEV)
    bp = torch.tensor(t["bp_pair"], dtype=torch.int32, device=DEV)
    n_game = len(t["bp_pair"])
    out = dict(alive=torch.tensor(t["alive"], dtype=torch.uint8, device=DEV), leader=torch.full((n_game,), -7, dtype=torch.int32, device=DEV),
               raw=torch.full((n_pair, 2), -7, dtype=torch.int64, device=DEV), paired_ref=torch.full((n_pair, 3), -7, dtype=torch.int64, device=DEV),
               paired_bp=torch.full((n_pair, 3), -7, dtype=torch.int64, device=DEV))
    rc = lib.hsad_search_round(scores.data_ptr(), n_pair, w if worlds is None else worlds, first.data_ptr(), n_game, bp.data_ptr(), num, den, min_n,
                               out["alive"].data_ptr(), out["leader"].data_ptr(), out["raw"].data_ptr(), out["paired_ref"].data_ptr(),
                               out["paired_bp"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    return rc, {k: v.cpu().tolist() for k, v in out.items()}, scores


@pytest.mark.parametrize("worlds", R.WORLD_COUNTS)
def test_round_kernel_equals_the_reference_to_the_bit(worlds):
    from hanabi_sad_amd import _lib
    lib = _lib.load_library()
    t = R.synthetic_table(worlds)
    for num, den in ((0, 1), (1, 1), (4, 1)):
        want = R.search_round_ref(t["scores"], t["first_pair"], t["bp_pair"], num, den, 2, t["alive"])
        rc, got, scores = _round(lib, t, num, den)
        _lib.check(rc)
        for name in ("leader", "raw", "paired_ref", "paired_bp", "alive"):
            assert got[name] == want[name], (name, num, den)
        assert scores.cpu().tolist() == t["scores"]                # the table is only read
        again = _round(lib, t, num, den)[1]
        assert again == got
    # a second round on the survivors: what was pruned stays out of the leader's choice and is never revived
    t2 = dict(t, alive=want["alive"])
    want2 = R.search_round_ref(t["scores"], t["first_pair"], t["bp_pair"], 1, 4, 1, t2["alive"])
    rc, got2, _ = _round(lib, t2, 1, 4, min_n=1)
    _lib.check(rc)
    assert got2 == want2 and all(a <= b for a, b in zip(got2["alive"], t2["alive"]))


def test_round_kernel_refuses_what_leaves_int64():
    from hanabi_sad_amd import _lib
    lib = _lib.load_library()
    t = R.synthetic_table(5)
    ok = dict(num=4, den=1, min_n=2, worlds=None)
    for bad in (dict(num=16385), dict(num=-1), dict(den=0), dict(den=1025), dict(min_n=0), dict(worlds=0), dict(worlds=4097)):
        rc, got, _ = _round(lib, t, **dict(ok, **bad))
        assert rc == INVALID, bad
        assert got["alive"] == t["alive"] and set(got["leader"]) == {-7}           # refused before anything ran
    rc, _, _ = _round(lib, t, 16384, 1024, min_n=1)
    _lib.check(rc)
    # the largest table: 4,096 worlds of the extreme difference, at the largest z^2 -- D^2 n z2_den just under 2^56, exact
    wide = dict(scores=[[25] * 4096, [0] * 4096, [0] * 4095 + [1]], first_pair=[0, 3], bp_pair=[0], alive=[1, 1, 1])
    for num, den in ((16384, 1024), (16384, 1), (0, 1024)):
        rc, got, _ = _round(lib, wide, num, den)
        _lib.check(rc)
        assert got == R.search_round_ref(wide["scores"], [0, 3], [0], num, den, 2, [1, 1, 1]), (num, den)
    assert got["paired_ref"][1] == [-25 * 4096, 625 * 4096, 4096]


# ------------------------------------------------------------------------------------------------------------------
# 3. the search in rounds against the flat search
# ------------------------------------------------------------------------------------------------------------------
def _pairs_of(root, sv):
    """the searched pairs in (game, action) order, the first pair of each game (+ the end) and the blueprint's pair per game"""
    from hanabi_sad_amd.search import search_jobs
    pairs, _ = search_jobs(root)
    games, first = np.unique(pairs[:, 0], return_index=True)
    bp = sv.blueprint_a.cpu().numpy()
    index = {(int(g), int(a)): i for i, (g, a) in enumerate(pairs)}
    return pairs, [int(f) for f in first] + [len(pairs)], [index[(int(g), int(bp[g]))] for g in games]


def _same(x, y):
    x, y = torch.as_tensor(x), torch.as_tensor(y).to(x.device)
    return x.dtype == y.dtype and torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0))


def check_rounds_against_flat(root, flat, one, sv, label):
    """flat: rounds=None; one: rounds=(WORLDS,); sv: rounds=ROUNDS, all of the same search otherwise"""
    G, A = root.G, root.A
    # one round of all worlds IS the flat search, and its table sums to the flat totals
    assert torch.equal(one.totals, flat.totals) and _same(one.values, flat.values) and torch.equal(one.blueprint_a, flat.blueprint_a), label
    assert flat.paired is None and flat.world_scores is None and flat.pruned_round is None and flat.paired_mean is None
    ws = one.world_scores
    assert ws.dtype == torch.uint8 and tuple(ws.shape) == (G, A, WORLDS)
    present = ws != 0xFF
    s = torch.where(present, ws.long(), torch.zeros_like(ws, dtype=torch.int64))
    assert torch.equal(torch.stack([s.sum(2), (s * s).sum(2), present.long().sum(2)], dim=2), flat.totals), label
    # the reference's round loop over that table
    pairs, first, bp_pair = _pairs_of(root, flat)
    table = ws.cpu().numpy()[pairs[:, 0], pairs[:, 1]]
    want = R.rounds_ref(table.tolist(), first, bp_pair, ROUNDS, Z2.numerator, Z2.denominator, 2)
    dropped = sum(r >= 0 for r in want["pruned_round"])
    print("%s: %d pairs, jobs per round %s of %d flat, %d dropped (rounds %s)" % (label, len(pairs), want["jobs"], len(pairs) * WORLDS, dropped,
                                                                                  sorted(set(want["pruned_round"]))))
    assert dropped >= 1 and sum(want["jobs"]) < len(pairs) * WORLDS, label
    played = np.full((G, A, WORLDS), 0xFF, dtype=np.uint8)
    pruned = np.full((G, A), -1, dtype=np.int32)
    paired = np.zeros((G, A, 3), dtype=np.int64)
    played[pairs[:, 0], pairs[:, 1]] = np.asarray(want["played"], dtype=np.uint8)
    pruned[pairs[:, 0], pairs[:, 1]] = want["pruned_round"]
    paired[pairs[:, 0], pairs[:, 1]] = want["paired_bp"]
    got = sv.world_scores.cpu().numpy()
    assert ((got == 0xFF) | (got == ws.cpu().numpy())).all(), label          # every played (g, a, w) has the score of the flat table
    assert np.array_equal(got, played), label                                 # and exactly the expected entries were played
    assert sv.pruned_round.dtype == torch.int32 and np.array_equal(sv.pruned_round.cpu().numpy(), pruned), label
    assert sv.paired.dtype == torch.int64 and np.array_equal(sv.paired.cpu().numpy(), paired), label
    assert torch.equal(sv.blueprint_a, flat.blueprint_a)
    p = torch.from_numpy(played).to(DEV)
    s = torch.where(p != 0xFF, p.long(), torch.zeros_like(p, dtype=torch.int64))
    assert torch.equal(sv.totals, torch.stack([s.sum(2), (s * s).sum(2), (p != 0xFF).long().sum(2)], dim=2)), label
    n = sv.paired[..., 2]
    assert sv.paired_mean.dtype == torch.float32 and torch.equal(torch.isnan(sv.paired_mean), n == 0)
    assert _same(sv.paired_mean, torch.where(n > 0, sv.paired[..., 0].float() / n.clamp(min=1).float(), torch.full_like(sv.values, float("nan"))))
    return want


@pytest.fixture(scope="module", params=["bf16", "fp32", "3p"])
def searched(request):
    from hanabi_sad_amd.search import policy_action_values
    from tests.test_policy_search_gpu import _agent, _make_root
    agent, P = _agent(request.param)
    root, hid = _make_root(agent, P, 5 if P == 2 else 4)
    flat = {s: policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64, sampler=s) for s in ("rejection", "stratified")}
    yield request.param, agent, root, hid, flat
    root.close()


@pytest.mark.parametrize("sampler", ["rejection", "stratified"])
def test_rounds_play_what_the_reference_uncovers_of_the_flat_table(searched, sampler):
    from hanabi_sad_amd.search import PolicySearch, choose_action_paired, policy_action_values
    kind, agent, root, hid, flat = searched
    before = [root.export_state().clone(), hid["h0"].clone()]
    kw = dict(sampler=sampler, prune_z=PRUNE_Z)
    one = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64, rounds=(WORLDS,), **kw)
    ps = PolicySearch(root, agent, 64, sampler=sampler)
    sv = ps.search(root, hid, WORLDS, SEED, rounds=ROUNDS, prune_z=PRUNE_Z)
    jobs = list(ps.round_jobs)
    ps.close()
    want = check_rounds_against_flat(root, flat[sampler], one, sv, "%s %s" % (kind, sampler))
    assert jobs == want["jobs"]
    assert torch.equal(root.export_state(), before[0]) and torch.equal(hid["h0"], before[1])
    if sampler == "rejection":          # capacity: another chunking of the same jobs
        wide = policy_action_values(root, agent, hid, WORLDS, SEED, capacity=96, rounds=ROUNDS, **kw)
        for name in ("totals", "paired", "pruned_round", "world_scores", "blueprint_a"):
            assert torch.equal(getattr(wide, name), getattr(sv, name)), name
        assert _same(wide.paired_sem, sv.paired_sem) and _same(wide.values, sv.values)
    # the choice: never a dropped action, and the blueprint's where nothing gains
    chosen = choose_action_paired(sv, 0.05)
    g = torch.arange(root.G, device=DEV)
    assert bool((sv.pruned_round[g, chosen] < 0).all()) and torch.equal(choose_action_paired(sv, float("inf")), sv.blueprint_a)
    with pytest.raises(ValueError):
        policy_action_values(root, agent, hid, WORLDS, SEED, capacity=64, rounds=(2, 2))


def test_rounds_with_replay_and_consistent_only_on_a_sad_root():
    from hanabi_sad_amd.search import policy_action_values
    from tests.test_search_replay_gpu import play_root
    h = play_root("small", 1, 0, 3)
    kw = dict(capacity=64, replay=True, log=h.log, consistent_only=True, prune_z=PRUNE_Z)
    flat = policy_action_values(h.root, h.agent, h.hid, WORLDS, SEED, **kw)
    one = policy_action_values(h.root, h.agent, h.hid, WORLDS, SEED, rounds=(WORLDS,), **kw)
    sv = policy_action_values(h.root, h.agent, h.hid, WORLDS, SEED, rounds=ROUNDS, **kw)
    check_rounds_against_flat(h.root, flat, one, sv, "small sad=1 replay consistent_only")
    assert torch.equal(sv.mismatch, flat.mismatch)
    # a world the mask leaves out is absent for every action of its game
    keep = flat.mismatch == 0
    keep = torch.where(keep.any(dim=1, keepdim=True), keep, torch.ones_like(keep))
    legal = flat.totals[..., 2] > 0
    assert torch.equal(one.world_scores != 0xFF, legal.unsqueeze(2) & keep.unsqueeze(1))
    print("worlds kept per game:", keep.sum(1).tolist())
    h.root.close()
    h.root0.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. play_with_search and the command
# ------------------------------------------------------------------------------------------------------------------
def test_play_with_search_in_rounds_repeats_and_never_deviating_is_evaluate():
    from hanabi_sad_amd.eval import evaluate
    from hanabi_sad_amd.search import play_with_search
    from tests.test_policy_search_gpu import _agent
    agent, _ = _agent("bf16")
    kw = dict(worlds=4, rounds=(2, 2), prune_z=1.0, search_seed=3, capacity=128, device=DEV)
    one = play_with_search(agent, 3, 11, 0, False, threshold=0.05, **kw)
    two = play_with_search(agent, 3, 11, 0, False, threshold=0.05, **kw)
    assert one.scores == two.scores and torch.equal(one.deviations, two.deviations)
    assert len(one.trace) == len(two.trace) and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(one.trace, two.trace))
    assert all(0 <= s <= 25 for s in one.scores)
    assert torch.equal(one.deviations, sum(((ch >= 0) & (ch != bp)).long() for ch, bp in one.trace))
    _, _, scores, _ = evaluate(agent, 3, 11, 0, False, device=DEV)
    never = play_with_search(agent, 3, 11, 0, False, threshold=float("inf"), **kw)
    assert never.scores == scores and never.deviations.tolist() == [0, 0, 0] and all(torch.equal(ch, bp) for ch, bp in never.trace)
    print("scores", one.scores, "deviations", one.deviations.tolist())
    with pytest.raises(ValueError):
        play_with_search(agent, 3, 11, 0, False, worlds=4, rounds=(3, 2), device=DEV)


def test_eval_model_command_with_search_rounds_prints_its_two_lines():
    cmd = [sys.executable, "-m", "hanabi_sad_amd.eval_model", "--paper", "op", "--method", "sad", "--root", os.path.join("tests", "golden", "op_zoo"),
           "--num_game", "2", "--device", DEV, "--idx", "0", "--search_worlds", "4", "--search_rounds", "2,2", "--search_prune_z", "1.0",
           "--search_deviate_z", "0"]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)     # a fresh child process
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len([l for l in lines if re.match(r"blueprint: \S+ \+/- \S+ ; perfect:  \S+$", l)]) == 1
    found = [m for m in (re.match(r"blueprint \+ search \(4 worlds\): (\S+) \+/- (\S+) ; perfect:  (\S+) ; deviations per game: (\S+)$", l)
                         for l in lines) if m]
    assert len(found) == 1
    mean, sem, perfect, dev = (float(x) for x in found[0].groups())
    assert 0.0 <= mean <= 25.0 and sem >= 0.0 and 0.0 <= perfect <= 1.0 and dev >= 0.0
