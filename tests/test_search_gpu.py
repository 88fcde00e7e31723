"""GPU: hanabi_sad_amd.search.mc_action_values equals the loop over fork / determinize / step / playout it is built from, does not
depend on how its jobs are chunked, repeats exactly, and marks illegal actions and finished roots with NaN."""
import numpy as np
import pytest
import torch

from tests import search_fixtures as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def root():
    from hanabi_sad_amd import BatchedHanabiEnv
    s = SF.SEARCH_ROOT
    env = BatchedHanabiEnv(s["G"], seed=s["seed"], eps_list=SF.EPS, device=DEV, **SF.env_kwargs(s["config"], False, False, 0))
    env.rollout_random(s["iters"], s["pseed"])
    return env


@pytest.fixture(scope="module")
def values(root):
    from hanabi_sad_amd.search import mc_action_values
    s = SF.SEARCH_ROOT
    before = root.export_state()
    out = {cap: mc_action_values(root, s["worlds"], s["search_seed"], capacity=cap) for cap in (64, 96, 4096)}
    assert torch.equal(root.export_state(), before), "the search changed its root"
    return out


def _same(a, b):
    return a.dtype == b.dtype == torch.float32 and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_values_do_not_depend_on_the_chunking_and_repeat(root, values):
    from hanabi_sad_amd.search import mc_action_values
    s = SF.SEARCH_ROOT
    assert values[64].shape == (root.G, root.A)
    assert _same(values[64], values[96]) and _same(values[64], values[4096])
    assert _same(values[96], mc_action_values(root, s["worlds"], s["search_seed"], capacity=96))
    other = mc_action_values(root, s["worlds"], s["search_seed"] + 1, capacity=96)
    assert not _same(values[96], other), "the seed has no effect"


def test_nan_exactly_at_illegal_actions_and_finished_roots(root, values):
    from hanabi_sad_amd.search import mc_greedy_action
    q = root.query().cpu().numpy()
    legal = root.legal_move.cpu().numpy()
    live = (q[:, 14] == 1) & (q[:, 0] == 0)
    assert live.sum() >= 2 and (~live).any()
    want = np.stack([(legal[g, q[g, 1]] != 0) & live[g] for g in range(root.G)])
    v = values[4096].cpu().numpy()
    assert np.array_equal(~np.isnan(v), want)
    best = mc_greedy_action(values[4096]).cpu().numpy()
    for g in range(root.G):
        assert best[g] == (int(np.nanargmax(v[g])) if live[g] else -1)
    assert (v[~np.isnan(v)] >= 0).all() and (v[~np.isnan(v)] <= 10).all()


def test_values_equal_the_loop_over_the_primitives(root, values):
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.search import world_key, world_seed
    s = SF.SEARCH_ROOT
    one = BatchedHanabiEnv(1, seed=0, eps_list=(0.0,), device=DEV, track_deck_history=False, **root.config)
    q = root.query().cpu().numpy()
    legal = root.legal_move.cpu().numpy()
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
                one.playout_random(80, s["search_seed"], key=[world_key(g, w)])
                qq = one.query()[0].cpu().numpy()
                assert qq[0] == 1
                total += int(qq[2])
            want[g, a] = np.float32(total) / np.float32(s["worlds"])
    one.check_errors()
    assert _same(values[64], torch.from_numpy(want).to(DEV))
