"""CPU: the tensor code of blueprint-policy search (search.choose_action, search.SearchValues) on hand-made inputs."""
import numpy as np
import torch

NAN = float("nan")


def test_choose_action_ties_threshold_nan_and_passthrough():
    from hanabi_sad_amd.search import choose_action
    values = torch.tensor([
        [1.0, 3.0, 3.0, NAN],      # a tie of two better actions: the lowest uid
        [1.0, 1.5, NAN, NAN],      # a gain exactly equal to the threshold keeps the blueprint
        [1.0, 1.5, NAN, NAN],      # ... and the same gain from another blueprint does not (1.5 - 1.0 vs. blueprint 1)
        [2.0, NAN, NAN, 1.0],      # the blueprint is already the best
        [NAN, 0.0, NAN, 0.0],      # NaN never wins, whatever sits next to it
        [NAN, NAN, NAN, NAN],      # nothing searched
        [5.0, 9.0, NAN, NAN],      # -1 is passed through, whatever the row holds
        [1.0, 1.5625, NAN, NAN],   # a gain just above the threshold deviates
    ], dtype=torch.float32)
    blueprint = torch.tensor([0, 0, 1, 0, 3, -1, -1, 0], dtype=torch.int64)
    got = choose_action(values, blueprint, threshold=0.5)
    assert got.dtype == torch.int64
    assert got.tolist() == [1, 0, 1, 0, 3, -1, -1, 1]
    # an infinite threshold never deviates; a negative one deviates to an equally good action of lower uid
    assert choose_action(values, blueprint, threshold=float("inf")).tolist() == blueprint.tolist()
    assert choose_action(values, blueprint, threshold=-1.0).tolist() == [1, 1, 1, 0, 1, -1, -1, 1]
    # the default threshold
    assert choose_action(torch.tensor([[1.0, 1.04], [1.0, 1.06]]), torch.tensor([0, 0])).tolist() == [0, 1]


def test_search_values_statistics_from_integer_totals():
    from hanabi_sad_amd.search import SearchValues
    rng = np.random.default_rng(5)
    G, A = 3, 6
    totals = np.zeros((G, A, 3), dtype=np.int64)
    scores = {}
    for g in range(G):
        for a in range(A):
            n = int(rng.integers(0, 9))              # made-up per-world scores, 0 worlds included
            if (g, a) == (0, 0):
                n = 0
            if (g, a) == (1, 1):
                n = 1
            sc = rng.integers(0, 26, size=n).astype(np.int64)
            scores[g, a] = sc
            totals[g, a] = (sc.sum(), (sc * sc).sum(), n)
    sv = SearchValues(torch.from_numpy(totals), torch.tensor([2, -1, 0]))
    assert sv.values.dtype == torch.float32 and sv.sem.dtype == torch.float32 and sv.totals.dtype == torch.int64
    assert sv.values.shape == (G, A) and sv.sem.shape == (G, A) and sv.blueprint_a.tolist() == [2, -1, 0]
    for (g, a), sc in scores.items():
        v, s = float(sv.values[g, a]), float(sv.sem[g, a])
        if len(sc) == 0:
            assert np.isnan(v) and np.isnan(s)
            continue
        # the mean is ONE float32 division of the exact integer sum; the sem is float64 arithmetic rounded to float32
        assert v == float(np.float32(sc.sum()) / np.float32(len(sc)))
        assert abs(v - sc.mean()) <= 25 * 2.0 ** -23
        assert abs(s - np.std(sc) / np.sqrt(len(sc))) <= 25 * 2.0 ** -22
    assert float(sv.sem[1, 1]) == 0.0


def test_move_seed_and_world_seed_are_functions_of_their_arguments():
    from hanabi_sad_amd.search import move_seed
    seeds = {move_seed(s, t) for s in (0, 1, 7) for t in range(50)}
    assert len(seeds) == 150 and all(0 <= x < 2 ** 63 for x in seeds)
    assert move_seed(3, 4) == move_seed(3, 4)
