"""No GPU: the host side of the cross-play tournament (eval.play_seatings / cross_play, `python -m hanabi_sad_amd.eval_model`):
which rows of a tournament batch a model owns, the result table's layout against the reference's published table
(tests/golden/op_raw_data_sad.txt = the first table of models/op_raw_data.txt, recorded results), and the refusals, which must
come before any device is touched."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("P", [2, 3])
def test_row_lists_partition_the_batch_and_follow_the_seatings(P):
    from hanabi_sad_amd.eval import seating_rows
    rng = np.random.RandomState(5 + P)
    for K in range(1, 6):
        for trial in range(6):
            S, n = int(rng.randint(1, 8)), int(rng.randint(1, 7))
            seatings = rng.randint(0, K, size=(S, P))
            if trial == 0:
                seatings[0, :] = seatings[0, 0]          # one model on every seat of a seating
            rows = seating_rows(seatings, n, K)
            assert len(rows) == K
            allr = np.concatenate(rows)
            assert np.array_equal(np.sort(allr), np.arange(S * n * P))        # an exact partition
            for k, r in enumerate(rows):
                assert r.dtype == np.int32 and np.all(np.diff(r) > 0)          # fixed ascending order
                g, p = r // P, r % P
                assert np.all(seatings[g // n, p] == k)


def test_table_printer_reproduces_the_published_table():
    from hanabi_sad_amd.eval import format_cross_play_table, parse_cross_play_table
    text = open(os.path.join(GOLD, "op_raw_data_sad.txt")).read()
    want = text.rstrip("\n").split("\n")
    assert len(want) == 16                     # title, rule, header, dashes, twelve rows
    title, names, mean, row_mean = parse_cross_play_table(text)
    assert title == "self-play & cross-play of SAD" and names == ["M%d" % i for i in range(12)] and mean.shape == (12, 12)
    got = format_cross_play_table(title, names, mean).split("\n")
    assert got[:4] == want[:4]                 # title, rule, header, dashes: line for line
    assert len(got) == len(want)
    for g, w in zip(got[4:], want[4:]):
        assert g.split()[:-1] == w.split()[:-1] and g[:-6] == w[:-6]          # the name and the twelve score columns, verbatim
        assert abs(float(g.split()[-1]) - float(w.split()[-1])) <= 0.01 + 1e-9   # the file's means come from unrounded scores
    assert abs(mean[0].sum() - 78.6) < 1e-9 and abs(mean.mean(axis=1)[0] - 78.6 / 12) < 1e-12      # row mean includes the diagonal


def _weights(in_dim, out_dim=21, hid=16):
    from hanabi_sad_amd.selfplay import init_weights
    return init_weights(in_dim, hid, out_dim, 5, 0)


def test_env_dims_are_the_encoder_sizes():
    from hanabi_sad_amd.eval import env_dims
    assert env_dims(2, 5, False) == (783, 21) and env_dims(2, 5, True) == (838, 21)
    assert env_dims(5, 4, False)[1] == 2 * 4 + 4 * 10 + 1


def test_refusals_come_before_any_device_work(monkeypatch):
    from hanabi_sad_amd import eval as ev

    def no_device(*a, **k):
        raise AssertionError("a device object was created before the arguments were checked")
    monkeypatch.setattr(ev, "BatchedHanabiEnv", no_device)
    monkeypatch.setattr(ev, "_acting_agent", no_device)
    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    w838, w783 = _weights(838), _weights(783)
    for bad in ([0, 0], [[0]], [[0, 0], [0]], [[0] * 6]):                 # no [S, players] table with 2..5 players
        with pytest.raises(ValueError, match=r"seatings must be \[S, players\]"):
            ev.play_seatings([w838], bad, 4, 1, 0, True)
    with pytest.raises(ValueError, match="seating 1 seat 0 names model 2"):
        ev.play_seatings([w838, w838], [[0, 1], [2, 0]], 4, 1, 0, True)
    with pytest.raises(ValueError, match="seating 0 seat 1 names model -1"):
        ev.play_seatings([w838], [[0, -1]], 4, 1, 0, True)
    with pytest.raises(ValueError, match="model 1 has 783 inputs and 21 actions; the env of this game has 838 features"):
        ev.play_seatings([w838, w783], [[0, 1]], 4, 1, 0, True)
    with pytest.raises(ValueError, match="model 0 has 838 inputs"):
        ev.play_seatings([w838], [[0, 0]], 4, 1, 0, False)
    with pytest.raises(ValueError, match="model 0 has 838 inputs and 21 actions; the env of this game has 1138 features and 31 actions"):
        ev.play_seatings([w838], [[0, 0, 0]], 4, 1, 0, True)             # a 2-player model in a 3-player game: wrong width for it
    with pytest.raises(ValueError, match="model 0 has 783 inputs and 20 actions"):
        ev.play_seatings([_weights(783, 20)], [[0, 0]], 4, 1, 0, False)
    # cross_play builds [K^2, 2] seatings: a pool member of the wrong size is named the same way
    with pytest.raises(ValueError, match="model 1 has 783 inputs"):
        ev.cross_play([w838, w783], 4, 1, 0, True)
