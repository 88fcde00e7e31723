"""The surface of soft-target cloning without a device, after tests/test_clone_value_surface_cpu.py: the two entry points are declared in
include/hsad.h, exported by the library and bound in _lib.py with the argument lists the header gives; CompositeLearner.clone_loss calls
the new entry point only for a batch with a "target" key and refuses one of the wrong shape before any library call; soft_targets,
search_targets and check_targets refuse a bad temperature and targets of the wrong shape or count; CloneDataset carries `target` through
take / split / batches (CPU tensors); the command line refuses a bad temperature before any device work; play_with_search and SearchPlay
have the new optional arguments with defaults that change nothing."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from hanabi_sad_amd import clone
from tests.test_abi_and_host import ROOT, header_functions
from tests.test_clone_value_surface_cpu import declared_arguments, fake_batch, fake_dataset, fake_learner

NEW = ("hsad_clone_soft_tail", "hsad_r2d2_clone_soft_fwd")


def test_both_symbols_are_declared_exported_and_bound(hsad_lib):
    from hanabi_sad_amd import _lib
    declared = header_functions()
    ctype_kind = {C.c_void_p: "ptr", C.c_int: "int", C.c_float: "float"}
    for name in NEW:
        assert name in declared and hasattr(hsad_lib, name) and name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        assert [ctype_kind[a] for a in argtypes] == declared_arguments(name), name
    # one pointer more than the entry points they extend, which keep their argument lists
    assert len(_lib.SIGNATURES["hsad_clone_soft_tail"][1]) == len(_lib.SIGNATURES["hsad_clone_value_tail"][1]) + 1 == 22
    assert len(_lib.SIGNATURES["hsad_r2d2_clone_soft_fwd"][1]) == len(_lib.SIGNATURES["hsad_r2d2_clone_value_fwd"][1]) + 1 == 19
    txt = open(os.path.join(ROOT, "include", "hsad.h")).read()
    for name in NEW:
        before = txt[:txt.index("int " + name)]
        assert before.rstrip().endswith("*/"), "%s is not documented" % name
    # the row is a header of its own, which the CPU suite compiles
    row = open(os.path.join(ROOT, "hanabi_sad_amd", "csrc", "hsad_clone_soft.h")).read()
    assert "cs_row" in row and "__host__ __device__" in row
    assert "cs_row(" in open(os.path.join(ROOT, "hanabi_sad_amd", "csrc", "r2d2", "clone_soft.inc")).read()


def test_clone_loss_routes_a_target_to_the_new_entry_point(monkeypatch):
    from hanabi_sad_amd import _lib, composite
    assert list(inspect.signature(composite.CompositeLearner.clone_loss).parameters) == ["self", "batch", "weight", "compute_grad", "value_weight",
                                                                                         "policy_weight"]
    lr = fake_learner(monkeypatch)
    batch, weight = fake_batch()
    T, B, A = batch["legal_move"].shape
    # without the key: the old calls (tests/test_clone_value_surface_cpu.py holds them in full)
    lr.clone_loss(batch, weight)
    assert [c[0] for c in lr.lib.calls] == ["hsad_r2d2_clone_fwd", "hsad_r2d2_loss_bwd"]
    lr.lib.calls.clear()
    target = torch.full((T, B, A), 1.0 / A)
    loss, stats = lr.clone_loss(dict(batch, target=target), weight)
    assert [c[0] for c in lr.lib.calls] == ["hsad_r2d2_clone_soft_fwd", "hsad_r2d2_loss_bwd"]
    args = lr.lib.calls[0][1]
    assert len(args) == 19 and args[5] == lr._alive[-1].data_ptr() and args[6] is None and args[9:11] == (1.0, 0.0) and args[17] == 1
    assert isinstance(stats, composite.CloneStats) and set(stats) == {"hits", "decisions", "bad", "steps", "value_loss"} and loss.shape == (B,)
    # with the value term: the returns too, and no backward when none is asked for
    lr.lib.calls.clear()
    with pytest.raises(_lib.HsadError, match="ret"):
        lr.clone_loss(dict(batch, target=target), weight, value_weight=1.0)
    assert not lr.lib.calls
    ret = torch.arange(T * B, dtype=torch.float32).view(T, B)
    lr.clone_loss(dict(batch, target=target, ret=ret), weight, compute_grad=False, value_weight=0.5, policy_weight=2.0)
    assert [c[0] for c in lr.lib.calls] == ["hsad_r2d2_clone_soft_fwd"]
    args = lr.lib.calls[0][1]
    assert args[5] == lr._alive[-1].data_ptr() and args[6] == lr._alive[-2].data_ptr() and args[9:11] == (2.0, 0.5) and args[17] == 0
    # a target of the wrong shape or kind: refused before any library call
    lr.lib.calls.clear()
    for wrong in (torch.zeros(T, B, A + 1), torch.zeros(T, B), torch.zeros(B, T, A), torch.zeros(T, B, A, dtype=torch.int64), [[0.0] * A] * B):
        with pytest.raises(_lib.HsadError, match="target"):
            lr.clone_loss(dict(batch, target=wrong), weight)
    assert not lr.lib.calls


class Rec:
    """a record as the host-side checks see it"""

    def __init__(self, n, moves=None, players=2):
        self.rules = dict(players=players, hand_size=2, colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1, bomb=0)
        self.moves = list(moves) if moves is not None else [0] * n
        self.greedy = list(self.moves)
        self.n_moves, self.meta = n, {}


def test_the_target_makers_refuse_what_they_cannot_use():
    from hanabi_sad_amd import game_record as gr
    recs = [Rec(3, [0, 1, 2]), Rec(2, [4, 4])]
    A = gr.num_actions(recs[0].rules)
    assert A == 2 * 2 + (2 + 5) + 1
    values = [np.full((3, A), np.nan, dtype=np.float32), np.full((2, A), np.nan, dtype=np.float32)]
    values[0][1, [1, 3, 5]] = [10.0, 10.5, 9.0]
    for tau in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            clone.search_targets(recs, values, tau)
        with pytest.raises(ValueError, match="temperature"):
            clone.soft_targets(values[0], np.ones((3, A)), [0, 1, 2], tau)
    tg = clone.search_targets(recs, values, 0.5)
    assert [t.shape for t in tg] == [(3, A), (2, A)] and all(t.dtype == np.float32 for t in tg)
    assert tg[0][0].tolist() == [1.0] + [0.0] * (A - 1) and tg[1][1, 4] == 1.0                # no search: the move made
    want = np.exp((np.array([10.0, 10.5, 9.0]) - 10.5) / 0.5)
    assert np.allclose(tg[0][1, [1, 3, 5]], want / want.sum(), rtol=0, atol=1e-7) and tg[0][1].sum() == pytest.approx(1.0, abs=1e-6)
    with pytest.raises(ValueError, match="value arrays"):
        clone.search_targets(recs, values[:1], 0.5)
    with pytest.raises(ValueError, match="n_moves"):
        clone.search_targets(recs, [values[0], values[1][:1]], 0.5)
    # check_targets: what sequences_from_records(targets=...) does before any device work
    assert [t.shape for t in clone.check_targets(recs, tg, A)] == [(3, A), (2, A)]
    for wrong, what in (((tg[0],), "target arrays"), ((tg[0], tg[1][:, :-1]), "n_moves"), ((tg[0][:2], tg[1]), "n_moves"),
                        ((tg[0], tg[1].astype(np.int64)), "float"), ((tg[0] * 0.5, tg[1]), "distribution"), ((-tg[0], tg[1]), "distribution"),
                        ((np.where(tg[0] > 0, np.nan, tg[0]), tg[1]), "distribution")):
        with pytest.raises(ValueError, match=what):
            clone.check_targets(recs, wrong, A)
    sig = inspect.signature(clone.sequences_from_records).parameters
    assert sig["targets"].default is None and list(sig)[-1] == "targets" and sig["gamma"].default is None
    with pytest.raises(ValueError, match="target arrays"):      # ... and it is reached before a device is
        clone.sequences_from_records(recs, 1, targets=[tg[0]], device="cuda:0")


def test_the_dataset_carries_the_targets():
    ds = fake_dataset()
    T, N, A = ds.legal_move.shape
    assert ds.target is None and ds.take([1, 2]).target is None and all("target" not in b for b, _, _ in ds.batches(8, seed=2))
    g = torch.Generator().manual_seed(1)
    tg = torch.rand(T, N, A, generator=g) * (torch.arange(T).view(T, 1, 1) < ds.seq_len.view(1, N, 1))
    ds = clone.CloneDataset(ds.priv_s, None, ds.legal_move, ds.a, ds.seq_len, ds.game, ds.seat, 0, ds.ret, tg)
    part = ds.take([5, 0, 19])
    assert torch.equal(part.target, tg[:, [5, 0, 19]]) and torch.equal(part.ret, ds.ret[:, [5, 0, 19]])
    train, held = ds.split(0.3, seed=4)
    assert train.target.shape == (T, 14, A) and held.target.shape == (T, 6, A)
    for side in (train, held):
        for c in range(side.n_rows):
            assert torch.equal(side.target[:, c], tg[:, int(side.game[c]) * 2 + int(side.seat[c])])
    seen = 0
    for batch, weight, index in ds.batches(8, seed=2):
        assert batch["target"].shape == (T, 8, A) and batch["target"].dtype == torch.float32
        for c, j in enumerate(index.tolist()):
            if j >= 0:
                assert torch.equal(batch["target"][:, c], tg[:, j])
                seen += 1
            else:      # padding columns: zero rows, seq_len 0 -- never read
                assert not batch["target"][:, c].any() and float(weight[c]) == 0.0 and float(batch["seq_len"][c]) == 0.0
    assert seen == N
    # the entropy the command line subtracts: that of the rows, 0 log 0 = 0
    flat = torch.tensor([[[0.5, 0.5, 0.0, 0.0]], [[1.0, 0.0, 0.0, 0.0]], [[0.25, 0.25, 0.25, 0.25]]])
    small = clone.CloneDataset(torch.zeros(3, 1, 2), None, torch.ones(3, 1, 4), torch.zeros(3, 1, dtype=torch.int64), torch.tensor([3.0]),
                               torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 0, None, flat)
    assert clone.target_entropy(small) == pytest.approx(np.log(2.0) + np.log(4.0), abs=1e-12)
    assert clone.target_entropy(fake_dataset()) == 0.0


def test_the_command_line_refuses_a_bad_temperature_before_device_work():
    for bad in ("-0.5", "nan", "inf"):
        with pytest.raises(SystemExit, match="target_temperature"):
            clone.main(["--blueprint", "nothing.pthw", "--search_worlds", "4", "--target_temperature", bad])
    with pytest.raises(SystemExit, match="needs --blueprint"):
        clone.main(["--teacher", "piers", "--target_temperature", "0.5"])
    with pytest.raises(SystemExit, match="either"):
        clone.main(["--teacher", "piers", "--blueprint", "nothing.pthw"])
    with pytest.raises(SystemExit, match="no such weight file"):
        clone.main(["--blueprint", "nothing.pthw", "--search_worlds", "4", "--target_temperature", "0.5"])
    args = clone.parse_args(["--teacher", "piers"])
    assert args.target_temperature == 0.0 and args.blueprint == "" and args.search_worlds == 0 and args.searcher == "all"
    assert args.search_rounds is None and clone.parse_args(["--search_rounds", "2,2"]).search_rounds == (2, 2)


def test_play_with_search_takes_records_and_defaults_to_none():
    from hanabi_sad_amd import search
    sig = inspect.signature(search.play_with_search).parameters
    assert sig["records"].default is False and sig["records"].kind is inspect.Parameter.KEYWORD_ONLY
    sp = search.SearchPlay([3, 4], 10, torch.zeros(2, dtype=torch.int64), [])
    assert sp.records is None and sp.search_values is None and sp.mean == 3.5
