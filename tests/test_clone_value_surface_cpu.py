"""The surface of the cloning value term without a device: the two entry points are declared in include/hsad.h, exported by the library
and bound in _lib.py with the argument lists the header gives; CompositeLearner.clone_loss with its defaults calls the entry point it
called before and only the new keywords reach the new one; CloneDataset carries `ret` through take / split / batches (CPU tensors)."""
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch

from hanabi_sad_amd import clone
from tests.test_abi_and_host import ROOT, header_functions

NEW = ("hsad_clone_value_tail", "hsad_r2d2_clone_value_fwd")


def declared_arguments(name):
    """the C types of a declaration's arguments, comments stripped: 'ptr' | 'int' | 'float'"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hsad.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, "%s is not declared in include/hsad.h" % name
    kinds = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        kinds.append("ptr" if "*" in arg else "float" if arg.startswith("float ") else "int")
    return kinds


def test_both_symbols_are_declared_exported_and_bound(hsad_lib):
    from hanabi_sad_amd import _lib
    declared = header_functions()
    ctype_kind = {C.c_void_p: "ptr", C.c_int: "int", C.c_float: "float"}
    for name in NEW:
        assert name in declared and hasattr(hsad_lib, name) and name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        assert [ctype_kind[a] for a in argtypes] == declared_arguments(name), name
    # the neighbours they extend keep their argument lists
    assert len(_lib.SIGNATURES["hsad_clone_tail"][1]) == 16 and len(_lib.SIGNATURES["hsad_r2d2_clone_fwd"][1]) == 13
    assert len(_lib.SIGNATURES["hsad_clone_value_tail"][1]) == 21 and len(_lib.SIGNATURES["hsad_r2d2_clone_value_fwd"][1]) == 18
    # and the header says what they compute
    txt = open(os.path.join(ROOT, "include", "hsad.h")).read()
    for name in NEW:
        before = txt[:txt.index("int " + name)]
        assert before.rstrip().endswith("*/"), "%s is not documented" % name


class Recorder:
    """stands in for the library: notes which entry points are called, with what"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def fake_learner(monkeypatch):
    from hanabi_sad_amd import composite
    monkeypatch.setattr(composite, "_s", lambda dev: None)
    lr = object.__new__(composite.CompositeLearner)
    lr.lib, lr.h, lr.device, lr._alive = Recorder(), 1, torch.device("cpu"), []
    lr.online = types.SimpleNamespace(Fp=64)
    lr._ensure = lambda T, rows: None
    return lr


def fake_batch(T=4, B=3, F=5, A=6):
    return {"priv_s": torch.zeros(T, B, F), "legal_move": torch.ones(T, B, A), "a": torch.zeros(T, B, dtype=torch.int64),
            "seq_len": torch.tensor([4.0, 2.0, 0.0])}, torch.ones(B)


def test_clone_loss_defaults_route_to_the_old_entry_point(monkeypatch):
    from hanabi_sad_amd import _lib, composite
    sig = inspect.signature(composite.CompositeLearner.clone_loss)
    assert sig.parameters["value_weight"].default == 0.0 and sig.parameters["policy_weight"].default == 1.0
    assert list(sig.parameters)[:4] == ["self", "batch", "weight", "compute_grad"]
    lr = fake_learner(monkeypatch)
    batch, weight = fake_batch()
    loss, stats = lr.clone_loss(batch, weight)
    assert [c[0] for c in lr.lib.calls] == ["hsad_r2d2_clone_fwd", "hsad_r2d2_loss_bwd"]
    assert len(lr.lib.calls[0][1]) == 13
    assert isinstance(stats, composite.CloneStats) and set(stats) == {"hits", "decisions", "bad"} and loss.shape == (3,)
    # steps and value_loss exist all the same (made when asked for: the call itself launches nothing new)
    stats["bad"].zero_()
    assert stats["steps"].tolist() == [4, 2, 0] and stats["steps"].dtype == torch.int32
    assert stats["value_loss"].tolist() == [0.0, 0.0, 0.0] and stats["value_loss"].dtype == torch.float32
    with pytest.raises(KeyError):
        stats["nothing"]
    lr.lib.calls.clear()
    lr.clone_loss(batch, weight, compute_grad=False, value_weight=0.0, policy_weight=1.0)
    assert [c[0] for c in lr.lib.calls] == ["hsad_r2d2_clone_fwd"]
    # the value term: the new entry point, with the returns and both weights
    lr.lib.calls.clear()
    with pytest.raises(_lib.HsadError, match="ret"):
        lr.clone_loss(batch, weight, value_weight=1.0)
    assert not lr.lib.calls
    batch["ret"] = torch.arange(12, dtype=torch.float32).view(4, 3)
    loss, stats = lr.clone_loss(batch, weight, value_weight=0.5)
    assert [c[0] for c in lr.lib.calls] == ["hsad_r2d2_clone_value_fwd", "hsad_r2d2_loss_bwd"]
    args = lr.lib.calls[0][1]
    assert len(args) == 18 and args[8:10] == (1.0, 0.5) and args[5] == lr._alive[-1].data_ptr() and args[16] == 1
    assert set(stats) == {"hits", "decisions", "bad", "steps", "value_loss"} and stats["steps"].dtype == torch.int32
    assert stats["value_loss"].shape == (3,) and stats["value_loss"].dtype == torch.float32
    with pytest.raises(_lib.HsadError, match="ret must be"):
        lr.clone_loss(dict(batch, ret=torch.zeros(3, 4)), weight, value_weight=1.0)
    # policy_weight alone also needs the new kernel, and no returns
    lr.lib.calls.clear()
    del batch["ret"]
    lr.clone_loss(batch, weight, policy_weight=0.5)
    assert lr.lib.calls[0][0] == "hsad_r2d2_clone_value_fwd" and lr.lib.calls[0][1][5] is None and lr.lib.calls[0][1][8:10] == (0.5, 0.0)


def fake_dataset(n_game=10, P=2, T=6, F=5, A=4, with_ret=True):
    N = n_game * P
    game = torch.arange(n_game).repeat_interleave(P)
    seat = torch.arange(P).repeat(n_game)
    seq_len = torch.arange(1, N + 1, dtype=torch.float32).clamp(max=T)
    ret = (1000.0 * game.float().view(1, N) + torch.arange(T).float().view(T, 1)) * (torch.arange(T).view(T, 1) < seq_len.view(1, N))
    return clone.CloneDataset(priv_s=torch.arange(T * N * F, dtype=torch.float32).view(T, N, F), priv_s_bf16=None, legal_move=torch.ones(T, N, A),
                              a=torch.zeros(T, N, dtype=torch.int64), seq_len=seq_len, game=game, seat=seat, truncated=0, ret=ret if with_ret else None)


def test_the_dataset_carries_the_returns():
    ds = fake_dataset()
    part = ds.take([5, 0, 19])
    assert torch.equal(part.ret, ds.ret[:, [5, 0, 19]]) and part.ret.shape == (6, 3)
    train, held = ds.split(0.3, seed=4)
    assert train.ret.shape == (6, 14) and held.ret.shape == (6, 6)
    for side in (train, held):      # a column's returns are its game's
        for c in range(side.n_rows):
            j = int(side.game[c]) * 2 + int(side.seat[c])
            assert torch.equal(side.ret[:, c], ds.ret[:, j])
    seen = 0
    for batch, weight, index in ds.batches(8, seed=2):
        assert batch["ret"].shape == (6, 8) and batch["ret"].dtype == torch.float32
        for c, j in enumerate(index.tolist()):
            if j >= 0:
                assert torch.equal(batch["ret"][:, c], ds.ret[:, j])
                seen += 1
            else:
                assert not batch["ret"][:, c].any() and float(weight[c]) == 0.0      # padding columns: 0
    assert seen == 20
    # without returns nothing changes: no key, no field
    plain = fake_dataset(with_ret=False)
    assert plain.ret is None and plain.take([1, 2]).ret is None and plain.split(0.3, seed=4)[0].ret is None
    assert all("ret" not in batch for batch, _, _ in plain.batches(8, seed=2))
    assert "gamma" in inspect.signature(clone.sequences_from_records).parameters
    assert inspect.signature(clone.sequences_from_records).parameters["gamma"].default is None
