"""The float64 reference of the soft-target cloning tail (tests/clone_soft_ref.py), clone.soft_targets, and the row function of
hanabi_sad_amd/csrc/hsad_clone_soft.h compiled on its own, all without a device:
  - on one-hot targets the reference EQUALS tests/clone_value_ref.py's, and its gradient is autograd of the soft cross-entropy;
  - the rules by which a row is bad;
  - soft_targets: rows are distributions over the finite set, the limits in tau, the one-hot fall-back, what it refuses;
  - tests/clone_soft/clone_soft_main.cc, built with g++ -fsanitize=address,undefined (the sanitizers' runtimes linked statically: the
    program needs nothing loaded before it) and run directly, reproduces the fp32 restatement row_f32 bit for bit on seeded rows."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from hanabi_sad_amd import clone
from tests import clone_soft_ref as R
from tests import clone_value_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "clone_soft", "clone_soft_main.cc")
INC = os.path.join(ROOT, "hanabi_sad_amd", "csrc")
SHAPES = [(21, 37), (12, 19), (49, 62), (32, 48), (33, 49)]
CASES = [(1, 1), (5, 3), (97, 3), (130, 3)]
WEIGHTS = [(1.0, 0.0), (1.0, 1.0), (0.5, 2.0)]


@pytest.mark.parametrize("A,ldh", SHAPES)
@pytest.mark.parametrize("T,B", CASES)
@pytest.mark.parametrize("pw,vw", WEIGHTS)
def test_on_one_hot_targets_it_is_the_clone_value_reference(A, ldh, T, B, pw, vw):
    c, _ = V.clone_value_case(A, ldh, T, B)
    tg = R.one_hot_targets(c["action"], c["seq_len"], T, B, A)
    args = (c["heads"], c["legal"], c["action"])
    old = V.clone_value_tail(*args, c["ret"], c["seq_len"], c["weight"], T, B, A, 64, pw, vw)
    new = R.clone_soft_tail(*args, tg, c["ret"], c["seq_len"], c["weight"], T, B, A, 64, pw, vw)
    for k in ("loss", "vloss", "hits", "decisions", "bad", "steps", "dheads", "xent", "hub", "zero_row", "good"):
        assert torch.equal(old[k], new[k]), k
    assert torch.isfinite(new["dheads"]).all() and torch.isfinite(new["loss"]).all()      # the NaN rows past seq_len never show
    assert not new["target_bad"][old["good"]].any()


@pytest.mark.parametrize("A,ldh", [SHAPES[0], SHAPES[2]])
@pytest.mark.parametrize("pw,vw", WEIGHTS)
def test_reference_gradient_is_autograd_of_the_soft_cross_entropy(A, ldh, pw, vw):
    T, B = 97, 3
    c, _ = V.clone_value_case(A, ldh, T, B)
    tg = R.soft_targets_case(c, T, B, A)
    ref = R.clone_soft_tail(c["heads"], c["legal"], c["action"], tg, c["ret"], c["seq_len"], c["weight"], T, B, A, 64, pw, vw)
    assert not ref["target_bad"].any() and int(ref["decisions"].sum()) > 50
    sig = ref["sigma"][ref["multi"]]
    assert float((sig - 1).abs().max()) <= A * 2.0 ** -23 and bool((sig != 1).any()) and bool((sig == 1).any())
    good, multi = ref["good"], ref["multi"]
    h = c["heads"].double().clone().requires_grad_(True)
    l = c["legal"] != 0
    z = h[:, :A].masked_fill(~l, float("-inf"))
    logp = torch.log_softmax(torch.where(multi[:, None], z, torch.zeros_like(z)), 1)
    pi = torch.where(multi[:, None] & l, tg.double(), torch.zeros(T * B, A, dtype=torch.float64))
    xent = -(pi * torch.where(l & multi[:, None], logp, torch.zeros_like(logp))).sum(1)
    al = h[:, :A] * c["legal"].double()
    q = h[:, A:A + 1] + al - al.mean(1, keepdim=True)
    qa = q.gather(1, c["action"].clamp(0, A - 1)[:, None])[:, 0]
    hub = torch.nn.functional.smooth_l1_loss(qa, torch.where(good, c["ret"].double(), qa.detach()), reduction="none") * good.double()
    loss, vloss = xent.view(T, B).sum(0), hub.view(T, B).sum(0)
    ((pw * loss + vw * vloss) * c["weight"].double()).mean().backward()
    assert torch.allclose(loss, ref["loss"], rtol=0, atol=1e-11 * T)
    if vw:
        assert torch.allclose(vloss, ref["vloss"], rtol=0, atol=1e-12 * T)
    assert torch.allclose(h.grad[:, :A + 1], ref["dheads"][:, :A + 1], rtol=0, atol=1e-13)
    assert not ref["dheads"][:, A + 1:].any()
    assert float(ref["e_xent"].max()) <= 2 * A * 2.0 ** -24 * 60.0 and bool((ref["e_xent"][multi] > 0).any()) and not ref["e_xent"][~multi].any()


def test_the_rules_by_which_a_row_is_bad():
    A, ldh, T, B = 21, 37, 97, 3
    c, _ = V.clone_value_case(A, ldh, T, B)
    tg = R.soft_targets_case(c, T, B, A)
    clean = R.clone_soft_tail(c["heads"], c["legal"], c["action"], tg, c["ret"], c["seq_len"], c["weight"], T, B, A, 64)
    rows = [int(m) for m in torch.nonzero(clean["multi"] & (torch.arange(T * B) % B == 0) & (c["legal"] == 0).any(1))[:6, 0]]
    single = int(torch.nonzero(clean["single"])[0, 0])
    broken = tg.clone()
    lg = c["legal"]
    first, second = [int(torch.nonzero(lg[m])[0, 0]) for m in rows], [int(torch.nonzero(lg[m])[1, 0]) for m in rows]
    broken[rows[0], first[0]], broken[rows[0], second[0]] = -0.25, float(tg[rows[0], second[0]] + tg[rows[0], first[0]]) + 0.25     # negative, mass 1
    broken[rows[1], first[1]] = float("nan")
    broken[rows[2], int(torch.nonzero(lg[rows[2]] == 0)[0, 0])] = 0.125                       # mass on an illegal column
    broken[rows[3]] *= 0.9                                                                    # mass 0.9
    broken[rows[4]] *= 1.0 + 5e-4                                                             # inside the limit: NOT bad
    broken[single] = 0.0
    broken[single, int(torch.nonzero(lg[single] == 0)[0, 0])] = 1.0                           # a single-legal row with its mass elsewhere
    want_bad = rows[:4] + [single]
    ref = R.clone_soft_tail(c["heads"], c["legal"], c["action"], broken, c["ret"], c["seq_len"], c["weight"], T, B, A, 64)
    assert sorted(int(m) for m in torch.nonzero(ref["target_bad"])[:, 0]) == sorted(want_bad)
    assert int(ref["bad"].sum()) == int(clean["bad"].sum()) + 5 and int(ref["steps"].sum()) == int(clean["steps"].sum()) - 5
    assert int(ref["decisions"].sum()) == int(clean["decisions"].sum()) - 4
    assert not ref["dheads"][want_bad].any() and bool(ref["dheads"][rows[4]].any())
    # they contribute nothing: the same results as the clean targets with those rows' actions out of range
    action = c["action"].clone()
    action[want_bad] = -1
    tg2 = tg.clone()
    tg2[rows[4]] = broken[rows[4]]
    same = R.clone_soft_tail(c["heads"], c["legal"], action, tg2, c["ret"], c["seq_len"], c["weight"], T, B, A, 64)
    for k in ("loss", "vloss", "dheads", "hits", "decisions", "bad", "steps"):
        assert torch.equal(ref[k], same[k]), k


def test_soft_targets_rows_are_distributions_over_the_finite_set():
    rng = np.random.default_rng(5)
    n, A = 400, 51
    legal = rng.random((n, A)) < 0.4
    legal[:, A - 1] |= ~legal.any(1)
    a = np.array([rng.choice(np.nonzero(legal[i])[0]) for i in range(n)])
    values = np.where(legal & (rng.random((n, A)) < 0.8), rng.random((n, A)) * 25.0, np.nan).astype(np.float32)
    values[::7] = np.nan                                   # moves without a search
    values[3::7] = np.nan
    values[3::7][np.arange(len(a[3::7])), a[3::7]] = 12.0    # exactly one estimate
    finite = np.isfinite(values)
    few = finite.sum(1) < 2
    assert few.sum() > 100 and (~few).sum() > 100
    onehot = np.zeros((n, A), dtype=np.float32)
    onehot[np.arange(n), a] = 1.0
    for tau in (1e-6, 0.05, 0.5, 4.0, 1e6):
        p = clone.soft_targets(values, legal, a, tau)
        assert p.dtype == np.float32 and p.shape == (n, A) and (p >= 0).all()
        assert np.abs(p.astype(np.float64).sum(1) - 1.0).max() <= A * 2.0 ** -23
        assert not p[~few][~finite[~few]].any()
        assert np.array_equal(p[few], onehot[few])                                     # fewer than two finite values: the move made
        best = np.nanargmax(np.where(finite, values, -np.inf)[~few], 1)
        if tau == 1e-6:                                                                # -> the argmax (no two values of this set tie)
            assert np.array_equal(p[~few].argmax(1), best) and (p[~few].max(1) == 1.0).all()
        if tau == 1e6:                                                                 # -> uniform over the finite set
            want = finite[~few] / finite[~few].sum(1, keepdims=True)
            assert np.abs(p[~few] - want).max() <= 26e-6
        if tau == 0.5:                                                                 # the definition, and shift invariance
            v = values[~few].astype(np.float64)
            e = np.where(finite[~few], np.exp((v - np.nanmax(v, 1, keepdims=True)) / tau), 0.0)
            assert np.array_equal(p[~few], (e / e.sum(1, keepdims=True)).astype(np.float32))
            shifted = clone.soft_targets(values - np.float32(4.0), legal, a, tau)      # (multiples of 2^-20 up to 32: the shift is exact)
            assert np.abs(shifted - p).max() <= 2e-6
    # tensors in, a tensor out
    pt = clone.soft_targets(torch.from_numpy(values), torch.from_numpy(legal), torch.from_numpy(a), 0.5)
    assert torch.is_tensor(pt) and pt.dtype == torch.float32 and np.array_equal(pt.numpy(), clone.soft_targets(values, legal, a, 0.5))
    # what it refuses
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            clone.soft_targets(values, legal, a, tau)
    with pytest.raises(ValueError, match="illegal"):
        bad = values.copy()
        bad[0, np.nonzero(~legal[0])[0][0]] = 1.0
        clone.soft_targets(bad, legal, a, 1.0)
    with pytest.raises(ValueError):
        clone.soft_targets(values, legal[:, :-1], a, 1.0)
    with pytest.raises(ValueError):
        clone.soft_targets(values, legal, np.full(n, A), 1.0)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("clone_soft") / "clone_soft_main")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", INC, SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("A,ldo,pw,vw", [(21, 64, 1.0, 0.0), (21, 22, 1.0, 1.0), (49, 64, 0.5, 2.0), (12, 13, 0.0, 1.0), (51, 128, 1.0, 0.25)])
def test_the_header_equals_the_restatement_under_asan_and_ubsan(program, tmp_path, A, ldo, pw, vw):
    n = 240
    rows = R.seeded_rows(A, n, seed=100 * A + ldo)
    path = str(tmp_path / "rows.bin")
    R.write_rows(path, rows, A, ldo, pw, vw)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program, path], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK"
    at, seen = 0, dict(bad=0, single=0, dec=0, grad=0, hit=0)
    for i, r in enumerate(rows):
        want = R.row_f32(r["h"], r["legal"], r["pi"], r["act"], r["ret"], pw, vw, r["scale"], ldo)
        head = "row %d %d %d %d %d %d %d %d" % (i, want["bad"], want["step"], want["dec"], want["hit"], int(want["grad"] is not None),
                                             int(np.float32(want["xent"]).view(np.uint32)), int(np.float32(want["hub"]).view(np.uint32)))
        assert lines[at] == head, "row %d: the header printed %r, the restatement %r" % (i, lines[at], head)
        at += 1
        if want["grad"] is not None:
            got = np.array(lines[at].split()[1:], dtype=np.uint64).astype(np.uint32)
            assert lines[at].startswith("g ") and np.array_equal(got, want["grad"].view(np.uint32)), "row %d: gradient bits differ" % i
            at += 1
        seen["bad"] += want["bad"]
        seen["single"] += want["step"] and not want["dec"]
        seen["dec"] += want["dec"]
        seen["hit"] += want["hit"]
        seen["grad"] += want["grad"] is not None
    assert at == len(lines) - 1
    assert min(seen["bad"], seen["dec"], seen["grad"]) >= 20 and seen["single"] >= 5, seen
    # ... and the fp32 restatement is the float64 reference within fp32's reach (one sequence of n steps, one row each)
    c = dict(heads=torch.from_numpy(np.stack([r["h"] for r in rows])), legal=torch.from_numpy(np.stack([r["legal"] for r in rows])),
             action=torch.tensor([r["act"] for r in rows], dtype=torch.int64), ret=torch.tensor([float(r["ret"]) for r in rows]),
             target=torch.from_numpy(np.stack([r["pi"] for r in rows])))
    ref = R.clone_soft_tail(c["heads"], c["legal"], c["action"], c["target"], c["ret"], torch.tensor([float(n)]), torch.tensor([1.0]), n, 1, A, ldo, pw, vw)
    wants = [R.row_f32(r["h"], r["legal"], r["pi"], r["act"], r["ret"], pw, vw, 1.0, ldo) for r in rows]
    assert [w["bad"] for w in wants] == (~ref["good"]).long().tolist() and [w["dec"] for w in wants] == ref["multi"].long().tolist()
    x32 = torch.tensor([float(w["xent"]) for w in wants], dtype=torch.float64)
    assert float(((x32 - ref["xent"][:, 0]).abs() - (1e-4 + ref["e_xent"])).max()) <= 0.0
    g32 = torch.stack([torch.from_numpy(w["grad"]).double() if w["grad"] is not None else torch.zeros(ldo, dtype=torch.float64) for w in wants])
    assert float((g32 - ref["dheads"]).abs().max()) <= 1e-4
