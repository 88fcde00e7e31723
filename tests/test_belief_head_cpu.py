"""The row of the learned hand belief (hanabi_sad_amd/csrc/hsad_belief_head.h; include/hsad.h, hsad_belief_tail) without a GPU:
  - the float64 reference tests/belief_head_ref.py against what the model promises: at z = 0 it IS the exact belief (unrank's
    conditionals as Python fractions, the hand's score log N - log prod falling counts), its gradient is autograd's, every sampled
    hand is consistent, and stratified uniforms reproduce the enumerated distribution;
  - tests/belief_head/belief_head_main.cc, built with g++ -fsanitize=address,undefined (the sanitizers' runtimes linked statically: the
    program needs nothing loaded before it) and run directly, reproduces the fp32 restatement row_f32 bit for bit, in score and in
    sample mode."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import belief_head_ref as R
from tests import hand_belief_ref as HB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "hanabi_sad_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "belief_head", "belief_head_main.cc")


def positions(n, seed, sizes=(5, 4, 2)):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        Hs = sizes[k % len(sizes)]
        pool, cms, cards = R.deal_case(rng, Hs, variant=(k % 4 == 3))
        out.append((Hs, pool, cms, cards))
    pool, cms, cards = R.dead_end_case()
    out.append((2, pool, cms, cards))
    return out


def test_zero_logits_are_the_exact_belief():
    seen = 0
    for Hs, pool, cms, cards in positions(60, 1):
        n = R.occupied(cards)
        z = [0.0] * (Hs * 25)
        r = R.row(z, pool, cms, cards)
        assert not r["bad"]
        if n == 0:
            assert r["nll0"] == 0.0 and r["nll"] == 0.0
            continue
        hand = cards[:n]
        cond = R.exact_conditionals(pool, cms[:n], hand)
        # unrank's conditionals: type t takes q[t] C(later, q - e_t) of the ranks the slot still has -- the same integers, as fractions
        q, N = list(pool), HB.total_of(pool, cms[:n])
        block = N
        for i, c in enumerate(hand):
            later = tuple(range(i + 1, n))
            ws = {t: q[t] * HB.count(HB.less_one(q, t), cms[:n], later) for t in range(25) if q[t] * cms[i][t]}
            ws = {t: w for t, w in ws.items() if w}
            assert sum(ws.values()) == block      # the types' blocks tile the ranks the slots before left
            assert cond[i] == {t: Fraction(w, block) for t, w in ws.items()}
            s = r["slots"][i]
            assert s["F"] == sorted(ws) and all(Fraction(s["w"][t], sum(s["w"])) == cond[i][t] for t in ws)
            block = ws[c] // q[c]      # one physical copy of c: the ranks handed to the next slot
            q[c] -= 1
        want = math.log(N) - math.log(R.falling_product(pool, hand))
        assert abs(r["nll0"] - want) <= 1e-12 * max(1.0, abs(want)) and r["nll"] == r["nll0"] and r["hit"] == r["hit0"]
        seen += 1
    assert seen >= 40


def test_the_reference_gradient_is_autograd_of_the_float64_nll():
    rng = np.random.default_rng(7)
    checked = 0
    for Hs, pool, cms, cards in positions(30, 2):
        n = R.occupied(cards)
        if n == 0:
            continue
        z = rng.standard_normal(Hs * 25) * 2.0
        r = R.row(list(z), pool, cms, cards)
        zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        nll = torch.zeros((), dtype=torch.float64)
        for i, s in enumerate(r["slots"]):
            F = torch.tensor(s["F"])
            logw = torch.log(torch.tensor([float(s["w"][t]) for t in s["F"]], dtype=torch.float64))
            lp = torch.log_softmax(zt[i * 25 + F] + logw, 0)
            nll = nll - lp[s["F"].index(s["c"])]
        nll.backward()
        assert abs(float(nll.detach()) - r["nll"]) <= 1e-10
        assert float((zt.grad - torch.tensor(r["grad"], dtype=torch.float64)).abs().max()) <= 1e-12
        checked += 1
    assert checked >= 20


def consistent(pool, cms, hand):
    q = list(pool)
    for i, c in enumerate(hand):
        if not cms[i][c] or q[c] <= 0:
            return False
        q[c] -= 1
    return True


def test_sampled_hands_are_always_consistent():
    rng = np.random.default_rng(3)
    n_dead = 0
    for k, (Hs, pool, cms, cards) in enumerate(positions(45, 3)):
        n = R.occupied(cards)
        for rep in range(6):
            z = list(rng.standard_normal(Hs * 25) * (8.0 if rep % 2 else 1.0))
            us = R.draws(1000 + rep, k, n)
            s = R.sample(z, pool, cms[:n], us)
            assert s is not None and consistent(pool, cms[:n], s["cards"]), (k, rep)
            assert s["q"] == [pool[t] - s["cards"].count(t) for t in range(25)]
            got = R.row_f32(z, pool, cms, None, us, n)
            assert not got["bad"] and consistent(pool, cms[:n], got["hand"])
            assert s["near"] or got["hand"] == s["cards"]
    # the dead-end position: slot 0 must never take the card slot 1 is pinned to, whatever the logits say
    pool, cms, _ = R.dead_end_case()
    z = [0.0] * 50
    z[4] = 30.0      # push slot 0 towards the pinned card
    for u in range(0, 1 << 32, 1 << 26):
        s = R.sample(z, pool, cms, [u, 12345])
        assert s["cards"][1] == 4 and s["cards"][0] != 4
        assert R.row_f32(z, pool, cms, None, [u, 12345], 2)["hand"] == s["cards"]
        n_dead += 1
    assert n_dead == 64


def test_stratified_uniforms_reproduce_the_enumerated_distribution():
    """a position of two slots with a handful of hands; k bits of uniform per slot, every combination once: each hand must come up
    2^2k prod_i p_i times, give or take the strata its boundaries cut"""
    pool = [0] * 25
    for t, c in ((0, 2), (1, 1), (5, 2), (6, 1), (10, 1)):
        pool[t] = c
    cms = [[1 if t % 5 == 0 else 0 for t in range(25)], [1 if t // 5 <= 1 else 0 for t in range(25)]]
    rng = np.random.default_rng(11)
    z = list(rng.standard_normal(50))
    dist = R.hand_distribution(z, pool, cms)
    assert abs(sum(dist.values()) - 1.0) <= 1e-12 and len(dist) >= 6
    k = 7
    counts = {}
    for a in range(1 << k):
        for b in range(1 << k):
            us = [((2 * a + 1) << (31 - k)), ((2 * b + 1) << (31 - k))]      # the mid-points of the strata
            s = R.sample(z, pool, cms, us)
            counts[tuple(s["cards"])] = counts.get(tuple(s["cards"]), 0) + 1
    total = 1 << (2 * k)
    assert set(counts) <= set(dist)
    for hand, pr in dist.items():
        # slot 0 is cut into 2^k strata (each boundary misplaces at most one), and so is slot 1 inside each of them
        assert abs(counts.get(hand, 0) / total - pr) <= 2.0 * 2.0 ** -k + 2.0 ** -k, (hand, counts.get(hand, 0) / total, pr)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("belief_head") / "belief_head_main")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", INC, SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def seeded_rows(Hs, n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        pool, cms, cards = R.deal_case(rng, Hs, variant=(i % 5 == 2))
        if i % 17 == 5:
            pool, cms2, cards2 = R.dead_end_case()
            if Hs >= 2:
                cms, cards = cms2 + [[0] * 25] * (Hs - 2), cards2 + [-1] * (Hs - 2)
        z = (rng.standard_normal(Hs * 25) * (30.0 if i % 5 == 4 else 3.0)).clip(-30, 30).astype(np.float32)
        if i % 9 == 0:
            z[:] = 0
        nocc = R.occupied(cards)
        row = dict(pool=pool, cms=cms, z=z, scale=np.float32(rng.random() * 2.0))
        if i % 3 == 2:
            row.update(cards=None, n_sample=nocc, us=[int(rng.integers(0, 1 << 32)) for _ in range(5)])
            if i % 12 == 2 and nocc:
                row["us"][0] = 0xFFFFFFFF      # the top of the range: the "none exceeds" fallback's neighbourhood
        else:
            cards = list(cards)
            if i % 8 == 3 and nocc:
                kind = (i // 8) % 4
                if kind == 0:
                    cms = [list(cm) for cm in cms]
                    cms[0][cards[0]] = 0
                    row["cms"] = cms
                elif kind == 1:
                    cards[nocc - 1] = 25
                elif kind == 2 and nocc < Hs:
                    cards[nocc] = -1
                    cards = [-1] + cards[:Hs - 1]
                else:
                    z[int(rng.integers(0, nocc * 25))] = np.inf if i % 16 < 8 else np.nan
            row["cards"] = cards
        rows.append(row)
    return rows


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("Hs,ldo", [(5, 128), (5, 125), (4, 104), (2, 56)])
def test_the_header_equals_the_restatement_under_asan_and_ubsan(program, tmp_path, Hs, ldo):
    n = 150
    rows = seeded_rows(Hs, n, seed=100 * Hs + ldo)
    path = str(tmp_path / "rows.bin")
    R.write_rows(path, rows, Hs, ldo)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program, path], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK"
    at, seen = 0, dict(bad=0, score=0, sample=0, grad=0, zero=0)
    for i, r in enumerate(rows):
        score = r.get("cards") is not None
        want = R.row_f32(r["z"], r["pool"], r["cms"], r["cards"] if score else None, r.get("us"), r.get("n_sample", 0), r["scale"], ldo if score else None)
        hand = sum(c << (5 * k) for k, c in enumerate(want["hand"])) if not want["bad"] else 0
        head = "row %d %d %d %d %d %d %d %d %d %d" % (i, want["bad"], want["cards"], want["hit"], want["hit0"], int(want["grad"] is not None),
                                                     int(np.float32(want["nll"]).view(np.uint32)), int(np.float32(want["nll0"]).view(np.uint32)), hand,
                                                     R.pack_pool(want["q"]))
        assert lines[at] == head, "row %d: the header printed %r, the restatement %r" % (i, lines[at], head)
        at += 1
        if want["grad"] is not None:
            got = np.array(lines[at].split()[1:], dtype=np.uint64).astype(np.uint32)
            assert lines[at].startswith("g ") and np.array_equal(got, want["grad"].view(np.uint32)), "row %d: gradient bits differ" % i
            at += 1
        seen["bad"] += want["bad"]
        seen["score"] += score and not want["bad"]
        seen["sample"] += (not score) and not want["bad"]
        seen["grad"] += want["grad"] is not None
        if not want["bad"] and not np.any(r["z"]):
            seen["zero"] += 1
            assert np.float32(want["nll"]).view(np.uint32) == np.float32(want["nll0"]).view(np.uint32)      # z = 0: the same bits
        # ... and the fp32 restatement is the float64 reference within the bound the GPU test grants the kernel
        if score:
            ref = R.row([float(x) for x in r["z"]], r["pool"], r["cms"], r["cards"])
            assert ref["bad"] == want["bad"]
            if not ref["bad"]:
                assert (ref["cards"], ref["hit0"]) == (want["cards"], want["hit0"])
                assert abs(float(want["nll"]) - ref["nll"]) <= ref["e_nll"] and abs(float(want["nll0"]) - ref["nll0"]) <= ref["e_nll0"]
                g64 = float(np.float32(r["scale"])) * np.asarray(ref["grad"])
                bound = float(np.float32(r["scale"])) * (np.asarray(ref["e_p"]) + 2 * R.U * np.abs(np.asarray(ref["grad"])))
                assert np.all(np.abs(want["grad"][:Hs * 25].astype(np.float64) - g64) <= bound)
    assert at == len(lines) - 1
    assert min(seen["bad"], seen["score"], seen["sample"], seen["grad"]) >= 10 and seen["zero"] >= 5, seen
