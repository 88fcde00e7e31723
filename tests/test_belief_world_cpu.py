"""The per-slot stratified uniforms of the learned belief's worlds (hanabi_sad_amd/csrc/hsad_belief_world.h; include/hsad.h,
hsad_env_determinize_belief_worlds) without a GPU:
  - the restatement tests/belief_world_ref.py against what the scheme promises: per slot the worlds' strata are a permutation, every
    k_i lies in its stratum, W = 1 is a plain draw, draws over many groups reproduce the enumerated distribution (and the exact belief
    at zero logits), and slot 0 of a game's worlds is stratified;
  - tests/belief_world/belief_world_main.cc, built with g++ -fsanitize=address,undefined (the sanitizers' runtimes linked statically:
    the program needs nothing loaded before it) and run directly, reproduces the restatement bit for bit -- the uniforms and the
    sample-mode rows through bh_row;
  - the precondition of tests/test_env_belief_worlds_gpu.py on the very states and inputs it uses."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import belief_head_ref as R
from tests import belief_world_cases as WC
from tests import belief_world_ref as BW
from tests import hand_belief_ref as HB
from tests import search_fixtures as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "hanabi_sad_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "belief_world", "belief_world_main.cc")
WS = (1, 2, 3, 8, 12, 16, 97, 4096)
KEYS = [(2025, 0), (6, SF.key_of(3)), (2 ** 64 - 1, (5 << 32) | 0), (0x1234567890ABCDEF, -3)]


def test_the_strata_of_every_slot_are_a_permutation_and_every_k_lies_in_its_stratum():
    for seed, group in KEYS:
        for W in WS:
            a = [BW.stride(seed, group, W, i) for i in range(5)]
            o = [BW.offset(seed, group, W, i) for i in range(5)]
            assert all(1 <= x < max(W, 2) and math.gcd(x, W) == 1 for x in a) and all(0 <= x < W for x in o), (seed, group, W, a, o)
            worlds = range(W) if W <= 97 else list(range(0, W, 41)) + [W - 1]
            if W > 97:      # the permutation itself, from the stride and offset: one hash-free line per world
                for i in range(5):
                    assert sorted((a[i] * w + o[i]) % W for w in range(W)) == list(range(W))
            seen = [set() for _ in range(5)]
            for w in worlds:
                s, k = BW.strata(seed, group, W, w), BW.ks(seed, group, W, w)
                assert s == [(a[i] * w + o[i]) % W for i in range(5)]
                for i in range(5):
                    assert 0 <= k[i] < 1 << 24 and (s[i] << 24) <= k[i] * W < ((s[i] + 1) << 24), (seed, group, W, w, i)
                    seen[i].add(s[i])
                assert BW.uniforms(seed, group, W, w) == [x << 8 for x in k]
            if W <= 97:
                assert all(x == set(range(W)) for x in seen), (seed, group, W)
    # the slots' permutations differ: a design, not five copies of one
    assert len({tuple(BW.strata(2025, 7, 97, w)[i] for w in range(97)) for i in range(5)}) == 5


def test_one_world_is_a_plain_draw_and_bad_worlds_are_refused():
    for seed, group in KEYS:
        assert BW.uniforms(seed, group, 1, 0) == [(BW.h(seed, group, (1 << 8) | i) >> 8) << 8 for i in range(5)]
        assert BW.strata(seed, group, 1, 0) == [0] * 5
    for W, w in ((0, 0), (8, -1), (8, 8), ((1 << 20) + 1, 0), (1, 1)):
        assert BW.uniforms(1, 2, W, w) is None
    assert BW.uniforms(1, 2, 1 << 20, (1 << 20) - 1) is not None


def small_position():
    """two slots, a handful of hands (tests/test_belief_head_cpu.py's)"""
    pool = [0] * 25
    for t, c in ((0, 2), (1, 1), (5, 2), (6, 1), (10, 1)):
        pool[t] = c
    cms = [[1 if t % 5 == 0 else 0 for t in range(25)], [1 if t // 5 <= 1 else 0 for t in range(25)]]
    return pool, cms


def chi2_upper(dof):
    """the 99.9 % point of chi^2 with dof degrees of freedom (Wilson-Hilferty; a stratified sample lies below a plain one)"""
    z = 3.0902
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * math.sqrt(2.0 / (9.0 * dof))) ** 3


@pytest.mark.parametrize("zero", [False, True], ids=["random-logits", "zero-logits"])
def test_draws_over_many_groups_reproduce_the_enumerated_distribution(zero):
    pool, cms = small_position()
    rng = np.random.default_rng(11)
    z = [0.0] * 50 if zero else list(rng.standard_normal(50))
    dist = R.hand_distribution(z, pool, cms)
    assert abs(sum(dist.values()) - 1.0) <= 1e-12 and len(dist) >= 6
    if zero:      # zero logits: the exact belief -- a hand's share of the N weighted assignments
        N = HB.total_of(pool, cms)
        for hand, pr in dist.items():
            assert abs(pr - R.falling_product(pool, hand) / N) <= 1e-12
    W, groups = 8, 600
    counts = {}
    for grp in range(groups):
        for w in range(W):
            s = BW.sample(z, pool, cms, 77, grp, W, w)
            counts[tuple(s["cards"])] = counts.get(tuple(s["cards"]), 0) + 1
    n = W * groups
    assert set(counts) <= set(dist)
    chi2 = sum((counts.get(hand, 0) - n * pr) ** 2 / (n * pr) for hand, pr in dist.items())
    print("chi^2 = %.2f over %d hands, %d draws (99.9 %% point %.2f)" % (chi2, len(dist), n, chi2_upper(len(dist) - 1)))
    assert chi2 <= chi2_upper(len(dist) - 1)
    # world w alone, over the groups, is a plain draw as well: the same test on each single world's marginal of slot 0
    p0 = {}
    for hand, pr in dist.items():
        p0[hand[0]] = p0.get(hand[0], 0.0) + pr
    for w in (0, W - 1):
        c0 = {}
        for grp in range(groups):
            t = BW.sample(z, pool, cms, 77, grp, W, w)["cards"][0]
            c0[t] = c0.get(t, 0) + 1
        chi2 = sum((c0.get(t, 0) - groups * pr) ** 2 / (groups * pr) for t, pr in p0.items())
        assert chi2 <= chi2_upper(len(p0) - 1), (w, chi2)


def slot0_cases():
    rng = np.random.default_rng(5)
    for k in range(12):
        pool, cms, cards = R.deal_case(rng, 5, variant=(k % 4 == 3))
        n = R.occupied(cards)
        z = list(rng.standard_normal(125) * 3.0)
        if n:
            for W in (8, 12, 97):
                yield k, W, z, pool, cms[:n]


def test_slot_0_of_a_games_worlds_is_stratified_in_its_cumulative_counts():
    """slot 0's conditional is the same in every world of a game, and its W uniforms lie one in each of the W equal parts of [0, 1).  So
    the number of worlds whose uniform lies below a boundary c of the cumulative distribution is floor(W c) or floor(W c) + 1: the
    worlds that hold a type <= t in slot 0 number W P_0[<= t] to within 1 (plus the worlds the float bound puts at that boundary).  This
    much any one-point-per-part design gives; the per-type bound of the next test needs the jitter to be common to the worlds"""
    checked = 0
    for k, W, z, pool, cms in slot0_cases():
        count, p, near = BW.slot0_counts(z, pool, cms, 31 + k, k, W)
        assert sum(count) == W
        cum_n, cum_p = 0, 0.0
        for t in range(25):
            cum_n, cum_p = cum_n + count[t], cum_p + p[t]
            assert abs(cum_n - W * cum_p) <= 1.0 + near[t] + 1e-9, (k, W, t, cum_n, W * cum_p, near[t])
        got = [0] * 25
        for w in range(W):
            got[BW.sample(z, pool, cms, 31 + k, k, W, w)["cards"][0]] += 1
        assert got == count
        checked += 1
    assert checked >= 20


def test_slot_0_of_a_games_worlds_is_stratified():
    """the number of a game's W worlds that hold type t in slot 0 lies within W p_0[t] +- 1 (plus the worlds the float bound of the
    reference puts at a boundary).  A type's interval of the cumulative distribution has two boundaries, so this needs more than one point
    per part of [0, 1): with a jitter of its own per world an interval that cuts a little off two neighbouring parts can hold both
    their points, and the count strays up to 2 (measured with such a jitter on these cases: 4 of 900 pairs beyond 1, the largest 1.57).
    The jitter j_i is therefore ONE per (group, slot): a slot's W points are a lattice of spacing 1 / W, and any interval of length p
    holds floor(W p) or ceil(W p) of them.  On these 36 (position, W) cases the largest |count - W p_0[t]| is 0.974."""
    worst, over, seen = 0.0, [], 0
    for k, W, z, pool, cms in slot0_cases():
        count, p, near = BW.slot0_counts(z, pool, cms, 31 + k, k, W)
        for t in range(25):
            d = abs(count[t] - W * p[t])
            seen += 1
            worst = max(worst, d - near[t])
            if d > 1.0 + near[t] + 1e-9:
                over.append((k, W, t, count[t], round(W * p[t], 3)))
    print("slot 0: %d of %d (case, type) pairs beyond +- 1; largest |count - W p| less the float allowance: %.3f" % (len(over), seen, worst))
    assert not over, over


# ---- the header under the sanitizers --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("belief_world") / "belief_world_main")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", INC, SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def write_cases(path, cases, Hs):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<ii", len(cases), Hs))
        for c in cases:
            cm = [R.pack_mask(m) for m in c["cms"]] + [0] * (5 - len(c["cms"]))
            fh.write(struct.pack("<QQiiiQ5I", c["seed"] & R.M64, c["group"] & R.M64, c["W"], c["w"], c["n"], R.pack_pool(c["pool"]), *cm[:5]))
            fh.write(np.asarray(c["z"], dtype="<f4").tobytes())


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("Hs", [5, 4, 2])
def test_the_header_equals_the_restatement_under_asan_and_ubsan(program, tmp_path, Hs):
    rng = np.random.default_rng(300 + Hs)
    cases = []
    for W in (1, 2, 3, 8, 12, 97, 4096, 1 << 20):
        for seed, group in KEYS:
            for w in sorted({0, W - 1, W // 2, int(rng.integers(0, W))}):
                pool, cms, cards = R.deal_case(rng, Hs, variant=(len(cases) % 5 == 2))
                z = (rng.standard_normal(Hs * 25) * 3.0).astype(np.float32)
                if len(cases) % 7 == 0:
                    z[:] = 0
                cases.append(dict(seed=seed, group=group, W=W, w=w, n=R.occupied(cards), pool=pool, cms=cms, z=z))
    zero = np.zeros(Hs * 25, dtype=np.float32)
    for W, w in ((0, 0), (8, -1), (8, 8), ((1 << 20) + 1, 0), (1, 1), (-5, 0)):
        cases.append(dict(seed=1, group=2, W=W, w=w, n=-1, pool=[0] * 25, cms=[], z=zero))
    path = str(tmp_path / "cases.bin")
    write_cases(path, cases, Hs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program, path], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK"
    at, rows, refused, zeros = 0, 0, 0, 0
    for i, c in enumerate(cases):
        us = BW.uniforms(c["seed"], c["group"], c["W"], c["w"])
        if us is None:
            want = "u 0" + " 0" * 10
            refused += 1
        else:
            want = "u 1 " + " ".join(str(x) for x in us + BW.strata(c["seed"], c["group"], c["W"], c["w"]))
        assert lines[at] == want, "case %d (W %d, w %d): the header printed %r, the restatement %r" % (i, c["W"], c["w"], lines[at], want)
        at += 1
        if us is None or c["n"] < 0:
            continue
        r = BW.row_f32(c["z"], c["pool"], c["cms"], c["n"], c["seed"], c["group"], c["W"], c["w"])
        hand = sum(x << (5 * k) for k, x in enumerate(r["hand"])) if not r["bad"] else 0
        want = "row %d %d %d %d %d" % (r["bad"], int(np.float32(r["nll"]).view(np.uint32)), int(np.float32(r["nll0"]).view(np.uint32)), hand,
                                      R.pack_pool(r["q"]))
        assert lines[at] == want, "case %d: bh_row under the header's uniforms printed %r, the restatement %r" % (i, lines[at], want)
        at += 1
        rows += not r["bad"]
        if not r["bad"] and not np.any(c["z"]):
            zeros += 1
            assert np.float32(r["nll"]).view(np.uint32) == np.float32(r["nll0"]).view(np.uint32)
    assert at == len(lines) - 1 and rows >= 60 and refused == 6 and zeros >= 5, (rows, refused, zeros)


# ---- the precondition of the GPU tests -------------------------------------------------------------------------------------------------
def oracle_states(case):
    from tests.test_determinize_cpu import _oracle_rows
    _, config, sad, sc, seed, pseed, iters, _ = case
    return _oracle_rows(config, sad, sc, 0, WC.G, seed, pseed, iters)


@pytest.mark.parametrize("case", WC.CASES, ids=WC.IDS)
def test_the_float64_reference_is_rarely_near_a_boundary_on_the_states_the_gpu_tests_sample(case):
    P, H = SF.CONFIGS[case[1]]["players"], SF.CONFIGS[case[1]]["hand_size"]
    rows, term = oracle_states(case)
    viewer, _ = SF.viewers_and_keys(WC.G, P)
    live = [g for g in range(WC.G) if viewer[g] >= 0 and not term[g]]
    assert len(live) >= 20
    know = {g: HB.pool_and_masks(rows[g], P, H, int(viewer[g])) for g in live}
    for mode in WC.MODES:
        for W in WC.WORLDS:
            inp = WC.inputs(case, H, mode, W)
            zs = inp["logits"].numpy()
            near = moved = 0
            for g in live:
                pool, cms, hand = know[g]
                s = BW.sample([float(x) for x in zs[WC.row_of(inp, g)]], pool, cms, inp["seed"], int(inp["group"][g]), W, int(inp["world"][g]))
                assert s is not None
                near += s["near"]
                moved += s["cards"] != hand
            print("%s %s W=%d: %d of %d live rows near a boundary" % (case[0], mode, W, near, len(live)))
            assert near <= 0.01 * len(live), "%s %s W=%d: %d of %d draws lie at a boundary: pick another seed" % (case[0], mode, W, near, len(live))
            assert moved >= 5
