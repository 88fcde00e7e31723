"""CPU: hanabi_sad_amd/csrc/hsad_act_sample.h -- the sampler core of hsad_act_sample_q -- compiled on its own with
`g++ -fsanitize=address,undefined` (the sanitizers' runtimes linked statically: the program needs nothing loaded before it) into a
stand-alone program (tests/act_sample/act_sample_main.cc, its own main, run directly) and held to the Python restatement
(tests/act_sample_ref.py) on 15 seeded cases: A = 21, 31, 49 times tau = 1e-6, 0.25, 1, 4, 1e6, ROWS rows each, their legal masks with
0, 1, some and all actions legal, |z| < 8 on three rows of four and up to 10240 on the fourth.

The integer outputs (hh, hs, the keyed hs, the two 24-bit uniforms, the exploration branch) must match line for line; the picked actions
are held to the boundary rule of act_sample_ref with MARGIN = 1e-5, and at most 1 % of the sampled rows may fall under its excuse -- a
count that depends on the reference and u alone and is checked on its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import act_sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "act_sample", "act_sample_main.cc")
INC = os.path.join(ROOT, "hanabi_sad_amd", "csrc")
ROWS = 1106          # 15 cases x 1106 rows = 16,590 rows, each sampled twice (unkeyed and keyed uniform)
AS = (21, 31, 49)


def test_the_header_exists_and_names_the_clone_loss():
    text = open(os.path.join(INC, "hsad_act_sample.h")).read()
    assert "clone_tail_kernel" in text and "as_pick" in text


def test_the_hash_is_a_uniform_source():
    """65,536 rows of one seed and counter: the counts of u in 21 equal bins stay within 5 standard deviations, unkeyed and keyed"""
    seed, counter, sample_seed = 0x1234ABCD, 77, 0xFEED5
    us = [R.u24(R.sample_hash(R.eps_hash(seed, m, counter))) / 16777216.0 for m in range(65536)]
    uk = [R.u24(R.sample_hash_keyed(sample_seed, m * 7 - 1000)) / 16777216.0 for m in range(65536)]
    ue = [R.u24(R.eps_hash(seed, m, counter)) / 16777216.0 for m in range(65536)]
    for name, u in (("sample", us), ("keyed", uk), ("eps", ue)):
        s = R.bin_sigma(u)
        print("bins of the %s uniform: worst %.2f standard deviations" % (name, s))
        assert s < 5.0
    # the sample draw is not the exploration draw again
    assert np.corrcoef(us, ue)[0, 1] ** 2 < 1e-3


def test_the_excuse_is_rare_in_the_seeded_cases():
    """a property of the reference and u alone: at MARGIN, at most 1 % of the sampled rows lie within the margin of a boundary"""
    near = total = 0
    for c in range(15):
        k = R.seeded_case(c, AS[c // 5], ROWS)
        tau = R.TAUS[c % 5]
        for i in range(ROWS):
            hh = R.eps_hash(k["seed"], i, k["counter"])
            for hs in (R.sample_hash(hh), R.sample_hash_keyed(k["sample_seed"], int(k["key"][i]))):
                _, idx, cdf = R.pick(k["z"][i], k["legal"][i], tau, R.u24(hs) / 16777216.0)
                if len(idx) > 1:
                    total += 1
                    near += bool(np.abs(cdf[:-1] - R.u24(hs) / 16777216.0).min() <= R.MARGIN)
    print("%d of %d sampled rows lie within %g of a boundary" % (near, total, R.MARGIN))
    assert total > 20000 and near <= total // 100


@pytest.fixture(scope="module")
def program_lines(tmp_path_factory):
    """the program's output, one list of lines per case: [the "case" line, ROWS "row" lines, ROWS + 3 "tail" lines]"""
    exe = str(tmp_path_factory.mktemp("act_sample") / "act_sample_main")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", INC, SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, str(ROWS)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    lines = run.stdout.splitlines()
    per = 1 + ROWS + ROWS + 3
    assert lines[-1] == "OK" and len(lines) == 15 * per + 1
    return [lines[c * per:(c + 1) * per] for c in range(15)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_header_equals_the_restatement_under_asan_and_ubsan(program_lines):
    at, excused, sampled = 0, 0, 0
    seen = {0: 0, 1: 0, "all": 0}
    for c in range(15):
        A, tau = AS[c // 5], R.TAUS[c % 5]
        k = R.seeded_case(c, A, ROWS)
        lines, at = program_lines[c], 1
        assert lines[0] == "case %d %d" % (c, A)
        for i in range(ROWS):
            z, legal = k["z"][i], k["legal"][i]
            nlegal = int((legal != 0).sum())
            for n in (0, 1):
                seen[n] += nlegal == n
            seen["all"] += nlegal == A
            hh = R.eps_hash(k["seed"], i, k["counter"])
            hs, hsk = R.sample_hash(hh), R.sample_hash_keyed(k["sample_seed"], int(k["key"][i]))
            want = "row %d %d %d %d %d %d %d" % (i, hh, hs, hsk, R.u24(hs), R.u24(hsk), R.eps_draw(hh, k["eps"][i], nlegal))
            head, a, ak = lines[at].rsplit(" ", 2)
            assert head == want, "case %d: the header printed %r, the restatement %r" % (c, head, want)
            at += 1
            for got, h in ((int(a), hs), (int(ak), hsk)):
                if nlegal == 0:
                    assert got == -1
                    continue
                assert 0 <= got < A and legal[got] != 0, "case %d row %d: action %d is not legal" % (c, i, got)
                if nlegal > 1:
                    sampled += 1
                    excused += R.judge(got, z, legal, tau, R.u24(h) / 16777216.0) == "excused"
                else:
                    assert got == int(np.nonzero(legal)[0][0])
    print("%d of %d sampled rows fell under the boundary excuse" % (excused, sampled))
    assert excused <= sampled // 100
    assert min(seen.values()) > 100, seen


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_tail_row_equals_the_restatement(program_lines):
    """as_tail_row and as_q_at on the rows of act_sample_ref.tail_case (15 cases x (ROWS seeded rows + no / one / all legal)), each row
    without a temperature, at the case's tau with the unkeyed draw and with the keyed one.  greedy is exact on every row; a is exact
    without a temperature and wherever the exploration draw fires (the eps-greedy row); a sampled a is a legal action under the boundary
    rule (MARGIN, at most 1 % excused); qa at the action the program took and as_q_at at greedy equal the fp32 restatement bit for bit."""
    excused = sampled = fired = 0
    for c in range(15):
        A, tau = AS[c // 5], R.TAUS[c % 5]
        k = R.tail_case(c, A, ROWS)
        h, lg, n = k["h"], k["legal"], ROWS + 3
        got = np.array([[int(x) for x in line.split()[1:]] for line in program_lines[c][1 + ROWS:]], dtype=np.int64)
        assert program_lines[c][1 + ROWS].startswith("tail 0 ") and got.shape == (n, 9) and np.array_equal(got[:, 0], np.arange(n))
        greedy, a0, fires, nlegal = R.tail_row(h, lg, k["mn"], k["eps"], 0, k["seed"], k["counter"])
        assert np.array_equal(got[:, 1], greedy), "case %d: greedy differs on rows %s" % (c, np.nonzero(got[:, 1] != greedy)[0][:8])
        assert np.array_equal(got[:, 2], a0), "case %d: a without a temperature differs on rows %s" % (c, np.nonzero(got[:, 2] != a0)[0][:8])
        assert list(nlegal[ROWS:]) == [0, 1, A] and np.array_equal(got[ROWS:, 2][~fires[ROWS:]], greedy[ROWS:][~fires[ROWS:]])
        fired += int(fires.sum())
        for col, keyed in ((4, False), (6, True)):
            a = got[:, col]
            still = fires | (nlegal == 0)              # rows the temperature does not reach: the exploration draw, or nothing to sample
            assert np.array_equal(a[still], a0[still]), "case %d: a at tau %g differs where no sample is drawn" % (c, tau)
            for i in np.nonzero(~still)[0]:
                assert lg[i, a[i]] != 0, "case %d row %d: action %d is not legal" % (c, i, a[i])
                hh = R.eps_hash(k["seed"], int(i), k["counter"])
                hs = R.sample_hash_keyed(k["sample_seed"], int(k["key"][i])) if keyed else R.sample_hash(hh)
                if nlegal[i] > 1:
                    sampled += 1
                    excused += R.judge(int(a[i]), h[i, :A], lg[i], tau, R.u24(hs) / 16777216.0) == "excused"
                else:
                    assert a[i] == np.nonzero(lg[i])[0][0]
        for col, act in ((3, got[:, 2]), (5, got[:, 4]), (7, got[:, 6]), (8, greedy)):
            want = R.q_at(h, lg, act).view(np.uint32).astype(np.int64)
            bad = np.nonzero(got[:, col] != want)[0]
            assert len(bad) == 0, "case %d column %d: Q bits differ on rows %s" % (c, col, bad[:8])
    print("%d rows explored; %d of %d sampled rows fell under the boundary excuse" % (fired, excused, sampled))
    assert fired > 1000 and sampled > 20000 and excused <= sampled // 100
