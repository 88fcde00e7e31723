"""CPU: hanabi_sad_amd/csrc/hsad_hand_count.h -- the integer core of hsad_env_hand_belief and hsad_env_determinize_exact -- compiled
on its own with `g++ -fsanitize=address,undefined` (the sanitizers' runtimes linked statically: the program needs nothing loaded before it) into a stand-alone program (tests/hand_count/hand_count_main.cc, its own main,
run directly) and compared, line for line, with the Python restatement (tests/hand_belief_ref.py) on 60 seeded cases.

Both sides make case c = 0 .. 59 from the same generator:
    x_0 = (c + 1) * 0x9E3779B97F4A7C15 mod 2^64;   raw(): x <- x * 6364136223846793005 + 1442695040888963407 mod 2^64, returns x;
    next() = raw() >> 33;
    n = 1 + next() % 5;   pool[t] = next() % (full[t] + 1) for t = 0 .. 24, full[t] = 3, 2, 2, 2, 1 by rank t % 5;
    per slot i < n: colour mask = 1 + next() % 31, then rank mask = 1 + next() % 31;   fireworks[c] = next() % 6 for the 5 colours;
    W = 1 + next() % 40;   u64 = raw().
Printed per case: N; per slot num[i][0..24] and the trinary sums; unrank(r) (hand and the pool left) for every r when N <= 400, else
for r = floor(j N / 17), j = 0 .. 16, and N - 1; unrank(N) and unrank(-1), which must be refused; the stratified ranks of all W strata
for the uniform u64."""
import os
import shutil
import subprocess

import pytest

from tests import hand_belief_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hand_count", "hand_count_main.cc")
INC = os.path.join(ROOT, "hanabi_sad_amd", "csrc")
CASES = 60


def expected_lines():
    out = []
    for c in range(CASES):
        k = B.seeded_case(c)
        pool, cms, n = k["pool"], k["cms"], k["n"]
        N = B.total_of(pool, cms)
        out.append("case %d %d %d" % (c, n, N))
        num = B.marginals(pool, cms)
        tri = B.trinary(num, k["fireworks"])
        for i in range(n):
            out.append("num %d %s" % (i, " ".join(str(v) for v in num[i])))
            out.append("tri %d %d %d %d" % (i, tri[i][0], tri[i][1], tri[i][2]))
        ranks = list(range(N)) if N <= 400 else [N - 1 if j == 17 else (j * N) // 17 for j in range(18)]
        for r in ranks:
            cards, q = B.unrank(pool, cms, r)
            out.append("unrank %d 1 : %s | %s" % (r, " ".join(str(t) for t in cards), " ".join(str(v) for v in q)))
        out.append("unrank %d 0 :" % N)
        out.append("unrank -1 0 :")
        out.append("strata %d %d : %s" % (k["W"], k["u64"], " ".join(str(B.rank_from_u64(N, w, k["W"], k["u64"])) for w in range(k["W"]))))
    out.append("OK")
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_header_equals_the_restatement_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "hand_count_main")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", INC, SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, str(CASES)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    got, want = run.stdout.splitlines(), expected_lines()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "line %d: the header printed %r, the restatement %r" % (i, a, b)
    assert len(got) == len(want)
