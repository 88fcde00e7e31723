"""CPU: the host-side planning of the split-K GEMM entry points and the struct that crosses their C ABI.

hanabi_sad_amd/csrc/hsad_gemm_plan.h -- how hsad_gemm_nt_bf16_group_splitk (the 256 x 256 core: an even number of k tiles per range) and
gemm_launch (hsad_gemm_nt_bf16_splitk[_acc]: ceil(k tiles / split_k) per range) cut a contraction into K ranges -- is compiled on its own
with `g++ -fsanitize=address,undefined` (runtimes linked statically) into a stand-alone program (tests/gemm_plan/gemm_plan_main.cc, its own
main, run directly) and compared, line for line, with the Python restatement in tests/gemm_group.py for every K = 128 j, j = 1 .. 160, and
split_k = 1 .. 16.  The restatement is then held to what the launches rely on.

hsad_gemm_group_item: a few lines of C against include/hsad.h print the compiler's sizeof / offsetof, compared with the ctypes mirror that
every GPU case of tests/test_gemm_group_gpu.py passes its pointers through."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests import gemm_group as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_plan", "gemm_plan_main.cc")
LAYOUT_SRC = os.path.join(ROOT, "tests", "gemm_plan", "group_item_layout.c")
INC = os.path.join(ROOT, "hanabi_sad_amd", "csrc")
J_MAX, SPLIT_MAX = 160, 16
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")


def item_shape(j, s):
    return 256 * (1 + j % 3), 4 * (1 + (j + s) % 7)


def expected_lines():
    out = []
    for j in range(1, J_MAX + 1):
        for s in range(1, SPLIT_MAX + 1):
            K = 128 * j
            c, p = G.core_plan(K, s), G.plain_plan(K, s)
            h = G.plan_with_chunk(K, c[0])
            M, N = item_shape(j, s)
            out.append("plan %d %d | core %d %d %d | plain %d %d %d | handed %d %d %d | floats %d" % ((K, s) + c + p + h + (G.workspace_floats([(M, N, K, s)]),)))
    out.append("refused 0 0 0")
    out.append("OK")
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_plan_header_equals_the_restatement_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "gemm_plan_main")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + SAN + ["-I", INC, SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe, str(J_MAX), str(SPLIT_MAX)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **SAN_ENV))
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    got, want = run.stdout.splitlines(), expected_lines()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "line %d: the header printed %r, the restatement %r" % (i, a, b)
    assert len(got) == len(want) == J_MAX * SPLIT_MAX + 2


def test_what_the_launches_rely_on_holds_for_every_k_and_split():
    """Every core range is an even number of k tiles (the 256 x 256 kernel's k loop takes two per trip), both plans tile [0, K) exactly,
    the two plans agree on the COUNT of ranges when gemm_launch is asked for the core's count (the grouped entry point's HSAD_ERR_STATE
    check) though not on the ranges, which is why the fallback hands the range length over; that length reproduces the core's plan; and the
    workspace is the sum over the items of count x M x N."""
    differ = 0
    for j in range(1, J_MAX + 1):
        for s in range(1, SPLIT_MAX + 1):
            K = 128 * j
            nk = K // 64
            chunk, count, last = G.core_plan(K, s)
            assert chunk % 2 == 0 and chunk >= 2 and last % 2 == 0 and 2 <= last <= chunk, (K, s)
            assert 1 <= count <= s and (count - 1) * chunk + last == nk, (K, s)
            assert (count - 1) * chunk < nk <= count * chunk, (K, s)
            pc, pn, pl = G.plain_plan(K, s)
            assert 1 <= pl <= pc and 1 <= pn <= s and (pn - 1) * pc + pl == nk, (K, s)
            # gemm_launch asked for `count` ranges: as many as planned ...
            qc, qn, ql = G.plain_plan(K, count)
            assert qn == count, (K, s, qn, count)
            differ += (qc, ql) != (chunk, last)            # ... but not always the same ranges (K = 1280, split 3: 7 7 6 against 8 8 4)
            assert G.plan_with_chunk(K, chunk) == (chunk, count, last)
    assert G.core_plan(1280, 3) == (8, 3, 4) and G.plain_plan(1280, 3) == (7, 3, 6) and differ > 0
    assert G.core_plan(640, 4) == (4, 3, 2) and G.core_plan(10240, 3) == (54, 3, 52) and G.core_plan(128, 8) == (2, 1, 2) and G.core_plan(2560, 8) == (6, 7, 4)
    shapes = [(2048, 512, 10240, 3)] * 4 + [(512, 896, 10240, 8)]
    assert G.workspace_floats(shapes) == 4 * 3 * 2048 * 512 + G.core_plan(10240, 8)[1] * 512 * 896
    assert G.workspace_floats(shapes) == sum(G.core_plan(K, s)[1] * M * N for M, N, K, s in shapes)


def test_the_tile_order_rule_restated():
    """tests/gemm_group.tile_orders (g8_launch's rule) on the launches tests/test_gemm_group_gpu.py names, for a chip of 256 CUs"""
    assert G.tile_orders([(2048, 256, 1024, 8)], 256) == [1] and G.work_items([(2048, 256, 1024, 8)]) == [64]
    assert G.tile_orders([(256, 64, 768, 3), (2048, 256, 1024, 8)], 256) == [0, 0] and G.work_items([(256, 64, 768, 3)]) == [3]
    assert G.tile_orders([(8192, 2048, 128, 1)], 256) == [2] and G.work_items([(8192, 2048, 128, 1)]) == [256]
    assert G.tile_orders([(256, 4, 128, 1)], 256) == [0] and G.launch_grid([(256, 4, 128, 1)], 256) == 1


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_group_item_struct_is_laid_out_as_its_ctypes_mirror(tmp_path):
    exe = str(tmp_path / "group_item_layout")
    cmd = ["gcc", "-std=c11", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + SAN + ["-I", os.path.join(ROOT, "include"), LAYOUT_SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, **SAN_ENV))
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    lines = run.stdout.split("\n")
    assert lines[0] == "sizeof %d" % C.sizeof(G.GroupItem)
    got = [tuple(ln.split()) for ln in lines[1:] if ln]
    want = [(name, str(getattr(G.GroupItem, name).offset), str(getattr(G.GroupItem, name).size)) for name, _ in G.GroupItem._fields_]
    assert got == want
    # the header's own field list, in order (a field added in a padding hole would leave sizeof unchanged)
    text = open(os.path.join(ROOT, "include", "hsad.h")).read()
    body = re.search(r"typedef struct hsad_gemm_group_item \{(.*?)\} hsad_gemm_group_item;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            names += [re.sub(r"[\s*]", "", part.split()[-1]) for part in decl.split(",")]
    assert names == [name for name, _ in G.GroupItem._fields_]
    # pointers are pointers, the rest int32_t
    for name, tp in G.GroupItem._fields_:
        assert tp is (C.c_void_p if name in ("A", "B", "C", "row_map") else C.c_int32)
