"""Depth-limited search without a GPU:
  - hanabi_sad_amd/csrc/hsad_search_horizon.h, compiled on its own with g++ -fsanitize=address,undefined (the sanitizers' runtimes
    linked statically: the program needs nothing loaded before it) into tests/search_horizon/horizon_main.cc, held word for word to the
    numpy restatement tests/search_horizon_ref.py on generated rows;
  - SearchValues in fixed point (scale = 256) on CPU tensors, and scale = 1 equal to the expressions it has always had, bit for bit;
  - the ValueErrors of PolicySearch / policy_action_values / play_with_search / search(rounds=...) with no device present;
  - the usage errors of eval_model --search_depth and clone --search_depth;
  - the header, the ctypes table and the Python surface carry the entry point."""
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import search_horizon_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "hanabi_sad_amd", "csrc")]
SRC = os.path.join(ROOT, "tests", "search_horizon", "horizon_main.cc")
f32 = np.float32


# ---- the header under the sanitizers --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("search_horizon") / "horizon_main")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", INC[0], "-I", INC[1], SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def misc_word(num_step, term, started, last_score):
    return (num_step & 255) | (int(term) << 14) | (int(started) << 15) | (((last_score + 1) & 63) << 16) | (2 << 22)   # la_n: ignored


def board_word(fw, info=5, life=2):
    w = 0
    for c, f in enumerate(fw):
        w |= (f & 7) << (3 * c)
    return w | (info << 15) | (life << 19) | (1 << 24)


def special_q():
    """the fp32 values the rounding, the clamp and the finiteness test turn on"""
    ties = [k / 512.0 for k in range(-9, 10)] + [64.0 - 1 / 512.0, -64.0 + 1 / 512.0, 63.998046875, 12.001953125, -3.998046875]
    wide = [64.0, -64.0, 64.001, -64.001, 65.0, 1e9, -1e30, 3e38, -3e38]
    odd = [float("nan"), float("inf"), float("-inf"), -0.0, 1e-40, -1e-40]
    return [f32(x) for x in ties + wide + odd]


def make_cases():
    rng = np.random.default_rng(20)
    cases = []     # (misc, board, P, perfect, mode, q[5], fields for the reference)

    def add(P, perfect, mode, state, num_step, last_score, fw, q):
        started, term = state != "fresh", state == "finished"
        q5 = np.zeros(5, dtype=f32)
        q5[:P] = q
        q5[P:] = f32("nan")           # beyond the game's seats: must never be read
        cases.append(dict(misc=misc_word(num_step, term, started, last_score), board=board_word(fw), P=P, perfect=perfect, mode=mode, q=q5,
                          started=started, finished=started and term, last=last_score, fws=int(sum(fw)), step=num_step))

    for P in (2, 3, 5):
        for perfect, top in ((10, (5, 5, 0, 0, 0)), (12, (4, 4, 4, 0, 0)), (25, (5, 5, 5, 5, 5))):
            for mode in (R.MOVER, R.TEAM):
                for x in special_q():
                    for fw in ((0, 0, 0, 0, 0), top, (1, 2, 0, 0, 0)):     # the clamp at 0, at the perfect score, neither
                        step = int(rng.integers(0, 60))
                        q = rng.standard_normal(P).astype(f32)
                        if mode == R.MOVER:
                            q[step % P] = x
                        else:
                            q[:] = 0
                            q[int(rng.integers(0, P))] = x
                        add(P, perfect, mode, "live", step, -1, fw, q)
                # random rows in every state
                for _ in range(40):
                    state = ("live", "finished", "fresh")[int(rng.integers(0, 3))]
                    fw = rng.integers(0, 3, size=5)
                    add(P, perfect, mode, state, int(rng.integers(0, 256)), int(rng.integers(0, perfect + 1)), fw,
                        (rng.standard_normal(P) * 20).astype(f32))
                # a finished game's Q is not looked at, whatever it holds; neither is a fresh one's
                add(P, perfect, mode, "finished", 40, perfect, top, np.full(P, f32("nan")))
                add(P, perfect, mode, "finished", 7, 0, (0, 0, 0, 0, 0), np.full(P, f32("inf")))
                add(P, perfect, mode, "fresh", 0, -1, (0, 0, 0, 0, 0), np.full(P, f32("nan")))
        # the team sum is taken in seat order, one fp32 rounding per addition
        big = [f32(1e8), f32(1.0), f32(-1e8), f32(1.0), f32(1.0)][:P]
        add(P, 25, R.TEAM, "live", 3, -1, (1, 1, 0, 0, 0), np.asarray(big, dtype=f32))
        add(P, 25, R.TEAM, "live", 3, -1, (1, 1, 0, 0, 0), np.asarray(big[::-1], dtype=f32))
        add(P, 25, R.TEAM, "live", 3, -1, (1, 1, 0, 0, 0), np.asarray([f32(3e38)] * P, dtype=f32))                  # finite rows, infinite sum
        add(P, 25, R.TEAM, "live", 3, -1, (1, 1, 0, 0, 0), np.asarray([f32("inf"), f32("-inf")] + [f32(0)] * (P - 2), dtype=f32))
        add(P, 25, R.TEAM, "live", 3, -1, (1, 1, 0, 0, 0), np.asarray([f32(0.001953125)] * P, dtype=f32))            # ties made by the sum
    return cases


def reference(cases):
    out = []
    for c in cases:
        v, counted, cut, bad = R.slot_values([c["started"]], [c["finished"]], [c["last"]], [c["fws"]], [c["step"]], c["q"][None, :c["P"]],
                                             c["mode"], c["perfect"])
        out.append((int(v[0]) if counted[0] else 0, int(counted[0]), int(cut[0]), int(bad[0])))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_header_equals_the_restatement_under_asan_and_ubsan(program, tmp_path):
    cases = make_cases()
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for c in cases:
            fh.write(struct.pack("<IIiii", c["misc"], c["board"], c["P"], c["perfect"], c["mode"]) + c["q"].astype("<f4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program, path], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK" and len(lines) == len(cases) + 1
    got = [tuple(int(x) for x in l.split()) for l in lines[:-1]]
    want = reference(cases)
    wrong = [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong, wrong[:10]
    # every class of row occurred
    w = np.asarray(want)
    live = (w[:, 1] == 1) & (w[:, 2] == 1)
    assert (w[:, 1] == 0).sum() > 10 and ((w[:, 1] == 1) & (w[:, 2] == 0)).sum() > 10 and live.sum() > 100 and (w[:, 3] == 1).sum() > 20
    perfect = np.asarray([c["perfect"] for c in cases])
    fws = np.asarray([c["fws"] for c in cases])
    assert (live & (w[:, 0] == 0) & (fws == 0)).any() and (live & (w[:, 0] == perfect * 256) & (fws == perfect)).any()      # both clamps
    assert (live & (w[:, 0] % 256 != 0)).any()
    print("%d rows: %d live, %d finished, %d not started, %d with a Q that is not finite" % (len(cases), live.sum(),
          ((w[:, 1] == 1) & (w[:, 2] == 0)).sum(), (w[:, 1] == 0).sum(), (w[:, 3] == 1).sum()))


def test_the_restatement_rounds_half_to_even_and_clamps():
    b, bad = R.bootstrap([f32(k / 512.0) for k in (1, 3, 5, -1, -3, -5)] + [f32(64.5), f32(-1e30), f32("nan"), f32("inf"), f32("-inf")])
    assert b.tolist() == [0, 2, 2, 0, -2, -2, 16384, -16384, 0, 0, 0] and bad.tolist() == [False] * 8 + [True] * 3
    assert R.team_q(np.asarray([[1e8, 1.0, -1e8]], dtype=f32))[0] == 0.0 and R.team_q(np.asarray([[-1e8, 1e8, 1.0]], dtype=f32))[0] == 1.0
    v, counted, cut, nf = R.slot_values([1, 1, 0, 1], [0, 1, 0, 0], [-1, 7, -1, -1], [3, 9, 0, 24], [5, 9, 0, 2],
                                        np.asarray([[9.0, 1.25], [50.0, 50.0], [1.0, 1.0], [4.0, float("nan")]], dtype=f32), R.MOVER, 25)
    assert v.tolist() == [3 * 256 + 320, 7 * 256, 0, 25 * 256] and counted.tolist() == [True, True, False, True]
    assert cut.tolist() == [True, False, False, True] and nf.tolist() == [False] * 4


# ---- SearchValues ---------------------------------------------------------------------------------------------------------------------
def test_search_values_in_fixed_point_and_unchanged_at_scale_one():
    from hanabi_sad_amd.search import SearchValues
    rng = np.random.default_rng(4)
    n = rng.integers(0, 9, size=(5, 7))
    n[0, 0], n[1, 1] = 0, 1
    v = rng.integers(0, 25 * 256 + 1, size=(5, 7, 8))
    mask = np.arange(8)[None, None, :] < n[..., None]
    s, sq = (v * mask).sum(-1), (v * v * mask).sum(-1)
    totals = torch.from_numpy(np.stack([s, sq, n], axis=-1).astype(np.int64))
    bp = torch.zeros(5, dtype=torch.int64)
    cut = torch.from_numpy(n // 2)
    sv = SearchValues(totals, bp, scale=256, cut=cut, nonfinite=3)
    assert sv.scale == 256 and sv.nonfinite == 3 and torch.equal(sv.cut, cut) and sv.world_values is None and torch.equal(sv.totals, totals)
    with np.errstate(all="ignore"):
        nd = np.where(n > 0, n, 1).astype(np.float64)
        mean = np.where(n > 0, (s.astype(np.float64) / nd / 256).astype(f32), f32("nan"))
        var_n2 = np.maximum(nd.astype(np.int64) * sq - s * s, 0).astype(np.float64)
        sem = np.where(n > 0, (np.sqrt(var_n2) / nd / np.sqrt(nd) / 256).astype(f32), f32("nan"))
    assert sv.values.dtype == torch.float32 and sv.sem.dtype == torch.float32
    assert np.array_equal(sv.values.numpy(), mean, equal_nan=True) and np.array_equal(sv.sem.numpy(), sem, equal_nan=True)
    assert bool(torch.isnan(sv.values[0, 0])) and float(sv.sem[1, 1]) == 0.0
    # whole scores times 256 give the same means as the scores themselves, exactly where the mean is a float32
    whole = torch.tensor([[[3 * 256 + 5 * 256, (3 * 256) ** 2 + (5 * 256) ** 2, 2]]])
    assert float(SearchValues(whole, bp[:1], scale=256).values[0, 0]) == 4.0 and float(SearchValues(whole, bp[:1], scale=256).sem[0, 0]) == f32(1 / np.sqrt(2))
    # scale = 1, the default: the expressions SearchValues has always had
    small = torch.from_numpy(np.stack([s // 256, (sq // 65536), n], axis=-1).astype(np.int64))
    one = SearchValues(small, bp)
    assert one.scale == 1 and one.cut is None and one.nonfinite == 0 and one.world_values is None
    t0, t1, t2 = small[..., 0], small[..., 1], small[..., 2]
    counted = t2 > 0
    nf = torch.where(counted, t2, torch.ones_like(t2))
    nan = torch.full(t0.shape, float("nan"), dtype=torch.float32)
    old_values = torch.where(counted, t0.to(torch.float32) / nf.to(torch.float32), nan)
    old_sem = torch.where(counted, (torch.sqrt((nf * t1 - t0 * t0).clamp(min=0).to(torch.float64)) / nf.to(torch.float64)
                                    / torch.sqrt(nf.to(torch.float64))).to(torch.float32), nan)
    for got, want in ((one.values, old_values), (one.sem, old_sem), (SearchValues(small, bp, scale=1).values, old_values)):
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got).view(torch.int32), torch.nan_to_num(want).view(torch.int32))
    with pytest.raises(ValueError):
        SearchValues(small, bp, scale=0)


# ---- the refusals, with no device present ---------------------------------------------------------------------------------------------
def fake_agent(skip=False):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    return NS(online=NS(H=64, L=2, skip=skip), get_h0=boom, act=boom)


def fake_env():
    class Env:
        def __getattr__(self, name):
            raise AssertionError("the env was touched (%s)" % name)
    return Env()


BAD_DEPTHS = [-1, 200, 10 ** 6, 1.0, 2.5, "2", True, (2,)]       # max_steps = 200: depth must lie in [0, 200)


def test_policy_search_refuses_before_any_device_work(monkeypatch):
    from hanabi_sad_amd import search

    def boom(*a, **k):
        raise AssertionError("an env was built")
    monkeypatch.setattr(search, "BatchedHanabiEnv", boom)
    hid = {"h0": None, "c0": None}
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError, match="depth"):
            search.PolicySearch(fake_env(), fake_agent(), 64, depth=bad)
        with pytest.raises(ValueError, match="depth"):
            search.policy_action_values(fake_env(), fake_agent(), hid, 4, 0, capacity=64, depth=bad)
        with pytest.raises(ValueError, match="depth"):
            search.play_with_search(fake_agent(), 2, 1, 0, False, worlds=2, depth=bad)
    with pytest.raises(ValueError, match="depth"):
        search.PolicySearch(fake_env(), fake_agent(), 64, max_steps=5, depth=5)
    for kw in (dict(depth=2, horizon_value="sum"), dict(depth=None, horizon_value="q"), dict(depth=0, horizon_value=None)):
        with pytest.raises(ValueError, match="horizon_value"):
            search.PolicySearch(fake_env(), fake_agent(), 64, **kw)
        with pytest.raises(ValueError, match="horizon_value"):
            search.policy_action_values(fake_env(), fake_agent(), hid, 4, 0, **kw)
        with pytest.raises(ValueError, match="horizon_value"):
            search.play_with_search(fake_agent(), 2, 1, 0, False, worlds=2, **kw)
    for fn in (lambda: search.PolicySearch(fake_env(), fake_agent(skip=True), 64, depth=2),
               lambda: search.policy_action_values(fake_env(), fake_agent(skip=True), hid, 4, 0, depth=0, horizon_value="team"),
               lambda: search.play_with_search(fake_agent(skip=True), 2, 1, 0, False, worlds=2, depth=2)):
        with pytest.raises(ValueError, match="skip_connect"):
            fn()
    # a search in rounds does not combine with a depth
    ps = search.PolicySearch.__new__(search.PolicySearch)
    ps.depth = 2
    with pytest.raises(ValueError, match="out of scope"):
        ps.search(fake_env(), hid, 4, 0, rounds=(2, 2))
    with pytest.raises(ValueError, match="out of scope"):
        search.play_with_search(fake_agent(), 2, 1, 0, False, worlds=4, rounds=(2, 2), depth=2)


def test_the_commands_refuse_a_bad_search_depth():
    from hanabi_sad_amd import clone, eval_model
    op = ["--paper", "op", "--method", "sad", "--idx", "0", "--root", "nowhere"]
    with pytest.raises(SystemExit, match="--search_depth needs --search_worlds"):
        eval_model.main(op + ["--search_depth", "2"])
    with pytest.raises(SystemExit, match="do not combine"):
        eval_model.main(op + ["--search_worlds", "4", "--search_rounds", "2,2", "--search_depth", "2"])
    with pytest.raises(SystemExit, match="must not be negative"):
        eval_model.main(op + ["--search_worlds", "4", "--search_depth", "-1"])
    with pytest.raises(SystemExit):      # argparse: no such horizon value
        eval_model.main(op + ["--search_worlds", "4", "--search_depth", "1", "--search_horizon_value", "sum"])
    args = eval_model.parse_args(op + ["--search_worlds", "4"])
    assert args.search_depth is None and args.search_horizon_value == "mover"
    assert eval_model.parse_args(op + ["--search_depth", "3", "--search_horizon_value", "team"]).search_horizon_value == "team"
    bp = ["--blueprint", "nothing.pthw"]
    with pytest.raises(SystemExit, match="--search_depth needs --blueprint"):
        clone.main(bp + ["--search_depth", "2"])
    with pytest.raises(SystemExit, match="--search_depth needs --blueprint"):
        clone.main(["--teacher", "piers", "--search_worlds", "4", "--search_depth", "2"])
    with pytest.raises(SystemExit, match="do not combine"):
        clone.main(bp + ["--search_worlds", "4", "--search_rounds", "2,2", "--search_depth", "2"])
    with pytest.raises(SystemExit, match="must not be negative"):
        clone.main(bp + ["--search_worlds", "4", "--search_depth", "-3"])
    with pytest.raises(SystemExit, match="no such weight file"):      # a good depth goes on to the next check
        clone.main(bp + ["--search_worlds", "4", "--search_depth", "2"])
    args = clone.parse_args(["--teacher", "piers"])
    assert args.search_depth is None and args.search_horizon_value == "mover"


def test_header_ctypes_table_and_surface_carry_the_entry_point():
    from hanabi_sad_amd import _lib, search
    want = ("int hsad_search_horizon_stats(const hsad_env* env, const int32_t* job, int n_job, const float* q_rows, int mode, int64_t* stats, "
            "int64_t* cut, int64_t* nonfinite, const int32_t* world, int worlds, uint16_t* world_values, void* stream);")
    raw = open(os.path.join(ROOT, "include", "hsad.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    found = re.findall(r"\bint\s+hsad_search_horizon_stats\s*\([^;]*\);", txt)
    assert len(found) == 1 and re.sub(r"\s+", " ", found[0]) == want
    assert re.search(r"#define\s+HSAD_SEARCH_VALUE_SCALE\s+256\b", raw) and search.VALUE_SCALE == R.SCALE == 256
    assert re.search(r"HSAD_SEARCH_HORIZON_MOVER\s*=\s*0\s*,\s*HSAD_SEARCH_HORIZON_TEAM\s*=\s*1", raw)
    assert search.HORIZON_VALUES == ("mover", "team") and (R.MOVER, R.TEAM) == (0, 1)
    restype, argtypes = _lib.SIGNATURES["hsad_search_horizon_stats"]
    args = want[want.index("(") + 1:want.rindex(")")].split(", ")
    assert restype is C.c_int and argtypes == [C.c_void_p if "*" in a else C.c_int for a in args]
    for fn in (search.PolicySearch.__init__, search.policy_action_values, search.play_with_search):
        p = inspect.signature(fn).parameters
        assert p["depth"].default is None and p["horizon_value"].default == "mover", fn
    for fn in (search.PolicySearch.search, search.policy_action_values):
        assert inspect.signature(fn).parameters["keep_world_values"].default is False
    assert "hsad_search_horizon_stats" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
