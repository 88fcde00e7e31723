"""hsad_belief_tail (csrc/r2d2/belief_tail.inc) called directly through ctypes and held to the float64 reference of
tests/belief_head_ref.py, in the style of tests/test_clone_soft_kernel_gpu.py: every buffer between two guard bands, the cases of
the sibling tails (T = 1, 5, 97, 130 with B = 1 and 3: a single step, fewer steps than waves, trip counts that are no multiple of the
eight waves) for hands of 5, 4 and 2 slots and logits rows both tight and padded, random seq_len.  The integer outputs equal the
reference; nll, nll0 and dlogits stay within the per-row bounds the reference derives from the operation count and the bf16
rounding of the gradient (tests/belief_head_ref.py, module docstring); rows that must be zero are compared as bits; bad rows are
counted and contribute nothing; no input is written; a refused call touches no output."""
import numpy as np
import pytest
import torch

from tests import belief_head_ref as R
from tests.test_heads_loss_kernels_gpu import Pool, ok, p, untouched

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
CASES = [(1, 1), (5, 3), (97, 3), (130, 3)]
HANDS = [5, 4, 2]


@pytest.fixture(scope="module")
def lib():
    from hanabi_sad_amd import _lib
    return _lib.load_library()


@pytest.fixture(scope="module")
def st():
    from hanabi_sad_amd.r2d2 import _s
    return _s(torch.device(DEV))


@pytest.fixture(autouse=True)
def _end_the_session_after_a_device_fault():
    """a kernel that faulted leaves the context unusable: nothing more of this session may be started on the device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the device reported a fault: %s" % e, returncode=3)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


_CASES = {}


def case(T, B, Hs, bad_every):
    """the seeded inputs (tight rows) and their reference, computed once and never changed"""
    key = (T, B, Hs, bad_every)
    if key not in _CASES:
        c = R.tail_case(T, B, Hs, Hs * 25, seed=1000 * T + 10 * B + Hs, bad_every=bad_every)
        ref = R.tail(c["logits"], c["pool"], c["compat"], c["cards"], c["seq_len"], c["weight"], T, B, Hs, Hs * 25)
        _CASES[key] = (c, ref)
    return _CASES[key]


def with_ldz(c, ldz):
    """the same logits in rows of ldz columns; the padding is NaN -- the kernel must not read it"""
    M, n = c["logits"].shape
    z = np.full((M, ldz), np.nan, dtype=np.float32)
    z[:, :n] = c["logits"]
    return dict(c, logits=z)


def run(lib, st, c, T, B, Hs, ldz, ldo, grad=True):
    pool = Pool()
    d = {k: pool.put(torch.from_numpy(v)) for k, v in c.items()}
    out = dict(nll=pool.new(B), nll0=pool.new(B), cards_n=pool.new(B, torch.int32), hits=pool.new(B, torch.int32), hits0=pool.new(B, torch.int32),
               bad=pool.new(B, torch.int32), dlogits=pool.new((T * B, ldo), torch.bfloat16) if grad else None)
    ok(lib.hsad_belief_tail(p(d["logits"]), ldz, p(d["pool"]), p(d["compat"]), p(d["cards"]), p(d["seq_len"]), p(d["weight"]), T, B, Hs, p(out["nll"]),
                            p(out["nll0"]), p(out["cards_n"]), p(out["hits"]), p(out["hits0"]), p(out["bad"]), p(out["dlogits"]), ldo, st))
    pool.check()
    for k, v in d.items():
        assert torch.equal(bits(v), bits(torch.from_numpy(c[k]))), "input %s was written" % k
    return out


def hold(out, ref, T, B, Hs, ldo, what):
    for k in ("cards_n", "hits", "hits0", "bad"):
        assert out[k].cpu().long().tolist() == ref[k].tolist(), (what, k, out[k].cpu().tolist(), ref[k].tolist())
    for k in ("nll", "nll0"):
        err = np.abs(out[k].cpu().double().numpy() - ref[k])
        print("%s %s: largest error %.3e, the bound there %.3e" % (what, k, float(err.max()), float(ref["e_" + k][err.argmax()])))
        assert np.all(err <= ref["e_" + k]), (what, k, err.tolist(), ref["e_" + k].tolist())
    if out["dlogits"] is None:
        return
    got = out["dlogits"].float().cpu().double().numpy()
    n = Hs * 25
    want = np.zeros((T * B, ldo))
    want[:, :n] = ref["dlogits"][:, :n]
    e_d = np.zeros((T * B, ldo))
    e_d[:, :n] = ref["e_d"][:, :n]
    allowed = R.rne(want) + e_d * (1.0 + 2.0 ** -8)      # (the rounding to bf16 acts on the device's value, not the reference's)
    err = np.abs(got - want)
    print("%s dlogits: largest error beyond the bf16 rounding %.3e" % (what, float(np.clip(err - R.rne(want), 0, None).max())))
    assert np.all(err <= allowed), (what, float(err.max()), int(np.argmax(err - allowed)))
    raw = bits(out["dlogits"]).numpy()
    assert not raw[ref["zero_row"]].any(), what + ": a row that must be zero is not"
    assert not raw[:, n:].any(), what + ": the columns past the hand are not zero"
    assert not raw[:, :n][e_d[:, :n] == 0].any(), what + ": an infeasible column is not zero"      # (e_d is 0 exactly off the feasible sets)


@pytest.mark.parametrize("Hs", HANDS)
@pytest.mark.parametrize("T,B", CASES)
def test_against_float64(lib, st, T, B, Hs):
    c, ref = case(T, B, Hs, 0)
    assert not ref["bad"].any()
    n = Hs * 25
    for ldz, ldo in ((n, n), (n + 7, (n + 7) // 8 * 8)):
        out = run(lib, st, with_ldz(c, ldz), T, B, Hs, ldz, ldo)
        hold(out, ref, T, B, Hs, ldo, "T=%d B=%d Hs=%d ldz=%d" % (T, B, Hs, ldz))
        again = run(lib, st, with_ldz(c, ldz), T, B, Hs, ldz, ldo)
        for k in out:      # the same bits run to run
            assert torch.equal(bits(out[k]), bits(again[k])), k
        nograd = run(lib, st, with_ldz(c, ldz), T, B, Hs, ldz, ldo, grad=False)
        for k in ("nll", "nll0", "cards_n", "hits", "hits0", "bad"):
            assert torch.equal(bits(out[k]), bits(nograd[k])), k


@pytest.mark.parametrize("Hs", HANDS)
@pytest.mark.parametrize("T,B", [(5, 3), (97, 3)])
def test_bad_rows_are_counted_and_contribute_nothing(lib, st, T, B, Hs):
    c, ref = case(T, B, Hs, 7)
    assert int(ref["bad"].sum()) >= 1
    out = run(lib, st, c, T, B, Hs, Hs * 25, Hs * 25)
    hold(out, ref, T, B, Hs, Hs * 25, "bad rows T=%d B=%d Hs=%d" % (T, B, Hs))


@pytest.mark.parametrize("Hs", HANDS)
def test_zero_logits_score_the_exact_belief_bit_for_bit(lib, st, Hs):
    T, B = 5, 3
    c, _ = case(T, B, Hs, 0)
    c = dict(c, logits=np.zeros_like(c["logits"]))
    out = run(lib, st, c, T, B, Hs, Hs * 25, Hs * 25)
    assert torch.equal(bits(out["nll"]), bits(out["nll0"])) and float(out["nll0"].abs().sum()) > 0
    assert torch.equal(out["hits"].cpu(), out["hits0"].cpu())


def test_refused_calls_touch_no_output(lib, st):
    T, B, Hs = 5, 3, 5
    c, _ = case(T, B, Hs, 0)
    n = Hs * 25
    pool = Pool()
    d = {k: pool.put(torch.from_numpy(v)) for k, v in c.items()}
    o = dict(nll=pool.new(B), nll0=pool.new(B), cards_n=pool.new(B, torch.int32), hits=pool.new(B, torch.int32), hits0=pool.new(B, torch.int32),
             bad=pool.new(B, torch.int32), dlogits=pool.new((T * B, n), torch.bfloat16))

    def call(**kw):
        a = dict(logits=p(d["logits"]), ldz=n, pool=p(d["pool"]), compat=p(d["compat"]), cards=p(d["cards"]), seq_len=p(d["seq_len"]),
                 weight=p(d["weight"]), T=T, B=B, Hs=Hs, nll=p(o["nll"]), nll0=p(o["nll0"]), cards_n=p(o["cards_n"]), hits=p(o["hits"]),
                 hits0=p(o["hits0"]), bad=p(o["bad"]), dlogits=p(o["dlogits"]), ldo=n)
        a.update(kw)
        return lib.hsad_belief_tail(a["logits"], a["ldz"], a["pool"], a["compat"], a["cards"], a["seq_len"], a["weight"], a["T"], a["B"], a["Hs"],
                                    a["nll"], a["nll0"], a["cards_n"], a["hits"], a["hits0"], a["bad"], a["dlogits"], a["ldo"], st)

    refusals = [dict(logits=None), dict(pool=None), dict(compat=None), dict(cards=None), dict(seq_len=None), dict(nll=None), dict(nll0=None),
                dict(cards_n=None), dict(hits=None), dict(hits0=None), dict(bad=None), dict(T=0), dict(B=0), dict(Hs=0), dict(Hs=6), dict(ldz=n - 1),
                dict(weight=None), dict(ldo=n - 1), dict(T=9000)]
    for kw in refusals:
        assert call(**kw) == -1, kw
        assert len(lib.hsad_last_error()) > 0
    pool.check()
    for k, v in o.items():
        assert untouched(v), k
    assert call() == 0
    torch.cuda.synchronize()
