"""hsad_clone_soft_tail (csrc/r2d2/clone_soft.inc, its row csrc/hsad_clone_soft.h) called directly through ctypes, in the way
tests/test_clone_value_kernel_gpu.py holds hsad_clone_value_tail: every buffer between two guard bands, the cases of
tests/clone_value_ref.py (logits and values on a dyadic grid: counters exact) plus T = 130 -- more steps than the block's 128 threads, so
the stride loop runs twice --, NaN returns and NaN targets on every row the kernel must not read, zero rows compared as bits.

(a) One-hot targets: every output has the BITS of hsad_clone_value_tail.
(b) Seeded soft targets against the float64 reference of tests/clone_soft_ref.py.  Tolerances: the loss gets, per decision, the measured
    tol("xent_step") of tests/test_clone_kernel_gpu.py (__expf / __logf) plus e_xent = 2 A 2^-24 max |z_j - mx|, the standard fp32
    summation bound of the extra dot product (A products, weights summing to at most 1.001); vloss keeps the derived bound of
    tests/test_clone_value_kernel_gpu.py; a dheads element one bf16 rounding of the float64 value plus
    s (policy_weight (1.001 tol("softmax") + 2^-22) + value_weight e_bound): sigma <= 1.001 scales the softmax error, and sigma p_j - pi_j
    adds a handful of fp32 roundings of numbers below 1.001.  The largest errors seen go to clone_measured_errors.json under
    "clone_soft_tail"; on an MI355X: loss 4.6e-6 per decision (9.3 % of its bound at most), vloss 0.12 % of its bound, no dheads element
    more than 4.9e-9 s beyond the bf16 rounding of the float64 value (2.4e-7 s allowed).
(c) Bad rows of each kind are counted, give all-zero gradient bits and leave everything else as if the row's action were out of range.
(d) Two runs give the same bits; inputs are not written; the refusals leave the outputs untouched."""
import pytest
import torch

from tests import clone_soft_ref as R
from tests import clone_value_ref as V
from tests.heads_loss_ref import U
from tests.test_clone_kernel_gpu import SHAPE_IDS, SHAPES, record, tol
from tests.test_heads_loss_kernels_gpu import FP32_STEP, Pool, ok, p, untouched

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
ONE_HOT_WEIGHTS = [(1.0, 0.0), (1.0, 1.0), (0.5, 2.0)]
SOFT_WEIGHTS = [(1.0, 0.0), (1.0, 1.0), (0.5, 2.0)]
TS = [1, 5, 97, 130]


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


def outputs(pool, T, B, ldo, grad=True, value=True):
    return dict(loss=pool.new(B), vloss=pool.new(B) if value else None, hits=pool.new(B, torch.int32), decisions=pool.new(B, torch.int32),
                bad=pool.new(B, torch.int32), steps=pool.new(B, torch.int32), dheads=pool.new((T * B, ldo), torch.bfloat16) if grad else None)


def run_soft(lib, st, c, target, T, B, A, ldh, ldo, pw, vw, grad=True):
    with_ret = vw != 0.0
    pool = Pool()
    c = dict(c, target=target)
    d = {k: pool.put(v) for k, v in c.items() if k != "ret" or with_ret}
    out = outputs(pool, T, B, ldo, grad, with_ret)
    ok(lib.hsad_clone_soft_tail(p(d["heads"]), ldh, p(d["legal"]), p(d["action"]), p(d["target"]), p(d.get("ret")), p(d["seq_len"]), p(d["weight"]), T, B, A,
                                pw, vw, p(out["loss"]), p(out["vloss"]), p(out["hits"]), p(out["decisions"]), p(out["bad"]), p(out["steps"]),
                                p(out["dheads"]), ldo, st))
    pool.check()
    for k, v in d.items():
        assert torch.equal(bits(v), bits(c[k])), "input %s was written" % k
    return out


def run_value(lib, st, c, T, B, A, ldh, ldo, pw, vw, grad=True):
    with_ret = vw != 0.0
    pool = Pool()
    d = {k: pool.put(v) for k, v in c.items() if k != "ret" or with_ret}
    out = outputs(pool, T, B, ldo, grad, with_ret)
    ok(lib.hsad_clone_value_tail(p(d["heads"]), ldh, p(d["legal"]), p(d["action"]), p(d.get("ret")), p(d["seq_len"]), p(d["weight"]), T, B, A, pw, vw,
                                 p(out["loss"]), p(out["vloss"]), p(out["hits"]), p(out["decisions"]), p(out["bad"]), p(out["steps"]), p(out["dheads"]),
                                 ldo, st))
    pool.check()
    return out


def same_bits(a, b, what):
    for k in a:
        if a[k] is None:
            assert b[k] is None
        else:
            assert torch.equal(bits(a[k]), bits(b[k])), (what, k)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_on_one_hot_targets_the_bits_are_those_of_clone_value_tail(lib, st, shape, T, B):
    """(a) for each pair of weights, with and without gradient, ldo = A + 1 and wider"""
    A, _, ldh = shape
    c, _ = V.clone_value_case(A, ldh, T, B)
    tg = R.one_hot_targets(c["action"], c["seq_len"], T, B, A)
    for pw, vw in ONE_HOT_WEIGHTS:
        for ldo, grad in ((64, True), (A + 1, True), (64, False)):
            old = run_value(lib, st, c, T, B, A, ldh, ldo, pw, vw, grad)
            new = run_soft(lib, st, c, tg, T, B, A, ldh, ldo, pw, vw, grad)
            same_bits(old, new, (pw, vw, ldo, grad))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_soft_targets_against_float64(lib, st, shape, T, B):
    """(b), and (d): a second run gives the same bits"""
    A, _, ldh = shape
    ldo = 64
    c, _ = V.clone_value_case(A, ldh, T, B)
    tg = R.soft_targets_case(c, T, B, A)
    M = T * B
    scale = (c["weight"].double() / B)[torch.arange(M) % B].abs()[:, None]
    for pw, vw in SOFT_WEIGHTS:
        ref = R.clone_soft_tail(c["heads"], c["legal"], c["action"], tg, c["ret"], c["seq_len"], c["weight"], T, B, A, ldo, pw, vw)
        assert not ref["target_bad"].any()
        out = run_soft(lib, st, c, tg, T, B, A, ldh, ldo, pw, vw)
        same_bits(out, run_soft(lib, st, c, tg, T, B, A, ldh, ldo, pw, vw), "second run")
        for k in ("hits", "decisions", "bad", "steps"):
            assert out[k].cpu().long().tolist() == ref[k].tolist(), (k, pw, vw)
        loss = out["loss"].cpu().double()
        assert torch.isfinite(loss).all()                  # (the NaN targets and returns of the rows not to be read never show)
        decisions = ref["multi"].view(T, B).sum(0).double()
        err_loss = (loss - ref["loss"]).abs()
        loss_bound = decisions * tol("xent_step") + ref["e_xent"].view(T, B).sum(0)
        got = out["dheads"].float().cpu().double()
        assert torch.isfinite(got).all()
        err = (got - ref["dheads"]).abs()
        rne = R.rne(ref["dheads"])
        allowed = rne + scale * (pw * (1.001 * tol("softmax") + 2.0 ** -22) + vw * ref["e_bound"][:, None])
        excess = ((err - rne).clamp(min=0) / scale.clamp(min=1e-30))[scale[:, 0] > 0]
        measured = dict(xent_step=float((err_loss / decisions.clamp(min=1)).max()), loss_over_bound=float((err_loss / loss_bound.clamp(min=1e-30)).max()),
                        dheads_beyond_bf16=float(excess.max()) if excess.numel() else 0.0)
        if vw != 0.0:
            vloss = out["vloss"].cpu().double()
            assert torch.isfinite(vloss).all()
            hub = ref["hub"]
            step_bound = torch.minimum(ref["e_bound"].view(T, B) + 2 * U * (hub + 0.5), torch.full_like(hub, FP32_STEP)) * ref["good"].view(T, B)
            steps = ref["steps"].clamp(min=1).double()
            vbound = torch.minimum(step_bound.sum(0) + T * U * hub.sum(0), steps * FP32_STEP)
            err_v = (vloss - ref["vloss"]).abs()
            measured["vloss_over_bound"] = float((err_v / vbound.clamp(min=1e-30)).max())
        print("clone_soft_tail A=%d T=%d B=%d weights (%g, %g): %s" % (A, T, B, pw, vw, {k: "%.3e" % v for k, v in measured.items()}))
        record("clone_soft_tail", **measured)
        assert float((err_loss - loss_bound).max()) <= 0.0, ("loss", pw, vw, err_loss.tolist(), loss_bound.tolist())
        if vw != 0.0:
            assert float((err_v - vbound).max()) <= 0.0, ("vloss", pw, vw, err_v.tolist(), vbound.tolist())
        over = err - allowed
        assert float(over.max()) <= 0.0, "dheads (%g, %g): error %.3e at %d, allowed %.3e" % (
            pw, vw, float(err.flatten()[over.argmax()]), int(over.argmax()), float(allowed.flatten()[over.argmax()]))
        b16 = bits(out["dheads"])
        assert not b16[ref["zero_row"]].any()
        assert not b16[:, A + 1:].any()
        if vw == 0.0:
            assert not b16[:, A:].any()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=["A21", "A49"])
@pytest.mark.parametrize("pw,vw", [(1.0, 0.0), (1.0, 1.0)])
def test_bad_target_rows_are_counted_and_contribute_nothing(lib, st, shape, pw, vw):
    """(c) negative, NaN, mass on an illegal column, mass 0.9, a single-legal row with its mass elsewhere; mass 1 + 5e-4 is NOT bad"""
    A, _, ldh = shape
    T, B, ldo = 130, 3, 64
    c, _ = V.clone_value_case(A, ldh, T, B)
    tg = R.soft_targets_case(c, T, B, A)
    clean = R.clone_soft_tail(c["heads"], c["legal"], c["action"], tg, c["ret"], c["seq_len"], c["weight"], T, B, A, ldo, pw, vw)
    lg = c["legal"]
    # decisions of sequence 0 with an illegal column; two of them at t >= 128, the second trip of the stride loop
    pick = torch.nonzero(clean["multi"] & (torch.arange(T * B) % B == 0) & (lg == 0).any(1))[:, 0].tolist()
    rows = pick[:3] + pick[-2:]
    assert len(set(rows)) == 5 and rows[-1] // B >= 128
    single = int(torch.nonzero(clean["single"])[0, 0])
    first, second = [int(torch.nonzero(lg[m])[0, 0]) for m in rows], [int(torch.nonzero(lg[m])[1, 0]) for m in rows]
    broken = tg.clone()
    broken[rows[0], first[0]], broken[rows[0], second[0]] = -0.25, float(tg[rows[0], second[0]] + tg[rows[0], first[0]]) + 0.25
    broken[rows[1], first[1]] = float("nan")
    broken[rows[2], int(torch.nonzero(lg[rows[2]] == 0)[0, 0])] = 0.125
    broken[rows[4]] *= 0.9
    broken[rows[3]] *= 1.0 + 5e-4
    broken[single] = 0.0
    broken[single, int(torch.nonzero(lg[single] == 0)[0, 0])] = 1.0
    want_bad = [rows[0], rows[1], rows[2], rows[4], single]
    ref = R.clone_soft_tail(c["heads"], c["legal"], c["action"], broken, c["ret"], c["seq_len"], c["weight"], T, B, A, ldo, pw, vw)
    assert sorted(int(m) for m in torch.nonzero(ref["target_bad"])[:, 0]) == sorted(want_bad)
    out = run_soft(lib, st, c, broken, T, B, A, ldh, ldo, pw, vw)
    for k in ("hits", "decisions", "bad", "steps"):
        assert out[k].cpu().long().tolist() == ref[k].tolist(), k
    assert int(out["bad"].sum()) == int(clean["bad"].sum()) + 5
    b16 = bits(out["dheads"])
    assert not b16[want_bad].any() and bool(b16[rows[3]].any())
    # loss, vloss and every other row: the bits of the clean targets with those rows' actions out of range
    action = c["action"].clone()
    action[want_bad] = -1
    tg2 = tg.clone()
    tg2[rows[3]] = broken[rows[3]]
    same_bits(out, run_soft(lib, st, dict(c, action=action), tg2, T, B, A, ldh, ldo, pw, vw), "bad rows")


def test_refuses_what_it_cannot_run(lib, st):
    """(d) a NULL target, and what hsad_clone_value_tail refuses: the error code, outputs untouched"""
    from hanabi_sad_amd._lib import HsadError
    A, _, ldh = SHAPES[0]
    T, B = 5, 3
    c, _ = V.clone_value_case(A, ldh, T, B)
    pool = Pool()
    d = {k: pool.put(v) for k, v in dict(c, target=R.soft_targets_case(c, T, B, A)).items()}
    out = outputs(pool, T, B, 64)

    def call(**kw):
        g = lambda k, v: kw[k] if k in kw else v      # noqa: E731
        return lib.hsad_clone_soft_tail(p(d["heads"]), g("ldh", ldh), p(d["legal"]), p(d["action"]), g("target", p(d["target"])), g("ret", p(d["ret"])),
                                        p(d["seq_len"]), g("weight", p(d["weight"])), g("T", T), B, A, g("pw", 1.0), g("vw", 1.0), p(out["loss"]),
                                        g("vloss", p(out["vloss"])), p(out["hits"]), p(out["decisions"]), p(out["bad"]), g("steps", p(out["steps"])),
                                        p(out["dheads"]), g("ldo", 64), st)
    refused = [dict(target=None), dict(target=None, vw=0.0, ret=None, vloss=None),
               dict(ldo=A), dict(weight=None), dict(T=0), dict(T=1 << 20), dict(steps=None), dict(ret=None), dict(vloss=None), dict(ldh=A),
               dict(pw=-1.0), dict(vw=-0.5), dict(pw=float("inf")), dict(vw=float("inf")), dict(pw=float("nan")), dict(vw=float("nan"))]
    for kw in refused:
        with pytest.raises(HsadError):
            ok(call(**kw))
    pool.check()
    assert all(untouched(v) for v in out.values())
    ok(call(vw=0.0, ret=None, vloss=None))          # ... and without the value term neither is needed
    pool.check()
    assert untouched(out["vloss"]) and not untouched(out["loss"]) and not untouched(out["steps"])
