"""hsad_clone_value_tail (csrc/r2d2/clone_value.inc) called directly through ctypes and held to the float64 reference of
tests/clone_value_ref.py, in the way tests/test_clone_kernel_gpu.py holds hsad_clone_tail: every buffer between two guard bands, logits
and values on a dyadic grid (counters exact), the Huber kink hit exactly on rows fp32 computes without rounding and kept 2^-6 away on all
others, NaN returns on every row the kernel must not read, the rows that must be zero compared as bits.

Tolerances.  The value term is plain fp32 arithmetic, so its error is DERIVED, not measured: e = ret - q carries duel_q's forward-error
bound of q (A + 3 roundings) plus the rounding of the subtraction (e_bound of the reference); Huber is 1-Lipschitz in e and adds two
roundings of its own (e e and the halving is exact, or |e| - 1/2), and the ascending sum over T steps adds at most T roundings of the
running total -- and never more than FP32_STEP per step.  dheads: one bf16 rounding of the float64 value plus
s (policy_weight tol("softmax") + value_weight e_bound), g = -clamp(e) being 1-Lipschitz and |l_j (delta - 1/A)| <= 1.  The cross-entropy
keeps tests/test_clone_kernel_gpu.py's measured tol("xent_step").  The largest errors seen are written to clone_measured_errors.json
under "clone_value_tail"; on an MI355X: vloss 3.2e-7 per step (1.4 % of its bound at most), cross-entropy 3.2e-6 per step, no dheads
element beyond the bf16 rounding of the float64 value."""
import pytest
import torch

from tests import clone_value_ref as R
from tests.heads_loss_ref import U
from tests.test_clone_kernel_gpu import SHAPE_IDS, SHAPES, record, tol
from tests.test_heads_loss_kernels_gpu import FP32_STEP, Pool, ok, p, untouched

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
WEIGHTS = [(1.0, 1.0), (0.0, 1.0), (1.0, 0.25)]


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


def run(lib, st, c, T, B, A, ldh, ldo, pw, vw, grad=True, with_ret=True):
    pool = Pool()
    d = {k: pool.put(v) for k, v in c.items() if k != "ret" or with_ret}
    out = outputs(pool, T, B, ldo, grad, with_ret)
    ok(lib.hsad_clone_value_tail(p(d["heads"]), ldh, p(d["legal"]), p(d["action"]), p(d.get("ret")), p(d["seq_len"]), p(d["weight"]), T, B, A, pw, vw,
                                 p(out["loss"]), p(out["vloss"]), p(out["hits"]), p(out["decisions"]), p(out["bad"]), p(out["steps"]), p(out["dheads"]),
                                 ldo, st))
    pool.check()
    for k, v in d.items():
        assert torch.equal(bits(v), bits(c[k])), "input %s was written" % k
    return out


def run_old(lib, st, c, T, B, A, ldh, ldo, grad=True):
    pool = Pool()
    d = {k: pool.put(v) for k, v in c.items() if k != "ret"}
    out = dict(loss=pool.new(B), hits=pool.new(B, torch.int32), decisions=pool.new(B, torch.int32), bad=pool.new(B, torch.int32),
               dheads=pool.new((T * B, ldo), torch.bfloat16) if grad else None)
    ok(lib.hsad_clone_tail(p(d["heads"]), ldh, p(d["legal"]), p(d["action"]), p(d["seq_len"]), p(d["weight"]), T, B, A, p(out["loss"]),
                           p(out["hits"]), p(out["decisions"]), p(out["bad"]), p(out["dheads"]), ldo, st))
    pool.check()
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 5, 97])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_without_the_value_term_the_bits_are_those_of_clone_tail(lib, st, shape, T, B):
    """(a) policy_weight 1, value_weight 0, ret and vloss NULL: every output hsad_clone_tail has, bit for bit, from the same inputs"""
    A, _, ldh = shape
    c, _ = R.clone_value_case(A, ldh, T, B)
    old = run_old(lib, st, c, T, B, A, ldh, 64)
    new = run(lib, st, c, T, B, A, ldh, 64, 1.0, 0.0, with_ret=False)
    for k in ("loss", "hits", "decisions", "bad", "dheads"):
        assert torch.equal(bits(old[k]), bits(new[k])), k
    ref = R.clone_value_tail(c["heads"], c["legal"], c["action"], c["ret"], c["seq_len"], c["weight"], T, B, A, 64, 1.0, 0.0)
    assert new["steps"].cpu().long().tolist() == ref["steps"].tolist()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 5, 97])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_clone_value_tail_against_float64(lib, st, shape, T, B):
    """(b) both terms, the value term alone, and unequal weights"""
    A, _, ldh = shape
    ldo = 64
    c, mark = R.clone_value_case(A, ldh, T, B)
    M = T * B
    scale = (c["weight"].double() / B)[torch.arange(M) % B].abs()[:, None]
    alone = None
    for pw, vw in WEIGHTS:
        ref = R.clone_value_tail(c["heads"], c["legal"], c["action"], c["ret"], c["seq_len"], c["weight"], T, B, A, ldo, pw, vw)
        out = run(lib, st, c, T, B, A, ldh, ldo, pw, vw)
        # exact: the counters
        for k in ("hits", "decisions", "bad", "steps"):
            assert out[k].cpu().long().tolist() == ref[k].tolist(), (k, pw, vw)
        # the cross-entropy: as in tests/test_clone_kernel_gpu.py
        loss, vloss = out["loss"].cpu().double(), out["vloss"].cpu().double()
        assert torch.isfinite(loss).all() and torch.isfinite(vloss).all()          # (the NaN returns of the rows not to be read never show)
        decisions = ref["multi"].view(T, B).sum(0).clamp(min=1).double()
        err_loss = (loss - ref["loss"]).abs()
        # the Huber sums: per step e_bound (1-Lipschitz) + Huber's own two roundings, never more than FP32_STEP; + the T roundings of the sum
        hub = ref["hub"]
        step_bound = torch.minimum(ref["e_bound"].view(T, B) + 2 * U * (hub + 0.5), torch.full_like(hub, FP32_STEP)) * ref["good"].view(T, B)
        vbound = step_bound.sum(0) + T * U * hub.sum(0)
        steps = ref["steps"].clamp(min=1).double()
        vbound = torch.minimum(vbound, steps * FP32_STEP)
        err_v = (vloss - ref["vloss"]).abs()
        got = out["dheads"].float().cpu().double()
        assert torch.isfinite(got).all()
        err = (got - ref["dheads"]).abs()
        rne = ref["dheads"].abs() * 2.0 ** -8 + 2.0 ** -134
        allowed = rne + scale * (pw * tol("softmax") + vw * ref["e_bound"][:, None])
        excess = ((err - rne).clamp(min=0) / scale.clamp(min=1e-30))[scale[:, 0] > 0]
        measured = dict(xent_step=float((err_loss / decisions).max()), vloss_step=float((err_v / steps).max()),
                        vloss_over_bound=float((err_v / vbound.clamp(min=1e-30)).max()), dheads_beyond_bf16=float(excess.max()) if excess.numel() else 0.0)
        print("clone_value_tail A=%d T=%d B=%d weights (%g, %g): %s" % (A, T, B, pw, vw, {k: "%.3e" % v for k, v in measured.items()}))
        record("clone_value_tail", **measured)
        assert float((err_loss - decisions * tol("xent_step")).max()) <= 0.0, ("loss", pw, vw, err_loss.tolist())
        assert float((err_v - vbound).max()) <= 0.0, ("vloss", pw, vw, err_v.tolist(), vbound.tolist())
        over = err - allowed
        assert float(over.max()) <= 0.0, "dheads (%g, %g): error %.3e at %d" % (pw, vw, float(err.flatten()[over.argmax()]), int(over.argmax()))
        # zero as bits: invalid and bad rows, every column past the value column
        b16 = bits(out["dheads"])
        assert not b16[ref["zero_row"]].any()
        assert not b16[:, A + 1:].any()
        # the rows marked exact: e = 0 gives a zero row of the value term, |e| = 1 the full slope, in bf16 without error
        w_row = (c["weight"].double() / B)[torch.arange(M) % B]
        for m, k in enumerate(mark):
            if k in ("zero", "plus_one", "minus_one"):
                want = {"zero": 0.0, "plus_one": -1.0, "minus_one": 1.0}[k] * vw * float(w_row[m])
                assert float(got[m, A]) == float(torch.tensor(want).bfloat16()), (m, k, float(got[m, A]), want)
        # a single-legal row is not zero now: it is the value term alone (the same bits whatever the policy weight)
        single = ref["single"] & (scale[:, 0] > 0) & (ref["g"] != 0)
        if single.any():
            assert bool((b16[single][:, :A + 1] != 0).any(1).all())
        if (pw, vw) == (0.0, 1.0):
            alone = b16
        if (pw, vw) == (1.0, 1.0):
            both = b16
    assert torch.equal(both[ref["single"]], alone[ref["single"]])
    # weight 0: numerically zero everywhere
    if float(c["weight"].abs().min()) == 0.0:
        zero_w = (c["weight"] == 0)[torch.arange(M) % B]
        assert not got[zero_w].any()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=["A21", "A49"])
def test_without_gradient_and_narrow_rows(lib, st, shape):
    """(c) dheads NULL: the same sums and counters, nothing else written; ldo = A + 1 (no padding columns) stays inside its rows"""
    A, _, ldh = shape
    T, B = 5, 3
    c, _ = R.clone_value_case(A, ldh, T, B)
    full = run(lib, st, c, T, B, A, ldh, 64, 1.0, 1.0)
    none = run(lib, st, c, T, B, A, ldh, 64, 1.0, 1.0, grad=False)
    narrow = run(lib, st, c, T, B, A, ldh, A + 1, 1.0, 1.0)
    for k in ("loss", "vloss", "hits", "decisions", "bad", "steps"):
        assert torch.equal(bits(full[k]), bits(none[k])) and torch.equal(bits(full[k]), bits(narrow[k])), k
    assert torch.equal(bits(narrow["dheads"]), bits(full["dheads"][:, :A + 1]))


def test_refuses_what_it_cannot_run(lib, st):
    """(d) hsad_clone_tail's refusals, the value term without its buffers, negative and non-finite weights: outputs untouched"""
    from hanabi_sad_amd._lib import HsadError
    A, _, ldh = SHAPES[0]
    T, B = 5, 3
    c, _ = R.clone_value_case(A, ldh, T, B)
    pool = Pool()
    d = {k: pool.put(v) for k, v in c.items()}
    out = outputs(pool, T, B, 64)

    def call(**kw):
        g = lambda k, v: kw[k] if k in kw else v      # noqa: E731
        return lib.hsad_clone_value_tail(p(d["heads"]), g("ldh", ldh), p(d["legal"]), p(d["action"]), g("ret", p(d["ret"])), p(d["seq_len"]),
                                         g("weight", p(d["weight"])), g("T", T), B, A, g("pw", 1.0), g("vw", 1.0), p(out["loss"]),
                                         g("vloss", p(out["vloss"])), p(out["hits"]), p(out["decisions"]), p(out["bad"]), g("steps", p(out["steps"])),
                                         p(out["dheads"]), g("ldo", 64), st)
    refused = [dict(ldo=A), dict(weight=None), dict(T=0), dict(T=1 << 20), dict(steps=None),                    # hsad_clone_tail's, and the new counter
               dict(ret=None), dict(vloss=None), dict(ldh=A),                                                  # the value term without what it needs
               dict(pw=-1.0), dict(vw=-0.5), dict(pw=float("inf")), dict(vw=float("inf")), dict(pw=float("nan")), dict(vw=float("nan"))]
    for kw in refused:
        with pytest.raises(HsadError):
            ok(call(**kw))
    pool.check()
    assert all(untouched(v) for v in out.values())
    ok(call(vw=0.0, ret=None, vloss=None))          # ... and without the value term neither is needed
    pool.check()
    assert untouched(out["vloss"]) and not untouched(out["loss"]) and not untouched(out["steps"])
