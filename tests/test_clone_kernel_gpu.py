"""hsad_clone_tail (csrc/r2d2/clone_loss.inc) called directly through ctypes and held to the float64 reference of
tests/clone_loss_ref.py, in the style of tests/test_heads_loss_kernels_gpu.py: every buffer between two guard bands, inputs on a dyadic
grid so that maxima and ties -- and with them hits, decisions and bad -- are EXACT, the rows that must be zero compared as bits.

The cross-entropy, the loss and the softmax inside dheads go through __expf / __logf, whose error is measured, not derived:
CLONE_MEASURED holds the largest errors seen on an MI355X against the float64 reference (written on every run to
clone_measured_errors.json beside the other files of measured errors, and quoted in DESIGN.md 3c); the tolerance is twice that, never
more than the 1e-4 per step that fp32 round-off is granted elsewhere in the suite (which is also the limit while a value is None).
dheads additionally gets one bf16 rounding of the reference value (2^-8 relative)."""
import json
import os

import pytest
import torch

from tests import clone_loss_ref as R
from tests.test_heads_loss_kernels_gpu import FP32_STEP, Pool, ok, p, untouched
from tests.test_r2d2_precision_gpu import OUT as R2D2_MEASURED

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
OUT = os.path.join(os.path.dirname(R2D2_MEASURED), "clone_measured_errors.json")

SHAPES = [(21, 15, 37), (12, 6, 19), (49, 12, 62), (32, 15, 48), (33, 15, 49)]      # (A, NP, ldh) of tests/test_heads_loss_kernels_gpu.py
SHAPE_IDS = ["A%d" % s[0] for s in SHAPES]

# largest errors measured on an MI355X (this file's record() calls):
# xent_step: |xent of one (t, b) - float64| as it shows in loss[b] of a T = 1 call, and |loss[b] - float64| / T for longer ones (logits up
# to +-30: xent up to 61.4); softmax: the error of a probability inside dheads beyond the bf16 rounding of the reference, in units of
# weight[b] / B (none seen: every dheads element lay within 2^-8 of the float64 value)
CLONE_MEASURED = {"xent_step": 2.98e-6, "softmax": 0.0}


def tol(kind):
    m = CLONE_MEASURED[kind]
    return FP32_STEP if m is None else min(FP32_STEP, 2.0 * m)


def record(test, **vals):
    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        data = json.load(open(OUT)) if os.path.exists(OUT) else {}
        old = data.get(test, {})
        data[test] = {k: max(float(v), float(old.get(k, 0.0))) for k, v in vals.items()}
        json.dump(data, open(OUT, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


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


def run(lib, st, c, T, B, A, ldh, ldo, grad=True):
    pool = Pool()
    d = {k: pool.put(v) for k, v in c.items()}
    out = dict(loss=pool.new(B), hits=pool.new(B, torch.int32), decisions=pool.new(B, torch.int32), bad=pool.new(B, torch.int32),
               dheads=pool.new((T * B, ldo), torch.bfloat16) if grad else None)
    ok(lib.hsad_clone_tail(p(d["heads"]), ldh, p(d["legal"]), p(d["action"]), p(d["seq_len"]), p(d["weight"]), T, B, A, p(out["loss"]),
                           p(out["hits"]), p(out["decisions"]), p(out["bad"]), p(out["dheads"]), ldo, st))
    pool.check()
    for k, v in c.items():
        assert torch.equal(d[k].cpu(), v), "input %s was written" % k
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 5, 97])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_clone_tail_against_float64(lib, st, shape, T, B):
    A, _, ldh = shape
    ldo = 64
    c = R.clone_case(A, ldh, T, B)
    ref = R.clone_tail(c["heads"], c["legal"], c["action"], c["seq_len"], c["weight"], T, B, A, ldo)
    out = run(lib, st, c, T, B, A, ldh, ldo)
    # exact: the counters
    for k in ("hits", "decisions", "bad"):
        assert out[k].cpu().long().tolist() == ref[k].tolist(), k
    # the loss: T steps of the measured per-step error (the fp32 sum of T terms is far inside it: 2^-24 x T x 61.4 x T / 2 at most)
    loss = out["loss"].cpu().double()
    err_loss = (loss - ref["loss"]).abs()
    assert torch.isfinite(loss).all()
    steps = ref["multi"].view(T, B).sum(0).clamp(min=1).double()
    measured_step = float((err_loss / steps).max())
    got = out["dheads"].float().cpu().double()
    assert torch.isfinite(got).all()
    scale = (c["weight"].double() / B)[torch.arange(T * B) % B].abs()[:, None]
    err = (got - ref["dheads"]).abs()
    rne = ref["dheads"].abs() * 2.0 ** -8 + 2.0 ** -134          # what rounding the exact value to bf16 may move it by (+ the subnormal floor)
    excess = ((err - rne).clamp(min=0) / scale.clamp(min=1e-30))[scale[:, 0] > 0]
    measured_soft = float(excess.max()) if excess.numel() else 0.0
    print("clone_tail A=%d T=%d B=%d: loss error per step %.3e, softmax error beyond the bf16 rounding %.3e" % (A, T, B, measured_step, measured_soft))
    record("clone_tail", xent_step=measured_step, softmax=measured_soft)
    assert float((err_loss - steps * tol("xent_step")).max()) <= 0.0, "loss error %s over %s steps" % (err_loss.tolist(), steps.tolist())
    over = err - (ref["dheads"].abs() * 2.0 ** -8 + 2.0 ** -134 + scale * tol("softmax"))
    assert float(over.max()) <= 0.0, "dheads: error %.3e at %d" % (float(err.flatten()[over.argmax()]), int(over.argmax()))
    # the rows that are zero by definition are zero as bits: invalid, bad and single-legal rows; the value column and the padding always
    bits = out["dheads"].view(torch.int16).cpu()
    assert not bits[ref["zero_row"]].any()
    assert not bits[:, A:].any()
    # weight 0: numerically zero everywhere
    if float(c["weight"].abs().min()) == 0.0:
        zero_w = (c["weight"] == 0)[torch.arange(T * B) % B]
        assert not got[zero_w].any()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=["A21", "A49"])
def test_clone_tail_without_gradient_and_narrow_rows(lib, st, shape):
    """dheads NULL: the same loss and counters, nothing else written; ldo = A + 1 (no padding columns) stays inside its rows"""
    A, _, ldh = shape
    T, B = 5, 3
    c = R.clone_case(A, ldh, T, B)
    full = run(lib, st, c, T, B, A, ldh, 64)
    none = run(lib, st, c, T, B, A, ldh, 64, grad=False)
    narrow = run(lib, st, c, T, B, A, ldh, A + 1)
    for k in ("loss", "hits", "decisions", "bad"):
        assert torch.equal(full[k], none[k]) and torch.equal(full[k], narrow[k]), k
    assert torch.equal(narrow["dheads"].view(torch.int16), full["dheads"][:, :A + 1].contiguous().view(torch.int16))


def test_clone_tail_refuses_what_it_cannot_run(lib, st):
    from hanabi_sad_amd._lib import HsadError
    A, _, ldh = SHAPES[0]
    T, B = 5, 3
    c = R.clone_case(A, ldh, T, B)
    pool = Pool()
    d = {k: pool.put(v) for k, v in c.items()}
    loss, cnt, dh = pool.new(B), pool.new(B, torch.int32), pool.new((T * B, 64), torch.bfloat16)
    call = lambda **kw: lib.hsad_clone_tail(p(d["heads"]), ldh, p(d["legal"]), p(d["action"]), p(d["seq_len"]), kw.get("weight", p(d["weight"])),    # noqa: E731
                                            kw.get("T", T), B, A, p(loss), p(cnt), p(cnt), p(cnt), p(dh), kw.get("ldo", 64), st)
    for kw in (dict(ldo=A), dict(weight=None), dict(T=0), dict(T=1 << 20)):
        with pytest.raises(HsadError):
            ok(call(**kw))
    pool.check()
    assert untouched(loss) and untouched(dh)
