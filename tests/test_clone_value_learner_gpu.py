"""CompositeLearner.clone_loss(value_weight > 0) (hsad_r2d2_clone_value_fwd + the unchanged hsad_r2d2_loss_bwd / _optimizer_step): the value
head learns.  Gradients against fp32 torch autograd of the restatement on tests/r2d2_torch_ref.py (net_forward's q: masked log_softmax of
the recorded move PLUS smooth_l1 of the gathered q against the returns), isolation (the kernel without the value term leaves the bits of
the old call; a TD update behind a value-clone forward has the bits of one without; two value-clone updates have the same bits), and
convergence of the value loss on one fixed batch.

Tolerances as in tests/test_clone_learner_gpu.py: twice the value measured on an MI355X (CLONE_VALUE_MEASURED, written on every run to
clone_measured_errors.json), never more than a cap that comes from the TD learner and not from this code: the loss is a sum of T
cross-entropies, each 2-Lipschitz in the logits' largest error, and the value loss a sum of T Huber terms, each 1-Lipschitz in q; q is
held to TOL["bf16"]["q" | "full_q"] of tests/test_r2d2_precision_gpu.py, so |loss error| <= 2 T tol_q and |value loss error| <= T tol_q;
gradients 1.5 x the TD learner's "grad_rel" | "full_grad_rel"."""
import pytest
import torch

from tests import r2d2_torch_ref as ref
from tests.test_clone_kernel_gpu import record
from tests.test_clone_learner_gpu import SHAPES, make, ref_clone_loss, td
from tests.test_r2d2_precision_gpu import TOL, relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"

CAPS = {"plain": dict(loss=2 * 7 * TOL["bf16"]["q"], vloss=7 * TOL["bf16"]["q"], grad_rel=1.5 * TOL["bf16"]["grad_rel"]),
        "fused": dict(loss=2 * 80 * TOL["bf16"]["full_q"], vloss=80 * TOL["bf16"]["full_q"], grad_rel=1.5 * TOL["bf16"]["full_grad_rel"])}
# largest values measured on an MI355X: |loss[b] - fp32 autograd|, |value_loss[b] - fp32 autograd|, the largest relative Frobenius error of a
# gradient tensor (fc_v.* included)
# (plain: lstm.weight_hh_l0 is the largest, fc_v.weight 3.8e-3, fc_v.bias 1.5e-3; fused: net.0.weight, fc_v.weight 3.0e-3, fc_v.bias 2.9e-3;
# convergence: the value loss per step goes 5.024 -> 1.7e-5 over the 200 updates, the fp32 restatement under torch.optim.Adam 5.024 -> 1.3e-5)
CLONE_VALUE_MEASURED = {"plain": dict(loss=8.94e-4, vloss=2.65e-3, grad_rel=5.81e-3), "fused": dict(loss=1.145e-2, vloss=7.98e-3, grad_rel=3.99e-3)}


def tol(shape, kind):
    m, cap = CLONE_VALUE_MEASURED[shape][kind], CAPS[shape][kind]
    return cap if m is None else min(cap, 2.0 * m)


def with_returns(batch, lo, hi, seed=5):
    """the batch plus ret [T, B] drawn uniformly in [lo, hi) (NaN past seq_len: never read)"""
    T, B = batch["a"].shape
    g = torch.Generator().manual_seed(seed)
    ret = (torch.rand(T, B, generator=g) * (hi - lo) + lo).to(DEV)
    valid = torch.arange(T, device=DEV).unsqueeze(1) < batch["seq_len"].unsqueeze(0)
    return dict(batch, ret=torch.where(valid, ret, torch.full_like(ret, float("nan")))), valid


def ref_value_loss(Wd, batch, valid, masks=None):
    """smooth_l1 of net_forward's q at the recorded move against the returns, summed over the steps inside seq_len -> [B]"""
    T, B = batch["a"].shape
    H = Wd["fc_v.weight"].shape[1]
    h0 = torch.zeros(ref.num_layers(Wd), B, H, device=DEV)
    qa = ref.net_forward(Wd, batch["priv_s"], batch["legal_move"], batch["a"], h0, h0.clone(), masks)[0]
    target = torch.where(valid, batch["ret"], qa.detach())
    return (torch.nn.functional.smooth_l1_loss(qa, target, reduction="none") * valid.float()).sum(0)


@pytest.mark.parametrize("shape", ["plain", "fused"])
def test_gradients_against_fp32_autograd(shape):
    from hanabi_sad_amd.composite import CompositeLearner
    T, B, H, F, A = SHAPES[shape]
    W, Wt, batch, weight = make(shape)
    batch, valid = with_returns(batch, -2.0, 2.0)          # q of these nets is within +-1: errors on both sides of the Huber kink
    lr = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    loss, stats = lr.clone_loss(batch, weight, value_weight=1.0)
    torch.cuda.synchronize()
    lr.check_sync()
    plan = lr.plan()
    if shape == "fused":
        assert plan["fwd_kind"] == 2 and plan["fwd_nets"] == 1 and plan["bwd_kind"] == 2, plan
    else:
        assert plan["fwd_kind"] == 0 and plan["bwd_kind"] == 0, plan
    Wd = {k: v.to(DEV).requires_grad_(True) for k, v in W.items()}
    rloss, _, rdec, _ = ref_clone_loss(Wd, batch)
    rv = ref_value_loss(Wd, batch, valid)
    ((rloss + rv) * weight).mean().backward()
    assert torch.equal(stats["decisions"].long(), rdec.sum(0)) and torch.equal(stats["steps"].long(), valid.sum(0)) and not stats["bad"].any()
    inside = float(((batch["ret"] - ref.net_forward(Wd, batch["priv_s"], batch["legal_move"], batch["a"], *ref.zeros_hid(Wd, B, batch["priv_s"]))[0])
                    .detach().abs()[valid] < 1).float().mean())
    assert 0.2 < inside < 0.8, inside
    e_loss = float((loss - rloss.detach()).abs().max())
    e_vloss = float((stats["value_loss"] - rv.detach()).abs().max())
    want = {k: v.grad.clone() for k, v in Wd.items() if v.grad is not None}
    # net.* under the bf16 activation pattern, as everywhere in the suite (tests/test_clone_learner_gpu.py says why)
    raw = {k: relerr(lr.grad[k], want[k]) for k in want if k.startswith("net.")}
    masks, flips = ref.bf16_relu_masks(Wd, batch["priv_s"])
    assert all(worst <= 1.0 for _, worst in flips), ("a ReLU decision flips at a unit that is NOT within the bf16 rounding of zero", flips)
    for v in Wd.values():
        v.grad = None
    ((ref_clone_loss(Wd, batch, masks)[0] + ref_value_loss(Wd, batch, valid, masks)) * weight).mean().backward()
    want.update({k: v.grad.clone() for k, v in Wd.items() if k.startswith("net.")})
    rel = {k: relerr(lr.grad[k], want[k]) for k in want if not k.startswith("pred.")}
    print("value-clone learner %s: loss error %.3e (cap %.3e), value loss error %.3e (cap %.3e), gradient errors %s, net.* before the activation "
          "pattern %s, flipped units %s" % (shape, e_loss, CAPS[shape]["loss"], e_vloss, CAPS[shape]["vloss"], {k: "%.2e" % v for k, v in rel.items()},
                                           {k: "%.2e" % v for k, v in raw.items()}, flips))
    record("clone_value_learner_" + shape, loss=e_loss, vloss=e_vloss, grad_rel=max(rel.values()), **{"grad_rel." + k: v for k, v in rel.items()})
    # the value head learns now; the own-hand head still gets nothing
    for k in ("fc_v.weight", "fc_v.bias"):
        assert k in rel and float(lr.grad[k].abs().max()) > 0, k
    for k in ("pred.weight", "pred.bias"):
        assert not lr.grad[k].any(), k
    assert e_loss <= tol(shape, "loss"), e_loss
    assert e_vloss <= tol(shape, "vloss"), e_vloss
    assert max(rel.values()) <= tol(shape, "grad_rel"), rel
    lr.close()


def value_fwd(lr, batch, weight, pw, vw, want_grad=1):
    """hsad_r2d2_clone_value_fwd itself (clone_loss(value_weight=0) is, by design, the old entry point) -> loss, counters [4, B]"""
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.composite import _s
    T, B = batch["a"].shape
    lr._ensure(T, B)
    loss, vloss, cnt = torch.empty(B, device=DEV), torch.zeros(B, device=DEV), torch.empty(4, B, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else t.contiguous().data_ptr()      # noqa: E731
    _lib.check(lr.lib.hsad_r2d2_clone_value_fwd(lr.h, p(batch["priv_s"]), None, p(batch["legal_move"]), p(batch["a"]), p(batch.get("ret")),
                                                p(batch["seq_len"]), p(weight), pw, vw, p(loss), p(vloss) if vw else None, p(cnt[0]), p(cnt[1]),
                                                p(cnt[2]), p(cnt[3]), want_grad, _s(lr.device)))
    return loss, vloss, cnt


def i32(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", ["plain", "fused"])
def test_isolation_and_determinism(shape):
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.composite import CompositeLearner, _s
    W, Wt, batch, weight = make(shape)
    vbatch, _ = with_returns(batch, -2.0, 2.0)
    a = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    want_td = td(a, batch, weight)
    l_old, s_old = a.clone_loss(batch, weight)                    # the old call
    torch.cuda.synchronize()
    g_old = a.gflat.clone()
    b = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    # value_weight 0 through the new entry point: the bits of the old call
    l0, _, cnt = value_fwd(b, batch, weight, 1.0, 0.0)
    _lib.check(b.lib.hsad_r2d2_loss_bwd(b.h, _s(b.device)))
    torch.cuda.synchronize()
    assert torch.equal(i32(l0), i32(l_old)) and torch.equal(i32(b.gflat), i32(g_old))
    assert all(torch.equal(cnt[k], s_old[name]) for k, name in enumerate(("hits", "decisions", "bad")))
    assert torch.equal(cnt[3], s_old["steps"])
    # two value-clone updates from one state: the same bits
    l1, s1 = b.clone_loss(vbatch, weight, value_weight=1.0)
    torch.cuda.synchronize()
    g1 = b.gflat.clone()
    l2, s2 = b.clone_loss(vbatch, weight, value_weight=1.0)
    torch.cuda.synchronize()
    assert torch.equal(i32(l1), i32(l2)) and torch.equal(i32(g1), i32(b.gflat)) and all(torch.equal(s1[k], s2[k]) for k in s1)
    assert float(s1["value_loss"].min()) > 0 and not torch.equal(i32(g1), i32(g_old))
    # late weights stay refused behind it; the plain backward follows
    value_fwd(b, vbatch, weight, 1.0, 1.0)
    with pytest.raises(_lib.HsadError, match="clone_fwd"):
        _lib.check(b.lib.hsad_r2d2_loss_bwd_weighted(b.h, weight.data_ptr(), batch["seq_len"].data_ptr(), _s(b.device)))
    _lib.check(b.lib.hsad_r2d2_loss_bwd(b.h, _s(b.device)))
    torch.cuda.synchronize()
    assert torch.equal(i32(g1), i32(b.gflat))
    # refusals of the entry point itself: nothing launched, nothing handed to loss_bwd
    for pw, vw, drop in ((-1.0, 1.0, None), (1.0, float("nan"), None), (float("inf"), 1.0, None), (1.0, 1.0, "ret")):
        bb = {k: v for k, v in vbatch.items() if k != drop}
        with pytest.raises(_lib.HsadError):
            value_fwd(b, bb, weight, pw, vw)
    # a TD update behind a value-clone forward: the bits of one without
    got = td(b, batch, weight)
    for x, y, what in zip(got, want_td, ("loss", "priority", "gradient")):
        assert torch.equal(i32(x), i32(y)), what
    b.check_sync()
    a.close()
    b.close()


def test_the_value_loss_converges_on_one_batch():
    """200 updates of the value term alone (policy_weight 0, lr 5e-4) on one fixed batch of the plain shape with returns drawn in [0, 10):
    the value loss per step falls below a tenth of its first value.  (The fp32 restatement under torch.optim.Adam with the same data,
    eps and clip goes from 5.02 to 1.3e-5 in those 200 updates, run on the host while writing this test: the condition can be met.)"""
    from hanabi_sad_amd.composite import CompositeLearner
    W, Wt, batch, weight = make("plain")
    batch, valid = with_returns(batch, 0.0, 10.0, seed=11)
    lr = CompositeLearner(W, Wt, 3, 0.999, lr=5e-4, eps=1.5e-5, grad_clip=5.0, device=DEV)
    steps = float(valid.sum())
    per_step = []
    for k in range(200):
        _, stats = lr.clone_loss(batch, weight, policy_weight=0.0, value_weight=1.0)
        lr.optimizer_step()
        if k % 20 == 0:
            per_step.append(float(stats["value_loss"].sum()) / steps)
    _, stats = lr.clone_loss(batch, weight, compute_grad=False, policy_weight=0.0, value_weight=1.0)
    assert int(stats["steps"].sum()) == int(steps)
    last = float(stats["value_loss"].sum()) / steps
    lr.check_sync()
    print("value loss per step over 200 updates: %s -> %.4e" % (["%.3f" % v for v in per_step], last))
    record("clone_value_convergence", first=per_step[0], last=last)
    assert per_step[0] > 1.0 and last < 0.1 * per_step[0], (per_step, last)
    lr.close()
