"""CompositeLearner.clone_loss with batch["target"] (hsad_r2d2_clone_soft_fwd + the unchanged hsad_r2d2_loss_bwd / _optimizer_step), at the
two shapes of tests/test_clone_value_learner_gpu.py:
  - with a one-hot target the call gives the BITS of the call without one: loss, stats and the flat gradient -- with and without the value
    term;
  - with soft targets, gradients against fp32 torch autograd of the same objective on tests/r2d2_torch_ref.py (net_forward's q, illegal
    entries at -inf, log_softmax, -sum_j pi_j log p_j), inside tests/test_clone_value_learner_gpu.py's tol(shape, "grad_rel") and
    tol(shape, "loss"): the soft tail adds fp32 arithmetic on the head outputs only (tests/test_clone_soft_kernel_gpu.py bounds it at
    1e-4 per decision), the net before it is the same;
  - repeated updates on one fixed batch bring the mean KL divergence per decision below a tenth of its first value, the ratio and the
    step count of test_the_value_loss_converges_on_one_batch."""
import pytest
import torch

from tests import r2d2_torch_ref as ref
from tests.test_clone_kernel_gpu import record
from tests.test_clone_learner_gpu import SHAPES, make
from tests.test_clone_value_learner_gpu import i32, ref_value_loss, tol, with_returns
from tests.test_r2d2_precision_gpu import relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"


def valid_rows(batch):
    T = batch["a"].shape[0]
    return torch.arange(T, device=DEV).unsqueeze(1) < batch["seq_len"].unsqueeze(0)


def one_hot(batch):
    """float32 [T, B, A]: 1.0 at the recorded move; NaN rows past seq_len (never read)"""
    A = batch["legal_move"].shape[2]
    tg = torch.nn.functional.one_hot(batch["a"], A).float()
    return torch.where(valid_rows(batch).unsqueeze(2), tg, torch.full_like(tg, float("nan")))


def soft(batch, seed=9):
    """float32 [T, B, A]: a seeded distribution over the legal actions of every valid row (normalised in float64, rounded once);
    NaN rows past seq_len"""
    legal = batch["legal_move"].cpu().double()
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(legal.shape, generator=g, dtype=torch.float64) + 0.05) * legal
    tg = (w / w.sum(2, keepdim=True).clamp(min=1e-300)).float().to(DEV)
    return torch.where(valid_rows(batch).unsqueeze(2), tg, torch.full_like(tg, float("nan")))


def entropy(target, valid):
    p = torch.where(valid.unsqueeze(2), target, torch.zeros_like(target)).double()
    return float(-torch.where(p > 0, p * torch.log(p.clamp(min=1e-300)), torch.zeros_like(p)).sum())


def ref_soft_loss(Wd, batch, target, masks=None):
    """-sum_j pi_j log_softmax(q over the legal actions)_j, summed over the steps inside seq_len -> [B]"""
    priv, legal, a = batch["priv_s"], batch["legal_move"], batch["a"]
    T, B = a.shape
    H = Wd["fc_v.weight"].shape[1]
    h0 = torch.zeros(ref.num_layers(Wd), B, H, device=DEV)
    _, _, q, _ = ref.net_forward(Wd, priv, legal, a, h0, h0.clone(), masks)
    valid = valid_rows(batch)
    z = q.masked_fill((legal == 0) & valid.unsqueeze(2), float("-inf"))
    logp = torch.log_softmax(z, 2)
    on = (legal != 0) & valid.unsqueeze(2)
    pi = torch.where(on, target, torch.zeros_like(target))
    return -(pi * torch.where(on, logp, torch.zeros_like(logp))).sum(2).sum(0)


@pytest.mark.parametrize("shape", ["plain", "fused"])
def test_a_one_hot_target_gives_the_bits_of_the_call_without_it(shape):
    from hanabi_sad_amd.composite import CompositeLearner
    W, Wt, batch, weight = make(shape)
    vbatch, _ = with_returns(batch, -2.0, 2.0)
    lr = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    for b, kw in ((batch, {}), (vbatch, dict(value_weight=1.0)), (vbatch, dict(value_weight=2.0, policy_weight=0.5))):
        l0, s0 = lr.clone_loss(b, weight, **kw)
        torch.cuda.synchronize()
        g0 = lr.gflat.clone()
        s0 = {k: s0[k].clone() for k in ("hits", "decisions", "bad", "steps", "value_loss")}
        l1, s1 = lr.clone_loss(dict(b, target=one_hot(b)), weight, **kw)
        torch.cuda.synchronize()
        assert torch.equal(i32(l0), i32(l1)), kw
        assert torch.equal(i32(g0), i32(lr.gflat)), kw
        for k in s0:
            assert torch.equal(i32(s0[k]), i32(s1[k])), (kw, k)
        assert int(s1["decisions"].sum()) > 0 and not s1["bad"].any()
    lr.check_sync()
    lr.close()


@pytest.mark.parametrize("shape", ["plain", "fused"])
@pytest.mark.parametrize("vw", [0.0, 1.0])
def test_soft_target_gradients_against_fp32_autograd(shape, vw):
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.composite import CompositeLearner, _s
    T, B, H, F, A = SHAPES[shape]
    W, Wt, batch, weight = make(shape)
    batch, valid = with_returns(batch, -2.0, 2.0)
    target = soft(batch)
    lr = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    loss, stats = lr.clone_loss(dict(batch, target=target), weight, value_weight=vw)
    torch.cuda.synchronize()
    lr.check_sync()
    plan = lr.plan()
    if shape == "fused":
        assert plan["fwd_kind"] == 2 and plan["fwd_nets"] == 1 and plan["bwd_kind"] == 2, plan
    else:
        assert plan["fwd_kind"] == 0 and plan["bwd_kind"] == 0, plan
    Wd = {k: v.to(DEV).requires_grad_(True) for k, v in W.items()}

    def objective(masks=None):
        rl = ref_soft_loss(Wd, batch, target, masks)
        rv = ref_value_loss(Wd, batch, valid, masks) if vw else torch.zeros_like(rl)
        return rl, rv

    rloss, rv = objective()
    ((rloss + vw * rv) * weight).mean().backward()
    assert not stats["bad"].any() and torch.equal(stats["steps"].long(), valid.sum(0))
    assert torch.equal(stats["decisions"].long(), (valid & (batch["legal_move"].sum(2) >= 2)).sum(0))
    e_loss = float((loss - rloss.detach()).abs().max())
    want = {k: v.grad.clone() for k, v in Wd.items() if v.grad is not None}
    # net.* under the bf16 activation pattern, as everywhere in the suite (tests/test_clone_learner_gpu.py says why)
    masks, flips = ref.bf16_relu_masks(Wd, batch["priv_s"])
    assert all(worst <= 1.0 for _, worst in flips), ("a ReLU decision flips at a unit that is NOT within the bf16 rounding of zero", flips)
    for v in Wd.values():
        v.grad = None
    ml, mv = objective(masks)
    ((ml + vw * mv) * weight).mean().backward()
    want.update({k: v.grad.clone() for k, v in Wd.items() if k.startswith("net.")})
    skip = ("pred.",) if vw else ("pred.", "fc_v.")
    rel = {k: relerr(lr.grad[k], want[k]) for k in want if not k.startswith(skip)}
    print("soft-clone learner %s value_weight %g: loss error %.3e (tolerance %.3e), gradient errors %s (tolerance %.3e), flipped units %s"
          % (shape, vw, e_loss, tol(shape, "loss"), {k: "%.2e" % v for k, v in rel.items()}, tol(shape, "grad_rel"), flips))
    record("clone_soft_learner_%s_vw%g" % (shape, vw), loss=e_loss, grad_rel=max(rel.values()))
    for k in ("pred.weight", "pred.bias") + (() if vw else ("fc_v.weight", "fc_v.bias")):
        assert not lr.grad[k].any(), k
    assert e_loss <= tol(shape, "loss"), e_loss
    assert max(rel.values()) <= tol(shape, "grad_rel"), rel
    if vw:
        assert float((stats["value_loss"] - rv.detach()).abs().max()) <= tol(shape, "vloss")
    # the weighted backward stays refused behind it, the plain one follows; a missing target is refused before anything is launched
    g_first, l_first = lr.gflat.clone(), loss.clone()
    cnt = torch.empty(4, B, dtype=torch.int32, device=DEV)
    out, vout = torch.empty(B, device=DEV), torch.zeros(B, device=DEV)

    def soft_fwd(tg):      # the entry point itself, forward half only
        _lib.check(lr.lib.hsad_r2d2_clone_soft_fwd(lr.h, batch["priv_s"].data_ptr(), None, batch["legal_move"].data_ptr(), batch["a"].data_ptr(), tg,
                                                   batch["ret"].data_ptr() if vw else None, batch["seq_len"].data_ptr(), weight.data_ptr(), 1.0, vw,
                                                   out.data_ptr(), vout.data_ptr() if vw else None, cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr(),
                                                   cnt[3].data_ptr(), 1, _s(lr.device)))

    soft_fwd(target.data_ptr())
    with pytest.raises(_lib.HsadError, match="clone_fwd"):
        _lib.check(lr.lib.hsad_r2d2_loss_bwd_weighted(lr.h, weight.data_ptr(), batch["seq_len"].data_ptr(), _s(lr.device)))
    _lib.check(lr.lib.hsad_r2d2_loss_bwd(lr.h, _s(lr.device)))
    torch.cuda.synchronize()
    assert torch.equal(i32(out), i32(l_first)) and torch.equal(i32(lr.gflat), i32(g_first))      # ... and a second update has the same bits
    out.fill_(-7.0)
    with pytest.raises(_lib.HsadError, match="target"):
        soft_fwd(None)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    lr.close()


def test_the_kl_divergence_converges_on_one_batch():
    """200 updates (lr 5e-4) on one fixed batch of the plain shape with seeded soft targets: the mean KL divergence per decision -- the
    loss less the targets' entropy -- falls below a tenth of its first value"""
    from hanabi_sad_amd.composite import CompositeLearner
    W, Wt, batch, weight = make("plain")
    target = soft(batch, seed=13)
    valid = valid_rows(batch)
    H = entropy(target, valid)
    batch = dict(batch, target=target)
    ones = torch.ones_like(weight)
    lr = CompositeLearner(W, Wt, 3, 0.999, lr=5e-4, eps=1.5e-5, grad_clip=5.0, device=DEV)
    kl = []
    for k in range(200):
        loss, stats = lr.clone_loss(batch, ones)
        lr.optimizer_step()
        if k % 20 == 0:
            kl.append((float(loss.double().sum()) - H) / float(stats["decisions"].sum()))
    loss, stats = lr.clone_loss(batch, ones, compute_grad=False)
    assert not stats["bad"].any()
    last = (float(loss.double().sum()) - H) / float(stats["decisions"].sum())
    lr.check_sync()
    print("KL per decision over 200 updates: %s -> %.4e (target entropy per decision %.4f)" % (["%.4f" % v for v in kl], last, H / float(stats["decisions"].sum())))
    record("clone_soft_convergence", first=kl[0], last=last)
    assert kl[0] > 0 and last > -1e-3 and last < 0.1 * kl[0], (kl, last)
    lr.close()
