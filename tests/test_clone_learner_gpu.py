"""CompositeLearner.clone_loss (hsad_r2d2_clone_fwd + the unchanged hsad_r2d2_loss_bwd / _optimizer_step): gradients against fp32 torch
autograd of a masked log_softmax restatement on tests/r2d2_torch_ref.py, isolation from the TD path (same bits after a clone forward as
without one), determinism, three Adam updates tracked against torch.optim.Adam, and the way from records to a net that plays.

Measured on an MI355X (written on every run to clone_measured_errors.json, quoted in DESIGN.md 3c): CLONE_LEARNER_MEASURED.  A tolerance is
twice the measured value and never more than its cap.  The caps come from the TD learner, not from this code: the loss is a sum of T
cross-entropies, each 2-Lipschitz in the logits' maximum error, and the logits are held to TOL["bf16"]["q" | "full_q"] (2 x measured) of
tests/test_r2d2_precision_gpu.py, so |loss error| <= 2 T tol_q; the gradient cap is three times the TD learner's measured relative
Frobenius error at the shape (its tolerances are 2 x measured: 1.5 x "grad_rel" | "full_grad_rel") -- beyond that is a bug to find."""
import os

import pytest
import torch

from tests import r2d2_torch_ref as ref
from tests.test_clone_kernel_gpu import OUT, record          # noqa: F401  (the same file of measured errors)
from tests.test_r2d2_precision_gpu import TOL, relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"

# shape id -> (T, B, H, F, A); "plain": per-layer GEMM + unchunked recurrence, "fused": fused forward + the wide fused BPTT
SHAPES = {"plain": (7, 5, 128, 838, 21), "fused": (80, 32, 512, 838, 21)}
CAPS = {"plain": dict(loss=2 * 7 * TOL["bf16"]["q"], grad_rel=1.5 * TOL["bf16"]["grad_rel"]),
        "fused": dict(loss=2 * 80 * TOL["bf16"]["full_q"], grad_rel=1.5 * TOL["bf16"]["full_grad_rel"])}
# largest values measured on an MI355X: |loss[b] - fp32 autograd|, the largest relative Frobenius error of a gradient tensor, and
# |mean(loss * weight) - reference| over the three updates of test_three_updates_track_adam
# (the TD learner at the fused shape's size: grad_rel 3.3e-3, tests/test_r2d2_precision_gpu.py; end to end on one batch of 32 sequences of
# the steady bot: agreement 0.21 -> 1.00 over 160 decisions of the small variant in 200 updates, 0.08 -> 1.00 over 1057 decisions of the
# standard game in 300)
CLONE_LEARNER_MEASURED = {"plain": dict(loss=8.94e-4, grad_rel=4.59e-3), "fused": dict(loss=1.145e-2, grad_rel=4.0e-3), "three_updates": 2.06e-4}


def tol(shape, kind):
    m, cap = CLONE_LEARNER_MEASURED[shape][kind], CAPS[shape][kind]
    return cap if m is None else min(cap, 2.0 * m)


def make(shape, seed=3):
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    T, B, H, F, A = SHAPES[shape]
    W, Wt = _rand_net(F, H, A, seed=seed), _rand_net(F, H, A, seed=seed + 1)
    batch, weight = _rand_batch(T, B, F, A, seed=7 + B)
    return W, Wt, batch, weight


def ref_clone_loss(Wd, batch, masks=None):
    """the restatement: net_forward's q, illegal entries at -inf, log_softmax, gather the action, mask by seq_len -> loss [B], and
    hits / decisions / the gap between the reference's two best legal values (a near-tie may legitimately be decided either way)"""
    priv, legal, a, seq_len = batch["priv_s"], batch["legal_move"], batch["a"], batch["seq_len"]
    T, B = a.shape
    H = Wd["fc_v.weight"].shape[1]
    h0 = torch.zeros(ref.num_layers(Wd), B, H, device=priv.device)
    _, _, q, _ = ref.net_forward(Wd, priv, legal, a, h0, h0.clone(), masks)
    valid = torch.arange(T, device=priv.device).unsqueeze(1) < seq_len.unsqueeze(0)
    z = q.masked_fill((legal == 0) & valid.unsqueeze(2), float("-inf"))          # (rows past seq_len have no legal action: left finite, masked below)
    xent = -torch.log_softmax(z, 2).gather(2, a.unsqueeze(2)).squeeze(2) * valid.float()
    with torch.no_grad():
        decision = valid & (legal.sum(2) >= 2)
        zz = z.detach().masked_fill(~valid.unsqueeze(2), 0.0)
        hit = decision & (zz.argmax(2) == a)
        top2 = zz.masked_fill(~decision.unsqueeze(2), 0.0).topk(2, dim=2).values
        gap = torch.where(decision, top2[..., 0] - top2[..., 1], torch.full_like(top2[..., 0], float("inf")))
    return xent.sum(0), hit, decision, gap


GRAD_KEYS_WITHOUT_GRADIENT = ("fc_v.weight", "fc_v.bias", "pred.weight", "pred.bias")      # cloning gives the value and the own-hand head none


@pytest.mark.parametrize("shape", ["plain", "fused"])
def test_gradients_against_fp32_autograd(shape):
    from hanabi_sad_amd.composite import CompositeLearner
    T, B, H, F, A = SHAPES[shape]
    W, Wt, batch, weight = make(shape)
    lr = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    loss, stats = lr.clone_loss(batch, weight)
    torch.cuda.synchronize()
    lr.check_sync()
    plan = lr.plan()
    if shape == "fused":
        assert plan["fwd_kind"] == 2 and plan["fwd_nets"] == 1 and plan["bwd_kind"] == 2 and plan["wide_requested"] == 1, plan
    else:
        assert plan["fwd_kind"] == 0 and plan["bwd_kind"] == 0, plan
    Wd = {k: v.to(DEV).requires_grad_(True) for k, v in W.items()}
    rloss, rhit, rdec, gap = ref_clone_loss(Wd, batch)
    (rloss * weight).mean().backward()
    hits, decisions = stats.read()
    assert decisions == int(rdec.sum()) and torch.equal(stats["decisions"].long(), rdec.sum(0))
    near = int((gap < 2 * TOL["bf16"]["full_q"]).sum())
    assert abs(hits - int(rhit.sum())) <= near, (hits, int(rhit.sum()), near)
    e_loss = float((loss - rloss.detach()).abs().max())
    want = {k: v.grad.clone() for k, v in Wd.items() if v.grad is not None}
    # net.* as everywhere in the suite (tests/test_r2d2_arch_gpu.py): a first-layer unit whose fp32 pre-activation is within the bf16 rounding
    # of zero takes its ReLU decision the other way and moves the net.0 gradients by a whole term -- with the 35 rows of the plain shape two
    # such units are 3.3 % of their norm (measured raw: net.0.weight 3.30e-2, net.0.bias 2.27e-2, every other tensor <= 4.3e-3; the fp32
    # restatement alone, with and without the two units' decisions exchanged, differs by 3.28e-2 and 2.25e-2).  Held to a
    # property instead of a tolerance: every flipped unit provably sits within the rounding bound of zero (bf16_relu_masks), and against
    # the fp32 network UNDER the bf16 activation pattern net.* meet the same tolerance as every other tensor.
    raw = {k: relerr(lr.grad[k], want[k]) for k in want if k.startswith("net.")}
    masks, flips = ref.bf16_relu_masks(Wd, batch["priv_s"])
    assert all(worst <= 1.0 for _, worst in flips), ("a ReLU decision flips at a unit that is NOT within the bf16 rounding of zero", flips)
    for v in Wd.values():
        v.grad = None
    (ref_clone_loss(Wd, batch, masks)[0] * weight).mean().backward()
    want.update({k: v.grad.clone() for k, v in Wd.items() if k.startswith("net.")})
    rel = {k: relerr(lr.grad[k], want[k]) for k in want if k not in GRAD_KEYS_WITHOUT_GRADIENT}
    print("clone learner %s: loss error %.3e (cap %.3e), gradient errors %s, net.* before the activation pattern %s, flipped units %s"
          % (shape, e_loss, CAPS[shape]["loss"], {k: "%.2e" % v for k, v in rel.items()}, {k: "%.2e" % v for k, v in raw.items()}, flips))
    record("clone_learner_" + shape, loss=e_loss, grad_rel=max(rel.values()), relu_flips=float(sum(n for n, _ in flips)),
           **{"grad_rel." + k: v for k, v in rel.items()}, **{"grad_rel_raw." + k: v for k, v in raw.items()})
    for k in GRAD_KEYS_WITHOUT_GRADIENT:
        assert not lr.grad[k].any(), k                      # exactly zero; autograd's own is round-off around zero (pred.*: none at all)
        assert k not in want or float(want[k].abs().max()) <= 1e-4 * float(want["fc_a.weight"].abs().max()), k
    assert e_loss <= tol(shape, "loss"), e_loss
    assert max(rel.values()) <= tol(shape, "grad_rel"), rel
    lr.close()


def td(lr, batch, weight):
    loss, prio = lr.loss(batch, weight, 0.0)
    torch.cuda.synchronize()
    return loss.clone(), prio.clone(), lr.gflat.clone()


@pytest.mark.parametrize("shape", ["plain", "fused"])
def test_a_clone_forward_leaves_the_td_path_alone_and_is_deterministic(shape):
    """learner A: TD loss + backward.  Learner B: clone_loss + backward (no optimizer step) twice -- the same bits both times --, then
    the same TD loss + backward: the same bits as A."""
    from hanabi_sad_amd.composite import CompositeLearner
    W, Wt, batch, weight = make(shape)
    a = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    want = td(a, batch, weight)
    plan_a = a.plan()
    b = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    l1, s1 = b.clone_loss(batch, weight)
    torch.cuda.synchronize()
    g1 = b.gflat.clone()
    if shape == "fused":
        assert b.plan()["fwd_nets"] == 1 and plan_a["fwd_nets"] == 2
    l2, s2 = b.clone_loss(batch, weight)
    torch.cuda.synchronize()
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)) and torch.equal(g1.view(torch.int32), b.gflat.view(torch.int32))
    assert all(torch.equal(s1[k], s2[k]) for k in s1) and float(g1.abs().max()) > 0
    got = td(b, batch, weight)
    assert b.plan() == plan_a
    for x, y, what in zip(got, want, ("loss", "priority", "gradient")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what
    again = td(a, batch, weight)                                 # (and A itself repeats: the comparison above compares like with like)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(again, want))
    b.check_sync()
    a.close()
    b.close()


def test_weights_arriving_late_are_refused_after_a_clone_forward():
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.composite import CompositeLearner, _s
    W, Wt, batch, weight = make("plain")
    lr = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    T, B = batch["a"].shape
    lr._ensure(T, B)
    loss, cnt = torch.empty(B, device=DEV), torch.empty(3, B, dtype=torch.int32, device=DEV)
    p = lambda t: t.contiguous().data_ptr()      # noqa: E731
    _lib.check(lr.lib.hsad_r2d2_clone_fwd(lr.h, p(batch["priv_s"]), None, p(batch["legal_move"]), p(batch["a"]), p(batch["seq_len"]), p(weight),
                                          p(loss), p(cnt[0]), p(cnt[1]), p(cnt[2]), 1, _s(lr.device)))
    with pytest.raises(_lib.HsadError, match="clone_fwd"):
        _lib.check(lr.lib.hsad_r2d2_loss_bwd_weighted(lr.h, p(weight), p(batch["seq_len"]), _s(lr.device)))
    _lib.check(lr.lib.hsad_r2d2_loss_bwd(lr.h, _s(lr.device)))          # the plain backward still follows
    with pytest.raises(_lib.HsadError):                                  # ... once
        _lib.check(lr.lib.hsad_r2d2_loss_bwd(lr.h, _s(lr.device)))
    with pytest.raises(_lib.HsadError):                                  # no gradient without weights
        _lib.check(lr.lib.hsad_r2d2_clone_fwd(lr.h, p(batch["priv_s"]), None, p(batch["legal_move"]), p(batch["a"]), p(batch["seq_len"]), None,
                                              p(loss), p(cnt[0]), p(cnt[1]), p(cnt[2]), 1, _s(lr.device)))
    torch.cuda.synchronize()
    lr.close()


def test_a_bad_recorded_move_is_counted_and_raises_when_read():
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.composite import CompositeLearner
    W, Wt, batch, weight = make("plain")
    batch = dict(batch)
    a = batch["a"].clone()
    legal = batch["legal_move"]
    a[0, 0] = int((legal[0, 0] == 0).nonzero()[0])          # an illegal move in a valid row
    a[1, 1] = legal.shape[2] + 2                             # out of range
    batch["a"] = a
    lr = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    loss, stats = lr.clone_loss(batch, weight)
    assert stats["bad"].tolist()[:2] == [1, 1] and int(stats["bad"].sum()) == 2 and bool(torch.isfinite(loss).all())
    with pytest.raises(_lib.HsadError, match="2 recorded moves"):
        stats.read()
    lr.close()


THREE_LR = 1e-3


def test_three_updates_track_adam():
    """three clone updates (lr 1e-3, eps 1.5e-5, clip 5) next to the restatement under torch.optim.Adam + clip_grad_norm_: the weighted
    mean loss tracks the reference's, and the reference's own falls from update to update (so that tracking it says something)"""
    from hanabi_sad_amd.composite import CompositeLearner
    shape = "plain"
    W, Wt, batch, weight = make(shape)
    lr = CompositeLearner(W, Wt, 3, 0.999, lr=THREE_LR, eps=1.5e-5, grad_clip=5.0, device=DEV)
    Wd = {k: v.to(DEV).clone().requires_grad_(True) for k, v in W.items()}
    opt = torch.optim.Adam(list(Wd.values()), lr=THREE_LR, eps=1.5e-5)
    got, want = [], []
    for _ in range(3):
        loss, _ = lr.clone_loss(batch, weight)
        lr.optimizer_step()
        got.append(float((loss * weight).mean()))
        opt.zero_grad()
        rloss = ref_clone_loss(Wd, batch)[0]
        obj = (rloss * weight).mean()
        obj.backward()
        torch.nn.utils.clip_grad_norm_(list(Wd.values()), 5.0)
        opt.step()
        want.append(float(obj.detach()))
    err = max(abs(g - w) for g, w in zip(got, want))
    print("three clone updates: device %s, reference %s" % (got, want))
    record("clone_three_updates", loss_mean=err)
    assert want[0] > want[1] > want[2], want
    m = CLONE_LEARNER_MEASURED["three_updates"]
    cap = CAPS[shape]["loss"] * float(weight.mean())
    assert err <= (cap if m is None else min(cap, 2.0 * m)), (got, want)
    lr.close()


# ---- end to end: records of a deterministic teacher -> sequences -> a net that plays ---------------------------------------------------
SMALL = dict(colors=2, ranks=5, max_information_tokens=8, max_life_tokens=1)      # with hands of 2: games of a few moves
FULL = dict(colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3)


def steady_bot():
    """every preset of rulebot.py ends in a *_RANDOM rule; this is `cautious` without it: no rule draws a random move (when none fires
    the lowest legal move is taken), so the teacher is a function of the position"""
    from hanabi_sad_amd import rulebot as rb
    rules = [r for r in rb.PRESETS["cautious"].rules if r[0] not in (rb.HINT_RANDOM, rb.DISCARD_RANDOM, rb.LEGAL_RANDOM)]
    assert len(rules) == len(rb.PRESETS["cautious"].rules) - 1
    return rb.RuleBot(rules, "steady")


@pytest.mark.parametrize("name,rules,hand,max_len,updates", [("small", SMALL, 2, 24, 200), ("standard", FULL, 5, 80, 300)])
def test_records_to_a_net_that_plays(name, rules, hand, max_len, updates, tmp_path):
    from hanabi_sad_amd import clone
    from hanabi_sad_amd.actor import NetPartner, PartnerSeats
    from hanabi_sad_amd.checkpoint import load_weights, save_weights
    from hanabi_sad_amd.composite import CompositeLearner
    from hanabi_sad_amd.eval import env_dims, evaluate
    from hanabi_sad_amd.selfplay import init_weights
    from tests.test_actor_partner_gpu import Side, make_actor
    P, H = 2, 256
    records = clone.records_from_teacher([steady_bot()], 16, 11, 1, num_player=P, device=DEV, hand_size=hand, **rules)
    assert len(records) == 16 and all(r.meta["seats"] == ["steady", "steady"] for r in records)
    data = clone.sequences_from_records(records, True, max_len=max_len, device=DEV)
    assert data.n_rows == 32 and data.T == max_len
    (batch, weight, index), = list(data.batches(32, seed=1))
    assert int((index >= 0).sum()) == 32
    F, A = env_dims(P, hand, True, **rules)
    assert A == data.legal_move.shape[2] and data.priv_s_bf16.shape[2] == (F + 63) // 64 * 64
    W = init_weights(F, H, A, hand, 5)
    lr = CompositeLearner(W, W, 1, 0.999, lr=1e-3, eps=1.5e-5, grad_clip=5.0, device=DEV)
    loss0, st0 = lr.clone_loss(batch, weight, compute_grad=False)
    h0, n0 = st0.read()
    assert n0 > 0
    first = float(loss0.sum()) / n0
    for _ in range(updates):
        lr.clone_loss(batch, weight)
        lr.optimizer_step()
    loss1, st1 = lr.clone_loss(batch, weight, compute_grad=False)
    h1, n1 = st1.read()
    last = float(loss1.sum()) / n1
    lr.check_sync()
    print("clone e2e %s: loss per decision %.4f -> %.4f, agreement %.4f -> %.4f over %d decisions" % (name, first, last, h0 / n0, h1 / n1, n1))
    record("clone_e2e_" + name, loss_first=first, loss_last=last, agreement_untrained=h0 / n0, agreement_trained=h1 / n1)
    assert n1 == n0 and last < first and h1 / n1 > h0 / n0
    path = os.path.join(str(tmp_path), "clone.pthw")
    save_weights(lr.online.w, path)
    lr.close()
    weights = load_weights(path)
    mean, _, scores, _ = evaluate(weights, 8, 3, 0, 1, num_player=P, hand_size=hand, device=DEV, **rules)
    assert len(scores) == 8 and 0 <= mean <= rules["colors"] * rules["ranks"]
    side = Side(32, P, hand, 1, rules, max_len)
    ac = make_actor(side, PartnerSeats.alternate(32, P, [NetPartner(path, name="cloned")], bot_seed=1))
    for _ in range(12):
        for _ in range(10):
            ac.step()
        torch.cuda.synchronize()
        if side.replay.num_add() > 0:          # (a finished game's sequence reaches the replay; n_finished counts the last step only)
            break
    assert side.replay.num_add() > 0, "no game next to the cloned partner ended within 120 steps"
