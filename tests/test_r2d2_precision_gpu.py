"""Every golden-vector test of the R2D2 kernels in TWO parametrisations:

  fp32  the exact mode (hanabi_sad_amd/r2d2_f32.py, csrc/hsad_r2d2_f32.hip: fp32 operands on v_mfma_f32_32x32x2_f32): the
        reference's own arithmetic type; tolerance 1e-4 (fp32 round-off over <= 80 recurrent steps),
  bf16  the production kernels (bf16 MFMA operands, fp16 gate storage, fp32 accumulate / state): tolerance = 2 x the error
        measured on MI355X for the same test (TOL below; the measured numbers are written to
        gpurun_out/r2d2_measured_errors.json by this test and quoted in DESIGN.md §3c).

Golden vectors: tests/golden/*.npz, generated from the reference's pyhanabi/r2d2.py by tests/golden/make_r2d2_golden.py.
Full-size cases (BASELINE configs[2] shapes) compare with the fp32 torch restatement those vectors pin
(tests/r2d2_torch_ref.py, tests/test_r2d2_golden_cpu.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import r2d2_torch_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
OUT = os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "r2d2_measured_errors.json")

# max abs error (values) / relative Frobenius error (gradients).  fp32: round-off.  bf16: 2 x measured (see module docstring).
TOL = {
    "fp32": {"q": 1e-4, "lstm_o": 1e-4, "priority": 1e-4, "loss": 1e-4, "grad_rel": 1e-4, "hidden": 1e-4, "full_q": 2e-4,
             "full_loss": 2e-3, "full_grad_rel": 5e-4},
    "bf16": {"q": 6e-4, "lstm_o": 1e-3, "priority": 1.5e-3, "loss": 1.2e-3, "grad_rel": 8.5e-3, "hidden": 1e-3, "full_q": 5.5e-3,
             "full_loss": 4e-2, "full_grad_rel": 7e-3},
}


def record(precision, test, **vals):
    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        data = json.load(open(OUT)) if os.path.exists(OUT) else {}
        data.setdefault(test, {})[precision] = {k: float(v) for k, v in vals.items()}
        json.dump(data, open(OUT, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def maxerr(a, b):
    a = torch.as_tensor(a).float().cpu()
    b = torch.as_tensor(b).float().cpu()
    return float((a - b).abs().max())


def relerr(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


def nets(z, precision):
    from hanabi_sad_amd.r2d2 import R2D2NetKernels
    Won, Wtg = ref.weights_from_npz(z, "online_net."), ref.weights_from_npz(z, "target_net.")
    return Won, Wtg, R2D2NetKernels.make(Won, DEV, precision), R2D2NetKernels.make(Wtg, DEV, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_td_priority_against_golden(precision):
    from hanabi_sad_amd.r2d2 import td_loss
    tol = TOL[precision]
    z = np.load(os.path.join(GOLD, "r2d2_iql_sad_small.npz"))
    Won, Wtg, online, target = nets(z, precision)
    t = lambda k: torch.tensor(z[k]).to(DEV)
    priv, legal, a = t("loss.priv_s"), t("loss.legal_move"), t("loss.a")
    qa, greedy, q, o = online.forward(priv, legal, a)
    Wd = {k: v.to(DEV) for k, v in Won.items()}
    T, B = a.shape
    h0 = torch.zeros(2, B, online.H, device=DEV)
    rqa, rgreedy, rq, ro = ref.net_forward(Wd, priv, legal, a, h0, h0.clone())
    e_q, e_o = maxerr(q, rq), maxerr(o.float(), ro)
    tqa, _, _, _ = target.forward(priv, legal, rgreedy)
    err, prio, loss, _ = td_loss(qa, tqa, t("loss.reward"), t("loss.bootstrap"), t("loss.seq_len"), int(z["meta"][8]),
                                 float(z["gamma"][0]), weight=t("loss.weight"))
    e_p, e_l = maxerr(prio, z["loss.rl.priority"]), maxerr(loss, z["loss.rl.loss"])
    record(precision, "forward_td_priority_golden", q=e_q, lstm_o=e_o, priority=e_p, loss=e_l)
    assert e_q <= tol["q"] and e_o <= tol["lstm_o"], (e_q, e_o)
    assert e_p <= tol["priority"] and e_l <= tol["loss"], (e_p, e_l)
    if precision == "fp32":
        assert torch.equal(greedy, rgreedy)
    else:   # bf16 may only flip a greedy action where the top-2 legal q are within its tolerance
        diff = greedy != rgreedy
        if diff.any():
            top2 = ((1 + rq - rq.min()) * legal).topk(2, dim=2).values
            assert ((top2[..., 0] - top2[..., 1])[diff] < 2 * tol["q"]).all()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("tag,pw", [("rl", 0.0), ("aux", 0.25)])
def test_learner_loss_and_gradients_against_golden(tag, pw, precision):
    """loss / priority / every parameter gradient of (loss*weight).mean() vs the reference's autograd"""
    from hanabi_sad_amd.r2d2 import R2D2Learner
    tol = TOL[precision]
    z = np.load(os.path.join(GOLD, "r2d2_iql_sad_small.npz"))
    Won, Wtg = ref.weights_from_npz(z, "online_net."), ref.weights_from_npz(z, "target_net.")
    lr = R2D2Learner(Won, Wtg, int(z["meta"][8]), float(z["gamma"][0]), device=DEV, precision=precision)
    t = lambda k: torch.tensor(z[k]).to(DEV)
    batch = {k: t("loss." + k) for k in ("priv_s", "legal_move", "a", "reward", "bootstrap", "seq_len", "own_hand")}
    loss, prio = lr.loss(batch, t("loss.weight"), pw)
    e_l, e_p = maxerr(loss, z["loss.%s.loss" % tag]), maxerr(prio, z["loss.%s.priority" % tag])
    rel = {}
    for k, g in lr.grad.items():
        want = torch.tensor(z["loss.%s.grad.%s" % (tag, k)])
        if want.abs().max() == 0:
            assert g.abs().max() < 1e-6, k
            continue
        rel[k] = relerr(g, want)
    record(precision, "learner_golden_" + tag, loss=e_l, priority=e_p, grad_rel_max=max(rel.values()),
           **{"grad_rel." + k: v for k, v in rel.items()})
    assert e_l <= tol["loss"] and e_p <= tol["priority"], (e_l, e_p)
    assert max(rel.values()) <= tol["grad_rel"], rel


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_agent_act_and_compute_priority_against_golden(precision):
    from hanabi_sad_amd.r2d2 import R2D2Agent
    tol = TOL[precision]
    z = np.load(os.path.join(GOLD, "r2d2_iql_sad_small.npz"))
    _, _, on, tg = nets(z, precision)
    agent = R2D2Agent(on, tg, int(z["meta"][8]), float(z["gamma"][0]))
    flat = lambda k: torch.tensor(z[k]).flatten(0, 1).to(DEV)

    def hid(hk, ck):
        f = lambda h: torch.tensor(h).reshape(h.shape[0] * h.shape[1], 2, -1).transpose(0, 1).contiguous().to(DEV)
        return {"h0": f(z[hk]), "c0": f(z[ck])}
    obs = {"priv_s": flat("act.priv_s"), "legal_move": flat("act.legal_move"), "eps": torch.zeros(flat("act.priv_s").shape[0], device=DEV)}
    reply, new_hid = agent.act(obs, hid("act.h0", "act.c0"))
    want = torch.tensor(z["act.out_greedy_a"].reshape(-1)).to(DEV)
    assert torch.equal(reply["a"], reply["greedy_a"])
    G = want.shape[0]
    e_h = maxerr(new_hid["h0"].transpose(0, 1), z["act.out_h0"].reshape(G, 2, -1))
    e_c = maxerr(new_hid["c0"].transpose(0, 1), z["act.out_c0"].reshape(G, 2, -1))
    nobs = {"priv_s": flat("prio.next_priv_s"), "legal_move": flat("prio.next_legal_move")}
    p = agent.compute_priority(obs, flat("prio.a"), nobs, hid("act.h0", "act.c0"), hid("prio.next_h0", "prio.next_c0"),
                               flat("prio.reward"), flat("prio.bootstrap"))
    e_p = maxerr(p, z["prio.out"].reshape(-1))
    agree = float((reply["greedy_a"] == want).float().mean())
    record(precision, "agent_golden", h=e_h, c=e_c, priority=e_p, greedy_agreement=agree)
    assert e_h <= tol["hidden"] and e_c <= 2 * tol["hidden"] and e_p <= tol["priority"], (e_h, e_c, e_p)
    assert agree == 1.0 if precision == "fp32" else agree >= 0.9


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_vdn_learner_and_priority_against_golden(precision):
    from hanabi_sad_amd.r2d2 import R2D2Agent, R2D2Learner, R2D2NetKernels
    tol = TOL[precision]
    z = np.load(os.path.join(GOLD, "r2d2_vdn_small.npz"))
    Won, Wtg = ref.weights_from_npz(z, "online_net."), ref.weights_from_npz(z, "target_net.")
    n, gamma = int(z["meta"][8]), float(z["gamma"][0])
    lr = R2D2Learner(Won, Wtg, n, gamma, device=DEV, precision=precision)
    batch = {k[5:]: torch.tensor(z[k]).to(DEV) for k in z.files if k.startswith("loss.") and k.count(".") == 1}
    loss, prio = lr.loss(batch, batch["weight"], 0.0)
    e_l, e_p = maxerr(loss, z["loss.rl.loss"]), maxerr(prio, z["loss.rl.priority"])
    rel = {}
    for k, g in lr.grad.items():
        want = torch.tensor(z["loss.rl.grad." + k])
        if float(want.norm()) < 1e-7:
            assert float(g.norm()) < 1e-5, k
            continue
        rel[k] = relerr(g, want)
    P = z["act.priv_s"].shape[2]
    agent = R2D2Agent(R2D2NetKernels.make(Won, DEV, precision), R2D2NetKernels.make(Wtg, DEV, precision), n, gamma)
    f2 = lambda k: torch.tensor(z[k]).flatten(0, 2).to(DEV)

    def hid(hk, ck):
        f = lambda h: torch.tensor(h).reshape(h.shape[0] * h.shape[1], 2, -1).transpose(0, 1).contiguous().to(DEV)
        return {"h0": f(z[hk]), "c0": f(z[ck])}
    obs = {"priv_s": f2("act.priv_s"), "legal_move": f2("act.legal_move")}
    nobs = {"priv_s": f2("prio.next_priv_s"), "legal_move": f2("prio.next_legal_move")}
    p = agent.compute_priority(obs, f2("prio.a"), nobs, hid("act.h0", "act.c0"), hid("prio.next_h0", "prio.next_c0"),
                               torch.tensor(z["prio.reward"]).flatten().to(DEV),
                               torch.tensor(z["prio.bootstrap"]).flatten().to(DEV), num_player=P)
    e_cp = maxerr(p, z["prio.out"].reshape(-1))
    record(precision, "vdn_golden", loss=e_l, priority=e_p, compute_priority=e_cp, grad_rel_max=max(rel.values()))
    # VDN sums two players' Q-values: twice the per-row error budget
    assert e_l <= 2 * tol["loss"] and e_p <= 2 * tol["priority"] and e_cp <= 2 * tol["priority"], (e_l, e_p, e_cp)
    assert max(rel.values()) <= 2 * tol["grad_rel"], rel


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16-composite"])
def test_full_size_learner_against_fp32_autograd(precision):
    """BASELINE configs[2] shapes (F=838, H=512, A=21, T=80, B=128, aux task on): loss, priorities and every gradient vs
    torch autograd on the fp32 restatement the golden vectors pin.  bf16-composite = the product path (library composite entry
    points, fused recurrences); bf16 = the Python-orchestrated chunk-pipelined schedule.

    Every value is held to the tolerance on the MAXIMUM -- except where the reference itself has a near-tie: a TD error at (t, b) reads
    Q_target(s_{t+n}, argmax_a Q_online(s_{t+n}, a)); if the two best legal Q_online values of the REFERENCE at (t+n, b) are closer than
    the Q tolerance, either action is a legitimate answer of a finite-precision implementation and the priority at (t, b) (and the loss
    of sequence b) may differ by O(0.1).  Every outlier must be such a provable near-tie; anything else fails, in fp32 mode as well."""
    from hanabi_sad_amd.r2d2 import R2D2Learner, check_sync
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    composite = precision.endswith("composite")
    tol = TOL["bf16" if composite else precision]
    n = 3
    F, A, H, T, B = 838, 21, 512, 80, 128
    W, Wt = _rand_net(F, H, A, seed=3), _rand_net(F, H, A, seed=4)
    batch, weight = _rand_batch(T, B, F, A)
    if composite:
        from hanabi_sad_amd.composite import CompositeLearner
        lr = CompositeLearner(W, Wt, n, 0.999, device=DEV)
    else:
        lr = R2D2Learner(W, Wt, n, 0.999, device=DEV, precision=precision)
    loss, prio = lr.loss(batch, weight, 0.25)
    torch.cuda.synchronize()
    lr.check_sync() if composite else check_sync()
    Wd = {k: v.to(DEV).requires_grad_(True) for k, v in W.items()}
    rloss, rprio = ref.loss(Wd, {k: v.to(DEV) for k, v in Wt.items()}, batch, n, 0.999, 0.25)
    (rloss * weight).mean().backward()
    # the reference's own Q_online and the gap between its two best legal values per (t, b)
    with torch.no_grad():
        h0 = torch.zeros(2, B, H, device=DEV)
        _, _, rq, _ = ref.net_forward({k: v.detach() for k, v in Wd.items()}, batch["priv_s"], batch["legal_move"], batch["a"], h0, h0.clone())
        top2 = ((1 + rq - rq.min()) * batch["legal_move"]).topk(2, dim=2).values
        gap = top2[..., 0] - top2[..., 1]                                   # [T, B]
    tie = 2 * tol["full_q"]
    dp = (prio - rprio.detach()).abs()
    out_p = torch.nonzero(dp > tol["full_q"])
    for t, b in out_p.tolist():
        assert t + n < T and float(gap[t + n, b]) < tie, ("priority outlier without a near-tie", t, b, float(dp[t, b]), float(gap[min(t + n, T - 1), b]))
    dl = (loss - rloss.detach()).abs()
    seq_with_tie = set(b for _, b in out_p.tolist())
    for b in torch.nonzero(dl > tol["full_loss"]).flatten().tolist():
        assert b in seq_with_tie, ("loss outlier without a near-tie in its sequence", b, float(dl[b]))
    clean_p = dp.clone()
    clean_p[dp > tol["full_q"]] = 0
    clean_l = dl.clone()
    clean_l[dl > tol["full_loss"]] = 0
    rel = {k: relerr(lr.grad[k], Wd[k].grad) for k in Wd if Wd[k].grad is not None and float(Wd[k].grad.norm()) > 0}
    record(precision, "full_size_learner", loss_max_excl_ties=float(clean_l.max()), loss_max=float(dl.max()), priority_max_excl_ties=float(clean_p.max()),
           priority_max=float(dp.max()), near_tie_priorities=int(out_p.shape[0]), grad_rel_max=max(rel.values()),
           **{"grad_rel." + k: v for k, v in rel.items()})
    assert out_p.shape[0] <= (0 if precision == "fp32" else 8), out_p.shape[0]          # measured: 0 (fp32), 1-2 (bf16) of 10,240
    assert max(rel.values()) <= tol["full_grad_rel"], rel


@pytest.mark.parametrize("B,vdn", [(32, False), (96, False), (32, True)])
def test_small_batch_learner_against_fp32_autograd(B, vdn):
    """The learner's default schedule at the batch sizes where the wide BPTT launch leaves XCDs without a row block -- B = 32 / 96 sequences
    (2 / 6 of 8) and VDN at batchsize 32 (64 rows: 4) -- against torch autograd on the fp32 restatement, T = 80.  Outliers of priorities and
    losses must be near-ties of the reference (tests/near_tie.py; VDN: the closest of the players' two best actions at s_{t+n})."""
    from hanabi_sad_amd.composite import CompositeLearner
    from tests.near_tie import assert_sequence_outliers_are_near_ties, top2_gap
    from tests.test_lstm_stall_gpu import _batch
    from tests.test_r2d2_kernels_gpu import _rand_net
    tol = dict(TOL["bf16"])
    if vdn:      # the loss of a game sums two players' Q errors over 80 steps: measured 0.062 outside near-ties (MI355X)
        tol["full_loss"] = 0.125
    n, pw = 3, (0.0 if vdn else 0.25)
    F, A, H, T = 838, 21, 512, 80
    W, Wt = _rand_net(F, H, A, seed=3), _rand_net(F, H, A, seed=4)
    batch, weight = _batch(B, vdn, seed=7 + B)
    lr = CompositeLearner(W, Wt, n, 0.999, device=DEV)
    loss, prio = lr.loss(batch, weight, pw)
    torch.cuda.synchronize()
    lr.check_sync()
    Wd = {k: v.to(DEV).requires_grad_(True) for k, v in W.items()}
    rloss, rprio = ref.loss(Wd, {k: v.to(DEV) for k, v in Wt.items()}, batch, n, 0.999, pw)
    (rloss * weight).mean().backward()
    with torch.no_grad():
        priv, legal, a = batch["priv_s"], batch["legal_move"], batch["a"]
        if vdn:
            priv, legal, a = priv.flatten(1, 2), legal.flatten(1, 2), a.flatten(1, 2)
        h0 = torch.zeros(2, priv.shape[1], H, device=DEV)
        _, _, rq, _ = ref.net_forward({k: v.detach() for k, v in Wd.items()}, priv, legal, a, h0, h0.clone())
        gap = top2_gap(rq, legal)
        if vdn:
            gap = gap.view(T, B, 2).min(2).values
    rel = {k: relerr(lr.grad[k], Wd[k].grad) for k in Wd if Wd[k].grad is not None and float(Wd[k].grad.norm()) > 0}
    record("bf16-composite", "small_batch_learner_B%d%s_raw" % (B, "_vdn" if vdn else ""), loss_max=float((loss - rloss.detach()).abs().max()),
           priority_max=float((prio - rprio.detach()).abs().max()), grad_rel_max=max(rel.values()))
    ties, e_p, e_l = assert_sequence_outliers_are_near_ties(prio, rprio.detach(), loss, rloss.detach(), gap, n, tol["full_q"], tol["full_loss"],
                                                            tag=(B, vdn))
    record("bf16-composite", "small_batch_learner_B%d%s" % (B, "_vdn" if vdn else ""), loss_max_excl_ties=e_l, priority_max_excl_ties=e_p,
           near_tie_priorities=ties, grad_rel_max=max(rel.values()), **{"grad_rel." + k: v for k, v in rel.items()})
    assert ties <= 8, ties
    assert max(rel.values()) <= tol["full_grad_rel"], rel
