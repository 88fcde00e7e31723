"""Plain float64 restatements of what csrc/r2d2/heads_loss_optim.inc and csrc/r2d2/act.inc compute, written from the formulas in the
header comments of include/hsad.h and from the lines of the reference's pyhanabi/r2d2.py those comments cite -- not from the kernels.

Every function takes the kernel's fp32 (or bf16) operands converted to float64 and returns float64 results together with a FORWARD-ERROR
BOUND per element:

    bound = (number of fp32 roundings on the element's path) x 2^-24 x (sum of the absolute values of the terms added on that path)

computed from the float64 operands (first order in 2^-24; the counts are written next to each formula).  A kernel whose result leaves
the bound is wrong, whatever its summation order.  Gradients are float64 torch autograd of the composite objective; the hand-written
formulas beside them are checked against autograd in tests/test_heads_loss_ref_cpu.py."""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit round-off of fp32 (round to nearest)
BF16_ULP = 2.0 ** -8    # one bf16 ulp relative to the value (8 significand bits)
F64 = torch.float64


def f64(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64) if not torch.is_tensor(x) else x.detach().cpu().double())


# ---------------------------------------------------------------------------------------------------
# dueling head (r2d2.py:124-131 _duel, :110 qa, :113-115 greedy)
# ---------------------------------------------------------------------------------------------------
def duel_q(adv, value, legal, action=None):
    """adv, legal [M, A], value [M] -> dict(q [M, A], q_bound, qa, qa_bound, greedy)
    q = v + a l - mean_A(a l).  Roundings on a q element: the product (1), the A additions of the mean, its division (1), the two
    additions that form q (2) = A + 3.  Terms added: |v|, |a_j l_j| and the mean's |a_k l_k| / A.
    greedy = argmax_j (1 + q - min_all q) l, first maximal index."""
    adv, value, legal = f64(adv), f64(value), f64(legal)
    A = adv.shape[1]
    al = adv * legal
    q = value[:, None] + al - al.mean(1, keepdim=True)
    bound = (A + 3) * U * (value.abs()[:, None] + al.abs() + al.abs().sum(1, keepdim=True) / A)
    out = {"q": q, "q_bound": bound, "greedy": greedy_of(q, legal)}
    if action is not None:
        idx = torch.as_tensor(action).long().view(-1, 1)
        out["qa"], out["qa_bound"] = q.gather(1, idx)[:, 0], bound.gather(1, idx)[:, 0]
    return out


def greedy_of(score_src, legal, lo=None):
    """argmax_j (1 + x - min_all x) * legal, first maximal index (torch.argmax on CPU returns the first)"""
    lo = score_src.min() if lo is None else lo
    s = ((1.0 + score_src - lo) * legal).numpy()
    return torch.as_tensor(np.argmax(s, axis=1))    # np.argmax: first occurrence


def q_at(adv, value, legal, action):
    """q of duel_q at one action per row, with its bound"""
    d = duel_q(adv, value, legal, action)
    return d["qa"], d["qa_bound"]


# ---------------------------------------------------------------------------------------------------
# exploration hash (comments of act.inc: two rounds of mix64 keyed (seed, row) then counter)
# ---------------------------------------------------------------------------------------------------
_M1, _M2, _M3, _KROW = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB),
                        np.uint64(0xD1342543DE82EF95))


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _M1
        z = (z ^ (z >> np.uint64(30))) * _M2
        z = (z ^ (z >> np.uint64(27))) * _M3
    return z ^ (z >> np.uint64(31))


def act_hash(seed, row, counter):
    """-> (u, low32): u = bits 40..63 of the hash / 2^24 in [0, 1), low32 = its low 32 bits (uint64 arrays)"""
    row = np.asarray(row, dtype=np.uint64)
    counter = np.asarray(counter, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix64(mix64(np.uint64(seed) ^ (_KROW * row)) + counter)
    u = ((h >> np.uint64(40)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return u, h & np.uint64(0xFFFFFFFF)


def act_index(low32, nlegal):
    """index of the random legal move: (low32 * nlegal) >> 32"""
    return ((np.asarray(low32, dtype=np.uint64) * np.asarray(nlegal, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------
# acting tail (r2d2.py:235-277)
# ---------------------------------------------------------------------------------------------------
def act_tail(adv, value, legal, eps, seed, counter, adv_t=None, value_t=None):
    """greedy by advantage only, (1 + adv - min_all adv) legal; explore where u < eps and a legal move exists, then the k-th legal move
    with k = act_index; Q_online(s, a) and Q_target(s, greedy) as duel_q values (A + 3 roundings)."""
    adv, legal = f64(adv), f64(legal)
    N, A = adv.shape
    greedy = greedy_of(adv, legal)
    nlegal = (legal != 0).sum(1).numpy()
    u, low = act_hash(seed, np.arange(N), counter)
    e = np.zeros(N) if eps is None else np.asarray(f64(eps))
    explore = (e > 0) & (nlegal > 0) & (u < e)
    k = act_index(low, np.maximum(nlegal, 1))
    order = np.cumsum((legal != 0).numpy(), axis=1) - 1                 # rank of every legal move in its row
    kth = np.argmax(((legal != 0).numpy()) & (order == k[:, None]), axis=1)
    a = torch.as_tensor(np.where(explore, kth, greedy.numpy()))
    out = {"a": a, "greedy": greedy, "explore": torch.as_tensor(explore)}
    if value is not None:
        out["qa"], out["qa_bound"] = q_at(adv, value, legal, a)
    if adv_t is not None:
        out["tq"], out["tq_bound"] = q_at(adv_t, value_t, legal, greedy)
    return out


# ---------------------------------------------------------------------------------------------------
# n-step TD error, Huber loss, priorities (r2d2.py:403-428, 472-478; compute_priority :355-360)
# ---------------------------------------------------------------------------------------------------
def gamma_n(gamma, n):
    """python's gamma ** n in double, then an fp32 scalar (it multiplies fp32 tensors): an operand, not a rounding of the kernel"""
    return float(np.float32(float(gamma) ** int(n)))


def huber(e):
    ae = e.abs()
    return torch.where(ae < 1.0, 0.5 * e * e, ae - 0.5)     # smooth_l1(e, 0), beta = 1


def td(online_qa, target_qa, reward, bootstrap, seq_len, n, gamma, weight=None, qa_bound=None, tq_bound=None, tree=128):
    """all [T, B] but seq_len / weight [B].  -> dict with err, priority, loss [B], dqa = d mean_b(w_b loss_b) / d online_qa (autograd) and
    bounds.  target[t] = r[t] + boot[t] gamma^n tq[t + n] (0 for t + n >= T); err = (target - qa) mask, mask = t < seq_len.
    Roundings of err: two products and the sum of the target (3), the difference (1) = 4 (the mask product is exact); terms |r|,
    |boot gamma^n tq|, |qa|.  Bounds of the inputs (qa_bound, tq_bound), when given, are carried through.
    Huber term: 2 more roundings (e e, or |e| - 1/2), and it moves with err by at most min(|e|, 1) per unit: 6 per term.
    Huber sum of a sequence: `tree` partial sums of ceil(T / tree) terms each, then a binary tree: log2(tree) + ceil(T / tree) additions.
    dqa = -clamp(e, -1, 1) mask w / B: the product and the division (2) after err's own bound."""
    qa = f64(online_qa).clone().requires_grad_(True)
    tq, r, boot, sl = f64(target_qa), f64(reward), f64(bootstrap), f64(seq_len)
    T, B = qa.shape
    gn = gamma_n(gamma, n)
    shifted = torch.zeros_like(tq)
    if n < T:
        shifted[:T - n] = tq[n:]
    mask = (torch.arange(T, dtype=F64)[:, None] < sl[None, :]).double()
    boot_term = boot * gn * shifted
    err = (r + boot_term - qa) * mask
    loss = huber(err).sum(0)
    w = torch.ones(B, dtype=F64) if weight is None else f64(weight)
    (w * loss).mean().backward()
    err = err.detach()
    e_bound = 4 * U * (r.abs() + boot_term.abs() + qa.detach().abs())
    if qa_bound is not None:
        e_bound = e_bound + f64(qa_bound)
    if tq_bound is not None:
        sb = torch.zeros_like(tq)
        if n < T:
            sb[:T - n] = f64(tq_bound)[n:]
        e_bound = e_bound + (boot * gn).abs() * sb
    e_bound = e_bound * mask
    slope = err.abs().clamp(max=1.0)
    h = huber(err)
    adds = int(math.log2(tree)) + (T + tree - 1) // tree
    loss_bound = (adds + 2) * U * h.sum(0) + (slope * e_bound).sum(0)
    dqa = qa.grad
    dqa_bound = (e_bound * (w / B)[None, :] + 2 * U * dqa.abs()) * mask
    return {"err": err, "err_bound": e_bound, "priority": err.abs(), "loss": loss.detach(), "loss_bound": loss_bound, "dqa": dqa,
            "dqa_bound": dqa_bound, "mask": mask, "hand_dqa": -err.clamp(-1.0, 1.0) * mask * (w / B)[None, :]}


def nstep_priority(qa, tq, reward, bootstrap, n, gamma):
    """|r + boot gamma^n tq - qa|: two products, a sum, a difference = 4 roundings"""
    qa, tq, r, boot = f64(qa), f64(tq), f64(reward), f64(bootstrap)
    bt = boot * gamma_n(gamma, n) * tq
    return (r + bt - qa).abs(), 4 * U * (r.abs() + bt.abs() + qa.abs())


# ---------------------------------------------------------------------------------------------------
# own-hand cross-entropy (r2d2.py:133-153) and the head gradient
# ---------------------------------------------------------------------------------------------------
def aux_xent_steps(logits, own_hand):
    """logits, own_hand [M, NP] (NP = 3 slots) -> xent per row [M]:
    -(sum_slots mask_s sum_k t_sk log softmax(logit_s)_k) / max(sum_s mask_s, 1e-6), mask_s = sum_k t_sk"""
    M, NP = own_hand.shape
    lg, tg = logits.reshape(M, NP // 3, 3), own_hand.reshape(M, NP // 3, 3)
    logq = torch.log_softmax(lg, -1)
    mask = tg.sum(-1)
    return -((tg * logq).sum(-1) * mask).sum(-1) / mask.sum(-1).clamp(min=1e-6)


def aux_xent(logits, own_hand, T, B):
    """-> (xent_sum [B] = sum over t, xent per step [T, B])"""
    x = aux_xent_steps(f64(logits), f64(own_hand)).view(T, B)
    return x.sum(0), x


def head_grad(heads, legal, action, dqa, A, own_hand=None, weight=None, pred_scale=0.0, B=1):
    """heads [M, >= A + 1 + NP] = [advantage | value | aux logits].  Autograd (float64) of
        sum_m dqa_m q(heads)_m[action_m]  +  pred_scale sum_m w_(m mod B) xent_m(heads)
    wrt heads -> (grad [M, A + 1 + NP], bound of the dueling columns, softmax scale per row).
    Dueling columns: da_j = dqa l_j (delta_j,act - 1/A): the reciprocal, the difference and two products = 4 roundings of one term;
    dv = dqa exactly.  The aux columns go through exp and log: their error is measured, not derived; in units of
    scale = pred_scale w / max(sum mask, 1e-6) it is the error of a softmax probability."""
    h = f64(heads).clone().requires_grad_(True)
    lg = f64(legal)
    M = h.shape[0]
    NP = 0 if own_hand is None else own_hand.shape[1]
    al = h[:, :A] * lg
    q = h[:, A:A + 1] + al - al.mean(1, keepdim=True)
    obj = (f64(dqa) * q.gather(1, torch.as_tensor(action).long().view(-1, 1))[:, 0]).sum()
    scale = torch.zeros(M, dtype=F64)
    if own_hand is not None and pred_scale != 0.0:
        w = f64(weight)[torch.arange(M) % B]
        obj = obj + pred_scale * (w * aux_xent_steps(h[:, A + 1:A + 1 + NP], f64(own_hand))).sum()
        scale = pred_scale * w / f64(own_hand).sum(1).clamp(min=1e-6)
    obj.backward()
    g = h.grad[:, :A + 1 + NP].clone()
    if own_hand is None or pred_scale == 0.0:
        g[:, A + 1:] = 0
    bound = torch.zeros_like(g)
    bound[:, :A] = 4 * U * g[:, :A].abs()
    return g, bound, scale


def hand_head_grad(heads, legal, action, dqa, A, own_hand, weight, pred_scale, B):
    """the formulas of include/hsad.h's heads_backward comment written out (checked against head_grad on the CPU)"""
    h, lg, d = f64(heads), f64(legal), f64(dqa)
    M = h.shape[0]
    onehot = torch.zeros(M, A, dtype=F64)
    onehot[torch.arange(M), torch.as_tensor(action).long()] = 1.0
    da = d[:, None] * lg * (onehot - 1.0 / A)
    tg = f64(own_hand)
    NP = tg.shape[1]
    t3 = tg.view(M, NP // 3, 3)
    sm = t3.sum(-1, keepdim=True)
    p = torch.softmax(h[:, A + 1:A + 1 + NP].reshape(M, NP // 3, 3), -1)
    scale = pred_scale * f64(weight)[torch.arange(M) % B] / tg.sum(1).clamp(min=1e-6)
    dl = ((p * sm - t3) * sm).view(M, NP) * scale[:, None]
    return torch.cat([da, d[:, None], dl], 1)


def loss_objective(heads, heads_t, legal, action, reward, bootstrap, seq_len, weight, own_hand, T, B, A, n, gamma, pred_weight):
    """the learner's objective mean_b(w_b (huber_sum_b + pred_weight xent_sum_b)) through duel_q, double DQN (r2d2.py:399-428, 461-490):
    -> dict(greedy, target_qa (+ bound), td results with carried bounds, xent_sum, loss, grad = d objective / d heads by autograd)"""
    h = f64(heads).clone().requires_grad_(True)
    ht, lg = f64(heads_t), f64(legal)
    M = T * B
    NP = 0 if own_hand is None else own_hand.shape[1]
    al = h[:, :A] * lg
    q = h[:, A:A + 1] + al - al.mean(1, keepdim=True)
    act = torch.as_tensor(action).long().view(-1, 1)
    qa = q.gather(1, act)[:, 0]
    on = duel_q(h.detach()[:, :A], h.detach()[:, A], lg, action)
    greedy = on["greedy"]
    tq, tq_bound = q_at(ht[:, :A], ht[:, A], lg, greedy)
    r = td(on["qa"].view(T, B), tq.view(T, B), f64(reward).view(T, B), f64(bootstrap).view(T, B), seq_len, n, gamma, weight,
           qa_bound=on["qa_bound"].view(T, B), tq_bound=tq_bound.view(T, B))
    w = torch.ones(B, dtype=F64) if weight is None else f64(weight)
    # the same objective once more with the graph attached to the heads
    gn = gamma_n(gamma, n)
    shifted = torch.zeros(T, B, dtype=F64)
    if n < T:
        shifted[:T - n] = tq.view(T, B)[n:]
    err = (f64(reward).view(T, B) + f64(bootstrap).view(T, B) * gn * shifted - qa.view(T, B)) * r["mask"]
    loss = huber(err).sum(0)
    xs = torch.zeros(B, dtype=F64)
    if own_hand is not None and pred_weight > 0:
        xs = aux_xent_steps(h[:, A + 1:A + 1 + NP], f64(own_hand)).view(T, B).sum(0)
        loss = loss + pred_weight * xs
    (w * loss).mean().backward()
    g = h.grad[:, :A + 1 + NP].clone()
    if own_hand is None or pred_weight <= 0:
        g[:, A + 1:] = 0
    scale = torch.zeros(M, dtype=F64)
    if own_hand is not None and pred_weight > 0:
        scale = (pred_weight / B) * w[torch.arange(M) % B] / f64(own_hand).sum(1).clamp(min=1e-6)
    return {"q": on["q"], "q_bound": on["q_bound"], "qa": on["qa"], "greedy": greedy, "target_qa": tq, "target_qa_bound": tq_bound,
            "td": r, "xent_sum": xs.detach(), "loss": loss.detach(), "grad": g, "aux_scale": scale, "legal": lg,
            "action": act[:, 0]}


# ---------------------------------------------------------------------------------------------------
# column sums and operand preparation
# ---------------------------------------------------------------------------------------------------
def colsum(x, N, rows_per_block, serial, out0=None, col_map=None, n_out=None):
    """x [M, >= N] -> out0 + column sums scattered through col_map, and the bound.
    Roundings: `serial` additions in a thread, the 4-way fold of a block (3), one addition per row block onto the output
    (ceil(M / rows_per_block)); terms: |x| of the column and |out0|."""
    x = f64(x)[:, :N]
    M = x.shape[0]
    n_out = N if n_out is None else n_out
    out = torch.zeros(n_out, dtype=F64) if out0 is None else f64(out0).clone()
    mag = out.abs().clone()
    idx = torch.arange(N) if col_map is None else torch.as_tensor(col_map).long()
    out.index_add_(0, idx, x.sum(0))
    mag.index_add_(0, idx, x.abs().sum(0))
    n = serial + 3 + (M + rows_per_block - 1) // rows_per_block
    return out, n * U * mag


def to_bf16_bits(x):
    """fp32 -> bf16 bit pattern, round to nearest even (finite inputs)"""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_bits_to_f64(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def prepare_weight(w, perm=None):
    """-> (weight[perm] as bf16 bits [R, C], its transpose [C, R]): casts and moves are exact"""
    w = np.asarray(w, dtype=np.float32)
    if perm is not None:
        w = w[np.asarray(perm)]
    b = to_bf16_bits(w)
    return b, np.ascontiguousarray(b.T)


def bias_sum_perm(a, b=None, perm=None):
    """out[i] = a[perm[i]] + b[perm[i]]: one rounding of |a| + |b|"""
    a = np.asarray(a, dtype=np.float64)
    b = np.zeros_like(a) if b is None else np.asarray(b, dtype=np.float64)
    p = np.arange(len(a)) if perm is None else np.asarray(perm)
    return a[p] + b[p], U * (np.abs(a[p]) + np.abs(b[p]))


def matmul_bound(a, b, bias=None):
    """a [M, K], b [N, K] (float64 values of bf16 operands) -> a b^T + bias and K + 1 roundings of sum |a b| + |bias|
    (valid for every order in which K products can be added)"""
    a, b = f64(a), f64(b)
    c = a @ b.t()
    mag = a.abs() @ b.abs().t()
    if bias is not None:
        c, mag = c + f64(bias)[None, :], mag + f64(bias).abs()[None, :]
    return c, (a.shape[1] + 1) * U * mag
