"""TEST INFRASTRUCTURE: float64 reference of the behaviour-cloning loss WITH the value term on the head outputs, from its definition
(include/hsad.h, hsad_clone_value_tail).  Never imported by the product package.

The policy part is tests/clone_loss_ref.py's clone_tail.  On top of it, for every valid row m = t B + b that is not bad:
    q = duel_q(adv, value, legal)[act] = v + z_act l_act - mean_A(z l)      (tests/heads_loss_ref.py, with its forward-error bound)
    e = ret[m] - q,  hub = huber(e) (smooth_l1, beta = 1),  g = -clamp(e, -1, 1)
    dheads[m, j] = s (policy_weight (p_j - delta_j,act) [>= 2 legal] + value_weight g l_j (delta_j,act - 1/A)),  dheads[m, A] = s value_weight g
with s = weight[b] / B; vloss[b] = sum_t hub in ascending t; steps[b] = the number of such rows."""
import torch

from tests import clone_loss_ref as P
from tests.heads_loss_ref import U, duel_q, huber

KINK_MARGIN = 2.0 ** -6          # every row that is not marked "exact" keeps |e| at least this far from the Huber kink at 1
MARKS = ("inside", "outside_plus", "outside_minus", "zero", "plus_one", "minus_one")
_E_OF_MARK = {"inside": 0.25, "outside_plus": 3.0, "outside_minus": -2.5, "zero": 0.0, "plus_one": 1.0, "minus_one": -1.0}
_E_UNMARKED = (0.5, -0.375, 1.75, -4.0, 0.75)


def _rows(c, T, B, A):
    """valid / bad / good (valid, not bad) per row, and the action clamped into range"""
    M = T * B
    t_of, b_of = torch.arange(M) // B, torch.arange(M) % B
    valid = t_of.double() < c["seq_len"].double()[b_of]
    act = c["action"].long()
    safe = act.clamp(0, A - 1)
    act_legal = (c["legal"].gather(1, safe[:, None])[:, 0] != 0) & (act >= 0) & (act < A)
    return valid, valid & ~act_legal, valid & act_legal, safe


def clone_value_case(A, ldh, T, B, seed=0):
    """clone_loss_ref.clone_case plus a value column on the dyadic grid (multiples of 2^-6 in [-8, 8]) and ret [T*B] float32.
    Sequence 0's special rows (kind = (t + A) % 8 in 0..6) are kept as they are.  MARKED rows -- sequence 0's ordinary rows (kind 7), mark
    (t // 8) % 6, and with B = 3 sequence 1's valid rows, mark t % 6 -- put the error e = ret - q at: `inside` 0.25, `outside_plus` 3,
    `outside_minus` -2.5, and EXACTLY at `zero` 0, `plus_one` 1, `minus_one` -1.  The three exact marks rebuild the row so that fp32
    computes q without rounding: every legal logit 0 but the action's, which is A / 64 -- the sum of z l is that one term, its mean 1 / 64,
    q = v + (A - 1) / 64 and ret = q + e are multiples of 2^-6 below 2^5.  On every other good row e is one of _E_UNMARKED (up to the
    rounding of ret to fp32), at least KINK_MARGIN away from +-1: the fp32 error of q cannot carry it across the kink.  Rows past seq_len
    and bad rows carry NaN in ret: the kernel must not read it.  -> clone_case's dict + ret, mark (list of str | None per row)"""
    c = P.clone_case(A, ldh, T, B, seed)
    g = torch.Generator().manual_seed(77 + 1000 * A + 10 * T + B + seed)
    M = T * B
    heads = c["heads"]
    heads[:, A] = torch.randint(-512, 513, (M,), generator=g).float() / 64.0
    valid, bad, good, safe = _rows(c, T, B, A)
    mark = [None] * M
    for t in range(T):
        if (t + A) % 8 == 7:
            mark[t * B] = MARKS[(t // 8) % 6]
        if B >= 2 and t < float(c["seq_len"][1]):
            mark[t * B + 1] = MARKS[t % 6]
    for m in range(M):
        if not bool(good[m]):
            mark[m] = None
        elif mark[m] in ("zero", "plus_one", "minus_one"):
            a = int(safe[m])
            heads[m, :A] = torch.where(c["legal"][m] != 0, torch.zeros(A), heads[m, :A])
            heads[m, a] = A / 64.0
    q = duel_q(heads[:, :A], heads[:, A], c["legal"], safe)["qa"]
    e = torch.tensor([_E_OF_MARK[mark[m]] if mark[m] else _E_UNMARKED[m % len(_E_UNMARKED)] for m in range(M)], dtype=torch.float64)
    ret = (q + e).float()
    ret[~good] = float("nan")
    return dict(c, heads=heads, ret=ret), mark


def check_case(c, mark, T, B, A):
    """the properties clone_value_case promises (asserted on the CPU): -> the float64 e of every row (0 where not good)"""
    valid, bad, good, safe = _rows(c, T, B, A)
    d = duel_q(c["heads"][:, :A], c["heads"][:, A], c["legal"], safe)
    e = torch.where(good, c["ret"].double() - d["qa"], torch.zeros(T * B, dtype=torch.float64))
    assert torch.isnan(c["ret"][~good]).all() and torch.isfinite(c["ret"][good]).all()
    for m in range(T * B):
        if not bool(good[m]):
            assert mark[m] is None
        elif mark[m] in ("zero", "plus_one", "minus_one"):
            assert float(e[m]) == _E_OF_MARK[mark[m]], (m, mark[m], float(e[m]))
            # ... and fp32 gets there without a rounding: the operands are multiples of 2^-6, the mean is one term over A
            z, l = c["heads"][m, :A], c["legal"][m]
            assert float((z * l).abs().sum()) == A / 64.0 and float(z[int(safe[m])]) == A / 64.0
            assert float(torch.tensor(A / 64.0, dtype=torch.float32) / A) == 1.0 / 64.0
        else:
            assert abs(abs(float(e[m])) - 1.0) >= KINK_MARGIN, (m, float(e[m]))
            assert float(d["qa_bound"][m]) + U * (abs(float(c["ret"][m])) + abs(float(d["qa"][m]))) < KINK_MARGIN / 4
            if mark[m] == "inside":
                assert abs(float(e[m])) < 0.5
            if mark[m] in ("outside_plus", "outside_minus"):
                assert abs(float(e[m])) > 2.0 and (float(e[m]) > 0) == (mark[m] == "outside_plus")
    return e


def clone_value_tail(heads, legal, action, ret, seq_len, weight, T, B, A, ldo, policy_weight=1.0, value_weight=1.0):
    """-> clone_loss_ref.clone_tail's dict (loss, hits, decisions, bad, multi, p; xent [T, B]) with
    dheads [T*B, ldo] of both terms BEFORE the bf16 rounding, vloss [B] (ascending-t sum), hub [T, B], steps [B], good [T*B],
    e / e_bound [T*B] (the error and the fp32 forward-error bound of it: duel_q's qa_bound plus the rounding of the subtraction),
    g [T*B], zero_row [T*B] (rows the kernel must write as all-zero bits), single [T*B] (good rows with one legal action)"""
    pol = P.clone_tail(heads, legal, action, seq_len, weight, T, B, A, ldo)
    c = dict(legal=legal, action=action, seq_len=seq_len)
    valid, bad, good, safe = _rows(c, T, B, A)
    M = T * B
    b_of = torch.arange(M) % B
    out = dict(pol)
    zero = torch.zeros(M, dtype=torch.float64)
    d = pol["dheads"] * float(policy_weight)
    e, e_bound, g, hub = zero.clone(), zero.clone(), zero.clone(), zero.clone()
    if value_weight != 0.0:
        dq = duel_q(heads[:, :A], heads[:, A], legal, safe)
        r = torch.where(good, ret.double(), zero)
        e = torch.where(good, r - dq["qa"], zero)
        e_bound = torch.where(good, dq["qa_bound"] + U * (r.abs() + dq["qa"].abs()), zero)
        hub = huber(e)
        g = -e.clamp(-1.0, 1.0)
        s = weight.double()[b_of] / B
        onehot = torch.zeros(M, A, dtype=torch.float64)
        onehot[torch.arange(M), safe] = 1.0
        l = (legal.double() != 0).double()
        d = d.clone()
        d[:, :A] += (s * float(value_weight) * g)[:, None] * l * (onehot - 1.0 / A) * good[:, None]
        d[:, A] = s * float(value_weight) * g
    vloss = torch.zeros(B, dtype=torch.float64)
    for t in range(T):
        vloss = vloss + hub.view(T, B)[t]
    out.update(dheads=d, vloss=vloss, hub=hub.view(T, B), steps=good.view(T, B).sum(0), good=good, e=e, e_bound=e_bound, g=g,
               zero_row=~good if value_weight != 0.0 else ~pol["multi"], single=good & ~pol["multi"])
    return out


def objective(heads, legal, action, ret, seq_len, weight, T, B, A, policy_weight, value_weight):
    """the same objective as torch autograd sees it (float64): policy_weight x the masked log_softmax loss + value_weight x smooth_l1
    of the dueling q at the action against ret, per row, summed over the valid rows, (. * weight).mean().  Bad rows must have been
    taken out by the caller (as in tests/test_clone_ref_cpu.py).  -> (objective, loss [B], vloss [B])"""
    M = T * B
    t_of, b_of = torch.arange(M) // B, torch.arange(M) % B
    valid = t_of.to(seq_len.dtype) < seq_len[b_of]
    _, loss = P.masked_log_softmax_loss(heads, legal, action, seq_len, weight, T, B, A)
    al = heads[:, :A] * legal
    q = heads[:, A:A + 1] + al - al.mean(1, keepdim=True)
    qa = q.gather(1, action.clamp(0, A - 1)[:, None])[:, 0]
    target = torch.where(valid, ret.to(heads.dtype), qa.detach())
    hub = torch.nn.functional.smooth_l1_loss(qa, target, reduction="none") * valid.to(heads.dtype)
    vloss = hub.view(T, B).sum(0)
    return ((policy_weight * loss + value_weight * vloss) * weight).mean(), loss, vloss
