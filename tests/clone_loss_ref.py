"""TEST INFRASTRUCTURE: float64 reference of the behaviour-cloning loss on the head outputs, from its definition (include/hsad.h,
hsad_clone_tail).  Never imported by the product package.

Row m = t B + b: z = heads[m, :A], l = legal[m] (0 / 1), act = action[m]; valid = t < seq_len[b]; bad = valid and (act outside
[0, A) or l[act] == 0).  For the other valid rows xent = log sum_legal exp(z - mx) - (z[act] - mx) with mx = max_legal z, and
p = l exp(z - mx) / sum; a row with ONE legal action is xent = 0 and a zero gradient row by definition."""
import torch


def clone_tail(heads, legal, action, seq_len, weight, T, B, A, ldo):
    """heads [T*B, ldh], legal [T*B, A], action [T*B] int64, seq_len / weight [B] -> dict of float64 / int64 tensors:
    xent [T, B], loss [B] (ascending-t sum), hits / decisions / bad [B], dheads [T*B, ldo] BEFORE the bf16 rounding,
    zero_row [T*B] bool (rows the kernel must write as all-zero bits), p [T*B, A]"""
    z = heads.double()[:, :A]
    l = (legal.double() != 0)
    act = action.long()
    M = T * B
    t_of = torch.arange(M) // B
    b_of = torch.arange(M) % B
    valid = t_of.double() < seq_len.double()[b_of]
    in_range = (act >= 0) & (act < A)
    safe = act.clamp(0, A - 1)
    act_legal = l.gather(1, safe[:, None])[:, 0] & in_range
    bad = valid & ~act_legal
    good = valid & act_legal
    nlegal = l.sum(1)
    neg = torch.full_like(z, float("-inf"))
    zl = torch.where(l, z, neg)
    mx = torch.where(nlegal > 0, zl.max(1).values, torch.zeros(M, dtype=torch.float64))
    e = torch.where(l, torch.exp(z - mx[:, None]), torch.zeros_like(z))
    s = e.sum(1)
    multi = good & (nlegal >= 2)
    s1 = torch.where(multi, s, torch.ones_like(s))
    xent = torch.where(multi, torch.log(s1) - (z.gather(1, safe[:, None])[:, 0] - mx), torch.zeros_like(s))
    p = torch.where(multi[:, None], e / s1[:, None], torch.zeros_like(e))
    top = zl == zl.max(1, keepdim=True).values               # ties go to the lowest index: taken explicitly among the maxima
    first_max = torch.where(top, torch.arange(A)[None, :].expand(M, A), torch.full((M, A), A)).min(1).values
    hit = multi & (first_max == act)
    onehot = torch.zeros(M, A, dtype=torch.float64)
    onehot[torch.arange(M)[multi], act[multi]] = 1.0
    d = torch.zeros(M, ldo, dtype=torch.float64)
    d[:, :A] = (weight.double()[b_of] / B)[:, None] * (p - onehot) * multi[:, None]
    per_b = lambda x: x.view(T, B).sum(0)      # noqa: E731
    loss = torch.zeros(B, dtype=torch.float64)
    for t in range(T):
        loss = loss + xent.view(T, B)[t]
    return dict(xent=xent.view(T, B), loss=loss, hits=per_b(hit.long()), decisions=per_b(multi.long()), bad=per_b(bad.long()), dheads=d,
                zero_row=~multi, p=p, multi=multi)


def clone_case(A, ldh, T, B, seed=0):
    """one input set of the kernel test, on the CPU: logits on a dyadic grid (multiples of 2^-6 in [-8, 8]; +-30 rows), so that
    maxima, ties and with them hits / decisions are exact in fp32.  Sequence 0 runs the full length and carries the special rows,
    kind = (t + A) % 8: 0 a single legal action (the no-op), 1 every action legal, 2 logits +-30, 3 an illegal recorded action,
    4 an out-of-range one (A, -1, 2^40), 5 / 6 a tie at the top with the action on its second / first member, 7 ordinary.  With B = 3,
    sequence 1 stops in between (its later rows have NO legal action and wild action values) and sequence 2 has length 0."""
    g = torch.Generator().manual_seed(1000 * A + 10 * T + B + seed)
    M = T * B
    heads = torch.randint(-512, 513, (M, ldh), generator=g).float() / 64.0
    legal = (torch.rand(M, A, generator=g) < 0.4).float()
    legal[:, A - 1] = (legal[:, :A - 1].sum(1) == 0).float()
    two = legal.sum(1) < 2                                 # ordinary rows are decisions
    legal[two, 0] = 1.0
    legal[two, 1] = 1.0
    pick = torch.rand(M, A, generator=g) * legal
    action = pick.argmax(1)                                # a random legal action
    seq_len = torch.tensor([float(T), float(T // 2), 0.0][:B])
    weight = torch.tensor([1.5, 0.75, 2.0][:B])
    if B == 1 and T == 5:
        weight[0] = 0.0
    for t in range(T):
        m, kind = t * B, (t + A) % 8
        if kind == 0:
            legal[m] = 0.0
            legal[m, A - 1] = 1.0
            action[m] = A - 1
        elif kind == 1:
            legal[m] = 1.0
            action[m] = (7 * t) % A
        elif kind == 2:
            heads[m, :A] = torch.where(torch.arange(A) % 3 == 0, 30.0, -30.0)
            legal[m, 1] = 1.0                               # a legal -30 next to the legal +30s
            legal[m, 3] = 1.0
            action[m] = 1 if t % 2 else 3
        elif kind == 3:
            legal[m, 2] = 0.0
            action[m] = 2
        elif kind == 4:
            action[m] = (A, -1, 1 << 40)[t % 3]
        elif kind in (5, 6):
            heads[m, :A] = heads[m, :A].clamp(max=7.0)
            legal[m, 4] = legal[m, 9] = 1.0
            heads[m, 4] = heads[m, 9] = 8.0
            action[m] = 9 if kind == 5 else 4
    for b in range(1, B):
        for t in range(T):
            if t >= seq_len[b]:
                legal[t * B + b] = 0.0
                action[t * B + b] = (0, A + 3, -5)[t % 3]
    return dict(heads=heads, legal=legal, action=action, seq_len=seq_len, weight=weight)


def masked_log_softmax_loss(heads, legal, action, seq_len, weight, T, B, A):
    """the same objective as torch autograd sees it: illegal logits at -inf, log_softmax, gather, mask, (loss * weight).mean().
    Rows that are bad (illegal / out-of-range action) must not be handed in.  -> (objective, loss [B])"""
    z = heads[:, :A]
    t_of = torch.arange(T * B, device=z.device) // B
    valid = (t_of.to(seq_len.dtype) < seq_len[torch.arange(T * B, device=z.device) % B])
    # (a row past seq_len may have no legal action at all: it is masked below, and must not put log_softmax(all -inf) into the graph)
    zl = z.masked_fill((legal == 0) & valid[:, None], float("-inf"))
    logp = torch.log_softmax(zl, dim=1)
    picked = logp.gather(1, action.clamp(0, A - 1)[:, None])[:, 0]
    xent = torch.where(valid, -picked, torch.zeros_like(picked))
    loss = xent.view(T, B).sum(0)
    return (loss * weight).mean(), loss
