"""TEST INFRASTRUCTURE: float64 reference of the soft-target cloning tail on the head outputs, from its definition (include/hsad.h,
hsad_clone_soft_tail).  Never imported by the product package.

tests/clone_value_ref.py's clone_value_tail with the one-hot of the recorded action replaced by a target row pi [A] per row.  A valid row is
bad when its action is bad by that file's rule, a pi_j is negative or NaN, an illegal column has pi_j != 0, or |sigma - 1| > 1e-3 with
sigma = sum_legal pi_j.  For every other valid row with >= 2 legal actions
    xent = sigma log S - sum_legal pi_j (z_j - mx),     policy gradient column j: s policy_weight (sigma p_j - pi_j)
with mx, S, p as there; the value term, hits and decisions still go by the recorded action.  On one-hot targets (1.0 and zeros) every
float64 result EQUALS clone_value_tail's: sigma is 1, the products are exact, and the operations are written in that file's order.

Also here: row_f32, the fp32 restatement of ONE row in the order of operations of csrc/hsad_clone_soft.h (expf / logf are libm's, called
through ctypes, so that the stand-alone program of tests/clone_soft/clone_soft_main.cc can be held to it bit for bit)."""
import ctypes
import ctypes.util
import struct

import numpy as np
import torch

from tests import clone_value_ref as V

MASS_TOL = 1e-3


def rne(dheads):
    """what rounding the exact gradient to bf16 may move it by (+ the subnormal floor), as the sibling kernel tests grant it"""
    return dheads.abs() * 2.0 ** -8 + 2.0 ** -134


def target_ok(target, legal):
    """bool [M]: the row is a distribution over its legal actions (the three target rules; the action's rule is the caller's)"""
    pi = target.double()
    l = legal != 0
    nonneg = (pi >= 0).all(1)                                   # (a NaN fails the comparison)
    off = ((pi != 0) & ~l).any(1)
    sigma = torch.where(l, pi, torch.zeros_like(pi)).sum(1)
    return nonneg & ~off & ((sigma - 1.0).abs() <= MASS_TOL)


def one_hot_targets(action, seq_len, T, B, A):
    """float32 [T*B, A]: 1.0 at the action where it is in range (all zeros where not: such a row is bad by its action anyway);
    rows past seq_len are NaN -- the kernel must not read them"""
    M = T * B
    act = action.long()
    tg = torch.zeros(M, A, dtype=torch.float32)
    inr = (act >= 0) & (act < A)
    tg[torch.arange(M)[inr], act[inr]] = 1.0
    valid = (torch.arange(M) // B).double() < seq_len.double()[torch.arange(M) % B]
    tg[~valid] = float("nan")
    return tg


def soft_targets_case(c, T, B, A, seed=0):
    """seeded soft targets for a clone_value_case: on every valid row a distribution over the LEGAL actions -- random weights, about a
    third of them exactly 0, normalised in float64 and rounded to float32 (sigma within A 2^-24 of 1, as an honest row is); every
    fourth such row instead on the dyadic grid k / 64 (sigma exactly 1).  A row with no mass left gets it all on its first legal action.
    Rows past seq_len are NaN."""
    g = torch.Generator().manual_seed(4242 + 1000 * A + 10 * T + B + seed)
    M = T * B
    l = (c["legal"] != 0)
    w = torch.rand(M, A, generator=g, dtype=torch.float64) * (torch.rand(M, A, generator=g) > 0.33) * l
    first = torch.where(l, torch.arange(A)[None, :].expand(M, A), torch.full((M, A), A)).min(1).values.clamp(max=A - 1)
    empty = w.sum(1) == 0
    w[torch.arange(M)[empty], first[empty]] = 1.0
    pi = w / w.sum(1, keepdim=True)
    grid = torch.floor(pi * 64.0)
    grid[torch.arange(M), pi.argmax(1)] += 64.0 - grid.sum(1)         # the remainder goes to the largest entry
    use_grid = (torch.arange(M) % 4 == 3)
    pi = torch.where(use_grid[:, None], grid / 64.0, pi).float()
    valid = (torch.arange(M) // B).double() < c["seq_len"].double()[torch.arange(M) % B]
    pi[~valid] = float("nan")
    return pi


def clone_soft_tail(heads, legal, action, target, ret, seq_len, weight, T, B, A, ldo, policy_weight=1.0, value_weight=1.0):
    """-> clone_value_ref.clone_value_tail's dict with the policy term taken against `target` [T*B, A]:
    xent [T, B], loss [B] (ascending-t sum), dheads [T*B, ldo] BEFORE the bf16 rounding, the counters (bad includes the rows whose
    target is no distribution), and additionally sigma [T*B], target_bad [T*B] (valid rows bad by their target alone or too),
    e_xent [T*B] = 2 A 2^-24 max_legal |z_j - mx|: the fp32 summation bound of the extra dot product (A products, weights summing to at
    most 1.001), 0 on rows without a decision"""
    M = T * B
    t_of, b_of = torch.arange(M) // B, torch.arange(M) % B
    valid = t_of.double() < seq_len.double()[b_of]
    tbad = valid & ~target_ok(target, legal)
    action2 = torch.where(tbad, torch.full_like(action, -1), action)      # out of range: bad by the old rule, in every count
    base = V.clone_value_tail(heads, legal, action2, ret, seq_len, weight, T, B, A, ldo, policy_weight, value_weight)
    multi, p = base["multi"], base["p"]
    z = heads.double()[:, :A]
    l = legal.double() != 0
    zero = torch.zeros(M, A, dtype=torch.float64)
    pi = torch.where(multi[:, None] & l, target.double(), zero)
    sigma = pi.sum(1)
    zl = torch.where(l, z, torch.full_like(z, float("-inf")))
    mx = torch.where(l.any(1), zl.max(1).values, torch.zeros(M, dtype=torch.float64))
    dz = torch.where(l, z - mx[:, None], zero)
    s = torch.where(l, torch.exp(dz), zero).sum(1)
    s1 = torch.where(multi, s, torch.ones_like(s))
    xent = torch.where(multi, sigma * torch.log(s1) - (pi * dz).sum(1), torch.zeros_like(s))
    d = torch.zeros(M, ldo, dtype=torch.float64)
    d[:, :A] = (weight.double()[b_of] / B)[:, None] * (sigma[:, None] * p - pi) * multi[:, None]
    d = d * float(policy_weight)
    if value_weight != 0.0:      # the value term alone: clone_value_tail at policy weight 0
        d = d + V.clone_value_tail(heads, legal, action2, ret, seq_len, weight, T, B, A, ldo, 0.0, value_weight)["dheads"]
    loss = torch.zeros(B, dtype=torch.float64)
    for t in range(T):
        loss = loss + xent.view(T, B)[t]
    e_xent = torch.where(multi, 2.0 * A * 2.0 ** -24 * dz.abs().max(1).values, torch.zeros_like(s))
    out = dict(base)
    out.update(xent=xent.view(T, B), loss=loss, dheads=d, sigma=sigma, target_bad=tbad, e_xent=e_xent)
    return out


# ---- one row in fp32, in the header's order of operations -----------------------------------------------------------------------------
_libm = None


def libm():
    global _libm
    if _libm is None:
        m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for name in ("expf", "logf"):
            getattr(m, name).restype = ctypes.c_float
            getattr(m, name).argtypes = [ctypes.c_float]
        _libm = m
    return _libm


def row_f32(h, legal, pi, act, ret, policy_weight, value_weight, scale, ldo):
    """cs_row of csrc/hsad_clone_soft.h on numpy float32 scalars: h [A + 1], legal / pi [A] float32, act int, the rest floats ->
    dict(xent, hub float32; hit, dec, bad, step int; grad None | float32 [ldo])"""
    f = np.float32
    m = libm()
    ex = lambda x: f(m.expf(float(x)))      # noqa: E731
    A = len(legal)
    pw, vw, scale, ret = f(policy_weight), f(value_weight), f(scale), f(ret)
    out = dict(xent=f(0), hub=f(0), hit=0, dec=0, bad=0, step=0, grad=None)
    a = int(act) if 0 <= int(act) < A else -1
    mx, sigma, bi, nlegal, ok = f(-3.4e38), f(0), 0, 0, True
    with np.errstate(all="ignore"):
        for j in range(A):
            pj = pi[j]
            if not pj >= f(0):
                ok = False
            if legal[j] != 0:
                nlegal += 1
                sigma = f(sigma + pj)
                if h[j] > mx:
                    mx, bi = h[j], j
            elif pj != 0:
                ok = False
        if not abs(f(sigma - f(1))) <= f(MASS_TOL):
            ok = False
        if a < 0 or legal[a] == 0 or not ok:
            out["bad"] = 1
            return out
        out["step"] = 1
        multi = nlegal >= 2
        s = f(1)
        if multi:
            s, dot = f(0), f(0)
            for j in range(A):
                if legal[j] != 0:
                    s = f(s + ex(f(h[j] - mx)))
                    dot = f(dot + f(pi[j] * f(h[j] - mx)))
            out["xent"] = f(f(sigma * f(m.logf(float(s)))) - dot)
            out["dec"], out["hit"] = 1, int(bi == a)
        grad = np.zeros(ldo, dtype=np.float32)
        if vw == 0:
            if multi:
                sp, inv = f(scale * pw), f(f(1) / s)
                for j in range(A):
                    if legal[j] != 0:
                        grad[j] = f(sp * f(f(sigma * f(ex(f(h[j] - mx)) * inv)) - pi[j]))
                out["grad"] = grad
            return out
        mean = f(0)
        for j in range(A):
            mean = f(mean + f(h[j] * legal[j]))
        mean = f(mean / f(A))
        q = f(f(h[A] + f(h[a] * legal[a])) - mean)
        e = f(ret - q)
        ae = abs(e)
        out["hub"] = f(f(f(0.5) * e) * e) if ae < f(1) else f(ae - f(0.5))
        g = f(-min(max(e, f(-1)), f(1)))
        inv, invA = f(f(1) / s), f(f(1) / f(A))
        for j in range(A):
            d = f(1) if j == a else f(0)
            pol = f(pw * f(f(sigma * f(ex(f(h[j] - mx)) * inv)) - pi[j])) if multi else f(0)
            if legal[j] != 0:
                grad[j] = f(scale * f(pol + f(f(f(vw * g) * legal[j]) * f(d - invA))))
        grad[A] = f(f(scale * vw) * g)
        out["grad"] = grad
    return out


def write_rows(path, rows, A, ldo, policy_weight, value_weight):
    """the input file of clone_soft_main: int32 n, A, ldo; float32 policy_weight, value_weight; then per row h [A + 1], legal [A],
    pi [A] float32, act int64, ret, scale float32"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<iiiff", len(rows), A, ldo, policy_weight, value_weight))
        for r in rows:
            fh.write(np.asarray(r["h"], dtype="<f4").tobytes() + np.asarray(r["legal"], dtype="<f4").tobytes()
                     + np.asarray(r["pi"], dtype="<f4").tobytes() + struct.pack("<qff", int(r["act"]), float(r["ret"]), float(r["scale"])))


def seeded_rows(A, n, seed):
    """n rows for row_f32 / clone_soft_main: logits in +-8 (every fifth row +-30), 0 .. A legal actions, targets of every kind -- honest
    soft rows, one-hot rows, and one in eight broken (negative, NaN, mass on an illegal column, mass 0.9) --, actions legal, illegal and
    out of range"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        h = (rng.standard_normal(A + 1) * (30.0 if i % 5 == 4 else 3.0)).clip(-30, 30).astype(np.float32)
        legal = (rng.random(A) < (0.15, 0.5, 1.0)[i % 3]).astype(np.float32)
        if i % 11 == 0:
            legal[:] = 0
            legal[A - 1] = 1
        idx = np.nonzero(legal)[0]
        pi = np.zeros(A, dtype=np.float32)
        act = int(rng.integers(0, A))
        if len(idx):
            act = int(rng.choice(idx)) if i % 7 else act
            w = rng.random(len(idx)) * (rng.random(len(idx)) > 0.3)
            if w.sum() == 0 or i % 6 == 0:
                w = (idx == (act if legal[act] else idx[0])).astype(np.float64)
                if w.sum() == 0:
                    w[0] = 1.0
            pi[idx] = (w / w.sum()).astype(np.float32)
        if i % 13 == 5:
            act = (A, -1, 1 << 40)[i % 3]
        if i % 8 == 3 and len(idx) >= 2:
            kind = (i // 8) % 4
            if kind == 0:
                pi[idx[0]], pi[idx[1]] = np.float32(-0.25), np.float32(pi[idx[1]] + pi[idx[0]] + 0.25)
            elif kind == 1:
                pi[idx[0]] = np.nan
            elif kind == 2 and len(idx) < A:
                pi[np.nonzero(legal == 0)[0][0]] = np.float32(0.125)
            else:
                pi *= np.float32(0.9)
        rows.append(dict(h=h, legal=legal, pi=pi, act=act, ret=np.float32(rng.standard_normal() * 3.0), scale=np.float32(rng.random() * 2.0)))
    return rows
