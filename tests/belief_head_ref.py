"""TEST INFRASTRUCTURE: reference of the learned hand belief's row (include/hsad.h, hsad_belief_tail / hsad_env_determinize_belief),
written from its specification.  Never imported by the product package.

The counts are Python ints (tests/hand_belief_ref.count), everything else float64:
    w_i[t] = q[t] compat_i[t] C(slots after i, q - e_t),  F_i = {t: w_i[t] != 0},  p_i[t] = w_i[t] exp(z_i[t] - mx_i) / S_i on F_i
    nll = sum_i -log p_i[card_i],  nll0 = the same at z = 0,  gradient column i 25 + t = p_i[t] - [t == card_i] on F_i
with q the pool less the cards of the slots before i.  row() scores a hand, sample() draws one from per-slot uniforms, tail() is the
whole [T, B] call of hsad_belief_tail with its per-row error bounds.

Also here: row_f32, the fp32 restatement of ONE row in the order of operations of csrc/hsad_belief_head.h (expf / logf are libm's,
called through ctypes, so that tests/belief_head/belief_head_main.cc can be held to it bit for bit).

Error bounds (U = 2^-24, the unit round-off of fp32; a device row differs from the float64 row by no more than this):
  exp     the device's __expf(d) is the hardware exp2 (1 ulp = 2 U relative) of d log2(e) rounded to fp32 (|d| U relative on the
          result), d = z - mx itself rounded (|d| U): E_exp(d) = (4 + 2 |d|) U with 2 U to spare for the constant's own rounding
  v       (float)w (U) times exp (E_exp) rounded (U):  E_v = 2 U + E_exp(dmax), dmax = the slot's largest |z - mx| over F
  S       at most 25 positive terms added in order: E_S = 25 U + E_v (relative)
  log     __logf(x) is the hardware log2 (1 ulp) times ln 2 rounded: 4 U (|log x| + 1) absolute, plus the relative error of x
  nll_i   E_S + 4 U (|log S| + 1) + U + 4 U (|log wf| + 1) + U |log S - log wf| + 2 U |z_c - mx| + U |nll_i|
  row     the slot terms added in slot order: + 5 U sum_i |nll_i|;  nll[b]: the rows added in ascending t: + T U sum_t |row_t|
  p_i[t]  v / S: p (E_v + E_S + 4 U);  a gradient element g = scale (p - delta): the subtraction and the product round once each,
          scale (that + 2 U |p - delta|), and one bf16 rounding of the reference value
  sample  a slot's draw is decided by thr = uf S against the running sums of v: both within (2 E_S + 2 U) S of their float64
          values; a draw whose thr lies that close to a boundary may fall on either side and is reported as `near`"""
import ctypes
import ctypes.util
import math
import struct
from fractions import Fraction

import numpy as np

from tests import hand_belief_ref as HB
from tests.determinize_ref import M64, policy_hash

U = 2.0 ** -24
STREAM = 66   # the hash stream of the learned belief's draws (64: rejection sampler, 65: stratified rank)


# ---- packing (csrc/hsad_hand_count.h) ---------------------------------------------------------------------------------------------
def pack_pool(pool):
    return sum(int(c) << (2 * t) for t, c in enumerate(pool))


def unpack_pool(q):
    q = int(q) & M64
    return [(q >> (2 * t)) & 3 for t in range(25)]


def pack_mask(cm):
    return sum(int(b) << t for t, b in enumerate(cm))


def unpack_mask(m):
    return [(int(m) >> t) & 1 for t in range(25)]


def occupied(cards):
    """the number of occupied slots (those before the first -1); -1 when a card follows an empty slot"""
    cards = [int(c) for c in cards]
    n = 0
    while n < len(cards) and cards[n] != -1:
        n += 1
    return -1 if any(c != -1 for c in cards[n:]) else n


def weights(q, cms, i):
    """w_i[t] as Python ints, q = the pool before slot i"""
    later = tuple(range(i + 1, len(cms)))
    return [q[t] * HB.count(HB.less_one(q, t), cms, later) if q[t] and cms[i][t] else 0 for t in range(25)]


# ---- float64 ------------------------------------------------------------------------------------------------------------------------
def slot(z, w):
    """-> dict(F, mx, v [25], S, p [25], best, best0, dmax) of one slot; None when it has no feasible type"""
    F = [t for t in range(25) if w[t]]
    if not F:
        return None
    mx = max(float(z[t]) for t in F)
    v = [w[t] * math.exp(float(z[t]) - mx) if w[t] else 0.0 for t in range(25)]
    S = sum(v[t] for t in F)
    best = max(F, key=lambda t: (v[t], -t))
    best0 = max(F, key=lambda t: (w[t], -t))
    return dict(F=F, mx=mx, v=v, S=S, p=[x / S for x in v], best=best, best0=best0, dmax=max(abs(float(z[t]) - mx) for t in F),
                S0=sum(w[t] for t in F))


def slot_bounds(s, z, w, c):
    """(nll_i, nll0_i, e_nll_i, e_nll0_i, E_p) of a scored slot (module docstring)"""
    e_v = 2 * U + (4 + 2 * s["dmax"]) * U
    e_s = 25 * U + e_v
    nll = -math.log(s["p"][c])
    nll0 = -math.log(w[c] / s["S0"])
    lw = math.log(w[c])

    def e(logS, zterm, val, es):
        return es + 4 * U * (abs(logS) + 1) + U + 4 * U * (abs(lw) + 1) + U * abs(logS - lw) + 2 * U * abs(zterm) + U * abs(val)
    return (nll, nll0, e(math.log(s["S"]), float(z[c]) - s["mx"], nll, e_s), e(math.log(s["S0"]), 0.0, nll0, 25 * U + 8 * U),
            e_v + e_s + 4 * U)


def row(z, pool, cms, cards):
    """score one row.  z: [>= Hs * 25] logits; pool: 25 counts; cms: compat lists of ALL Hs slots (ignored past the occupied ones);
    cards: Hs card ids, -1 = empty.  -> dict(bad, nll, nll0, cards, hit, hit0, grad [Hs * 25] (p - one-hot, unscaled), e_nll, e_nll0,
    e_p [Hs * 25] (absolute bound on the device's p), abs_sum (sum_i |nll_i|, for the caller's summation bound), n, slots)"""
    Hs = len(cards)
    zero = dict(bad=1, nll=0.0, nll0=0.0, cards=0, hit=0, hit0=0, grad=[0.0] * (Hs * 25), e_nll=0.0, e_nll0=0.0, e_p=[0.0] * (Hs * 25),
                abs_sum=0.0, n=0, slots=[])
    n = occupied(cards)
    if n < 0 or any(not 0 <= int(c) < 25 for c in cards[:n]):
        return zero
    if any(not math.isfinite(float(z[j])) for j in range(n * 25)):
        return zero
    cms = [list(cm) for cm in cms[:n]]
    q = list(pool)
    out = dict(zero, bad=0, n=n, grad=list(zero["grad"]), e_p=list(zero["e_p"]), slots=[])
    abs0 = 0.0
    for i in range(n):
        w = weights(q, cms, i)
        c = int(cards[i])
        s = slot(z[i * 25:(i + 1) * 25], w)
        if s is None or not w[c]:
            return zero
        nll, nll0, e1, e0, ep = slot_bounds(s, z[i * 25:(i + 1) * 25], w, c)
        out["nll"] += nll
        out["nll0"] += nll0
        out["e_nll"] += e1
        out["e_nll0"] += e0
        out["abs_sum"] += abs(nll)
        abs0 += abs(nll0)
        if len(s["F"]) >= 2:
            out["cards"] += 1
            out["hit"] += int(s["best"] == c)
            out["hit0"] += int(s["best0"] == c)
        for t in s["F"]:
            out["grad"][i * 25 + t] = s["p"][t] - (1.0 if t == c else 0.0)
            out["e_p"][i * 25 + t] = s["p"][t] * ep
        out["slots"].append(dict(s, w=w, c=c))
        q[c] -= 1
    out["e_nll"] += 5 * U * out["abs_sum"]
    out["e_nll0"] += 5 * U * abs0
    out["abs_sum0"] = abs0
    out["q"] = q
    return out


def uniform_of(u32):
    return (int(u32) >> 8) * 2.0 ** -24


def sample(z, pool, cms, us):
    """draw a hand: us = one 32-bit uniform per occupied slot, cms = the occupied slots' compat lists.  -> dict(cards, q, logp, logp0,
    near (a draw lay within the fp32 bound of a boundary: the device may pick the neighbour), e_logp); None when a slot has no
    feasible type or a logit of an occupied slot is not finite"""
    n = len(cms)
    if any(not math.isfinite(float(z[j])) for j in range(n * 25)):
        return None
    q, cards, logp, logp0, near, e_logp, abs_sum = list(pool), [], 0.0, 0.0, False, 0.0, 0.0
    for i in range(n):
        w = weights(q, cms, i)
        zi = z[i * 25:(i + 1) * 25]
        s = slot(zi, w)
        if s is None:
            return None
        thr = uniform_of(us[i]) * s["S"]
        e_s = 25 * U + 2 * U + (4 + 2 * s["dmax"]) * U
        margin = (2 * e_s + 2 * U) * s["S"]
        run, c = 0.0, None
        for t in s["F"]:
            run += s["v"][t]
            if abs(run - thr) <= margin and t != s["F"][-1]:
                near = True
            if c is None and run > thr:
                c = t
        if c is None:
            c = s["F"][-1]
        if thr >= s["S"] - margin:      # the device's "none exceeds" fallback picks the last type too
            pass
        nll, nll0, e1, _, _ = slot_bounds(s, zi, w, c)
        logp -= nll
        logp0 -= nll0
        e_logp += e1
        abs_sum += abs(nll)
        cards.append(c)
        q[c] -= 1
    return dict(cards=cards, q=q, logp=logp, logp0=logp0, near=near, e_logp=e_logp + 5 * U * abs_sum)


def hand_distribution(z, pool, cms):
    """{hand tuple: prod_i p_i} over every hand the model can produce (small positions only)"""
    out = {}

    def walk(i, q, hand, pr):
        if i == len(cms):
            out[tuple(hand)] = pr
            return
        w = weights(q, cms, i)
        s = slot(z[i * 25:(i + 1) * 25], w)
        assert s is not None, "a dead end: the count factor should have removed it"
        for t in s["F"]:
            walk(i + 1, HB.less_one(q, t), hand + [t], pr * s["p"][t])
    walk(0, list(pool), [], 1.0)
    return out


def exact_conditionals(pool, cms, hand):
    """[{t: Fraction}] per slot: the conditionals of hand_belief_ref.unrank along `hand` (type t takes the next q[t] C(later, q - e_t)
    ranks of the slot's block)"""
    q, out = list(pool), []
    for i, card in enumerate(hand):
        w = weights(q, cms, i)
        tot = sum(w)
        out.append({t: Fraction(w[t], tot) for t in range(25) if w[t]})
        q[card] -= 1
    return out


def falling_product(pool, hand):
    q, pr = list(pool), 1
    for t in hand:
        pr *= q[t]
        q[t] -= 1
    return pr


def tail(logits, pool, compat, cards, seq_len, weight, T, B, Hs, ldo):
    """hsad_belief_tail on numpy arrays: logits [T*B, ldz], pool int64 [T, B] (packed), compat / cards int32 [T, B, Hs], seq_len /
    weight [B].  -> dict(nll, nll0, e_nll, e_nll0 float64 [B]; cards_n, hits, hits0, bad int [B]; dlogits float64 [T*B, ldo] before
    the bf16 rounding; e_d [T*B, ldo] the bound on a device element beyond that rounding; zero_row bool [T*B])"""
    M = T * B
    out = dict(nll=np.zeros(B), nll0=np.zeros(B), e_nll=np.zeros(B), e_nll0=np.zeros(B), cards_n=np.zeros(B, dtype=np.int64),
               hits=np.zeros(B, dtype=np.int64), hits0=np.zeros(B, dtype=np.int64), bad=np.zeros(B, dtype=np.int64),
               dlogits=np.zeros((M, ldo)), e_d=np.zeros((M, ldo)), zero_row=np.ones(M, dtype=bool))
    pool, compat, cards = np.asarray(pool).reshape(M), np.asarray(compat).reshape(M, Hs), np.asarray(cards).reshape(M, Hs)
    abs1, abs0 = np.zeros(B), np.zeros(B)
    for t in range(T):
        for b in range(B):
            if not float(t) < float(seq_len[b]):
                continue
            m = t * B + b
            r = row([float(x) for x in logits[m, :Hs * 25]], unpack_pool(pool[m]), [unpack_mask(x) for x in compat[m]], [int(c) for c in cards[m]])
            if r["bad"]:
                out["bad"][b] += 1
                continue
            s = float(weight[b]) / B
            out["nll"][b] += r["nll"]
            out["nll0"][b] += r["nll0"]
            out["e_nll"][b] += r["e_nll"]
            out["e_nll0"][b] += r["e_nll0"]
            abs1[b] += r["abs_sum"]
            abs0[b] += r["abs_sum0"]
            out["cards_n"][b] += r["cards"]
            out["hits"][b] += r["hit"]
            out["hits0"][b] += r["hit0"]
            out["dlogits"][m, :Hs * 25] = s * np.asarray(r["grad"])
            out["e_d"][m, :Hs * 25] = abs(s) * (np.asarray(r["e_p"]) + 2 * U * np.abs(np.asarray(r["grad"])))
            out["zero_row"][m] = False
    out["e_nll"] += T * U * abs1
    out["e_nll0"] += T * U * abs0
    return out


def rne(x):
    """what rounding the exact gradient to bf16 may move it by (+ the subnormal floor)"""
    return np.abs(x) * 2.0 ** -8 + 2.0 ** -134


# ---- one row in fp32, in the header's order of operations ---------------------------------------------------------------------------
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


def row_f32(z, pool, cms, cards=None, us=None, n_sample=0, scale=1.0, ldo=None):
    """bh_row of csrc/hsad_belief_head.h on numpy float32 scalars.  Score mode: cards (Hs ids, -1 = empty); sample mode: cards None,
    us [n_sample] 32-bit uniforms.  cms: compat lists of HC_MAX_SLOTS or fewer slots (missing ones are empty).  -> dict(bad, nll, nll0
    float32; cards, hit, hit0 int; hand [n] card ids; q 25 counts; grad None | float32 [ldo])"""
    f = np.float32
    m = libm()
    ex = lambda x: f(m.expf(float(x)))      # noqa: E731
    lg = lambda x: f(m.logf(float(x)))      # noqa: E731
    out = dict(bad=1, nll=f(0), nll0=f(0), cards=0, hit=0, hit0=0, hand=[], q=list(pool), grad=None)
    Hs = len(cards) if cards is not None else len(cms)
    n = occupied(cards) if cards is not None else int(n_sample)
    if n < 0 or n > Hs or Hs > 5:
        return out
    cms_n = [list(cm) for cm in cms[:n]]
    z = np.asarray(z, dtype=np.float32)

    def stats(zi, w):
        mx, best0, w0, nfeas, last, finite = f(-3.4e38), -1, 0, 0, -1, True
        for t in range(25):
            if not np.isfinite(zi[t]):
                finite = False
            if w[t] == 0:
                continue
            nfeas += 1
            last = t
            if zi[t] > mx:
                mx = zi[t]
            if w[t] > w0:
                w0, best0 = w[t], t
        S, S0, vbest, best = f(0), f(0), f(-1), -1
        v = [f(0)] * 25
        if finite:
            for t in range(25):
                if w[t] == 0:
                    continue
                v[t] = f(f(w[t]) * ex(f(zi[t] - mx)))
                S = f(S + v[t])
                S0 = f(S0 + f(w[t]))
                if v[t] > vbest:
                    vbest, best = v[t], t
        return dict(mx=mx, S=S, S0=S0, best=best, best0=best0, nfeas=nfeas, last=last, finite=finite, v=v)

    with np.errstate(all="ignore"):
        q, nll, nll0, ncards, hit, hit0, hand = list(pool), f(0), f(0), 0, 0, 0, []
        for i in range(n):
            zi = z[i * 25:(i + 1) * 25]
            w = weights(q, cms_n, i)
            st = stats(zi, w)
            if not st["finite"] or st["nfeas"] == 0:
                return out
            if cards is not None:
                c = int(cards[i])
                if not 0 <= c < 25 or w[c] == 0:
                    return out
            else:
                uf = f(f(int(us[i]) >> 8) * f(2.0 ** -24))
                thr = f(uf * st["S"])
                run, c = f(0), st["last"]
                for t in range(25):
                    if w[t] == 0:
                        continue
                    run = f(run + st["v"][t])
                    if run > thr:
                        c = t
                        break
            nll = f(nll + f(f(lg(st["S"]) - lg(f(w[c]))) - f(zi[c] - st["mx"])))
            nll0 = f(nll0 + f(lg(st["S0"]) - lg(f(w[c]))))
            if st["nfeas"] >= 2:
                ncards += 1
                hit += int(st["best"] == c)
                hit0 += int(st["best0"] == c)
            hand.append(c)
            q[c] -= 1
        out.update(bad=0, nll=nll, nll0=nll0, cards=ncards, hit=hit, hit0=hit0, hand=hand, q=q)
        if cards is not None and ldo is not None:
            grad = np.zeros(ldo, dtype=np.float32)
            q, scale = list(pool), f(scale)
            for i in range(n):
                zi = z[i * 25:(i + 1) * 25]
                w = weights(q, cms_n, i)
                st = stats(zi, w)
                inv = f(f(1) / st["S"])
                for t in range(25):
                    if w[t]:
                        grad[i * 25 + t] = f(scale * f(f(st["v"][t] * inv) - (f(1) if t == hand[i] else f(0))))
                q[hand[i]] -= 1
            out["grad"] = grad
    return out


# ---- seeded rows shared by the CPU and GPU tests --------------------------------------------------------------------------------------
def deal_case(rng, Hs, variant=False, hints=True):
    """a position as a game leaves it: a full deck (or a variant's, with absent types) less some played cards, a true hand of up to Hs
    cards drawn from what is left, per-slot masks that contain the true card and what hints of random colours / ranks would leave.
    -> (pool 25 counts, cms [Hs] compat lists (zeros past the hand), cards [Hs] (-1 past the hand))"""
    full = list(HB.FULL)
    if variant:
        for t in range(25):
            if t // 5 >= 3 or t % 5 >= 4:
                full[t] = 0
    deck = [t for t in range(25) for _ in range(full[t])]
    rng.shuffle(deck)
    gone = int(rng.integers(0, max(1, len(deck) - Hs - 2)))
    deck = deck[gone:]
    n = Hs if rng.random() < 0.8 else int(rng.integers(0, Hs + 1))
    n = min(n, len(deck))
    hand = [int(c) for c in deck[:n]]
    seen = int(rng.integers(0, len(deck) - n + 1))      # the other cards the viewer sees (partner's hand): not in its pool
    rest = deck[n + seen:]
    pool = [0] * 25
    for c in hand + list(rest):
        pool[c] += 1
    cms = []
    for c in hand:
        cp, rp = 31, 31
        if hints:
            for _ in range(int(rng.integers(0, 4))):
                if rng.random() < 0.5:
                    col = int(rng.integers(0, 5))
                    cp = (1 << col) if col == c // 5 else cp & ~(1 << col)
                else:
                    rk = int(rng.integers(0, 5))
                    rp = (1 << rk) if rk == c % 5 else rp & ~(1 << rk)
        cms.append([((cp >> (t // 5)) & 1) & ((rp >> (t % 5)) & 1) for t in range(25)])
    return pool, cms + [[0] * 25] * (Hs - n), hand + [-1] * (Hs - n)


def dead_end_case():
    """slot 1 is pinned to the last copy of a type that slot 0 could also take: a slot-wise sampler without the count factor runs
    into a dead end whenever slot 0 takes it"""
    pool = [0] * 25
    pool[4] = 1      # one 5 of colour 0 left
    pool[0] = 2
    pool[1] = 1
    cm0 = [1 if t // 5 == 0 else 0 for t in range(25)]      # slot 0: any card of colour 0
    cm1 = [1 if t == 4 else 0 for t in range(25)]           # slot 1: that 5
    return pool, [cm0, cm1], [0, 4]


def tail_case(T, B, Hs, ldz, seed, bad_every=0):
    """seeded inputs of hsad_belief_tail: logits in +-3 (every fifth row +-30), positions from deal_case, random seq_len and weights.
    bad_every > 0: every bad_every-th valid row is broken in one of four ways (a true card outside F, a card id of 25, a card behind
    an empty slot, a NaN logit).  -> dict of numpy arrays"""
    rng = np.random.default_rng(seed)
    M = T * B
    logits = np.zeros((M, ldz), dtype=np.float32)
    pool = np.zeros((T, B), dtype=np.int64)
    compat = np.zeros((T, B, Hs), dtype=np.int32)
    cards = np.full((T, B, Hs), -1, dtype=np.int32)
    seq_len = np.asarray([float(rng.integers(0, T + 1)) for _ in range(B)], dtype=np.float32)
    seq_len[0] = T
    weight = rng.random(B).astype(np.float32) * 2
    k = 0
    for t in range(T):
        for b in range(B):
            m = t * B + b
            logits[m] = (rng.standard_normal(ldz) * (30.0 if m % 5 == 4 else 3.0)).clip(-30, 30)
            pl, cms, hand = deal_case(rng, Hs, variant=(m % 7 == 3))
            while m == 0 and occupied(hand) != Hs:      # (the first row always scores a full hand: the T = 1, B = 1 case is that row alone)
                pl, cms, hand = deal_case(rng, Hs)
            if t < seq_len[b]:
                k += 1
                if bad_every and k % bad_every == 0:
                    kind = (k // bad_every) % 4
                    n = occupied(hand)
                    if kind == 0 and n:
                        cms[0] = [0 if t_ == hand[0] else 1 for t_ in range(25)]
                    elif kind == 1 and n:
                        hand[n - 1] = 25
                    elif kind == 2 and n < Hs and Hs >= 2:
                        hand = [-1] + hand[:Hs - 1]
                        hand[1] = hand[1] if hand[1] != -1 else 3
                    else:
                        if n:
                            logits[m, int(rng.integers(0, n * 25))] = np.nan
            pool[t, b] = np.int64(pack_pool(pl))
            compat[t, b] = [pack_mask(cm) for cm in cms]
            cards[t, b] = hand
    return dict(logits=logits, pool=pool, compat=compat, cards=cards, seq_len=seq_len, weight=weight)


def write_rows(path, rows, Hs, ldo):
    """the input file of belief_head_main: int32 n, Hs, ldo; then per row: int32 mode (0 score, 1 sample), n_sample; uint64 pool;
    uint32 cm [5]; int32 cards [Hs]; uint32 u [5]; float32 scale; float32 z [Hs * 25]"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<iii", len(rows), Hs, ldo))
        for r in rows:
            cm = [pack_mask(c) for c in r["cms"]] + [0] * (5 - len(r["cms"]))
            us = list(r.get("us") or []) + [0] * 5
            cards = list(r["cards"]) if r.get("cards") is not None else [-1] * Hs
            fh.write(struct.pack("<iiQ5I", 0 if r.get("cards") is not None else 1, int(r.get("n_sample", 0)), pack_pool(r["pool"]), *cm[:5]))
            fh.write(struct.pack("<%di5If" % Hs, *cards, *[int(u) for u in us[:5]], float(r["scale"])))
            fh.write(np.asarray(r["z"], dtype="<f4").tobytes())


def draws(seed, key, n):
    return [policy_hash(seed, key & M64, i, STREAM) for i in range(n)]
