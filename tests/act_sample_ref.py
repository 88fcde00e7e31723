"""Restatement of hanabi_sad_amd/csrc/hsad_act_sample.h, written from the definitions in its head comment: the hashes, the uniform and the
exploration draw in Python integers, Pick in float64 taken from the fp32 inputs, and the boundary rule a fp32 Pick is held to.

Boundary rule.  cdf_i = (w_0 + .. + w_i) / S over the legal actions in ascending order (float64); the interior boundaries are the cdf_i
of every legal action but the last.  The reference action is the first legal one with cdf_i > u.  Where u is farther than MARGIN from
every interior boundary the fp32 action must equal it; elsewhere it must be one of the two legal actions on either side of the nearest
boundary (boundaries at exactly the same distance -- weights that are exactly 0 in float64 put several at one value -- count as one:
either side of any of them).  MARGIN = 1e-5: an fp32 weight of relative size p carries a relative error of about |arg| 2^-24 c from the
division and the exponential's argument scaling plus a few ulp, so weighted by p it stays below 1e-6 for every term that matters, and
fifty terms do not reach 1e-5."""
import numpy as np

M64 = (1 << 64) - 1
ROW_MUL = 0xD1342543DE82EF95
SAMPLE_XOR = 0xA0761D6478BD642F
MARGIN = 1e-5
TAUS = (1e-6, 0.25, 1.0, 4.0, 1e6)


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def eps_hash(seed, m, counter):
    return mix64((mix64((seed ^ (ROW_MUL * m)) & M64) + counter) & M64)


def sample_hash(hh):
    return mix64(hh ^ SAMPLE_XOR)


def sample_hash_keyed(sample_seed, row_key):
    return mix64(mix64((sample_seed ^ (ROW_MUL * (row_key & M64))) & M64) ^ SAMPLE_XOR)


def u24(h):
    return (h >> 40) & 0xFFFFFF


def eps_draw(hh, eps, nlegal):
    """-> the index among the legal actions the exploration draw takes, or -1 when it does not fire (eps: the fp32 value)"""
    if not (eps > 0 and nlegal > 0):
        return -1
    if u24(hh) / 16777216.0 < float(np.float32(eps)):
        return ((hh & 0xFFFFFFFF) * nlegal) >> 32
    return -1


def pick(z, legal, tau, u):
    """z, legal: fp32 rows; tau: the fp32 temperature; u in [0, 1) -> (action, legal indices, cdf float64 over them); action -1 when
    nothing is legal"""
    idx = np.nonzero(np.asarray(legal) != 0)[0]
    if len(idx) == 0:
        return -1, idx, np.zeros(0)
    if len(idx) == 1:
        return int(idx[0]), idx, np.ones(1)
    zz = np.asarray(z, dtype=np.float32)[idx].astype(np.float64)
    w = np.exp((zz - zz.max()) / float(np.float32(tau)))
    cdf = np.cumsum(w) / w.sum()
    hit = np.nonzero(cdf > u)[0]
    return int(idx[hit[0]] if len(hit) else idx[-1]), idx, cdf


def judge(got, z, legal, tau, u, margin=MARGIN):
    """-> "exact" when `got` is the reference action of a row no boundary excuses, "excused" when u lies within the margin of a
    boundary and `got` is a neighbour of the nearest; raises AssertionError otherwise"""
    want, idx, cdf = pick(z, legal, tau, u)
    if len(idx) <= 1:
        assert got == want, "got %d, the only choice is %d" % (got, want)
        return "exact"
    d = np.abs(cdf[:-1] - u)
    if d.min() > margin:
        assert got == want, "got %d, reference %d, u %.9g, nearest boundary %.3g away" % (got, want, u, d.min())
        return "exact"
    allowed = set()
    for b in np.nonzero(d == d.min())[0]:
        allowed.update((int(idx[b]), int(idx[b + 1])))
    assert got in allowed, "got %d; u %.9g is %.3g from a boundary between %s (reference %d)" % (got, u, d.min(), sorted(allowed), want)
    return "excused"


def q_at(h, lg, act):
    """as_q_at in numpy float32 on rows h [n, A + 1] (A advantages, then the value), lg [n, A], act [n]:
    h[A] + h[act] * lg[act] - (sum_j h[j] * lg[j]) / A, the sum in ascending j, every operation rounded to fp32 -> fp32 [n]"""
    h, lg = np.atleast_2d(np.asarray(h, np.float32)), np.atleast_2d(np.asarray(lg, np.float32))
    A, r = lg.shape[1], np.arange(lg.shape[0])
    act = np.atleast_1d(act)
    s = np.zeros(lg.shape[0], np.float32)
    for j in range(A):
        s = s + h[:, j] * lg[:, j]
    return h[:, A] + h[r, act] * lg[r, act] - s / np.float32(A)


def tail_row(h, lg, mn, eps, m0, seed, counter):
    """as_tail_row without a temperature, in numpy float32, on rows m0, m0 + 1, .. (h [n, A + 1], lg [n, A], eps [n]; mn: the fp32 global
    minimum) -> greedy [n] (argmax of (1 + h[j] - mn) * lg[j], strict >: ties to the lowest index), a [n] (the exploration draw's legal
    action where it fires, else greedy), fires [n] (bool), nlegal [n].  On a row with a temperature whose draw does not fire the
    action is Pick's (judge); greedy and the exploration draw are the same there."""
    h, lg = np.atleast_2d(np.asarray(h, np.float32)), np.atleast_2d(np.asarray(lg, np.float32))
    n, A = lg.shape
    best, greedy = np.full(n, -3.4e38, np.float32), np.zeros(n, np.int64)
    for j in range(A):
        sc = (np.float32(1) + h[:, j] - np.float32(mn)) * lg[:, j]
        up = sc > best
        best, greedy = np.where(up, sc, best), np.where(up, j, greedy)
    nlegal = (lg != 0).sum(1)
    a, fires = greedy.copy(), np.zeros(n, bool)
    for i in range(n):
        k = eps_draw(eps_hash(seed, m0 + i, counter), eps[i], int(nlegal[i]))
        if k >= 0:
            a[i], fires[i] = np.nonzero(lg[i] != 0)[0][k], True
    return greedy, a, fires, nlegal


def bin_sigma(us, bins=21):
    """the largest deviation of the counts of `us` (values in [0, 1)) in equal bins from their mean, in standard deviations"""
    n = len(us)
    counts = np.bincount(np.minimum((np.asarray(us) * bins).astype(np.int64), bins - 1), minlength=bins)
    p = 1.0 / bins
    return float(np.abs(counts - n * p).max() / np.sqrt(n * p * (1 - p)))


# ------------------------------------------------------------------------------------------------------------------------------
# the seeded rows of tests/act_sample/act_sample_main.cc (both sides make them from this generator)
# ------------------------------------------------------------------------------------------------------------------------------
class Gen:
    def __init__(self, c):
        self.x = ((c + 1) * 0x9E3779B97F4A7C15) & M64

    def raw(self):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & M64
        return self.x

    def next(self):
        return self.raw() >> 33


def seeded_case(c, A, rows):
    """case c: seed, counter, sample_seed = raw() each, then per row
        mode = next() % 8 (0: nothing legal; 1: only action next() % A; 2: everything; else legal[j] = next() & 1 for each j),
        big = next() % 4 == 0,  z[j] = (next() & 0xFFFFF) - 524288, times 5/256 when big (|z| up to 10240) else 1/65536 (|z| < 8): exact
        in fp32,  eps = 0.3 when next() % 3 == 0 else 0,  row_key = raw() read as int64"""
    g = Gen(c)
    out = dict(seed=g.raw(), counter=g.raw(), sample_seed=g.raw(), z=np.zeros((rows, A), np.float32), legal=np.zeros((rows, A), np.float32),
               eps=np.zeros(rows, np.float32), key=np.zeros(rows, np.int64))
    for i in range(rows):
        mode = g.next() % 8
        if mode == 1:
            out["legal"][i, g.next() % A] = 1
        elif mode == 2:
            out["legal"][i] = 1
        elif mode > 2:
            out["legal"][i] = [g.next() & 1 for _ in range(A)]
        big = g.next() % 4 == 0
        k = np.array([(g.next() & 0xFFFFF) - 524288 for _ in range(A)], dtype=np.int64)
        out["z"][i] = (k * 5 / 256.0) if big else (k / 65536.0)
        out["eps"][i] = 0.3 if g.next() % 3 == 0 else 0.0
        r = g.raw()
        out["key"][i] = r - (1 << 64) if r >> 63 else r
    return out


def tail_case(c, A, rows):
    """the rows act_sample_main.cc gives as_tail_row in case c: the seeded rows, then three more that take z and the key of rows 0, 1, 2
    with no legal action, one legal action ((7 c + 3) % A) and all legal, eps = 0.3 in the even cases and 0 in the odd ones.  h = z and the
    value -z[A - 1] / 2 (exact) behind it; mn = the minimum of every z of the case, legal or not, as adv_min_kernel takes it."""
    k = seeded_case(c, A, rows)
    legal3 = np.zeros((3, A), np.float32)
    legal3[1, (7 * c + 3) % A] = 1
    legal3[2] = 1
    z = np.concatenate([k["z"], k["z"][:3]])
    return dict(k, h=np.concatenate([z, -z[:, A - 1:] * np.float32(0.5)], axis=1), legal=np.concatenate([k["legal"], legal3]),
                eps=np.concatenate([k["eps"], np.full(3, 0.0 if c % 2 else 0.3, np.float32)]), key=np.concatenate([k["key"], k["key"][:3]]),
                mn=np.float32(k["z"].min()))
