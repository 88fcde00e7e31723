"""The kernels of csrc/r2d2/heads_loss_optim.inc and csrc/r2d2/act.inc, each called directly through ctypes and held to the float64
references of tests/heads_loss_ref.py: values inside the derived forward-error bound (roundings x 2^-24 x sum of |terms|), greedy and
chosen actions EXACT (inputs on a dyadic grid: distinct scores differ by >= 2^-6, equal scores come from identical operations), every
written buffer between two guard bands.

The own-hand cross-entropy and its gradient go through __expf / __logf (expf in the fp32 mode), whose error is measured, not derived:
AUX_MEASURED holds the largest errors seen on an MI355X against the float64 reference (also written on every run to
heads_loss_measured_errors.json, beside the r2d2_measured_errors.json of tests/test_r2d2_precision_gpu.py, and quoted in DESIGN.md 3c);
the tolerance is twice that, and never more than the 1e-4 per step that fp32 round-off is granted elsewhere in the suite."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import heads_loss_ref as R
from tests.test_r2d2_precision_gpu import OUT as R2D2_MEASURED

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
OUT = os.path.join(os.path.dirname(R2D2_MEASURED), "heads_loss_measured_errors.json")      # the directory of measured errors

# (A, NP, ldh): the standard game, a small variant, the 5-player variant (R = 138 / 88 staged rows), both sides of the A <= 32 switch
SHAPES = [(21, 15, 37), (12, 6, 19), (49, 12, 62), (32, 15, 48), (33, 15, 49)]
SHAPE_IDS = ["A%d" % s[0] for s in SHAPES]

# largest errors measured on an MI355X (this file's record() calls), and the tolerances they give
# xent_step: |xent of one (t, b) - float64| of hsad_aux_xent / hsad_loss_tail (__expf, __logf; logits up to +-30);
# softmax: error of a softmax probability in hsad_heads_backward_f32's aux columns (the bf16 outputs showed no excess over their rounding)
AUX_MEASURED = {"xent_step": 2.58e-6, "softmax": 1.67e-7}
FP32_STEP = 1e-4                                      # TOL["fp32"] of tests/test_r2d2_precision_gpu.py: the cap, and the limit until measured


def aux_tol(kind):
    m = AUX_MEASURED[kind]
    return FP32_STEP if m is None else min(FP32_STEP, 2.0 * m)


# (1 + u)^n - 1 <= n u / (1 - n u): with n <= 1600 roundings the first-order bound grows by less than this factor
SECOND_ORDER = 1.0001
SENT = -7.25e9          # guard bands and never-written output elements (int buffers: -77)


def record(test, **vals):
    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        data = json.load(open(OUT)) if os.path.exists(OUT) else {}
        old = data.get(test, {})
        data[test] = {k: max(float(v), float(old.get(k, 0.0))) for k, v in vals.items()}
        json.dump(data, open(OUT, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


class Pool:
    """device buffers with a guard band of 64 elements on both sides; outputs start out filled with the guard value"""
    PAD = 64

    def __init__(self):
        self.raw = []

    @staticmethod
    def _sent(dtype):
        return SENT if dtype.is_floating_point else -77

    def new(self, shape, dtype=torch.float32, like=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape)) if len(shape) else 1
        raw = torch.full((n + 2 * self.PAD,), self._sent(dtype), dtype=dtype, device=DEV)
        t = raw[self.PAD:self.PAD + n].view(shape)
        if like is not None:
            t.copy_(torch.as_tensor(like).to(dtype))
        self.raw.append(raw)
        return t

    def put(self, x):
        x = torch.as_tensor(x)
        return self.new(x.shape, x.dtype, like=x)

    def check(self):
        torch.cuda.synchronize()
        for k, raw in enumerate(self.raw):
            s = torch.full((1,), self._sent(raw.dtype), dtype=raw.dtype, device=DEV)
            assert bool((raw[:self.PAD] == s).all()) and bool((raw[-self.PAD:] == s).all()), "guard band of buffer %d was written" % k


def untouched(t):
    return bool((t == torch.full((1,), Pool._sent(t.dtype), dtype=t.dtype, device=DEV)).all())


def p(t):
    return None if t is None else t.data_ptr()


def d64(t):
    return t.detach().cpu().double()


def within(got, ref, bound, what=""):
    got, ref, bound = d64(got), R.f64(ref), R.f64(bound) * SECOND_ORDER
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    over = (got - ref).abs() - bound
    assert bool(torch.isfinite(got).all()) and float(over.max()) <= 0.0, \
        "%s: error %.3e over a bound of %.3e at %d" % (what, float((got - ref).abs().flatten()[over.argmax()]),
                                                       float(bound.flatten()[over.argmax()]), int(over.argmax()))


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.dtype == torch.bfloat16 else t.dtype)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def lib():
    from hanabi_sad_amd import _lib
    L = _lib.load_library()
    P, I = C.c_void_p, C.c_int
    local = {   # the library-internal seams hsad_learner.hip uses (declared there, not in include/hsad.h)
        "hsad_internal_heads_q_supported": (I, [I, I, I, I, P, P, P, P]),
        "hsad_internal_heads_q": (I, [P, P, P, P, P, P, I, I, I, I, P, P, P, P, P, P, P, P]),
        "hsad_internal_loss_tail": (I, [P, P, I, P, P, P, P, I, P, P, P, P, P, P, I, I, I, I, I, C.c_double, C.c_float, P, P, P, P, P, P, P,
                                        P, I, P, C.c_int64, P, P, I, P]),
    }
    for name, (res, args) in local.items():
        if name not in _lib.SIGNATURES:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


@pytest.fixture(scope="module")
def st():
    from hanabi_sad_amd.r2d2 import _s
    return _s(torch.device(DEV))


def ok(rc):
    from hanabi_sad_amd import _lib
    _lib.check(rc)


@pytest.fixture(autouse=True)
def _end_the_session_after_a_device_fault():
    """a kernel that faulted leaves the context unusable: nothing more of this session may be started on the device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the device reported a fault: %s" % e, returncode=3)


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def dyadic(shape, g, lim=8):
    """multiples of 2^-6 in [-lim, lim]"""
    return torch.randint(-64 * lim, 64 * lim + 1, shape, generator=g).float() / 64.0


def legal_moves(N, A, g):
    legal = (torch.rand(N, A, generator=g) < 0.4).float()
    legal[:, A - 1] = (legal[:, :A - 1].sum(1) == 0).float()
    return legal


def argmax_inputs(N, A, ldh, g):
    """heads [N, ldh] (advantage and value on the dyadic grid) + legal [N, A] with ties at the top (rows 0, 7, ..: two legal moves at the
    grid's maximum, the first must win), all-negative rows (3, 14, ..) and rows without a legal move (5, 18, ..)"""
    h = dyadic((N, ldh), g)
    legal = legal_moves(N, A, g)
    i = torch.arange(N)
    tie = i % 7 == 0
    j1 = (i // 7) % (A - 1)
    h[i[tie], j1[tie]] = 8.0
    h[tie, A - 1] = 8.0
    legal[i[tie], j1[tie]] = 1.0
    legal[tie, A - 1] = 1.0
    neg = i % 11 == 3
    h[neg, :A] = -h[neg, :A].abs() - 1.0 / 64
    legal[i % 13 == 5] = 0.0
    return h, legal


def own_hand_rows(M, NP, g):
    """one-hot or empty slots: rows 0, 3, .. all slots filled, rows 1, 4, .. some empty, rows 2, 5, .. all empty"""
    slots = NP // 3
    kind = torch.randint(0, 3, (M, slots), generator=g)
    some = torch.rand(M, slots, generator=g) < 0.5
    some[:, 0] = True
    some[:, -1] = False
    own = torch.zeros(M, slots, 3)
    for k in range(3):
        own[..., k] = (kind == k).float()
    i = torch.arange(M)
    own[i % 3 == 1] *= some[i % 3 == 1].float()[..., None]
    own[i % 3 == 2] = 0
    return own.view(M, NP)


def aux_logits(h, A, NP, g):
    """aux logits in [-4, 4]; rows 0, 5, .. at +-30 (the max subtraction does the work there)"""
    M = h.shape[0]
    lg = torch.rand(M, NP, generator=g) * 8 - 4
    far = torch.arange(M) % 5 == 0
    lg[far] = torch.where(torch.rand(int(far.sum()), NP, generator=g) < 0.5, -30.0, 30.0)
    h[:, A + 1:A + 1 + NP] = lg
    return h


# ---------------------------------------------------------------------------------------------------
# hsad_q_head
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,NP,ldh", SHAPES, ids=SHAPE_IDS)
def test_q_head_against_float64(lib, st, A, NP, ldh):
    for M in (1, 255, 256, 257, 700):
        g = torch.Generator().manual_seed(1000 * A + M)
        h, legal = argmax_inputs(M, A, ldh, g)
        action = torch.randint(0, A, (M,), generator=g)
        ref = R.duel_q(h[:, :A], h[:, A], legal, action)
        nb = (M + 255) // 256
        for with_action in (True, False):
            for with_greedy in (True, False):
                pool = Pool()
                dh, dl, da = pool.put(h), pool.put(legal), pool.put(action)
                q, qa, gr, scratch = pool.new((M, A)), pool.new(M), pool.new(M, torch.int64), pool.new(2 + nb)
                ok(lib.hsad_q_head(p(dh), ldh, p(dl), p(da) if with_action else None, M, A, p(q), p(qa) if with_action else None,
                                   p(gr) if with_greedy else None, p(scratch), st))
                pool.check()
                tag = "q_head A=%d M=%d action=%d greedy=%d" % (A, M, with_action, with_greedy)
                within(q, ref["q"], ref["q_bound"], tag + " q")
                if with_action:
                    within(qa, ref["qa"], ref["qa_bound"], tag + " qa")
                    assert same_bits(qa, q.gather(1, da.view(-1, 1))[:, 0]), tag
                else:
                    assert untouched(qa), tag
                # the scratch contract: scratch[1 + i] = min of q over rows [256 i, 256 i + 256), scratch[0] = the global minimum
                # (written with a greedy output only: nobody reads it otherwise)
                mins = torch.stack([q[256 * i:256 * (i + 1)].min() for i in range(nb)])
                assert same_bits(scratch[1:1 + nb], mins), tag
                if with_greedy:
                    assert same_bits(scratch[:1], q.min().view(1)), tag
                    assert torch.equal(gr.cpu(), ref["greedy"]), tag
                else:
                    assert untouched(gr) and untouched(scratch[:1]), tag


# ---------------------------------------------------------------------------------------------------
# hsad_q_at, hsad_act_select, _q, _q2
# ---------------------------------------------------------------------------------------------------
def eps_variants(N, g):
    mixed = torch.tensor([0.0, 0.05, 0.25, 0.5, 1.0])[torch.randint(0, 5, (N,), generator=g)]
    return [("null", None), ("zero", torch.zeros(N)), ("one", torch.ones(N)), ("mixed", mixed)]


@pytest.mark.parametrize("A,NP,ldh", SHAPES, ids=SHAPE_IDS)
def test_acting_tail_against_float64_and_the_hash(lib, st, A, NP, ldh):
    seed = 0xC0FFEE123
    for N in (1, 255, 257, 1000):
        g = torch.Generator().manual_seed(2000 * A + N)
        h, legal = argmax_inputs(N, A, ldh, g)
        ht = dyadic((N, ldh), g)
        nb = (N + 255) // 256
        for name, eps in eps_variants(N, g):
            explored = {}
            for counter in (9, 10):
                ref = R.act_tail(h[:, :A], h[:, A], legal, eps, seed, counter, ht[:, :A], ht[:, A])
                pool = Pool()
                dh, dt, dl = pool.put(h), pool.put(ht), pool.put(legal)
                de = None if eps is None else pool.put(eps)
                a = [pool.new(N, torch.int64) for _ in range(3)]
                gr = [pool.new(N, torch.int64) for _ in range(3)]
                qa = [pool.new(N) for _ in range(2)]
                tq, tq_at, scratch = pool.new(N), pool.new(N), [pool.new(2 + nb) for _ in range(3)]
                ok(lib.hsad_act_select(p(dh), ldh, p(dl), p(de), N, A, seed, counter, p(a[0]), p(gr[0]), p(scratch[0]), st))
                ok(lib.hsad_act_select_q(p(dh), ldh, p(dl), p(de), N, A, seed, counter, p(a[1]), p(gr[1]), p(qa[0]), p(scratch[1]), st))
                ok(lib.hsad_act_select_q2(p(dh), p(dt), ldh, p(dl), p(de), N, A, seed, counter, p(a[2]), p(gr[2]), p(qa[1]), p(tq),
                                          p(scratch[2]), st))
                ok(lib.hsad_q_at(p(dt), ldh, p(dl), p(gr[2]), N, A, p(tq_at), st))
                pool.check()
                tag = "act A=%d N=%d eps=%s counter=%d" % (A, N, name, counter)
                for k in range(3):      # exact, and therefore identical between the three entry points
                    assert torch.equal(gr[k].cpu(), ref["greedy"]), tag + " greedy of entry %d" % k
                    assert torch.equal(a[k].cpu(), ref["a"]), tag + " action of entry %d" % k
                for k in range(2):
                    within(qa[k], ref["qa"], ref["qa_bound"], tag + " qa")
                within(tq, ref["tq"], ref["tq_bound"], tag + " q_target(greedy)")
                within(tq_at, ref["tq"], ref["tq_bound"], tag + " q_at")
                assert same_bits(qa[0], qa[1]) and same_bits(tq, tq_at), tag
                has_legal = legal.sum(1) > 0
                assert bool((legal.gather(1, ref["a"].view(-1, 1))[:, 0][has_legal] == 1).all()), tag
                if name in ("null", "zero"):
                    assert torch.equal(a[0], gr[0]) and not bool(ref["explore"].any()), tag
                if name == "one":
                    assert torch.equal(ref["explore"], has_legal), tag
                explored[counter] = (ref["explore"], a[1].cpu())
            if name == "mixed" and N >= 255:
                # the draw depends on the counter: other rows explore, other moves are drawn
                assert not torch.equal(explored[9][0], explored[10][0]) and not torch.equal(explored[9][1], explored[10][1])


# ---------------------------------------------------------------------------------------------------
# hsad_td_loss, hsad_nstep_priority
# ---------------------------------------------------------------------------------------------------
PLANTED = [1.0, -1.0, 1.0 - 2.0 ** -20, -(1.0 - 2.0 ** -20), 1.0 + 2.0 ** -20, -(1.0 + 2.0 ** -20)]


def td_inputs(T, B, g):
    qa, tq, r = torch.randn(T, B, generator=g) * 3, torch.randn(T, B, generator=g) * 3, torch.randn(T, B, generator=g)
    boot = (torch.rand(T, B, generator=g) < 0.8).float()
    seq_len = torch.tensor([(T, T - 1, 1, 0)[b % 4] for b in range(B)], dtype=torch.float32)
    planted = []
    for k, e in enumerate(PLANTED[:T]):      # sequence 0 has full length: errors of exactly +-1 and one ulp-scale step to either side
        boot[k, 0], r[k, 0], qa[k, 0] = 0.0, 0.5, 0.5 - e
        planted.append((k, 0, e))
    return qa, tq, r, boot, seq_len, planted


@pytest.mark.parametrize("T", [1, 2, 3, 80, 129, 300])
def test_td_loss_and_nstep_priority_against_float64(lib, st, T):
    variants = [(0.999, True, True), (1.0, False, True), (0.999, True, False), (1.0, False, False), (1.0, True, True), (0.999, False, True)]
    for B in (1, 3, 130):
        g = torch.Generator().manual_seed(3000 * T + B)
        qa, tq, r, boot, seq_len, planted = td_inputs(T, B, g)
        weight = torch.rand(B, generator=g) + 0.5
        for n in (1, 3, T, T + 2):
            for gamma, with_w, with_dqa in variants:
                ref = R.td(qa, tq, r, boot, seq_len, n, gamma, weight if with_w else None)
                pool = Pool()
                dq, dt, dr, db, dl, dw = (pool.put(x) for x in (qa, tq, r, boot, seq_len, weight))
                err, prio, dqa, loss, pri_n = pool.new((T, B)), pool.new((T, B)), pool.new((T, B)), pool.new(B), pool.new((T, B))
                ok(lib.hsad_td_loss(p(dq), p(dt), p(dr), p(db), p(dl), T, B, n, gamma, p(err), p(prio), p(loss), p(dqa) if with_dqa else None,
                                    p(dw) if with_w else None, st))
                ok(lib.hsad_nstep_priority(p(dq), p(dt), p(dr), p(db), n, gamma, T * B, p(pri_n), st))
                pool.check()
                tag = "td T=%d B=%d n=%d gamma=%g w=%d dqa=%d" % (T, B, n, gamma, with_w, with_dqa)
                within(err, ref["err"], ref["err_bound"], tag + " err")
                within(prio, ref["priority"], ref["err_bound"], tag + " priority")
                within(loss, ref["loss"], ref["loss_bound"], tag + " loss")
                assert same_bits(prio, err.abs()), tag
                off = (1 - ref["mask"]).bool()
                assert float(d64(err)[off].abs().sum()) == 0.0 and float(d64(prio)[off].abs().sum()) == 0.0, tag + ": masked steps"
                if with_dqa:
                    within(dqa, ref["dqa"], ref["dqa_bound"], tag + " dqa")
                    assert float(d64(dqa)[off].abs().sum()) == 0.0, tag + ": masked steps of dqa"
                else:
                    assert untouched(dqa), tag
                for t, b, e in planted:          # reward 0.5, bootstrap 0, qa = 0.5 - e: every operation is exact
                    assert float(err[t, b]) == e, (tag, t, e)
                    if with_dqa:
                        want = np.float32(-max(-1.0, min(1.0, e))) * np.float32(float(weight[b]) if with_w else 1.0) / np.float32(B)
                        assert float(dqa[t, b]) == float(want), (tag, t, e)
                # the acting side's priority of the same numbers: target_qa already belongs to step t + n there (no shift, no mask)
                pr, pb = R.nstep_priority(qa, tq, r, boot, n, gamma)
                within(pri_n, pr, pb, tag + " nstep_priority")


# ---------------------------------------------------------------------------------------------------
# hsad_aux_xent, hsad_heads_backward, hsad_heads_backward_f32
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,NP,ldh", SHAPES, ids=SHAPE_IDS)
def test_aux_xent_against_float64(lib, st, A, NP, ldh):
    worst = 0.0
    for T in (1, 7):
        for B in (1, 3, 130):
            M = T * B
            g = torch.Generator().manual_seed(4000 * A + M)
            h = aux_logits(torch.randn(M, ldh, generator=g), A, NP, g)
            own = own_hand_rows(M, NP, g)
            xs_ref, steps = R.aux_xent(h[:, A + 1:A + 1 + NP], own, T, B)
            pool = Pool()
            dh, do = pool.put(h), pool.put(own)
            xs = pool.new(B)
            ok(lib.hsad_aux_xent(p(dh), ldh, p(do), T, B, A, NP, p(xs), st))
            pool.check()
            e = (d64(xs) - xs_ref).abs()
            worst = max(worst, float(e.max()) / T)
            assert bool(torch.isfinite(xs).all()) and float(e.max()) <= T * aux_tol("xent_step"), ("aux_xent", A, T, B, float(e.max()))
            if T == 1:      # an empty mask gives exactly zero
                empty = own.sum(1) == 0
                assert bool(empty.any()) or M == 1
                assert float(d64(xs)[empty].abs().sum()) == 0.0
    record("aux_xent", xent_step=worst)


@pytest.mark.parametrize("A,NP,ldh", SHAPES, ids=SHAPE_IDS)
def test_heads_backward_against_float64_autograd(lib, st, A, NP, ldh):
    worst = {"softmax_f32": 0.0, "softmax_bf16_excess": 0.0}
    for T, B in ((5, 3), (50, 3)):
        M = T * B
        g = torch.Generator().manual_seed(5000 * A + M)
        h = aux_logits(dyadic((M, ldh), g), A, NP, g)
        legal, action = legal_moves(M, A, g), torch.randint(0, A, (M,), generator=g)
        own, weight, dqa = own_hand_rows(M, NP, g), torch.rand(B, generator=g) + 0.5, torch.randn(M, generator=g) / B
        for pred_scale in (0.0, float(np.float32(0.25) / np.float32(B))):
            for with_own in (True, False):
                gref, gbound, scale = R.head_grad(h, legal, action, dqa, A, own if with_own else None, weight, pred_scale, B)
                ncol = A + 1 + (NP if with_own else 0)
                aux_on = with_own and pred_scale != 0.0
                for ldo in (64, A + 1 + NP):
                    for f32 in (True, False):
                        pool = Pool()
                        dh, dl, da, do, dw, dd = (pool.put(x) for x in (h, legal, action, own, weight, dqa))
                        out = pool.new((M, ldo), torch.float32 if f32 else torch.bfloat16)
                        fn = lib.hsad_heads_backward_f32 if f32 else lib.hsad_heads_backward
                        ok(fn(p(dd), p(dl), p(da), p(dh), ldh, p(do) if with_own else None, p(dw), M, B, A, NP, pred_scale, p(out), ldo, st))
                        pool.check()
                        tag = "heads_backward A=%d M=%d scale=%g own=%d ldo=%d f32=%d" % (A, M, pred_scale, with_own, ldo, f32)
                        got = d64(out)
                        ulp = 0.0 if f32 else R.BF16_ULP
                        # dueling part: the derived bound (fp32), plus one bf16 ulp of the reference (bf16)
                        within(got[:, :A], gref[:, :A], gbound[:, :A] + ulp * gref[:, :A].abs(), tag + " advantage")
                        within(got[:, A], R.f64(dqa), ulp * R.f64(dqa).abs(), tag + " value")
                        # columns past the last gradient column are exactly zero
                        last = A + 1 + (NP if aux_on else 0)
                        assert float(got[:, last:].abs().sum()) == 0.0, tag
                        if aux_on:
                            e = (got[:, A + 1:ncol] - gref[:, A + 1:]).abs()
                            tol = aux_tol("softmax") * scale[:, None] + ulp * gref[:, A + 1:].abs()
                            assert float((e - tol).max()) <= 0.0, (tag, float(e.max()))
                            live = scale > 0
                            rel = (e - ulp * gref[:, A + 1:].abs()).clamp(min=0)[live] / scale[live][:, None]
                            key = "softmax_f32" if f32 else "softmax_bf16_excess"
                            worst[key] = max(worst[key], float(rel.max()))
                            # an empty mask: exactly zero aux gradient
                            empty = own.sum(1) == 0
                            assert float(got[empty][:, A + 1:].abs().sum()) == 0.0, tag
    record("heads_backward", **worst)


# ---------------------------------------------------------------------------------------------------
# hsad_loss_tail against float64 and against the chain of entry points it replaces
# ---------------------------------------------------------------------------------------------------
def tail_inputs(T, B, A, NP, ldh, seed, plant_min=False):
    g = torch.Generator().manual_seed(seed)
    M = T * B
    h, legal = argmax_inputs(M, A, ldh, g)
    h[:, A] = dyadic((M,), g, lim=2)
    h = aux_logits(h, A, NP, g)
    ht = dyadic((M, ldh), g)
    if plant_min:
        # the global minimum of q in the LAST row (the last block of minima), more than 1 below every other row, at the row's only legal
        # move: a fold that misses the last minimum turns that row's score negative and its greedy action to 0
        h[M - 1, :A + 1] = -8.0
        legal[M - 1] = 0.0
        legal[M - 1, 5] = 1.0
    x = {"h": h, "ht": ht, "legal": legal, "action": torch.randint(0, A, (M,), generator=g), "own": own_hand_rows(M, NP, g),
         "reward": torch.randn(T, B, generator=g), "boot": (torch.rand(T, B, generator=g) < 0.8).float(),
         "seq_len": torch.tensor([(T, T - 1, 1, 0)[b % 4] for b in range(B)], dtype=torch.float32),
         "weight": torch.rand(B, generator=g) + 0.5}
    return x


def run_chain(lib, st, pool, x, T, B, A, NP, ldh, n, gamma, pw, ldo):
    """hsad_q_head (with greedy) -> hsad_q_at on the target heads -> hsad_td_loss -> hsad_aux_xent -> hsad_heads_backward"""
    M, nb = T * B, (T * B + 255) // 256
    d = {k: pool.put(v) for k, v in x.items()}
    o = {"q": pool.new((M, A)), "qa": pool.new(M), "greedy": pool.new(M, torch.int64), "scratch": pool.new(2 + nb), "tq": pool.new(M),
         "err": pool.new((T, B)), "prio": pool.new((T, B)), "loss": pool.new(B), "dqa": pool.new((T, B)), "xs": pool.new(B),
         "dheads": pool.new((M, ldo), torch.bfloat16)}
    ok(lib.hsad_q_head(p(d["h"]), ldh, p(d["legal"]), p(d["action"]), M, A, p(o["q"]), p(o["qa"]), p(o["greedy"]), p(o["scratch"]), st))
    ok(lib.hsad_q_at(p(d["ht"]), ldh, p(d["legal"]), p(o["greedy"]), M, A, p(o["tq"]), st))
    ok(lib.hsad_td_loss(p(o["qa"]), p(o["tq"]), p(d["reward"]), p(d["boot"]), p(d["seq_len"]), T, B, n, gamma, p(o["err"]), p(o["prio"]),
                        p(o["loss"]), p(o["dqa"]), p(d["weight"]), st))
    if pw > 0:
        ok(lib.hsad_aux_xent(p(d["h"]), ldh, p(d["own"]), T, B, A, NP, p(o["xs"]), st))
        o["loss"] += np.float32(pw) * o["xs"]                  # loss += pred_weight * xent (one product, one sum, fp32)
    ok(lib.hsad_heads_backward(p(o["dqa"]), p(d["legal"]), p(d["action"]), p(d["h"]), ldh, p(d["own"]), p(d["weight"]), M, B, A, NP,
                               float(np.float32(pw) / np.float32(B)), p(o["dheads"]), ldo, st))
    return d, o


def tail_outputs(pool, T, B, ldo):
    M = T * B
    return {"greedy": pool.new(M, torch.int64), "tq": pool.new(M), "err": pool.new((T, B)), "prio": pool.new((T, B)), "loss": pool.new(B),
            "xs": pool.new(B), "dqa": pool.new((T, B)), "dheads": pool.new((M, ldo), torch.bfloat16)}


def call_tail(lib, st, d, c, t, T, B, A, NP, ldh, n, gamma, pw, ldo, with_dheads=True, WT16=None, dO32=None, H=0, internal=False):
    nb = (T * B + 255) // 256
    args = [p(d["h"]), p(d["ht"]), ldh, p(d["legal"]), p(c["q"]), p(c["qa"]), p(c["scratch"]) + 4, nb, p(d["reward"]), p(d["boot"]),
            p(d["seq_len"]), p(d["weight"]), p(d["own"]), p(d["action"]), T, B, A, NP, n, gamma, pw, p(t["greedy"]), p(t["tq"]), p(t["err"]),
            p(t["prio"]), p(t["loss"]), p(t["xs"]), p(t["dqa"]), p(t["dheads"]) if with_dheads else None, ldo]
    if internal:
        return lib.hsad_internal_loss_tail(*(args + [None, 0, p(WT16), p(dO32), H, st]))
    return lib.hsad_loss_tail(*(args + [st]))


@pytest.mark.parametrize("A,NP,ldh", SHAPES, ids=SHAPE_IDS)
def test_loss_tail_against_float64_and_bit_identical_to_its_chain(lib, st, A, NP, ldh):
    n, gamma, ldo = 3, 0.999, 64
    worst = 0.0
    for T in (1, 5, 33, 130):
        for B in (1, 3):
            M = T * B
            plant = M > 256
            x = tail_inputs(T, B, A, NP, ldh, 6000 * A + M, plant_min=plant)
            for pw in (0.0, 0.25):
                ref = R.loss_objective(x["h"], x["ht"], x["legal"], x["action"], x["reward"], x["boot"], x["seq_len"], x["weight"], x["own"],
                                       T, B, A, n, gamma, pw)
                if plant:       # (precondition of the planted minimum)
                    assert float(ref["q"][M - 1].min()) < float(ref["q"][:M - 1].min()) - 1.0 and M - 1 >= 256
                pool = Pool()
                d, c = run_chain(lib, st, pool, x, T, B, A, NP, ldh, n, gamma, pw, ldo)
                for with_dheads in (True, False):
                    t = tail_outputs(pool, T, B, ldo)
                    ok(call_tail(lib, st, d, c, t, T, B, A, NP, ldh, n, gamma, pw, ldo, with_dheads))
                    pool.check()
                    tag = "loss_tail A=%d T=%d B=%d pw=%g dheads=%d" % (A, T, B, pw, with_dheads)
                    # (1) the float64 references
                    td = ref["td"]
                    assert torch.equal(t["greedy"].cpu(), ref["greedy"]), tag + " greedy"
                    within(t["tq"], ref["target_qa"], ref["target_qa_bound"], tag + " target_qa")
                    within(t["err"], td["err"], td["err_bound"], tag + " err")
                    within(t["prio"], td["priority"], td["err_bound"], tag + " priority")
                    within(t["dqa"], td["dqa"], td["dqa_bound"], tag + " dqa")
                    off = (1 - td["mask"]).bool()
                    assert float(d64(t["err"])[off].abs().sum()) == 0.0 and float(d64(t["dqa"])[off].abs().sum()) == 0.0, tag
                    lb = td["loss_bound"]
                    if pw > 0:
                        e = (d64(t["xs"]) - ref["xent_sum"]).abs()
                        worst = max(worst, float(e.max()) / T)
                        assert float(e.max()) <= T * aux_tol("xent_step"), (tag, float(e.max()))
                        lb = lb + pw * T * aux_tol("xent_step") + 2 * R.U * ref["loss"].abs()
                    else:
                        assert untouched(t["xs"]), tag
                    within(t["loss"], ref["loss"], lb, tag + " loss")
                    if with_dheads:
                        got, gref = d64(t["dheads"]), ref["grad"]
                        lg = ref["legal"]
                        onehot = torch.zeros(M, A, dtype=torch.float64)
                        onehot[torch.arange(M), ref["action"]] = 1.0
                        carried = td["dqa_bound"].reshape(-1, 1) * (lg * (onehot - 1.0 / A)).abs()
                        within(got[:, :A], gref[:, :A], carried + (4 * R.U + R.BF16_ULP) * gref[:, :A].abs(), tag + " d advantage")
                        within(got[:, A], td["dqa"].reshape(-1), td["dqa_bound"].reshape(-1) + R.BF16_ULP * td["dqa"].reshape(-1).abs(),
                               tag + " d value")
                        last = A + 1 + (NP if pw > 0 else 0)
                        assert float(got[:, last:].abs().sum()) == 0.0, tag
                        if pw > 0:
                            e = (got[:, A + 1:last] - gref[:, A + 1:]).abs()
                            tol = aux_tol("softmax") * ref["aux_scale"][:, None] + R.BF16_ULP * gref[:, A + 1:].abs()
                            assert float((e - tol).max()) <= 0.0, (tag, float(e.max()))
                    else:
                        assert untouched(t["dheads"]), tag
                    # (2) bit-identical to the chain it replaces (include/hsad.h)
                    assert torch.equal(t["greedy"], c["greedy"]) and same_bits(t["tq"], c["tq"]), tag + " chain"
                    assert same_bits(t["err"], c["err"]) and same_bits(t["prio"], c["prio"]) and same_bits(t["dqa"], c["dqa"]), tag + " chain"
                    assert same_bits(t["loss"], c["loss"]), tag + " chain loss"
                    if pw > 0:
                        assert same_bits(t["xs"], c["xs"]), tag + " chain xent"
                    if with_dheads:
                        assert same_bits(t["dheads"], c["dheads"]), tag + " chain dheads"
    record("loss_tail", xent_step=worst)


# ---------------------------------------------------------------------------------------------------
# hsad_internal_heads_q: both nets' head layers + the online dueling head in one launch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,NP,ldh", SHAPES, ids=SHAPE_IDS)
def test_heads_q_against_float64_and_q_head(lib, st, A, NP, ldh):
    NH = ldh
    for M in (128, 384):
        for H in (64, 512):
            g = torch.Generator().manual_seed(7000 * A + M + H)
            o16 = [(torch.randn(M, H, generator=g) * 0.5).to(torch.bfloat16) for _ in range(2)]
            W = [(torch.randn(NH, H, generator=g) * (2.0 / H ** 0.5)).to(torch.bfloat16) for _ in range(2)]
            bias = [torch.randn(NH, generator=g) for _ in range(2)]
            legal, action = legal_moves(M, A, g), torch.randint(0, A, (M,), generator=g)
            for nets in (1, 2):
                pool = Pool()
                do, dW, db = [pool.put(v) for v in o16], [pool.put(v) for v in W], [pool.put(v) for v in bias]
                dl, da = pool.put(legal), pool.put(action)
                heads = [pool.new((M, NH)) for _ in range(2)]
                q, qa, bmin = pool.new((M, A)), pool.new(M), pool.new(M // 128)
                two = nets == 2
                assert lib.hsad_internal_heads_q_supported(M, H, NH, A, p(dl), p(q), p(heads[0]), p(heads[1] if two else heads[0])) == 1
                ok(lib.hsad_internal_heads_q(p(do[0]), p(do[1]) if two else None, p(dW[0]), p(dW[1]) if two else None, p(db[0]),
                                             p(db[1]) if two else None, M, H, NH, A, p(heads[0]), p(heads[1]) if two else None, p(dl), p(da),
                                             p(q), p(qa), p(bmin), st))
                pool.check()
                tag = "heads_q A=%d M=%d H=%d nets=%d" % (A, M, H, nets)
                for k in range(nets):
                    ref, bound = R.matmul_bound(o16[k].double(), W[k].double(), bias[k])
                    within(heads[k], ref, bound, tag + " heads of net %d" % k)
                if not two:
                    assert untouched(heads[1]), tag
                # q, qa and the minima: hsad_q_head's bits on the heads this launch wrote
                q2, qa2, scratch = pool.new((M, A)), pool.new(M), pool.new(2 + (M + 255) // 256)
                ok(lib.hsad_q_head(p(heads[0]), NH, p(dl), p(da), M, A, p(q2), p(qa2), None, p(scratch), st))
                pool.check()
                assert same_bits(q, q2) and same_bits(qa, qa2), tag
                mins = torch.stack([q2[128 * i:128 * (i + 1)].min() for i in range(M // 128)])
                assert same_bits(bmin, mins), tag
                fold = torch.stack([bmin[2 * i:2 * i + 2].min() for i in range((M + 255) // 256)])
                assert same_bits(fold, scratch[1:1 + (M + 255) // 256]), tag
                hd = d64(heads[0])
                ref = R.duel_q(hd[:, :A], hd[:, A], legal, action)
                within(q, ref["q"], ref["q_bound"], tag + " q")


def test_heads_q_refuses_the_shapes_it_does_not_cover(lib, st):
    A, NH, H = 21, 37, 64
    pool = Pool()
    for M, nh, h in ((100, NH, H), (128, 65, H), (128, NH, 40), (128, 21, H)):
        g = torch.Generator().manual_seed(M + nh)
        Mp = max(M, 128)
        do, dW, db = pool.put(torch.zeros(Mp, 64, dtype=torch.bfloat16)), pool.put(torch.zeros(nh, 64, dtype=torch.bfloat16)), pool.put(torch.zeros(nh))
        dl, da = pool.put(legal_moves(Mp, A, g)), pool.put(torch.zeros(Mp, dtype=torch.int64))
        heads, q, qa, bmin = pool.new((Mp, nh)), pool.new((Mp, A)), pool.new(Mp), pool.new(4)
        assert lib.hsad_internal_heads_q_supported(M, h, nh, A, p(dl), p(q), p(heads), p(heads)) == 0
        assert lib.hsad_internal_heads_q(p(do), None, p(dW), None, p(db), None, M, h, nh, A, p(heads), None, p(dl), p(da), p(q), p(qa), p(bmin),
                                         st) != 0
        assert untouched(heads) and untouched(q) and untouched(qa) and untouched(bmin)
    pool.check()


# ---------------------------------------------------------------------------------------------------
# hsad_internal_loss_tail forming d loss / d o = dheads W_heads in the same launch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [5, 33, 130])
def test_loss_tail_forms_dO_in_the_same_launch(lib, st, T):
    n, gamma, pw, ldo = 3, 0.999, 0.25, 64
    for A, NP, ldh in SHAPES:
        for B in (1, 3):
            M = T * B
            x = tail_inputs(T, B, A, NP, ldh, 8000 * A + M)
            pool = Pool()
            d, c = run_chain(lib, st, pool, x, T, B, A, NP, ldh, n, gamma, pw, ldo)
            plain = tail_outputs(pool, T, B, ldo)
            ok(call_tail(lib, st, d, c, plain, T, B, A, NP, ldh, n, gamma, pw, ldo, internal=True))
            for H in (32, 256, 512):
                g = torch.Generator().manual_seed(H + A)
                WT = (torch.randn(H, ldo, generator=g) * 0.25).to(torch.bfloat16)          # W_heads^T: [H][64]
                dWT, dO = pool.put(WT), pool.new((M, H))
                fused = tail_outputs(pool, T, B, ldo)
                rc = call_tail(lib, st, d, c, fused, T, B, A, NP, ldh, n, gamma, pw, ldo, WT16=dWT, dO32=dO, H=H, internal=True)
                pool.check()
                tag = "fused dO A=%d T=%d B=%d H=%d" % (A, T, B, H)
                if T > 128 and H > 256:          # two waves hold 256 columns at most (include/hsad.h does not promise more)
                    assert rc != 0 and untouched(dO) and untouched(fused["dheads"]), tag
                    continue
                ok(rc)
                for k in plain:
                    assert same_bits(fused[k], plain[k]), tag + ": %s differs from the launch without dO" % k
                # rows t >= T of the padded 32-row blocks land behind the buffer: the guard band (checked above)
                ref, bound = R.matmul_bound(d64(fused["dheads"]), WT.double())
                within(dO, ref, bound, tag + " dO")
            # a head-gradient stride other than 64 cannot feed the matrix cores
            dWT, dO = pool.put(torch.zeros(32, 62, dtype=torch.bfloat16)), pool.new((M, 32))
            bad = tail_outputs(pool, T, B, 62)
            assert call_tail(lib, st, d, c, bad, T, B, A, NP, ldh, n, gamma, pw, 62, WT16=dWT, dO32=dO, H=32, internal=True) != 0
            assert untouched(dO)
            pool.check()


# ---------------------------------------------------------------------------------------------------
# column sums and operand preparation
# ---------------------------------------------------------------------------------------------------
COL_M, COL_N = (1, 127, 128, 129, 1000), (1, 63, 64, 65, 200)


@pytest.mark.parametrize("is_bf16", [0, 1], ids=["fp32", "bf16"])
def test_column_sums_against_float64(lib, st, is_bf16):
    dt = torch.bfloat16 if is_bf16 else torch.float32
    for M in COL_M:
        for N in COL_N:
            ld = N + 3
            g = torch.Generator().manual_seed(9000 + 7 * M + N)
            src = torch.randn(M, ld, generator=g).to(dt)
            out0, out20 = torch.randn(N, generator=g), torch.randn(N, generator=g)
            cmap = torch.randperm(N, generator=g).int()
            nblk = (M + 127) // 128
            pool = Pool()
            ds, dm = pool.put(src), pool.put(cmap)
            tag = "colsum M=%d N=%d %s" % (M, N, dt)
            # a thread adds 32 rows of its 128-row block (+1: onto the output)
            kw = dict(rows_per_block=128, serial=33)
            plain = pool.new(N)
            ok(lib.hsad_colsum(p(ds), is_bf16, M, N, ld, p(plain), st))
            ref, bound = R.colsum(src.double(), N, **kw)
            within(plain, ref, bound, tag)
            acc, acc2 = pool.put(out0), pool.put(out20)
            ok(lib.hsad_colsum_acc(p(ds), is_bf16, M, N, ld, p(acc), p(acc2), p(dm), st))
            for o, o0 in ((acc, out0), (acc2, out20)):
                ref, bound = R.colsum(src.double(), N, out0=o0, col_map=cmap, **kw)
                within(o, ref, bound, tag + " acc with col_map")
            acc1 = pool.put(out0)
            ok(lib.hsad_colsum_acc(p(ds), is_bf16, M, N, ld, p(acc1), None, None, st))
            ref, bound = R.colsum(src.double(), N, out0=out0, **kw)
            within(acc1, ref, bound, tag + " acc")
            runs = []
            for _ in range(2):
                o, scratch = pool.put(out0), pool.new((nblk, N))
                ok(lib.hsad_colsum_acc_ordered(p(ds), is_bf16, M, N, ld, p(o), p(scratch), st))
                within(o, ref, bound, tag + " ordered")
                runs.append(o)
            assert same_bits(runs[0], runs[1]), tag + ": the ordered sum must give the same bits on every run"
            pool.check()


def test_transpose_with_column_sums_is_exact_and_within_the_bound(lib, st):
    for Rr in (4, 124, 128, 132, 1000):       # the entry point takes multiples of 4 only (8-byte loads): the sizes of the column sums, rounded
        for Cc in (4, 60, 64, 68, 200):
            ls, ldd = Cc + 4, Rr + 4
            g = torch.Generator().manual_seed(11000 + 7 * Rr + Cc)
            src = torch.randn(Rr, ls, generator=g).to(torch.bfloat16)
            s0, s20 = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
            cmap = torch.randperm(Cc, generator=g).int()
            pool = Pool()
            ds, dm, cs, cs2 = pool.put(src), pool.put(cmap), pool.put(s0), pool.put(s20)
            dst = pool.new((Cc, ldd), torch.bfloat16)
            ok(lib.hsad_transpose_bf16_colsum(p(ds), Rr, Cc, ls, p(dst), ldd, p(cs), p(cs2), p(dm), st))
            pool.check()
            tag = "transpose_colsum R=%d C=%d" % (Rr, Cc)
            assert same_bits(dst[:, :Rr], ds[:, :Cc].t()), tag + ": the transpose moves bits"
            assert untouched(dst[:, Rr:]), tag + ": destination padding"
            for o, o0 in ((cs, s0), (cs2, s20)):     # 16 rows per thread, 4-way fold, one addition per 64-row tile
                ref, bound = R.colsum(src.double(), Cc, rows_per_block=64, serial=17, out0=o0, col_map=cmap)
                within(o, ref, bound, tag)
    pool = Pool()
    ds, dst, cs = pool.put(torch.zeros(127, 64, dtype=torch.bfloat16)), pool.new((64, 128), torch.bfloat16), pool.new(64)
    assert lib.hsad_transpose_bf16_colsum(p(ds), 127, 64, 64, p(dst), 128, p(cs), None, None, st) != 0
    assert untouched(dst) and untouched(cs)
    pool.check()


def test_bias_sum_perm_against_float64(lib, st):
    for n in (1, 255, 256, 257, 1000):
        g = torch.Generator().manual_seed(12000 + n)
        a, b, perm = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randperm(n, generator=g).int()
        for with_b in (True, False):
            for with_perm in (True, False):
                pool = Pool()
                da, db, dp, out = pool.put(a), pool.put(b), pool.put(perm), pool.new(n)
                ok(lib.hsad_bias_sum_perm(p(da), p(db) if with_b else None, p(dp) if with_perm else None, p(out), n, st))
                pool.check()
                ref, bound = R.bias_sum_perm(a.double().numpy(), b.double().numpy() if with_b else None, perm.numpy() if with_perm else None)
                within(out, ref, bound, "bias_sum_perm n=%d" % n)


def _weight_jobs(g):
    """twelve weight matrices over the sizes of the column sums: with / without permutation, either or both destinations, ld > C"""
    jobs = []
    sizes = [(1, 1), (127, 63), (128, 64), (129, 65), (1000, 200), (1, 200), (127, 1), (128, 65), (129, 64), (1000, 63), (65, 129), (64, 128)]
    for k, (Rr, Cc) in enumerate(sizes):
        jobs.append({"R": Rr, "C": Cc, "ld": Cc + (k % 3), "src": torch.randn(Rr, Cc + (k % 3), generator=g),
                     "perm": torch.randperm(Rr, generator=g).int() if k % 2 == 0 else None, "dst": k % 3 != 1, "dstT": k % 3 != 2,
                     "ldd": Cc + 2, "ldt": Rr + 5})
    return jobs


def _check_weight(job, dst, dstT, tag):
    want, wantT = R.prepare_weight(job["src"][:, :job["C"]].numpy(), None if job["perm"] is None else job["perm"].numpy())
    if dst is not None:
        got = dst.cpu().view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got[:, :job["C"]], want), tag + ": weight[perm] rounded to bf16"
        assert untouched(dst[:, job["C"]:]), tag + ": destination padding"
    if dstT is not None:
        got = dstT.cpu().view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got[:, :job["R"]], wantT), tag + ": the transposed copy"
        assert untouched(dstT[:, job["R"]:]), tag + ": destination padding"


def test_prepare_weight_and_the_batched_refresh_are_exact(lib, st):
    g = torch.Generator().manual_seed(13000)
    jobs = _weight_jobs(g)
    biases = []
    for k, n in enumerate((1, 255, 256, 257, 1000, 64, 2048, 513)):
        biases.append({"n": n, "a": torch.randn(n, generator=g), "b": torch.randn(n, generator=g) if k % 2 == 0 else None,
                       "perm": torch.randperm(n, generator=g).int() if k % 3 != 2 else None})
    pool = Pool()
    ok(lib.hsad_refresh_begin())
    held = []
    for j in jobs:
        ds, dp = pool.put(j["src"]), None if j["perm"] is None else pool.put(j["perm"])
        dst = pool.new((j["R"], j["ldd"]), torch.bfloat16) if j["dst"] else None
        dstT = pool.new((j["C"], j["ldt"]), torch.bfloat16) if j["dstT"] else None
        ok(lib.hsad_refresh_add_weight(p(ds), j["R"], j["C"], j["ld"], p(dp), p(dst), j["ldd"], p(dstT), j["ldt"]))
        held.append((ds, dp, dst, dstT))
    outs = []
    for b in biases:
        da, db, dp = pool.put(b["a"]), None if b["b"] is None else pool.put(b["b"]), None if b["perm"] is None else pool.put(b["perm"])
        out = pool.new(b["n"])
        ok(lib.hsad_refresh_add_bias(p(da), p(db), p(dp), p(out), b["n"]))
        outs.append((da, db, dp, out))
    # a weight job may not follow a bias job
    assert lib.hsad_refresh_add_weight(p(held[0][0]), 1, 1, 1, None, p(held[0][2]), 3, None, 0) != 0
    ok(lib.hsad_refresh_launch(st))
    pool.check()
    for k, (j, (_, _, dst, dstT)) in enumerate(zip(jobs, held)):
        _check_weight(j, dst, dstT, "refresh weight job %d" % k)
    for k, (b, (_, _, _, out)) in enumerate(zip(biases, outs)):
        ref, bound = R.bias_sum_perm(b["a"].double().numpy(), None if b["b"] is None else b["b"].double().numpy(),
                                     None if b["perm"] is None else b["perm"].numpy())
        within(out, ref, bound, "refresh bias job %d" % k)
    # the single-matrix entry point does the same work
    pool = Pool()
    for k, j in enumerate(jobs[:6]):
        ds, dp = pool.put(j["src"]), None if j["perm"] is None else pool.put(j["perm"])
        dst = pool.new((j["R"], j["ldd"]), torch.bfloat16) if j["dst"] else None
        dstT = pool.new((j["C"], j["ldt"]), torch.bfloat16) if j["dstT"] else None
        ok(lib.hsad_prepare_weight(p(ds), j["R"], j["C"], j["ld"], p(dp), p(dst), j["ldd"], p(dstT), j["ldt"], st))
        pool.check()
        _check_weight(j, dst, dstT, "prepare_weight job %d" % k)
    # the job list takes 20 matrices and 12 biases (include/hsad.h); one more of either is refused, nothing is launched
    ok(lib.hsad_refresh_begin())
    ds, dst, out = pool.put(torch.zeros(1, 1)), pool.new((1, 1), torch.bfloat16), pool.new(1)
    for _ in range(20):
        ok(lib.hsad_refresh_add_weight(p(ds), 1, 1, 1, None, p(dst), 1, None, 0))
    assert lib.hsad_refresh_add_weight(p(ds), 1, 1, 1, None, p(dst), 1, None, 0) != 0
    for _ in range(12):
        ok(lib.hsad_refresh_add_bias(p(ds), None, None, p(out), 1))
    assert lib.hsad_refresh_add_bias(p(ds), None, None, p(out), 1) != 0
    ok(lib.hsad_refresh_begin())       # leave the thread's job list empty
    assert untouched(dst) and untouched(out)
