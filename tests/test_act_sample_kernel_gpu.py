"""hsad_act_sample_q (act_sample_q_kernel / act_tail_kernel of csrc/r2d2/act.inc; specified in include/hsad.h and DESIGN.md section 3c) on synthetic heads, against
hsad_act_select_q / hsad_q_at (bit for bit: greedy always, a and qa on rows without a temperature, qa at a_out everywhere) and the
restatement tests/act_sample_ref.py (the sampled actions: the boundary rule, MARGIN = 1e-5, at most 1 % of the sampled rows excused).  Inputs come from numpy generators with fixed seeds, so which rows lie near a boundary is a property
of this file alone (tests/test_act_soft_surface_cpu.py counts them without a device).

Shapes (N, A, ldh): 549 x 21 / 37 = two full row blocks and a ragged third; 300 x 31 / 47 = R = 196 rows per block while adv_min blocks
by 256; 130 x 49 / 62 = a wide row (R = 138); 1 x 21 / 37 = a single row."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import act_sample_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda:0"
SHAPES = [(549, 21, 37), (300, 31, 47), (130, 49, 62), (1, 21, 37)]
IDS = ["N%d_A%d" % s[:2] for s in SHAPES]
# (with these seeds no sampled row of any shape lies within the margin of a boundary; tests/test_act_soft_surface_cpu.py holds that)
SEED, COUNTER, SAMPLE_SEED = 0xC0FFEE123, 9, 0x5EED5A12
PAD, SENT = 64, -77


def make_inputs(N, A, ldh, scale=2.0):
    """heads fp32 [N, ldh] (advantages ~ scale * normal, then the value and the hand logits), legal with rows of 0, 1, some and all
    actions legal (the single row of N = 1 has some), eps a mix of 0 and 0.3, temp a mix of 0 and the tau list, distinct row keys"""
    g = np.random.default_rng(1000 * A + N)
    heads = (g.standard_normal((N, ldh)) * scale).astype(np.float32)
    legal = (g.random((N, A)) < 0.5).astype(np.float32)
    mode = g.integers(0, 8, N) if N > 1 else np.array([5])
    for m in range(N):
        if mode[m] == 0:
            legal[m] = 0
        elif mode[m] == 1:
            legal[m] = 0
            legal[m, g.integers(0, A)] = 1
        elif mode[m] == 2:
            legal[m] = 1
        elif legal[m].sum() < 2:
            legal[m, :2] = 1
    eps = np.where(g.random(N) < 0.4, 0.3, 0.0).astype(np.float32)
    temp = np.array((0.0,) + R.TAUS, dtype=np.float32)[g.integers(0, 6, N)] if N > 1 else np.array([1.0], np.float32)
    key = (g.permutation(N).astype(np.int64) * 7919 - 1234567)
    return heads, legal, eps, temp, key


def expected_rows(heads, legal, eps, temp, key, A, seed=SEED, counter=COUNTER, sample_seed=SAMPLE_SEED):
    """per row with temp > 0 and a legal action: ("explore", action) when the exploration draw fires, else ("sample", u)"""
    out = {}
    for m in range(len(temp)):
        idx = np.nonzero(legal[m])[0]
        if temp[m] > 0 and len(idx):
            hh = R.eps_hash(seed, m, counter)
            k = R.eps_draw(hh, eps[m] if eps is not None else 0.0, len(idx))
            hs = R.sample_hash(hh) if key is None else R.sample_hash_keyed(sample_seed, int(key[m]))
            out[m] = ("explore", int(idx[k])) if k >= 0 else ("sample", R.u24(hs) / 16777216.0)
    return out


@pytest.fixture(scope="module")
def lib():
    from hanabi_sad_amd import _lib
    return _lib.load_library()


@pytest.fixture(scope="module")
def st():
    from hanabi_sad_amd.r2d2 import _s
    return _s(torch.device(DEV))


@pytest.fixture(autouse=True)
def _end_the_session_after_a_device_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the device reported a fault: %s" % e, returncode=3)


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def p(t):
    return None if t is None else t.data_ptr()


def guarded(N, dtype):
    return torch.full((N + 2 * PAD,), SENT, dtype=dtype, device=DEV)


def inner(t):
    assert bool((t[:PAD] == SENT).all()) and bool((t[-PAD:] == SENT).all()), "a kernel wrote outside its output"
    return t[PAD:-PAD].cpu()


def call(lib, st, which, heads, legal, eps, N, A, ldh, temp=None, key=None, sample_seed=SAMPLE_SEED, seed=SEED, counter=COUNTER):
    """-> (a, greedy, qa) on the host, qa as its int32 bit pattern; which = "select" | "sample"; operands are device tensors"""
    from hanabi_sad_amd import _lib
    a, g, qa = guarded(N, torch.int64), guarded(N, torch.int64), guarded(N, torch.float32)
    scratch = torch.zeros(8 + (N + 255) // 256, dtype=torch.float32, device=DEV)
    o = lambda t: t.data_ptr() + PAD * t.element_size()
    if which == "select":
        _lib.check(lib.hsad_act_select_q(p(heads), ldh, p(legal), p(eps), N, A, seed, counter, o(a), o(g), o(qa), p(scratch), st))
    else:
        _lib.check(lib.hsad_act_sample_q(p(heads), ldh, p(legal), p(eps), p(temp), p(key), sample_seed, N, A, seed, counter, o(a), o(g),
                                         o(qa), p(scratch), st))
    torch.cuda.synchronize()
    return inner(a), inner(g), inner(qa).view(torch.int32)


def q_at(lib, st, heads, legal, a, N, A, ldh):
    from hanabi_sad_amd import _lib
    qa = torch.empty(N, dtype=torch.float32, device=DEV)
    _lib.check(lib.hsad_q_at(p(heads), ldh, p(legal), p(a), N, A, p(qa), st))
    torch.cuda.synchronize()
    return qa.cpu().view(torch.int32)


@pytest.mark.parametrize("N,A,ldh", SHAPES, ids=IDS)
def test_without_a_temperature_the_rows_are_those_of_act_select_q(lib, st, N, A, ldh):
    heads, legal, eps, _, key = make_inputs(N, A, ldh)
    dh, dl, de, dk = dev(heads), dev(legal), dev(eps), dev(key)
    want = call(lib, st, "select", dh, dl, de, N, A, ldh)
    for name, temp, k in (("NULL", None, None), ("zeros", torch.zeros(N, device=DEV), None), ("zeros, keyed", torch.zeros(N, device=DEV), dk),
                          ("negative", torch.full((N,), -1.0, device=DEV), None)):
        got = call(lib, st, "sample", dh, dl, de, N, A, ldh, temp, k)
        for what, x, y in zip(("a", "greedy", "qa"), got, want):
            assert torch.equal(x, y), "temp %s: %s differs from hsad_act_select_q" % (name, what)
    if N > 1:
        assert not torch.equal(want[0], want[1]), "no row explored: the comparison shows nothing about the eps draw"


@pytest.mark.parametrize("keyed", [False, True], ids=["row_counter", "row_key"])
@pytest.mark.parametrize("N,A,ldh", SHAPES, ids=IDS)
def test_mixed_temperatures_against_the_restatement(lib, st, N, A, ldh, keyed):
    heads, legal, eps, temp, key = make_inputs(N, A, ldh)
    if not keyed:
        key = None
    dh, dl = dev(heads), dev(legal)
    sel = call(lib, st, "select", dh, dl, dev(eps), N, A, ldh)
    a, g, qa = call(lib, st, "sample", dh, dl, dev(eps), N, A, ldh, dev(temp), dev(key))
    assert torch.equal(g, sel[1]), "greedy differs from hsad_act_select_q"
    assert torch.equal(qa, q_at(lib, st, dh, dl, dev(a.numpy()), N, A, ldh)), "qa differs from hsad_q_at at a_out"
    exp = expected_rows(heads, legal, eps, temp, key, A)
    a = a.numpy()
    sampled = excused = 0
    for m in range(N):
        idx = np.nonzero(legal[m])[0]
        if len(idx):
            assert 0 <= a[m] < A and legal[m, a[m]] != 0, "row %d: action %d is illegal" % (m, a[m])
        if len(idx) == 1:
            assert a[m] == idx[0]
        if m not in exp:
            assert a[m] == int(sel[0][m]), "row %d has no temperature (or no legal action) and differs from hsad_act_select_q" % m
        elif exp[m][0] == "explore":
            assert a[m] == exp[m][1], "row %d: the exploration draw fires and takes action %d, got %d" % (m, exp[m][1], a[m])
        elif len(idx) > 1:
            sampled += 1
            excused += R.judge(int(a[m]), heads[m, :A], legal[m], temp[m], exp[m][1]) == "excused"
    print("N %d A %d: %d sampled rows, %d under the boundary excuse" % (N, A, sampled, excused))
    assert excused <= sampled // 100
    if N > 1:
        assert sampled > N // 4 and bool((a != g.numpy()).any())


@pytest.mark.parametrize("N,A,ldh", SHAPES, ids=IDS)
def test_a_cold_policy_is_the_greedy_one(lib, st, N, A, ldh):
    """tau = 1e-6 on heads whose legal advantages differ by >= 2^-9 > 1e-3: every other weight underflows, a == greedy on every row"""
    g = np.random.default_rng(7 * A + N)
    heads, legal, _, _, key = make_inputs(N, A, ldh)
    for m in range(N):
        heads[m, :A] = (g.permutation(A) - A // 2) * 2.0 ** -9
    temp = torch.full((N,), 1e-6, device=DEV)
    for k in (None, dev(key)):
        a, gr, _ = call(lib, st, "sample", dev(heads), dev(legal), None, N, A, ldh, temp, k)
        assert torch.equal(a, gr)


@pytest.mark.parametrize("N,A,ldh", SHAPES, ids=IDS)
def test_large_advantages_stay_finite_and_legal(lib, st, N, A, ldh):
    """|z| = 1e4 at every temperature of the list: in range, legal, and Q(s, a) finite"""
    g = np.random.default_rng(11 * A + N)
    heads, legal, eps, _, key = make_inputs(N, A, ldh)
    heads[:, :A] = np.where(g.random((N, A)) < 0.5, 1e4, -1e4).astype(np.float32)
    has = legal.sum(1) > 0
    for tau in R.TAUS:
        temp = torch.full((N,), tau, device=DEV)
        for k in (None, dev(key)):
            a, gr, qa = call(lib, st, "sample", dev(heads), dev(legal), dev(eps), N, A, ldh, temp, k)
            a = a.numpy()
            assert ((a >= 0) & (a < A)).all()
            assert (legal[np.arange(N), a][has] != 0).all(), "tau %g: an illegal action" % tau
            assert bool(torch.isfinite(qa.view(torch.float32)).all())


@pytest.mark.parametrize("N,A,ldh", SHAPES[:3], ids=IDS[:3])
def test_the_draw_is_a_function_of_its_keys(lib, st, N, A, ldh):
    heads, legal, eps, _, key = make_inputs(N, A, ldh)
    dh, dl, de, dk = dev(heads), dev(legal), dev(eps), dev(key)
    temp = torch.ones(N, device=DEV)
    base = call(lib, st, "sample", dh, dl, de, N, A, ldh, temp, None)
    again = call(lib, st, "sample", dh, dl, de, N, A, ldh, temp, None)
    assert all(torch.equal(x, y) for x, y in zip(base, again))
    other = call(lib, st, "sample", dh, dl, de, N, A, ldh, temp, None, counter=COUNTER + 1)
    assert not torch.equal(base[0], other[0]) and torch.equal(base[1], other[1])
    kb = call(lib, st, "sample", dh, dl, None, N, A, ldh, temp, dk)
    assert all(torch.equal(x, y) for x, y in zip(kb, call(lib, st, "sample", dh, dl, None, N, A, ldh, temp, dk)))
    # with a row key neither the counter nor the seed enters the sample draw (eps is NULL here) ...
    assert torch.equal(kb[0], call(lib, st, "sample", dh, dl, None, N, A, ldh, temp, dk, counter=COUNTER + 1, seed=SEED + 1)[0])
    # ... the sample seed does
    assert not torch.equal(kb[0], call(lib, st, "sample", dh, dl, None, N, A, ldh, temp, dk, sample_seed=SAMPLE_SEED + 1)[0])


@pytest.mark.parametrize("N,A,ldh", SHAPES[:3], ids=IDS[:3])
def test_with_a_row_key_permuted_rows_give_the_permuted_result(lib, st, N, A, ldh):
    heads, legal, _, temp, key = make_inputs(N, A, ldh)
    perm = np.random.default_rng(N).permutation(N)
    a0, g0, q0 = call(lib, st, "sample", dev(heads), dev(legal), None, N, A, ldh, dev(temp), dev(key))
    a1, g1, q1 = call(lib, st, "sample", dev(heads[perm]), dev(legal[perm]), None, N, A, ldh, dev(temp[perm]), dev(key[perm]))
    pt = torch.from_numpy(perm)
    assert torch.equal(a0[pt], a1) and torch.equal(g0[pt], g1) and torch.equal(q0[pt], q1)
