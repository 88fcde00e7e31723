"""GPU: the grouped split-K weight-gradient GEMM (hsad_gemm_nt_bf16_group_splitk: one launch of gemm8_kernel<G8_F32> over up to eight
problems + one g8_sum_slabs_kernel pass) and the slab-summing entry points next to it (hsad_gemm_nt_bf16_splitk, _splitk_acc) against an
fp64 CPU product -- EXACTLY: the operands are small integers (tests/gemm_group.py), so every partial sum in any k order, range cut and slab
order is an integer that fp32 holds, and each comparison is torch.equal over the full matrix.  A k range one tile short, a slab summed
twice or never, four columns at a ragged edge taken from the neighbour, a dropped `accumulate`, a tile order that is no bijection: each
changes an integer or leaves a NaN.  The poison around the operands, the workspace and C is described in tests/gemm_group.py.

The only tolerance in this file is the derived one of the rounded-operand accuracy cases: products of two bf16 values are exact in fp32
and a result is formed by at most K + nslab fp32 additions of relative error <= 2^-23 each (round to nearest or truncation), hence
|C - C64| <= (K + nslab) 2^-23 (|A| |B|^T) elementwise, the right-hand side in fp64."""
import contextlib

import pytest
import torch

from tests import gemm_group as G
from tests.gemm_group import Spec

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def cus():
    return torch.cuda.get_device_properties(torch.device(G.DEV)).multi_processor_count


def last_error():
    from hanabi_sad_amd import _lib
    return _lib.load_library().hsad_last_error().decode()


@contextlib.contextmanager
def gemm_pp(on):
    """hsad_gemm_set_pp(on) for the block, the default (1) afterwards"""
    from hanabi_sad_amd import _lib
    lib = _lib.load_library()
    try:
        _lib.check(lib.hsad_gemm_set_pp(on))
        yield
    finally:
        lib.hsad_gemm_set_pp(1)


def small_item(accumulate=1):
    """M = 128: one such item sends every item of its group to the 128 x 128 kernel"""
    return Spec(128, 68, 384, 2, n_out=65, row_map="scatter", accumulate=accumulate)


def launch(cases):
    """one grouped call over the cases; -> the workspace.  Asserts the entry point's own workspace size against the restatement."""
    items = [G.item_of(c) for c in cases]
    need = G.group_workspace_floats(items)
    assert need == G.workspace_floats([c.spec.shape for c in cases]) > 0
    ws = G.Workspace(need)
    rc = G.call_group(items, ws)
    assert rc == 0, last_error()
    assert ws.tail_intact(), "the workspace was written past the size hsad_gemm_group_workspace_floats gives"
    return ws


def run_exact(specs, seed, fallback=False):
    specs = ([small_item()] if fallback else []) + list(specs)
    cases = [G.make_case(s, seed * 100 + i) for i, s in enumerate(specs)]
    launch(cases)
    for c in cases:
        G.check_exact(c)
    return cases


# ---------------------------------------------------------------------------------------------------
# smallest launch, ragged N, n_out and ldc
# ---------------------------------------------------------------------------------------------------
def test_the_smallest_launch_one_work_item():
    """M = 256, N = 4, K = 128, split 1: one work item, a grid of one workgroup, a single valid group of four columns (all other B rows are
    clamped to row 3), and group_kchunk's floor of two k tiles"""
    s = Spec(256, 4, 128, 1)
    assert G.core_plan(128, 1) == (2, 1, 2) and G.work_items([s.shape]) == [1] and G.launch_grid([s.shape], cus()) == 1
    run_exact([s], 1)


@pytest.mark.parametrize("fallback", [False, True])
@pytest.mark.parametrize("N", [4, 252, 256, 260, 896])
def test_ragged_n_and_partial_output_rows(N, fallback):
    """M = 256, K = 256, split 2.  N = 4 and 252: the ragged edge inside the first column tile; 256: exactly at it; 260: four columns into
    the second tile; 896: the input layer's padded width.  n_out in {N, N - 1, N - 3, 1} with an odd ldc (output rows that are not 16-byte
    aligned), overwriting and accumulating, and the input layer's 838 of 896 columns at ldc = 838.  fallback: an M = 128 item in front."""
    outs = [(n_out, None) for n_out in sorted({N, N - 1, N - 3, 1})] + ([(838, 838)] if N == 896 else [])
    for i, (n_out, ldc) in enumerate(outs):
        for acc in (0, 1):
            s = Spec(256, N, 256, 2, n_out=n_out, ldc=ldc, accumulate=acc)
            assert s.ldc % 2 == 1 or ldc == 838
            run_exact([s], 10 + N + 2 * i + acc, fallback)


# ---------------------------------------------------------------------------------------------------
# short last range
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fallback", [False, True])
@pytest.mark.parametrize("K,split_k,plan", [(640, 4, (4, 3, 2)), (1280, 3, (8, 3, 4)), (2560, 8, (6, 7, 4)), (10240, 3, (54, 3, 52)), (128, 8, (2, 1, 2))])
def test_a_short_last_k_range(K, split_k, plan, fallback):
    """M = 256, N = 64.  plan = (k tiles per range, ranges, k tiles of the last range): 4 4 2; 8 8 4; six ranges of 6 and one of 4; the
    learner's 54 54 52; one range.  The slabs the entry point's workspace size implies are the restated plan's."""
    assert G.core_plan(K, split_k) == plan
    s = Spec(256, 64, K, split_k, accumulate=K == 1280)
    cases = run_exact([s], 200 + split_k, fallback)
    assert G.group_workspace_floats([G.item_of(cases[-1])]) == plan[1] * 256 * 64


# ---------------------------------------------------------------------------------------------------
# the learner's group
# ---------------------------------------------------------------------------------------------------
def wgrad_specs(K, lstm_split):
    """the five problems of grouped_wgrad (csrc/hsad_learner.hip) at contraction K: W_ih / W_hh of both LSTM layers (4H x H, rows un-blocked
    through gate_block_perm), and the input layer's 838 of 896 columns into rows of 3,352 bytes"""
    return [Spec(2048, 512, K, lstm_split, row_map="perm", accumulate=1) for _ in range(4)] + [Spec(512, 896, K, 8, n_out=838, ldc=838, accumulate=1)]


_CACHE = {}


def wgrad_cases(K, lstm_split, exact):
    """made once (operands and the fp64 products are shared between the tests that use them), C restored before every use"""
    key = (K, lstm_split, exact)
    if key not in _CACHE:
        _CACHE[key] = [G.make_case(s, 3000 + K + i, exact) for i, s in enumerate(wgrad_specs(K, lstm_split))]
    for c in _CACHE[key]:
        G.reset_case(c)
    return _CACHE[key]


def test_the_learners_group_one_item_per_workgroup():
    """K = 1280, split 3 (8 8 4 k tiles) for the LSTM problems, 8 (five ranges of 4) for the input layer: 4 x 48 + 40 = 232 work items, at
    most one per workgroup.  The grid (232) is a multiple of 8 and every LSTM problem starts at a multiple of 8 with 8 row tiles: order 1;
    the input layer has 2 row tiles: order 0."""
    cases = wgrad_cases(1280, 3, True)
    shapes = [c.spec.shape for c in cases]
    assert G.work_items(shapes) == [48, 48, 48, 48, 40]
    assert sum(G.work_items(shapes)) <= cus() and G.launch_grid(shapes, cus()) == 232, "a chip on which this is not one item per workgroup"
    assert G.tile_orders(shapes, cus()) == [1, 1, 1, 1, 0]
    launch(cases)
    for c in cases:
        G.check_exact(c)


def test_the_learners_group_on_the_128_kernel():
    """the same group with hsad_gemm_set_pp(0): one launch of the 128 x 128 kernel per item into the same slabs"""
    cases = wgrad_cases(1280, 3, True)
    with gemm_pp(0):
        launch(cases)
    for c in cases:
        G.check_exact(c)


def test_the_learners_group_several_items_per_workgroup():
    """K = 2048, split 8 everywhere: 4 x 128 + 64 = 576 work items on fewer workgroups, so every workgroup walks items of different
    problems and the descriptors, ldb, N and the k range change between consecutive items of one operand stream.  Order 1 for the LSTM
    problems (grid 256, starts 0, 128, 256, 384), order 0 for the input layer."""
    cases = wgrad_cases(2048, 8, True)
    shapes = [c.spec.shape for c in cases]
    assert G.work_items(shapes) == [128, 128, 128, 128, 64] and sum(G.work_items(shapes)) == 576
    assert 576 > cus(), "a chip with a CU per work item: no workgroup would walk two items"
    assert G.launch_grid(shapes, cus()) % 8 == 0 and G.tile_orders(shapes, cus()) == [1, 1, 1, 1, 0]
    launch(cases)
    for c in cases:
        G.check_exact(c)


def test_the_learners_group_is_deterministic_on_rounded_operands():
    """the header promises a deterministic sum (slabs added in range order): two runs on rounded operands give identical bits"""
    cases = wgrad_cases(2048, 8, False)
    assert sum(G.work_items([c.spec.shape for c in cases])) > cus()
    bits = []
    for _ in range(2):
        for c in cases:
            G.reset_case(c)
        launch(cases)
        bits.append([G.result_bits(c) for c in cases])
    for c, a, b in zip(cases, bits[0], bits[1]):
        G.check_canaries(c, c.C_dev.cpu())
        assert not torch.isnan(c.C_dev.cpu()[c.payload]).any()
        assert torch.equal(a, b), c.spec


# ---------------------------------------------------------------------------------------------------
# tile orders (the rule: g8_launch; restated in tests/gemm_group.tile_orders).  A wrong bijection leaves a NaN or a wrong block.
# ---------------------------------------------------------------------------------------------------
def test_tile_order_1_row_tiles_dealt_to_the_xcds():
    """M = 2048, N = 256, K = 1024, split 8: 8 x 1 tiles x 8 ranges = 64 work items, grid 64 (a multiple of 8), the problem starts at item
    0 and has 8 row tiles -> order 1; 8 tiles are not whole rounds of 256 -> not order 2"""
    s = Spec(2048, 256, 1024, 8, row_map="perm")
    assert G.work_items([s.shape]) == [64] and G.launch_grid([s.shape], cus()) == 64 and G.tile_orders([s.shape], cus()) == [1]
    run_exact([s], 41)


def test_tile_order_0_behind_an_unaligned_start():
    """the same problem behind an item of 3 work items (M = 256, N = 64, K = 768, split 3): it starts at item 3, not a multiple of 8, so the
    XCD-aware orders are off -> order 0 (the item in front has one row tile: order 0 as well)"""
    specs = [Spec(256, 64, 768, 3), Spec(2048, 256, 1024, 8, row_map="perm")]
    shapes = [s.shape for s in specs]
    assert G.work_items(shapes) == [3, 64] and G.launch_grid(shapes, cus()) == 64 and G.tile_orders(shapes, cus()) == [0, 0]
    run_exact(specs, 42)


def test_tile_order_2_patches_per_xcd_round():
    """M = 8192, N = 2048, K = 128, split 1: 32 x 8 = 256 tiles = whole rounds of the chip, 8 column tiles -> patches 4 wide, 8 row tiles
    high, 32 row tiles a multiple of 8, grid min(256, CUs) & ~7 a multiple of 8 -> order 2"""
    s = Spec(8192, 2048, 128, 1)
    assert cus() >= 64, "the grid is only rounded to a multiple of 8 from 64 workgroups on"
    assert G.work_items([s.shape]) == [256] and G.launch_grid([s.shape], cus()) % 8 == 0 and G.tile_orders([s.shape], cus()) == [2]
    run_exact([s], 43)


# ---------------------------------------------------------------------------------------------------
# eight items and the limits
# ---------------------------------------------------------------------------------------------------
def test_eight_distinct_items_in_one_call():
    specs = [Spec(256, 4, 128, 1), Spec(256, 8, 256, 3, accumulate=1), Spec(512, 36, 384, 2), Spec(256, 100, 640, 4, n_out=97),
             Spec(256, 256, 128, 2, row_map="scatter"), Spec(512, 260, 256, 1, row_map="scatter", accumulate=1), Spec(256, 12, 1280, 5, n_out=1),
             Spec(768, 64, 512, 16, accumulate=1)]
    assert len(specs) == 8
    run_exact(specs, 50)


def test_bad_arguments_are_refused_before_anything_is_launched():
    """n = 9, N % 4 != 0, K % 128 != 0, n_out > N, n_out = 0, a workspace one float too small, an A pointer off by 2 bytes: each is
    HSAD_ERR_INVALID from the host-side checks, with C, the operands and the workspace (NaN + tail pattern) untouched"""
    good = Spec(256, 64, 256, 2)
    need = G.workspace_floats([good.shape])
    trials = [("n = 9", good, dict(repeat=9)),
              ("N % 4", Spec(256, 6, 256, 2), {}),
              ("K % 128", Spec(256, 64, 192, 2), {}),
              ("n_out > N", Spec(256, 64, 256, 2, n_out=65), {}),
              ("n_out = 0", Spec(256, 64, 256, 2, n_out=0, ldc=9), {}),
              ("workspace one float short", good, dict(ws_arg=need - 1)),
              ("A off by 2 bytes", good, dict(a_off=2))]
    for i, (what, spec, kw) in enumerate(trials):
        c = G.make_case(spec, 600 + i)
        items = [G.item_of(c, kw.get("a_off", 0))] * kw.get("repeat", 1)
        ws = G.Workspace(16 * need)
        rc = G.call_group(items, ws, workspace_floats_arg=kw.get("ws_arg"))
        assert rc == G.HSAD_ERR_INVALID, (what, rc)
        assert G.canvas_untouched(c) and G.operands_intact(c) and ws.untouched(), what
    # the good item alone is taken
    run_exact([good], 699)


# ---------------------------------------------------------------------------------------------------
# the 128 x 128 kernel's path: identical bits on rounded operands (both paths cut the ranges the core plans)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,split_k", [(10240, 3), (1280, 3)])
def test_both_paths_give_identical_bits_on_rounded_operands(K, split_k):
    """hsad_gemm_set_pp(1) against (0).  At (1280, 3) the core cuts 8 8 4 k tiles where gemm_launch's own split would cut 7 7 6: the
    fallback hands the planned range length over, so the slabs hold the same partial sums, added in the same order."""
    specs = [Spec(256, 64, K, split_k), Spec(512, 260, K, split_k, n_out=257, row_map="scatter")]
    cases = [G.make_case(s, 7000 + K + i, exact=False) for i, s in enumerate(specs)]
    bits = {}
    for on in (1, 0):
        for c in cases:
            G.reset_case(c)
        with gemm_pp(on):
            launch(cases)
        bits[on] = [G.result_bits(c) for c in cases]
    for c, a, b in zip(cases, bits[1], bits[0]):
        G.check_canaries(c, c.C_dev.cpu())
        assert not torch.isnan(c.C_dev.cpu()[c.payload]).any()
        assert torch.equal(a, b), "%r: %d elements differ between the 256 x 256 core and the 128 x 128 kernel" % (c.spec, int((a != b).sum()))


# ---------------------------------------------------------------------------------------------------
# hsad_gemm_nt_bf16_splitk and _splitk_acc directly
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 512, 516])
@pytest.mark.parametrize("M", [37, 256, 300])
def test_splitk_and_splitk_acc_directly(M, N):
    """K in {128, 640, 2560} x split_k in {1, 4, 8} x with / without a row map, ldc = N + 4 > N: the plain form overwrites a NaN
    pre-fill, _acc adds to an integer pre-fill"""
    ws = G.Workspace(8 * M * N)
    for K in (128, 640, 2560):
        for row_map in (None, "scatter"):
            for acc in (0, 1):
                c = G.make_case(Spec(M, N, K, 1, ldc=N + 4, row_map=row_map, accumulate=acc), 9000 + M + N + K + acc)
                for split_k in (1, 4, 8):
                    c.spec.split_k = split_k
                    G.reset_case(c)
                    ws.poison()
                    rc = G.call_splitk(c, ws, acc)
                    assert rc == 0, last_error()
                    G.check_exact(c)
                    assert ws.tail_intact()


def test_splitk_acc_over_the_two_halves_of_a_contraction():
    """how the chunked schedule uses it: two _acc calls with the halves of a K = 1280 contraction equal one call over the whole"""
    spec = dict(ldc=520, row_map="scatter", accumulate=1)
    halves, whole = G.make_case(Spec(300, 516, 1280, 4, **spec), 9900), G.make_case(Spec(300, 516, 1280, 4, **spec), 9900)
    ws = G.Workspace(4 * 300 * 516)
    assert G.call_splitk(halves, ws, 1, K=640) == 0, last_error()
    ws.poison()
    assert G.call_splitk(halves, ws, 1, A_off=640, B_off=640, K=640) == 0, last_error()
    ws.poison()
    assert G.call_splitk(whole, ws, 1) == 0, last_error()
    G.check_exact(halves)
    G.check_exact(whole)
    assert torch.equal(G.result_bits(halves), G.result_bits(whole)) and ws.tail_intact()


# ---------------------------------------------------------------------------------------------------
# accuracy on rounded operands, one case per path, full matrices, the derived bound
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["core", "fallback", "splitk"])
def test_rounded_operands_within_the_derived_bound(path):
    K, split_k = 2560, 3
    if path == "splitk":
        c = G.make_case(Spec(300, 516, K, split_k, ldc=520, row_map="scatter"), 9990, exact=False)
        ws = G.Workspace(split_k * 300 * 516)
        assert G.call_splitk(c, ws, 0) == 0, last_error()
        assert ws.tail_intact()
        cases, plan = [c], G.plain_plan
    else:
        specs = ([small_item(accumulate=0)] if path == "fallback" else []) + [Spec(512, 260, K, split_k, n_out=257, row_map="scatter")]
        cases = [G.make_case(s, 9991 + i, exact=False) for i, s in enumerate(specs)]
        launch(cases)
        plan = G.core_plan
    for c in cases:
        ratio = G.rounded_error(c, plan(c.spec.K, c.spec.split_k)[1])
        print("%s %r: max |C - C64| / ((K + nslab) 2^-23 |A||B|^T) = %.4f" % (path, c.spec, ratio))
        assert ratio <= 1.0, (path, c.spec, ratio)
