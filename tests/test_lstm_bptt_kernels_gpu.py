"""GPU: the persistent BPTT launches called directly and held, element by element and step by step, to the fp64 reference of
tests/lstm_bptt_ref.py (its docstring derives the bound |got - ref| <= 2^-8 |ref| + (4H P + 16 T) 2^-23 M and describes teacher forcing,
canaries and poison).  hsad_lstm_backward_fused in both blockings (lstm_fused_bwd_kernel<64> / <32>, lstm_bptt_wide_kernel) and every
stage layout, a sequence cut into two chunks, hsad_lstm_backward_chunk_multi and hsad_lstm_layer_backward on row-major activations.

Inputs are synthetic (no forward pass): i, f, o in (0.02, 0.98), g in (-0.98, 0.98), |c| in [0.25, 3], weights randn / sqrt(H) as bf16,
dO randn 0.1, dc_io randn 0.05.  Nothing is excluded, there are no quantiles.  Every case prints its worst err / bound per stage and the
share of dG elements that equal the correctly rounded reference (a figure, not asserted); every timeout word must read 0."""
import pytest
import torch

from tests import lstm_bptt_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

WORST = {}


def report(spec, ratios, exact):
    print("BPTT-RATIO %r %s exact-share %.4f" % (spec, " ".join("%s=%.3f" % kv for kv in sorted(ratios.items())), exact))
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%r: err / bound above 1: %r" % (spec, bad)


def run_and_check(spec, inp=None):
    inp = R.make_inputs(spec) if inp is None else inp
    L = R.FusedLaunch(spec, inp)
    L.run()
    L.assert_inputs_unchanged()
    out = L.outputs()
    ratios, exact = R.check_fused(spec, inp, out)
    report(spec, ratios, exact)
    return L, inp, out


def cases_32x32():
    out, i = [], 0
    for T, Bn, H in ((3, 32, 512), (4, 64, 256), (5, 96, 256)):
        for mode in ("plain", "split", "proj", "sink"):
            for dgt in (False, True):
                for frag in (True, False):
                    out.append(R.Spec(T, Bn, H, mode=mode, dgt=dgt, frag=frag, sink_T=bool(i & 1), bias1=bool(i & 2), colmap_perm=bool(i & 4),
                                      c_before=bool(i & 8), mask=bool((i >> 1) & 1) or not (i & 1), seed=i))
                    i += 1
    # one and three stacked layers, two nets (at most 6 pipeline stages per launch)
    for nnet, nlayer, mode, T, Bn in ((1, 1, "plain", 4, 64), (1, 3, "plain", 5, 96), (1, 3, "split", 4, 64), (1, 3, "sink", 5, 96),
                                      (2, 2, "plain", 4, 64), (2, 2, "split", 4, 64), (2, 2, "proj", 4, 64), (2, 1, "plain", 4, 64)):
        for dgt in (False, True):
            out.append(R.Spec(T, Bn, 256, nnet=nnet, nlayer=nlayer, mode=mode, dgt=dgt, frag=not (i & 1), bias1=bool(i & 2), colmap_perm=bool(i & 4),
                              c_before=bool(i & 2), seed=i))
            i += 1
    return out


def spec_id(s):
    return "T%d-B%d-H%d-n%dx%d-%s%s%s%s%s%s%s" % (s.T, s.Bn, s.H, s.nnet, s.nlayer, s.mode, "-dGT" if s.dgt else "", "-frag" if s.frag else "-rows",
                                                  "-sinkT" if s.sink_T else "", "" if s.bias1 else "-nobias1", "-perm" if s.colmap_perm else "",
                                                  "-c0" if s.c_before else "")


@pytest.mark.parametrize("spec", cases_32x32(), ids=spec_id)
def test_32x32_kernel_against_the_fp64_reference(spec):
    run_and_check(spec)


def cases_wide():
    out, i = [], 100
    for T, Bn in ((2, 32), (5, 96), (3, 128), (1, 32)):            # the ordinary shapes before T = 1
        for sink_T, nobias1, perm, c0 in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1)):
            out.append(R.Spec(T, Bn, 512, mode="sink", dgt=True, frag=True, wide=True, sink_T=bool(sink_T), bias1=not nobias1, colmap_perm=bool(perm),
                              c_before=bool(c0), mask=True, seed=i))
            i += 1
    return out


@pytest.mark.parametrize("spec", cases_wide(), ids=spec_id)
def test_wide_kernel_against_the_fp64_reference(spec):
    props = torch.cuda.get_device_properties(0)
    assert props.multi_processor_count >= 256, "the 16 x 64 blocking needs 256 CUs: the launcher would run the 32 x 32 kernel instead"
    run_and_check(spec)       # (the hand-off tiles are read in the 16-row blocking: another kernel's tiles would not equal dG)


@pytest.mark.parametrize("mode", ["plain", "split", "proj", "sink"])
@pytest.mark.parametrize("frag", [True, False], ids=["frag", "rows"])
def test_32x32_kernel_in_two_chunks_against_the_reference_of_the_whole_sequence(mode, frag):
    """(6, 64, 256) cut 4 + 2: the later chunk first (has_next 0), then the earlier one (has_next 1: its last step reads slot Tc of dG16, the
    later chunk's first step; c_before points into cseq; dc_io carried in place), layout_steps 4 on both"""
    spec = R.Spec(6, 64, 256, mode=mode, frag=frag, c_before=True, seed=200 + frag)
    inp = R.make_inputs(spec)
    L = R.FusedLaunch(spec, inp)
    L.run(t0=4, Tc=2, has_next=0, layout_steps=4)
    L.run(t0=0, Tc=4, has_next=1, layout_steps=4)
    L.assert_inputs_unchanged()
    out = L.outputs(window=(0, 4))
    ratios, exact = R.check_fused(spec, inp, out)
    report(spec, ratios, exact)


# (hsad_lstm_backward_chunk_multi takes H in {256, 512}; H = 64 is hsad_lstm_layer_backward's per-step path)
ROW_MAJOR = [(e, T, Bn, H) for T, Bn, H in ((3, 40, 64), (4, 70, 256), (2, 128, 512)) for e in ("multi1", "multi2", "layer-sync", "layer-steps")
             if H != 64 or e.startswith("layer")]


@pytest.mark.parametrize("entry,T,Bn,H", ROW_MAJOR)
def test_row_major_entry_points_against_the_fp64_reference(entry, T, Bn, H):
    """hsad_lstm_backward_chunk_multi (one and two records) and hsad_lstm_layer_backward (sync_scratch given and NULL): row-major
    activations, Bn not a multiple of 32.  hsad_lstm_layer_backward starts from dc = 0 and hands no dc back."""
    g = torch.Generator().manual_seed(300 + T)
    layers = [R.make_layer_inputs(g, T, Bn, H, True, False, False, c_before=bool(k), mask=False) for k in range(2 if entry == "multi2" else 1)]
    if entry.startswith("layer"):
        layers[0]["dc0"] = torch.zeros(Bn, H)
    res = R.run_seq_entry("multi" if entry.startswith("multi") else "layer", T, Bn, H, layers, with_sync=entry != "layer-steps")
    ratios, exact = {}, []
    for d, (dG, tail, dc) in zip(layers, res):
        if entry.startswith("multi"):       # (hsad_lstm_layer_backward: "slot T is scratch", zeroed by one of its paths only)
            assert bool((tail == 0).all()), "dG16 slot T is not zero after a launch without has_next"
        ref, M, dc_ref, dc_abs = R.check_layer("", d, dG, H, T, d["dO"].double(), None, None, ratios, "rows", 1, exact)
        if entry.startswith("multi"):
            ratios["rows dc_io"] = max(ratios.get("rows dc_io", 0.0), R.worst_ratio(R.f32_values(dc), dc_ref, R.dc_bound(dc_abs, H, T)))
    report((entry, T, Bn, H), ratios, min(exact))


def edge_inputs(spec):
    """-> inputs with exact edges, and where they are: rows 3 and 17 have dO = 0 from step 1 on and dc_io = 0 (in both layers: the learner's
    padded steps); c_t = 0.0, i = 1.0, f = 0.0 at scattered elements; the sink mask is drawn from {0, -0.0, -1, 2^-126, 1}"""
    inp = R.make_inputs(spec)
    T, Bn, H = spec.T, spec.Bn, spec.H
    g = torch.Generator().manual_seed(77)
    pad_rows, s0 = [3, 17], 1
    where = {}
    for k, d in enumerate(inp[0]):
        d["dc0"][pad_rows] = 0.0
        if d["dO"] is not None:
            d["dO"][s0:, pad_rows] = 0.0
        czero = torch.rand(T, Bn, H, generator=g) < 0.02
        d["c"][czero] = 0.0
        gv = d["gates"].view(T, Bn, H // 32, 4, 32)
        ione = torch.rand(T, Bn, H // 32, 32, generator=g) < 0.02
        fzero = torch.rand(T, Bn, H // 32, 32, generator=g) < 0.02
        gv[:, :, :, 0, :][ione] = 1.0
        gv[:, :, :, 1, :][fzero] = 0.0
        where[k] = (czero.view(T, Bn, H // 32, 32), ione, fzero)
    vals = torch.tensor([0.0, -0.0, -1.0, 2.0 ** -126, 1.0]).to(torch.bfloat16)
    inp[0][-1]["mask"] = vals[torch.randint(0, 5, (T, Bn, H), generator=g)]
    return inp, pad_rows, s0, where


@pytest.mark.parametrize("wide", [False, True], ids=["32x32", "wide"])
def test_exact_edges(wide):
    spec = R.Spec(3, 64, 512, mode="sink", dgt=True, frag=True, wide=True, seed=400) if wide else R.Spec(4, 64, 256, mode="sink", dgt=True, frag=True, seed=401)
    inp, pad_rows, s0, where = edge_inputs(spec)
    L, inp, out = run_and_check(spec, inp)
    T, Bn, H = spec.T, spec.Bn, spec.H
    for k in range(2):
        bits = out[0][k]["dG"].view(T, Bn, H // 32, 4, 32)
        mag = bits & 0x7FFF           # 0 for +0 and -0
        assert bool((mag[s0:, pad_rows] == 0).all()), "layer %d: a padded row's dG is not a zero" % k
        czero, ione, fzero = where[k]
        assert int(czero.sum()) and int(ione.sum()) and int(fzero.sum())
        assert bool((mag[:, :, :, 3, :][czero] == 0).all()), "layer %d: c_t = 0 must give an o-gate gradient of exactly 0" % k
        assert bool((mag[:, :, :, 0, :][ione] == 0).all()), "layer %d: i = 1 must give an i-gate gradient of exactly 0" % k
        assert bool((mag[:, :, :, 1, :][fzero] == 0).all()), "layer %d: f = 0 must give an f-gate gradient of exactly 0" % k
        assert bool((mag != 0).float().mean() > 0.8)       # (zeros besides the planted ones: the f-gate column of step 0, c_before = 0)
    # the sink is "on" only where the mask is > 0: 2^-126 and 1 of the five values
    m = inp[0][1]["mask"].float()
    on = m > 0
    sink = out[0][1]["sink"]
    assert bool((sink[~on] == 0).all()) and 0.3 < float(on.float().mean()) < 0.5
    assert float((sink[on] != 0).float().mean()) > 0.95,"sink rows under a positive mask are missing"
    # padded rows: the sink's rows are zeros as well (dG is), whatever the mask
    assert bool(((sink[s0:, pad_rows] & 0x7FFF) == 0).all())


@pytest.mark.parametrize("wide", [False, True], ids=["32x32", "wide"])
def test_a_repeat_launch_gives_the_same_bits(wide):
    spec = R.Spec(3, 96, 512, mode="sink", dgt=True, frag=True, wide=True, sink_T=True, colmap_perm=True, seed=500) if wide else \
        R.Spec(5, 96, 256, mode="sink", dgt=True, frag=True, seed=501)
    L, inp, out = run_and_check(spec)
    first = R.deterministic_bits(spec, out)
    L.poison_outputs()
    L.run()
    second = R.deterministic_bits(spec, L.outputs())
    assert [n for n, _ in first] == [n for n, _ in second]
    for (name, a), (_, b) in zip(first, second):
        assert torch.equal(a, b), "%s differs between two launches of the same case" % name
    if wide:
        assert any(n == "bias0" for n, _ in first) and any(n == "sink_bias" for n, _ in first)      # ticketed sums: the same bits run to run


def test_zz_worst_ratios_of_the_module():
    """(prints the module's worst err / bound per kernel and stage: the figures quoted in DESIGN.md)"""
    for k, v in sorted(WORST.items()):
        print("BPTT-WORST %s %.3f" % (k, v))
    assert all(v <= 1.0 for v in WORST.values())
