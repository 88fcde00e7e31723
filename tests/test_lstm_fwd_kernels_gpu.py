"""GPU: the forward LSTM launches called directly and held, element by element and step by step, to the fp64 reference of
tests/lstm_fwd_ref.py (its docstring derives the bound as a sum of named roundings and describes teacher forcing, canaries and poison):
hsad_lstm_forward_fused (lstm_fused_fwd_kernel), hsad_lstm_forward_chunk_multi / _chunk / hsad_lstm_layer_forward (lstm_seq_fwd_kernel,
lstm_step_small_kernel<2..32>, lstm_step_kernel<128, 1>) and hsad_lstm_cell_fused / _pair (lstm_cell_gemm_kernel, lstm_cell_gemm256_kernel,
gemm8_kernel<G8_CELL / G8_CELL_NOSTATE>).

Inputs: x and the initial h ~ 0.5 randn as bf16, weights randn / sqrt(K) as bf16, bias 0.1 randn, |c_prev| in [0, 3]; one edge case per
family (pre-activations of +-30 / +-100, c_prev of +-20 / +-1e4 / -0.0, rows of all-zero x and h).  Nothing is excluded, there are no
quantiles.  Every case prints its worst err / bound per output (FWD-RATIO); the last test prints the module's worst (FWD-WORST) and
asserts every one <= 1; every timeout word must read 0."""
import pytest
import torch

from hanabi_sad_amd import _lib
from tests import lstm_fwd_ref as F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

WORST = {}


def report(what, ratios):
    print("FWD-RATIO %s %s" % (what, " ".join("%s=%.3f" % kv for kv in sorted(ratios.items()))))
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%s: err / bound above 1: %r" % (what, bad)


# ---------------------------------------------------------------------------------------------------
# hsad_lstm_forward_fused
# ---------------------------------------------------------------------------------------------------
FUSED = [  # T, Bn, H, nets, layers
    (2, 32, 256, 2, 3), (2, 32, 256, 1, 1), (3, 64, 512, 2, 2), (3, 64, 512, 1, 2), (5, 96, 256, 1, 3), (5, 96, 256, 1, 2), (33, 32, 256, 1, 2),
    (33, 32, 256, 2, 3), (4, 288, 256, 1, 1), (3, 128, 512, 2, 2), (3, 64, 512, 1, 1)]


@pytest.mark.parametrize("T,Bn,H,nnet,nlayer", FUSED, ids=lambda v: str(v))
def test_fused_forward_against_the_fp64_reference(T, Bn, H, nnet, nlayer):
    nets = F.make_fused_inputs(T, Bn, H, nnet, nlayer, seed=T + Bn)
    L = F.FusedFwd(T, Bn, H, nets)
    out = L.run()
    report(L.tag, L.check(out))
    # a repeat launch gives identical bits; without gates / cseq, and without hT, the same hseq16 / hT bits
    F.same_bits(out, L.run(), ("hseq", "gates", "cseq", "hT"))
    F.same_bits(out, L.run(keep=False), ("hseq", "hT"))
    F.same_bits(out, L.run(hT=False), ("hseq", "gates", "cseq"))
    F.same_bits(out, L.run(keep=False, hT=False), ("hseq",))


def test_fused_forward_edge_inputs():
    T, Bn, H = 4, 64, 256
    nets = F.make_fused_inputs(T, Bn, H, 1, 2, seed=9, edge=True)
    L = F.FusedFwd(T, Bn, H, nets)
    out = L.run()
    report(L.tag + " edge", L.check(out, "fused edge"))
    F.same_bits(out, L.run(keep=False), ("hseq", "hT"))


def test_fused_forward_cross_xcd_exchange_and_ping_pong_scratch():
    T, Bn, H = 5, 96, 256
    nets = F.make_fused_inputs(T, Bn, H, 1, 2, seed=11)
    L = F.FusedFwd(T, Bn, H, nets)
    out = L.run()
    report(L.tag, L.check(out))
    F.same_bits(out, L.run(partner=True), ("hseq", "gates", "cseq", "hT"))
    try:
        _lib.check(L.lib.hsad_lstm_set_exchange_mode(1))
        forced = L.run()
    finally:
        _lib.check(L.lib.hsad_lstm_set_exchange_mode(0))
    report(L.tag + " cross-XCD", L.check(forced, "fused cross-XCD"))
    F.same_bits(out, forced, ("hseq", "gates", "cseq", "hT"))


# ---------------------------------------------------------------------------------------------------
# hsad_lstm_forward_chunk_multi / _chunk / hsad_lstm_layer_forward
# ---------------------------------------------------------------------------------------------------
def seq_case(entry, T, Bn, H, nrec=1, edge=False, c_prev=True, kern=None, seed=0, **kw):
    recs = F.make_seq_inputs(T, Bn, H, nrec, seed=seed + Bn + H, edge=edge, c_prev=c_prev)
    S = F.SeqFwd(entry, T, Bn, H, recs, **kw)
    S.launch()
    out = S.outputs()
    report(S.tag + (" edge" if edge else ""), S.check(out, kern or ("seq" if entry != "steps" else "step H%d" % H)))
    return S, out


PERSISTENT = [  # Bn, H, T, records, xchg, c_prev, hT
    (1, 256, 3, 1, False, True, True), (1, 512, 2, 2, True, True, True), (31, 256, 5, 4, True, True, False), (31, 512, 3, 1, False, False, True),
    (40, 256, 4, 2, True, False, True), (40, 512, 5, 1, True, True, True), (70, 256, 5, 2, False, True, True), (70, 512, 3, 2, True, True, False),
    (128, 256, 5, 4, True, True, True), (128, 512, 2, 1, True, False, False), (128, 512, 4, 2, False, True, True), (128, 256, 3, 1, False, True, True)]


@pytest.mark.parametrize("Bn,H,T,nrec,xchg,c_prev,hT", PERSISTENT, ids=lambda v: str(v))
def test_chunk_multi_against_the_fp64_reference(Bn, H, T, nrec, xchg, c_prev, hT):
    seq_case("multi", T, Bn, H, nrec, c_prev=c_prev, xchg=xchg, hT=hT)


def test_chunk_multi_edge_inputs():
    seq_case("multi", 4, 70, 256, 2, edge=True, xchg=True, kern="seq edge")


@pytest.mark.parametrize("xchg", [False, True])
def test_a_sequence_cut_in_two_chunks_carries_its_state(xchg):
    T, Bn, H = 5, 40, 256
    recs = F.make_seq_inputs(T, Bn, H, 2, seed=21)
    whole = F.SeqFwd("multi", T, Bn, H, recs, xchg=xchg)
    whole.launch()
    want = whole.outputs()
    cut = F.SeqFwd("multi", T, Bn, H, recs, xchg=xchg)
    cut.launch(0, 3)
    cut.launch(3, 2)
    out = cut.outputs()
    report(cut.tag + " cut 3 + 2", cut.check(out, "seq"))
    for a, b in zip(want, out):
        for name in ("hseq", "cseq", "gates", "hT"):
            assert torch.equal(a[name], b[name]), name + " differs between the whole sequence and its two chunks"


@pytest.mark.parametrize("Bn,H", [(31, 256), (128, 512)])
def test_forward_chunk_and_persistent_layer_forward(Bn, H):
    seq_case("chunk", 4, Bn, H)
    seq_case("layer", 4, Bn, H)
    seq_case("layer", 3, Bn, H, h0=False, hT=False)


@pytest.mark.parametrize("H", [64, 128, 192, 256, 512, 1024])
@pytest.mark.parametrize("Bn", [1, 40])
def test_per_step_layer_forward_against_the_fp64_reference(Bn, H):
    S, out = seq_case("steps", 3, Bn, H, seed=1)
    # keep_gates = 0 leaves `gates` as it was and changes nothing else; h0 NULL = zeros
    Z, out0 = seq_case("steps", 3, Bn, H, seed=1, keep_gates=0, h0=bool(Bn & 1), hT=bool(Bn & 1))
    if Bn & 1:
        for name in ("hseq", "cseq", "hT"):
            assert torch.equal(out[0][name], out0[0][name]), name + " depends on keep_gates"


def test_per_step_layer_forward_large_batch_and_edge_inputs():
    seq_case("steps", 2, 1030, 64, kern="step 128-row")
    seq_case("steps", 2, 1030, 64, kern="step 128-row", keep_gates=0, h0=False)
    seq_case("steps", 3, 40, 128, edge=True, kern="step edge")
    seq_case("steps", 2, 40, 192, edge=True, kern="step edge")


# ---------------------------------------------------------------------------------------------------
# hsad_lstm_cell_fused / hsad_lstm_cell_fused_pair
# ---------------------------------------------------------------------------------------------------
SUBSETS = [(("c", "h32", "h16"), False), (("c",), False), (("h32",), False), (("h16",), False), (("c", "h32", "h16"), True), (("c", "h16"), True)]


def cell_case(kern, Bn, H, Kx, variant, outs=("c", "h32", "h16"), alias=False, ldx=None, edge=False, seed=0):
    d = F.make_cell_inputs(Bn, H, Kx, ldx=ldx, seed=seed + Bn + Kx, edge=edge)
    P = F.CellProblem(Bn, H, d, outs, alias)
    F.run_cell(P, variant)
    ratios = {}
    tag = "cell %s Bn%d H%d Kx%d ldx%d %s%s%s" % (kern, Bn, H, Kx, d["ldx"], "+".join(outs), " c_out=c_prev" if alias else "", " edge" if edge else "")
    P.check(tag, "cell " + kern, ratios)
    report(tag, ratios)


def cases_128():
    out, i = [], 0
    for Bn in (1, 37, 128, 129, 300):
        for H in (64, 256):
            for Kx in (64, 192, 896):
                outs, alias = SUBSETS[i % len(SUBSETS)]
                out.append((Bn, H, Kx, outs, alias))
                i += 1
    return out


@pytest.mark.parametrize("Bn,H,Kx,outs,alias", cases_128(), ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_cell_128_tile_against_the_fp64_reference(Bn, H, Kx, outs, alias):
    cell_case("128", Bn, H, Kx, (128, 1), outs, alias)


@pytest.mark.parametrize("outs,alias", SUBSETS, ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_cell_output_subsets_with_padded_rows_of_nan(outs, alias):
    """ldx = Kx + 8, the padding columns hold NaN: never read"""
    cell_case("128", 129, 64, 192, (128, 1), outs, alias, ldx=200)
    cell_case("256", 300, 64, 192, (256, 0), outs, alias, ldx=200)
    cell_case("gemm8", 256, 64, 192, (256, 1), outs, alias, ldx=200)


@pytest.mark.parametrize("Bn,H,Kx,variant,kern", [
    (256, 64, 64, (256, 0), "256"), (300, 256, 192, (256, 0), "256"), (300, 64, 896, (256, 0), "256"), (256, 256, 896, (256, 0), "256"),
    (256, 64, 64, (256, 1), "gemm8"), (512, 256, 256, (256, 1), "gemm8"), (512, 64, 192, (256, 1), "gemm8"), (256, 256, 896, (256, 1), "gemm8"),
    (512, 64, 128, (256, 1), "256"),                 # (Kx + H) / 64 odd: quietly the one-barrier kernel
    (4096, 64, 64, None, "gemm8")],                  # the default dispatch
    ids=lambda v: str(v))
def test_cell_256_tiles_against_the_fp64_reference(Bn, H, Kx, variant, kern):
    cell_case(kern, Bn, H, Kx, variant)


def test_cell_edge_inputs():
    cell_case("128 edge", 129, 64, 192, (128, 1), edge=True)
    cell_case("128 edge", 37, 256, 64, (128, 1), edge=True)
    cell_case("256 edge", 300, 64, 64, (256, 0), edge=True)
    cell_case("gemm8 edge", 256, 64, 192, (256, 1), edge=True, alias=True)


@pytest.mark.parametrize("Bn,kern", [(4096, "gemm8 pair"), (300, "128 pair")])
def test_cell_pair_against_the_fp64_reference(Bn, kern):
    """problem b stateless (only its bf16 output), as the target net of an acting step; Bn = 300: the fallback to two launches"""
    H, Kx = 64, 64
    da, db = F.make_cell_inputs(Bn, H, Kx, seed=31), F.make_cell_inputs(Bn, H, Kx, seed=32)
    Pa, Pb = F.CellProblem(Bn, H, da), F.CellProblem(Bn, H, db, ("h16",))
    F.run_cell_pair(Pa, Pb)
    ratios = {}
    Pa.check("pair a Bn%d" % Bn, "cell " + kern, ratios)
    Pb.check("pair b Bn%d" % Bn, "cell " + kern + " stateless", ratios)
    report("cell pair Bn%d" % Bn, ratios)


def test_zz_worst_ratios_of_the_module():
    print("FWD-WORST " + " ".join("%s=%.3f" % kv for kv in sorted(WORST.items())))
    assert WORST, "no case of this module ran before its summary"
    bad = {k: v for k, v in WORST.items() if not v <= 1.0}
    assert not bad, "err / bound above 1: %r" % bad
