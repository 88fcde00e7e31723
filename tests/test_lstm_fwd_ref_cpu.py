"""CPU: the fp64 forward reference and the bound of tests/lstm_fwd_ref.py are held to something independent before the GPU tests lean
on them -- without looking at the code under test.

* With rounding switched off (free running) the reference is torch.nn.LSTM in fp64 (weights copied, 2 layers) to 1e-12.
* HONEST MODELS: the kernels' arithmetic restated in fp32 on the CPU (fp32 matmul on the bf16 operand values, the kernels' own
  activation formulas -- sigmoidf_ / tanhf_ through exp2 and a reciprocal, and the clamped two-reciprocal cell update --, bf16 rounding
  of h), run on the GPU test's input generators, edge inputs included, and put through the very checkers the GPU outputs go through.
  Share of elements that may exceed err / bound = 1:  0.
* PLANTED ERRORS, each of which must give err / bound > 1: one dropped product of the K, i and f swapped for one unit, c_prev taken from
  the neighbouring row, h16 off by one bf16 ulp, c replaced by its bf16 rounding, the stacked layer reading x_{t-1} instead of x_t, one
  saved gate written to the neighbouring fragment slot.
* The ctypes mirrors of hsad_lstm_fwd_rec / hsad_lstm_fused_rec have the C compiler's sizeof and field offsets; the gate16 index map
  inverts r2d2.gate16_perm."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from hanabi_sad_amd import _lib, r2d2
from tests import lstm_fwd_ref as F
from tests.lstm_bptt_ref import _bits, pack_saved_c, pack_saved_gates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")


def test_the_unrounded_reference_is_nn_lstm_in_fp64():
    T, Bn, H, Fin = 5, 3, 32, 24
    torch.manual_seed(3)
    lstm = torch.nn.LSTM(Fin, H, num_layers=2).double()
    x = torch.randn(T, Bn, Fin, dtype=torch.float64)
    h0, c0 = torch.randn(2, Bn, H, dtype=torch.float64), torch.randn(2, Bn, H, dtype=torch.float64)
    with torch.no_grad():
        want, (hn, cn) = lstm(x, (h0, c0))
    seq = x
    for l in range(2):
        Wih, Whh = getattr(lstm, "weight_ih_l%d" % l).detach(), getattr(lstm, "weight_hh_l%d" % l).detach()
        bias = (getattr(lstm, "bias_ih_l%d" % l) + getattr(lstm, "bias_hh_l%d" % l)).detach()
        h, c, hs = h0[l], c0[l], []
        for t in range(T):
            r = F.step64(bias, seq[t], Wih, h, Whh, c)
            h, c = r["h"], r["c"]
            hs.append(h)
        seq = torch.stack(hs)
        assert float((h - hn[l]).abs().max()) < 1e-12 and float((c - cn[l]).abs().max()) < 1e-12
    assert float((seq - want).abs().max()) < 1e-12


def test_the_column_orders_invert():
    H = 64
    perm = r2d2.gate16_perm(H, "cpu")
    for gate in range(4):
        for unit in range(H):
            assert int(perm[F.gate16_row(gate, unit)]) == gate * H + unit
    assert sorted(F.gate16_row(g, u) for g in range(4) for u in range(H)) == list(range(4 * H))
    nat = torch.arange(3 * 4 * H, dtype=torch.float64).reshape(3, 4 * H)
    assert torch.equal(F.from_blocked(F.to_blocked(nat, H), H), nat) and not torch.equal(F.to_blocked(nat, H), nat)
    # gate-blocked column nb * 128 + gate * 32 + u holds gate `gate` of unit 32 nb + u
    assert float(F.to_blocked(nat, H)[0, 1 * 128 + 2 * 32 + 5]) == float(nat[0, 2 * H + 32 + 5])
    T, Bn, Hf = 2, 32, 256
    g = torch.randn(T, Bn, 4 * Hf)
    c = torch.randn(T, Bn, Hf)
    assert torch.equal(F.unpack_with(pack_saved_gates, pack_saved_gates(g, T, Bn, Hf).reshape(-1), T, Bn, 4 * Hf), g)
    assert torch.equal(F.unpack_with(pack_saved_c, pack_saved_c(c, T, Bn, Hf).reshape(-1), T, Bn, Hf), c)
    assert torch.equal(F.unpack_with(pack_saved_c, c.reshape(-1), T, Bn, Hf), r2d2.unpack_saved_c(c.reshape(-1), T, Bn, Hf))


# ---------------------------------------------------------------------------------------------------
# honest models in the harness' output format
# ---------------------------------------------------------------------------------------------------
def f32_bits(x):
    return _bits(x.to(torch.float32))


def sim_fused(T, Bn, H, nets, plant=None):
    """the fused forward, free running, in fp32 on the CPU -> out[net][layer] as FusedFwd.run returns it"""
    out = []
    for net in nets:
        below, row = None, []
        for l, d in enumerate(net["layers"]):
            xs = net["x"] if l == 0 else below
            h16, c = torch.zeros(Bn, H, dtype=torch.bfloat16), torch.zeros(Bn, H)
            hs, cs, gs, h32 = [], [], [], None
            for t in range(T):
                x_t = xs[t]
                if plant == "x_tm1" and l == 1 and t == 2:
                    x_t = xs[t - 1]
                p = F.preact_model(d["bias"], x_t, d["Wih"], h16, d["Whh"])
                if plant == "drop_product" and l == 0 and t == 1:
                    k = int((x_t[3].float() * d["Wih"][5].float()).abs().argmax())
                    p[3, 5] -= x_t[3, k].float() * d["Wih"][5, k].float()
                if plant == "swap_if" and l == 0 and t == 1:
                    p[:, [7, H + 7]] = p[:, [H + 7, 7]]
                cp = c.roll(1, 0) if (plant == "c_prev_neighbour" and l == 0 and t == 2) else c
                m = F.plain_model(p, cp)
                c, h16, h32 = m["c"], m["h16"], m["h32"]
                if plant == "c_bf16" and l == 0 and t == 1:
                    c = c.to(torch.bfloat16).float()
                if plant == "h16_ulp" and l == 0 and t == 1:
                    h16 = h16.clone()
                    h16[4] = (h16[4].view(torch.int16) + 1).view(torch.bfloat16)
                hs.append(h16)
                cs.append(c)
                gs.append(m["gates"])
            below = torch.stack(hs)
            gates = pack_saved_gates(F.to_blocked(torch.stack(gs), H), T, Bn, H).reshape(-1)
            if plant == "gate_slot" and l == 0:
                k = 4 * (64 * 5 + 9)                         # (i, f, g, o) of one lane: i lands in f's slot and f in i's
                gates[[k, k + 1]] = gates[[k + 1, k]]
            row.append(dict(hseq=_bits(below).reshape(T, Bn, H), gates=f32_bits(gates), cseq=f32_bits(pack_saved_c(torch.stack(cs), T, Bn, H).reshape(-1)),
                            hT=f32_bits(h32).reshape(Bn, H)))
        out.append(row)
    return out


def sim_seq(T, Bn, H, recs):
    out = []
    for d in recs:
        h16 = d["h0"].to(torch.bfloat16)
        c = d["c_prev"] if d["c_prev"] is not None else torch.zeros(Bn, H)
        hs, cs, gs, h32 = [], [], [], None
        for t in range(T):
            m = F.plain_model(F.preact_model(d["pre"][t], None, None, h16, d["Whh"]), c)
            c, h16, h32 = m["c"], m["h16"], m["h32"]
            hs.append(h16)
            cs.append(c)
            gs.append(m["gates"])
        out.append(dict(hseq=_bits(torch.stack(hs)).reshape(T, Bn, H), cseq=f32_bits(torch.stack(cs)).reshape(T, Bn, H),
                        gates=f32_bits(F.to_blocked(torch.stack(gs), H)).reshape(T, Bn, 4 * H), hT=f32_bits(h32).reshape(Bn, H)))
    return out


def sim_cell(d, plant=None):
    Kx = d["Kx"]
    p = F.preact_model(d["bias"], d["x"][:, :Kx], d["Wcat"][:, :Kx], d["h_prev"], d["Wcat"][:, Kx:])
    H = d["h_prev"].shape[1]
    if plant == "drop_product":
        k = int((d["x"][0, :Kx].float() * d["Wcat"][5, :Kx].float()).abs().argmax())
        p[0, 5] -= d["x"][0, k].float() * d["Wcat"][5, k].float()
    if plant == "swap_if":
        p[:, [20, H + 20]] = p[:, [H + 20, 20]]
    m = F.clamped_model(p, d["c_prev"].roll(1, 0) if plant == "c_prev_neighbour" else d["c_prev"])
    if plant == "c_bf16":
        m["c"] = m["c"].to(torch.bfloat16).float()
    if plant == "h16_ulp":
        m["h16"][4] = (m["h16"][4].view(torch.int16) + 1).view(torch.bfloat16)
    return m


def cell_ratios(d, m):
    r, b = F.cell_reference(d)
    ratios = {}
    F.ratio_into(ratios, "c", m["c"].double(), r["c"], b["c"])
    F.ratio_into(ratios, "h32", m["h32"].double(), r["h"], b["h32"])
    F.ratio_into(ratios, "h16", m["h16"].double(), r["h"], b["h16"])
    return ratios


def assert_inside(what, ratios):
    print("FWD-HONEST %s %s" % (what, " ".join("%s=%.3f" % kv for kv in sorted(ratios.items()))))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}          # the maximum over every element: the share that may exceed is 0
    assert not bad, "%s: the honest model exceeds the bound: %r" % (what, bad)


@pytest.mark.parametrize("T,Bn,H,nnet,nlayer,edge", [(3, 32, 256, 1, 2, False), (3, 32, 256, 1, 3, True), (2, 32, 512, 2, 2, False), (2, 32, 512, 1, 2, True)])
def test_the_honest_fused_model_stays_inside_the_bound(T, Bn, H, nnet, nlayer, edge):
    nets = F.make_fused_inputs(T, Bn, H, nnet, nlayer, seed=1, edge=edge)
    assert_inside("fused", F.check_fused(T, Bn, H, nets, sim_fused(T, Bn, H, nets)))


@pytest.mark.parametrize("T,Bn,H,edge,c_prev", [(3, 40, 256, False, True), (3, 40, 512, True, True), (2, 40, 64, True, True), (2, 7, 1024, False, False),
                                                (2, 33, 192, True, True)])
def test_the_honest_row_major_model_stays_inside_the_bound(T, Bn, H, edge, c_prev):
    recs = F.make_seq_inputs(T, Bn, H, 2, seed=2, edge=edge, c_prev=c_prev)
    assert_inside("row-major", F.check_seq(T, Bn, H, recs, sim_seq(T, Bn, H, recs), "seq"))


@pytest.mark.parametrize("Bn,H,Kx,edge", [(37, 64, 192, False), (37, 64, 64, True), (129, 256, 896, False), (129, 256, 896, True), (300, 256, 64, True)])
def test_the_honest_clamped_cell_model_stays_inside_the_bound(Bn, H, Kx, edge):
    d = F.make_cell_inputs(Bn, H, Kx, ldx=Kx + 8, seed=3, edge=edge)
    m = sim_cell(d)
    assert all(bool(torch.isfinite(m[k].float()).all()) for k in ("c", "h32", "h16"))
    assert_inside("cell", cell_ratios(d, m))


def test_the_edge_inputs_reach_the_clamps_and_the_overflow_of_expf():
    d = F.make_cell_inputs(37, 64, 64, seed=3, edge=True)
    r, _ = F.cell_reference(d)
    p = r["p"].abs()
    assert int((p[:, :64] > 25).sum()) > 0 and int((p[:, 128:192] > 12.5).sum()) > 0 and int((r["c"].abs() > 12.5).sum()) > 0
    assert int((p > 88.8).sum()) > 0                      # e^88.8 is past the largest fp32
    assert float(F.expf_model(torch.tensor(100.0))) == float("inf") and float(F.sigmoid_model(torch.tensor(-100.0))) == 0.0
    assert bool((d["x"][F.EDGE_ZERO_ROW, :64] == 0).all()) and bool((d["h_prev"][F.EDGE_ZERO_ROW] == 0).all())
    assert bool(torch.signbit(d["c_prev"][F.EDGE_NEG0_ROW]).all()) and bool((d["c_prev"][F.EDGE_NEG0_ROW] == 0).all())
    # all-zero operands: the pre-activation is the bias, exactly
    assert torch.equal(r["p"][F.EDGE_ZERO_ROW], d["bias"].double())


PLANTS = ("drop_product", "swap_if", "c_prev_neighbour", "h16_ulp", "c_bf16", "x_tm1", "gate_slot")


@pytest.mark.parametrize("plant", PLANTS)
def test_a_planted_error_in_the_fused_forward_is_caught(plant):
    T, Bn, H = 3, 32, 256
    nets = F.make_fused_inputs(T, Bn, H, 1, 2, seed=4)
    ratios = F.check_fused(T, Bn, H, nets, sim_fused(T, Bn, H, nets, plant))
    print("FWD-PLANT %s %s" % (plant, " ".join("%s=%.3g" % kv for kv in sorted(ratios.items()))))
    assert max(ratios.values()) > 1.0


@pytest.mark.parametrize("plant", PLANTS[:5])
def test_a_planted_error_in_the_clamped_cell_is_caught(plant):
    d = F.make_cell_inputs(37, 64, 192, seed=5)
    ratios = cell_ratios(d, sim_cell(d, plant))
    print("FWD-PLANT cell %s %s" % (plant, " ".join("%s=%.3g" % kv for kv in sorted(ratios.items()))))
    assert max(ratios.values()) > 1.0


LAYOUT_C = """#include <stddef.h>
#include <stdio.h>
#include "hsad.h"
#define A(f) printf(#f " %zu %zu\\n", offsetof(hsad_lstm_fwd_rec, f), sizeof(((hsad_lstm_fwd_rec*)0)->f))
#define B(f) printf(#f " %zu %zu\\n", offsetof(hsad_lstm_fused_rec, f), sizeof(((hsad_lstm_fused_rec*)0)->f))
int main(void) {
  printf("struct hsad_lstm_fwd_rec %zu\\n", sizeof(hsad_lstm_fwd_rec));
  A(gates); A(Whh_blocked); A(h_prev16); A(c_prev); A(hseq16); A(cseq); A(hT); A(xchg);
  printf("struct hsad_lstm_fused_rec %zu\\n", sizeof(hsad_lstm_fused_rec));
  B(Wih_blocked); B(Whh_blocked); B(bias_blocked); B(x16); B(gates); B(cseq); B(hseq16); B(hT);
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_ctypes_records_have_the_c_layout(tmp_path):
    src, exe = str(tmp_path / "fwd_rec_layout.c"), str(tmp_path / "fwd_rec_layout")
    with open(src, "w") as f:
        f.write(LAYOUT_C)
    cmd = ["gcc", "-std=c11", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + SAN + ["-I", os.path.join(ROOT, "include"), src, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, **SAN_ENV))
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    text = open(os.path.join(ROOT, "include", "hsad.h")).read()
    got, cur = {}, None
    for ln in run.stdout.splitlines():
        p = ln.split()
        if p[0] == "struct":
            cur = got.setdefault(p[1], dict(size=int(p[2]), fields=[]))
        else:
            cur["fields"].append((p[0], int(p[1]), int(p[2])))
    for name, mirror in (("hsad_lstm_fwd_rec", _lib.LstmFwdRec), ("hsad_lstm_fused_rec", _lib.LstmFusedRec)):
        assert got[name]["size"] == C.sizeof(mirror)
        assert got[name]["fields"] == [(f, getattr(mirror, f).offset, getattr(mirror, f).size) for f, _ in mirror._fields_]
        # the header's own field list, in order (a field added in a padding hole would leave sizeof unchanged)
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            if decl.strip():
                names += [re.sub(r"[\s*]", "", part.split()[-1]) for part in decl.split(",")]
        assert names == [f for f, _ in mirror._fields_]
