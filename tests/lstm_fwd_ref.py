"""Helper (not a test) of tests/test_lstm_fwd_ref_cpu.py and tests/test_lstm_fwd_kernels_gpu.py: a step-by-step fp64 reference of the
forward LSTM launches of include/hsad.h and the harness that calls those entry points directly:
  hsad_lstm_forward_fused                                     -> lstm_fused_fwd_kernel<KB>
  hsad_lstm_forward_chunk_multi / _chunk / _layer_forward      -> lstm_seq_fwd_kernel<KB>, lstm_step_small_kernel<KB>, lstm_step_kernel<128, 1>
  hsad_lstm_cell_fused / _pair                                 -> lstm_cell_gemm_kernel, lstm_cell_gemm256_kernel, gemm8_kernel<G8_CELL[_NOSTATE]>

The reference (plain torch in fp64, no project kernel).  One layer, one step, nn.LSTM's row order (row gate * H + unit, gates i f g o):

    p = pre + x W_ih^T + h_prev W_hh^T          bf16 operand values, summed in fp64; pre = the bias, or the fp32 projection the
                                                row-major entry points take in `gates`
    i, f, o = sigmoid(p_i, p_f, p_o);  g = tanh(p_g);  c = f c_prev + i g;  h = o tanh(c)

and next to it the same expressions on absolute values: Mp = |pre| + |x| |W_ih|^T + |h_prev| |W_hh|^T, Mc = |f c_prev| + |i g|.
The three column orders of the entry points are permutations of that row order: gate-blocked (r2d2.gate_block_perm; to_blocked /
from_blocked), gate16 (r2d2.gate16_perm, row 64 ub + 16 gate + u; gate16_row inverts it), and the fragment-major saved activations of
hsad_lstm_forward_fused, for which the packers of tests/lstm_bptt_ref.py are used as they are (unpack_with inverts a packer by packing
an index vector).

TEACHER FORCING.  The reference of step t reads h_{t-1} from the kernel's OWN bf16 hseq16, c_{t-1} from the kernel's own fp32 cseq, and a
stacked layer reads x_t from the kernel's own hseq16 of the layer below.  Every step of every layer is then an independent one-step
problem and an error belongs to the step and layer that made it.

THE BOUND, per element.  u = 2^-24 is half an ulp of fp32 (one rounding to nearest), U = 2^-23 = one ulp (v_exp_f32, v_rcp_f32:
1 ulp each, csrc/r2d2/lstm_cell.inc).  All terms are evaluated on the reference's values.
* accumulation:  A = (K + 2) U Mp on a pre-activation; K = the number of products (H, 2H, Kx + H), + 2 for adding `pre` and joining
  two partial sums.  A sum of n terms in any order is within n u sum|term|; U with the MFMA's internal order unknown.
* exponent:  e^x is formed as 2^(x log2 e): the product is rounded (u |x| log2 e in the exponent), the constant log2 e is an fp32 number
  (another u |x| log2 e), the instruction has 1 ulp:  relative error of e^x  eps(x) = (|x| + 1) U.
* activation, sigmoidf_ = rcp(1 + e^-x):  E_s = A / 4 + s (1 - s) eps(x) + 1.5 U s + FLOOR.  (slope of sigmoid <= 1/4 times the
  accumulation term; d s / d e * e = s (1 - s); the sum 1 + e is rounded (u) and rcp has 1 ulp (U), both relative to s.)
  tanhf_ = 1 - 2 rcp(1 + e^2x):  E_t = A + (1 - t^2) / 2 * eps(2x) + 1.5 U (1 - t) + u |t| + FLOOR  (slope 1; d t / d e * e = (1 - t^2) / 2;
  sum and rcp relative to 2 / (1 + e) = 1 - t; the final subtraction u |t|).  FLOOR = 2^-126: an fp32 result below the smallest normal
  number may be flushed to 0 (sigmoid(-100) = 3.7e-44 comes out as 0 when __expf overflows to inf).
* cell, plain kernels (c = gf * c_prev + gi * gg, three roundings):  E_c = |c_prev| E_f + |g| E_i + |i| E_g + E_i E_g + 2 U (Mc + those).
* clamped two-reciprocal cell (lstm_cell_shared_rcp_x2), c = (c_prev dig + (eg - 1) df) rcp(df dig), dig = (1 + ei)(1 + eg), df = 1 + ef:
  - the clamps: |sigmoid(x) - sigmoid(clamp(x, +-25))| <= e^-25 where |x| > 25, |tanh(x) - tanh(clamp(x, +-12.5))| <= 2 e^-25 where
    |x| > 12.5, else 0; eps uses the clamped argument (|x| <= 25);
  - the gates never exist on their own; their errors through the e's are E_s = A / 4 + s (1 - s) eps + clamp, E_t = A + (1 - t^2) / 2 eps + clamp
    and enter c as above (the formula is exactly f c_prev + i g in exact arithmetic on the same e's);
  - roundings of the formula: dig 3, c_prev dig 1 more; eg - 1, df, their product: 3; the sum 1 -- the numerator is within
    5 u (|c_prev dig| + |(eg - 1) df|), and (|c_prev dig| + |(eg - 1) df|) / (df dig) = |f c_prev| + |i g| = Mc: the cancellation of the two
    products is relative to Mc, not to c.  Denominator 5 roundings, rcp 1 ulp = 2 u, final product 1: 8 u |c|.  Together 13 u Mc <= 7 U Mc.
    E_c = |c_prev| E_f + |g| E_i + |i| E_g + E_i E_g + 7 U (Mc + those).
  - h = (ec - 1) rcp((1 + eo)(ec + 1)), ec = e^(2 clamp(c, +-12.5)):  tanh part E_tc = E_c + (1 - tc^2) / 2 eps(2c) + [|c| > 12.5] 2 e^-25,
    roundings ec - 1, 1 + eo, ec + 1, product, rcp (2 u), product: 7 u |h| <= 4 U |h|.
* propagation to h = o tanh(c) (product rule on the magnitudes):  E_tc = E_c + the activation terms of tanh at c (A = 0);
  E_h32 = |tc| E_o + |o| E_tc + E_o E_tc + R U (|h| + those), R = 1 (one product) for the plain kernels, 4 for the clamped cell.
* bf16 outputs:  E_h16 = E_h32 + 2^-8 (|h| + E_h32): one rounding to an 8-bit significand, as in the BPTT bound.
Where the bound is 0 the result must be a zero (worst_ratio of tests/lstm_bptt_ref.py).

Canaries: every output is longer than what the launch may write and pre-filled with POISON16 / POISON32; tails, outputs that were not
given, rows >= Bn of the hand-off tiles and every input are compared bitwise after the launch; a payload element nobody wrote stays NaN."""
import ctypes as C
import math

import torch

from hanabi_sad_amd import _lib, r2d2
from tests.lstm_bptt_ref import (DEV, POISON16, POISON32, TAIL, U23, _bits, _poison16, _poison32, bf16_round, bf16_values, f32_values,
                                 pack_saved_c, pack_saved_gates, worst_ratio)

U24 = 2.0 ** -24
FLOOR = 2.0 ** -126
E25 = math.exp(-25.0)
LOG2E_F32 = 1.4426950408889634


# ---------------------------------------------------------------------------------------------------
# column orders
# ---------------------------------------------------------------------------------------------------
def to_blocked(nat, H):
    """[.., 4H] nn.LSTM order -> gate-blocked columns (nb * 128 + gate * 32 + u)"""
    return nat[..., r2d2.gate_block_perm(H, "cpu")]


def from_blocked(blk, H):
    out = torch.empty_like(blk)
    out[..., r2d2.gate_block_perm(H, "cpu")] = blk
    return out


def to_gate16(nat, H):
    """[4H, ..] nn.LSTM row order -> gate16 rows (64 ub + 16 gate + u)"""
    return nat[r2d2.gate16_perm(H, "cpu")]


def gate16_row(gate, unit):
    """the gate16 row of (gate, hidden unit): the inverse of r2d2.gate16_perm, written from the header's sentence"""
    return 64 * (unit // 16) + 16 * gate + unit % 16


def unpack_with(packer, flat, T, Bn, W):
    """inverse of a packer of tests/lstm_bptt_ref.py (pack_saved_gates: W = 4H, pack_saved_c: W = H): packed[k] = rows[idx[k]]"""
    H = W // 4 if packer is pack_saved_gates else W
    idx = packer(torch.arange(T * Bn * W, dtype=torch.int64).reshape(T, Bn, W), T, Bn, H).reshape(-1)
    out = torch.empty(T * Bn * W, dtype=flat.dtype)
    out[idx] = flat.reshape(-1)
    return out.reshape(T, Bn, W)


# ---------------------------------------------------------------------------------------------------
# the reference and the bound
# ---------------------------------------------------------------------------------------------------
def step64(pre, x, Wih, h_prev, Whh, c_prev):
    """one layer, one step (or any number of independent ones: leading dimensions are free), everything fp64, nn.LSTM order.
    pre [.., 4H] or [4H]; x [.., Kx] / Wih [4H, Kx] (both None: no input product); h_prev [.., H]; Whh [4H, H]; c_prev [.., H]."""
    p = pre + h_prev @ Whh.T
    Mp = pre.abs() + h_prev.abs() @ Whh.abs().T
    K = Whh.shape[1]
    if x is not None:
        p = p + x @ Wih.T
        Mp = Mp + x.abs() @ Wih.abs().T
        K += Wih.shape[1]
    pi, pf, pg, po = p.chunk(4, dim=-1)
    i, f, g, o = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
    c = f * c_prev + i * g
    return dict(p=p, Mp=Mp, K=K, i=i, f=f, g=g, o=o, c=c, Mc=(f * c_prev).abs() + (i * g).abs(), h=o * torch.tanh(c), c_prev=c_prev)


def _eps(x, lim=None):
    x = x.abs()
    return ((x.clamp_max(lim) if lim is not None else x) + 1.0) * U23


def _sig_err(A, s, x, clamped):
    if clamped:
        return A / 4 + s * (1 - s) * _eps(x, 25.0) + (x.abs() > 25.0).double() * E25
    return A / 4 + s * (1 - s) * _eps(x) + 1.5 * U23 * s + FLOOR


def _tanh_err(A, t, x, clamped):
    if clamped:
        return A + (1 - t * t) / 2 * _eps(2 * x, 25.0) + (x.abs() > 12.5).double() * 2 * E25
    return A + (1 - t * t) / 2 * _eps(2 * x) + 1.5 * U23 * (1 - t) + U24 * t.abs() + FLOOR


def bounds(r, clamped=False):
    """the module docstring's bound for a step64 result -> dict(i, f, g, o: activated gates (plain kernels), c, h32, h16)"""
    A = (r["K"] + 2) * U23 * r["Mp"]
    Ai, Af, Ag, Ao = A.chunk(4, dim=-1)
    pi, pf, pg, po = r["p"].chunk(4, dim=-1)
    Ei, Ef, Eo = (_sig_err(a, s, x, clamped) for a, s, x in ((Ai, r["i"], pi), (Af, r["f"], pf), (Ao, r["o"], po)))
    Eg = _tanh_err(Ag, r["g"], pg, clamped)
    first = r["c_prev"].abs() * Ef + r["g"].abs() * Ei + r["i"].abs() * Eg + Ei * Eg
    Ec = first + (7 if clamped else 2) * U23 * (r["Mc"] + first)
    tc = torch.tanh(r["c"])
    Etc = _tanh_err(Ec, tc, r["c"], clamped)
    firsth = tc.abs() * Eo + r["o"].abs() * Etc + Eo * Etc
    Eh32 = firsth + (4 if clamped else 1) * U23 * (r["h"].abs() + firsth)
    return dict(i=Ei, f=Ef, g=Eg, o=Eo, c=Ec, h32=Eh32, h16=Eh32 + 2.0 ** -8 * (r["h"].abs() + Eh32))


def gates_nat(r):
    return torch.cat([r["i"], r["f"], r["g"], r["o"]], dim=-1)


def gate_bounds_nat(b):
    return torch.cat([b["i"], b["f"], b["g"], b["o"]], dim=-1)


def ratio_into(ratios, key, got, ref, bnd):
    v = worst_ratio(got, ref, bnd)
    if not torch.isfinite(got).all():
        v = float("inf")
    ratios[key] = max(ratios.get(key, 0.0), v)


# ---------------------------------------------------------------------------------------------------
# honest models: the kernels' arithmetic restated in fp32 on the CPU (tests/test_lstm_fwd_ref_cpu.py holds them to the bound)
# ---------------------------------------------------------------------------------------------------
def _f32(x):
    return x.to(torch.float32)


def expf_model(x):
    """__expf: v_exp_f32(x * log2 e)"""
    return torch.exp2(x * torch.tensor(LOG2E_F32, dtype=torch.float32))


def sigmoid_model(x):
    return 1.0 / (1.0 + expf_model(-x))


def tanh_model(x):
    return 1.0 - 2.0 * (1.0 / (1.0 + expf_model(2.0 * x)))


def preact_model(pre, x, Wih, h_prev, Whh):
    """fp32 matmuls on the bf16 operand values: the input product starts from `pre` (the fused kernels' accumulators start at the bias)
    and the recurrent product is added to it; the row-major kernels add `pre` to the finished recurrent product."""
    hp = _f32(h_prev) @ _f32(Whh).T
    if x is None:
        return hp + _f32(pre)
    xp = _f32(pre) + _f32(x) @ _f32(Wih).T
    return xp + hp


def plain_model(p32, c_prev):
    """lstm_fused_fwd_kernel, lstm_seq_fwd_kernel, lstm_step[_small]_kernel -> gates [.., 4H] nn.LSTM order, c, h32, h16 bits as values"""
    pi, pf, pg, po = p32.chunk(4, dim=-1)
    gi, gf, gg, go = sigmoid_model(pi), sigmoid_model(pf), tanh_model(pg), sigmoid_model(po)
    c = gf * _f32(c_prev) + gi * gg
    h = go * tanh_model(c)
    return dict(gates=torch.cat([gi, gf, gg, go], dim=-1), c=c, h32=h, h16=h.to(torch.bfloat16))


def clamped_model(p32, c_prev):
    """lstm_cell_shared_rcp_x2 -> c, h32, h16"""
    kL = torch.tensor(LOG2E_F32, dtype=torch.float32)

    def e2(x, lim, scale):
        return torch.exp2(x.clamp(-lim, lim) * scale)
    pi, pf, pg, po = p32.chunk(4, dim=-1)
    ei, ef, eg, eo = e2(pi, 25.0, -kL), e2(pf, 25.0, -kL), e2(pg, 12.5, 2.0 * kL), e2(po, 25.0, -kL)
    dig, df = (1.0 + ei) * (1.0 + eg), 1.0 + ef
    c = (_f32(c_prev) * dig + (eg - 1.0) * df) * (1.0 / (df * dig))
    ec = e2(c, 12.5, 2.0 * kL)
    h = (ec - 1.0) * (1.0 / ((1.0 + eo) * (ec + 1.0)))
    return dict(c=c, h32=h, h16=h.to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------
# inputs (CPU tensors, nn.LSTM row order; a test may edit them before the launch)
# ---------------------------------------------------------------------------------------------------
# (gate, unit, value): pre-activations of +-30 / +-100 drive __expf to inf / 0 and the clamped cell into its clamps at 25 and 12.5
EDGE_BIAS = ((0, 1, 30.0), (0, 2, -30.0), (1, 3, 100.0), (1, 4, -100.0), (2, 5, 30.0), (2, 6, -30.0), (3, 7, 100.0), (3, 8, -100.0),
             (2, 9, 100.0), (2, 10, -100.0), (0, 11, -100.0), (1, 12, -30.0), (3, 13, 30.0), (0, 14, 100.0), (2, 15, 13.0), (1, 16, 26.0))
EDGE_C = ((0, 0, 20.0), (0, 1, -20.0), (0, 2, 1e4), (0, 3, -1e4), (0, 5, 20.0), (0, 6, -1e4), (0, 9, 13.0), (0, 12, 1e4), (0, 17, -13.0))
EDGE_ZERO_ROW, EDGE_NEG0_ROW = 2, 1          # a row of all-zero x and h; a row whose c_prev is -0.0


def _gen(seed):
    return torch.Generator().manual_seed(7000 + seed)


def _rn(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float32)


def make_c_prev(g, Bn, H):
    """|c| in [0, 3], both signs"""
    return (torch.rand(Bn, H, generator=g) * 6.0 - 3.0).to(torch.float32)


def edge_bias(bias, H):
    for gate, u, v in EDGE_BIAS:
        bias[..., gate * H + u] = v
    return bias


def edge_c(c_prev):
    Bn = c_prev.shape[0]
    for r, u, v in EDGE_C:
        c_prev[min(r, Bn - 1), u] = v
    if Bn > EDGE_NEG0_ROW:
        c_prev[EDGE_NEG0_ROW] = -0.0
    return c_prev


def make_fused_inputs(T, Bn, H, nnet, nlayer, seed=0, edge=False):
    """per net: x16 [T, Bn, H] ~ 0.5 randn, per layer Wih, Whh [4H, H] randn / sqrt(2H) (K = 2H products), bias 0.1 randn"""
    g = _gen(seed)
    nets = []
    for _ in range(nnet):
        x = (0.5 * _rn(g, T, Bn, H)).to(torch.bfloat16)
        if edge:
            x[:, EDGE_ZERO_ROW] = 0
        layers = []
        for _ in range(nlayer):
            b = 0.1 * _rn(g, 4 * H)
            layers.append(dict(Wih=(_rn(g, 4 * H, H) / (2 * H) ** 0.5).to(torch.bfloat16), Whh=(_rn(g, 4 * H, H) / (2 * H) ** 0.5).to(torch.bfloat16),
                               bias=edge_bias(b, H) if edge else b))
        nets.append(dict(x=x, layers=layers))
    return nets


def make_seq_inputs(T, Bn, H, nrec, seed=0, edge=False, c_prev=True):
    """per record: pre [T, Bn, 4H] = 0.1 randn bias + a projection of 0.5 randn inputs by randn / sqrt(H) weights, in fp32 (what the
    projection GEMM leaves in `gates`); Whh randn / sqrt(H) bf16; h_prev ~ 0.5 randn (fp32, and its bf16 cast); c_prev or None"""
    g = _gen(100 + seed)
    recs = []
    for _ in range(nrec):
        bias = 0.1 * _rn(g, 4 * H)
        if edge:
            edge_bias(bias, H)
        pre = bias + (0.5 * _rn(g, T, Bn, 64)).to(torch.bfloat16).float() @ (_rn(g, 4 * H, 64) / 8.0).to(torch.bfloat16).float().T
        h0 = (0.5 * _rn(g, Bn, H)).to(torch.bfloat16).float()          # (exactly representable: the cast kernel cannot round it)
        c = make_c_prev(g, Bn, H) if c_prev else None
        if edge:
            if Bn > EDGE_ZERO_ROW:
                h0[EDGE_ZERO_ROW] = 0
            if c is not None:
                edge_c(c)
        recs.append(dict(pre=pre.contiguous(), Whh=(_rn(g, 4 * H, H) / H ** 0.5).to(torch.bfloat16), h0=h0, c_prev=c))
    return recs


def make_cell_inputs(Bn, H, Kx, ldx=None, seed=0, edge=False):
    """x [Bn, ldx] ~ 0.5 randn bf16 with NaN in the padding columns, h_prev ~ 0.5 randn bf16, Wcat [4H, Kx + H] randn / sqrt(Kx + H),
    bias 0.1 randn, c_prev |c| in [0, 3]"""
    g = _gen(200 + seed)
    ldx = Kx if ldx is None else ldx
    x = torch.full((Bn, ldx), float("nan"), dtype=torch.bfloat16)
    x[:, :Kx] = (0.5 * _rn(g, Bn, Kx)).to(torch.bfloat16)
    h = (0.5 * _rn(g, Bn, H)).to(torch.bfloat16)
    bias = 0.1 * _rn(g, 4 * H)
    c = make_c_prev(g, Bn, H)
    if edge:
        edge_bias(bias, H)
        edge_c(c)
        if Bn > EDGE_ZERO_ROW:
            x[EDGE_ZERO_ROW, :Kx] = 0
            h[EDGE_ZERO_ROW] = 0
    return dict(x=x, h_prev=h, Wcat=(_rn(g, 4 * H, Kx + H) / (Kx + H) ** 0.5).to(torch.bfloat16), bias=bias, c_prev=c, Kx=Kx, ldx=ldx)


# ---------------------------------------------------------------------------------------------------
# harness plumbing
# ---------------------------------------------------------------------------------------------------
class _Kept:
    """bit copies of the inputs of a launch"""

    def __init__(self):
        self.items = []

    def add(self, name, t):
        self.items.append((name, t, _bits(t).clone()))
        return t

    def assert_unchanged(self, tag):
        for name, t, before in self.items:
            assert torch.equal(_bits(t), before), "%s: the launch changed its input %s" % (tag, name)


def _clean(x, poison, what):
    assert bool((x == poison).all()), what + " was written"


def _written(x, poison, what):
    assert not bool((x == poison).any()), what + ": a payload element was never written"


def _ptr(t, offset_bytes=0):
    return None if t is None else t.data_ptr() + offset_bytes


# ---------------------------------------------------------------------------------------------------
# the harness: hsad_lstm_forward_fused
# ---------------------------------------------------------------------------------------------------
class FusedFwd:
    def __init__(self, T, Bn, H, nets):
        self.T, self.Bn, self.H, self.nets = T, Bn, H, nets
        self.nnet, self.nlayer = len(nets), len(nets[0]["layers"])
        self.lib = _lib.load_library()
        self.kept = _Kept()
        self.dev = []
        for q, net in enumerate(nets):
            x = self.kept.add("x16", net["x"].contiguous().to(DEV))
            row = []
            for l, d in enumerate(net["layers"]):
                b = dict(x=x if l == 0 else None)
                for name in ("Wih", "Whh"):
                    b[name] = self.kept.add(name, to_blocked(d[name].T, H).T.contiguous().to(DEV))
                b["bias"] = self.kept.add("bias", to_blocked(d["bias"], H).contiguous().to(DEV))
                row.append(b)
            self.dev.append(row)
        self.tag = "fused T%d Bn%d H%d %dx%d" % (T, Bn, H, self.nnet, self.nlayer)

    def run(self, keep=True, hT=True, partner=False):
        """one launch into fresh, poisoned outputs -> per (net, layer) dict of CPU bit tensors; canaries asserted on the way"""
        T, Bn, H = self.T, self.Bn, self.H
        nrec, nrb = self.nnet * self.nlayer, Bn // 32
        n1, n4 = T * Bn * H, T * Bn * 4 * H
        words = nrec * nrb * (T + 2)
        sync = torch.zeros(words + 4, dtype=torch.int32, device=DEV)
        other = torch.full((words + 4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if partner else None
        recs = (_lib.LstmFusedRec * nrec)()
        outs = []
        for q in range(self.nnet):
            for l in range(self.nlayer):
                b, r = self.dev[q][l], recs[q * self.nlayer + l]
                o = dict(hseq=_poison16(n1 + TAIL), gates=_poison32(n4 + TAIL), cseq=_poison32(n1 + TAIL), hT=_poison32(Bn * H + TAIL))
                r.Wih_blocked, r.Whh_blocked, r.bias_blocked = b["Wih"].data_ptr(), b["Whh"].data_ptr(), b["bias"].data_ptr()
                r.x16 = _ptr(b["x"])
                r.gates, r.cseq = (o["gates"].data_ptr(), o["cseq"].data_ptr()) if keep else (None, None)
                r.hseq16, r.hT = o["hseq"].data_ptr(), o["hT"].data_ptr() if hT else None
                outs.append(o)
        _lib.check(self.lib.hsad_lstm_forward_fused(self.nnet, self.nlayer, T, Bn, H, C.byref(recs), sync.data_ptr(), _ptr(other), None))
        torch.cuda.synchronize()
        assert int(sync[words].item()) == 0, self.tag + ": the launch's sticky timeout word is set"
        if partner:
            o_ = other.cpu()
            assert bool((o_[:words] == 0).all()), self.tag + ": the ping-pong partner is not zero after the launch"
            assert bool((o_[words:] == 0x5A5A5A5A).all()), self.tag + ": the launch wrote behind the partner's counters"
        self.kept.assert_unchanged(self.tag)
        res = []
        for k, o in enumerate(outs):
            tag = "%s record %d" % (self.tag, k)
            c = {name: v.cpu() for name, v in o.items()}
            _clean(c["hseq"][n1:], POISON16, tag + " hseq16 past its end")
            _written(c["hseq"][:n1], POISON16, tag + " hseq16")
            for name, n, on in (("gates", n4, keep), ("cseq", n1, keep), ("hT", Bn * H, hT)):
                if on:
                    _clean(c[name][n:], POISON32, "%s %s past its end" % (tag, name))
                    _written(c[name][:n], POISON32, "%s %s" % (tag, name))
                else:
                    _clean(c[name], POISON32, "%s %s (not given)" % (tag, name))
            res.append(dict(hseq=c["hseq"][:n1].reshape(T, Bn, H), gates=c["gates"][:n4] if keep else None,
                            cseq=c["cseq"][:n1] if keep else None, hT=c["hT"][:Bn * H].reshape(Bn, H) if hT else None))
        return [res[q * self.nlayer:(q + 1) * self.nlayer] for q in range(self.nnet)]

    def check(self, out, kern="fused"):
        return check_fused(self.T, self.Bn, self.H, self.nets, out, kern, self.tag)


def check_fused(T, Bn, H, nets, out, kern="fused", tag=""):
    """outputs of a launch that kept gates / cseq (bit tensors as FusedFwd.run returns them) against the teacher-forced reference
    -> {output: worst err / bound}"""
    ratios = {}
    for q, net in enumerate(nets):
        for l, d in enumerate(net["layers"]):
            o = out[q][l]
            key = "%s %s" % (kern, "layer0" if l == 0 else "stacked")
            hseq = bf16_values(o["hseq"])
            x = net["x"].double() if l == 0 else bf16_values(out[q][l - 1]["hseq"])
            c_rows = unpack_with(pack_saved_c, f32_values(o["cseq"]), T, Bn, H)
            h_prev = torch.cat([torch.zeros(1, Bn, H, dtype=torch.float64), hseq[:-1]])
            c_prev = torch.cat([torch.zeros(1, Bn, H, dtype=torch.float64), c_rows[:-1]])
            r = step64(d["bias"].double(), x, d["Wih"].double(), h_prev, d["Whh"].double(), c_prev)
            b = bounds(r)
            ratio_into(ratios, key + " gates", f32_values(o["gates"]).reshape(T, Bn, 4 * H),
                       pack_saved_gates(to_blocked(gates_nat(r), H), T, Bn, H), pack_saved_gates(to_blocked(gate_bounds_nat(b), H), T, Bn, H))
            ratio_into(ratios, key + " cseq", f32_values(o["cseq"]).reshape(T, Bn, H), pack_saved_c(r["c"], T, Bn, H), pack_saved_c(b["c"], T, Bn, H))
            ratio_into(ratios, key + " hseq16", hseq, r["h"], b["h16"])
            if o["hT"] is not None:
                ratio_into(ratios, key + " hT", f32_values(o["hT"]), r["h"][-1], b["h32"][-1])
                assert torch.equal(_bits(f32_values(o["hT"]).float().to(torch.bfloat16)), o["hseq"][-1].reshape(-1)), \
                    "%s net %d layer %d: bf16(hT) is not the last hseq16 row" % (tag, q, l)
    return ratios


def same_bits(a, b, names):
    """per (net, layer): the named outputs of two launches hold the same bits"""
    for ra, rb in zip(a, b):
        for oa, ob in zip(ra, rb):
            for name in names:
                if oa[name] is not None and ob[name] is not None:
                    assert torch.equal(oa[name], ob[name]), "%s differs between two launches" % name


# ---------------------------------------------------------------------------------------------------
# the harness: hsad_lstm_forward_chunk_multi / hsad_lstm_forward_chunk / hsad_lstm_layer_forward (row-major, gate-blocked, any Bn)
# ---------------------------------------------------------------------------------------------------
def read_fwd_tiles(x, T, Bn, H):
    """hand-off tiles [T][ceil(Bn / 32)][H / 32][32 rows][32 units] -> [T, 32 ceil(Bn / 32), H]"""
    nrb = (Bn + 31) // 32
    return x[:T * nrb * 32 * H].reshape(T, nrb, H // 32, 32, 32).permute(0, 1, 3, 2, 4).reshape(T, nrb * 32, H)


class SeqFwd:
    """entry 'multi' | 'chunk' | 'layer' | 'steps' (hsad_lstm_layer_forward with sync_scratch NULL: one launch per step)"""

    def __init__(self, entry, T, Bn, H, recs, xchg=False, hT=True, h0=True, keep_gates=1):
        assert entry in ("multi", "chunk", "layer", "steps") and (entry == "multi" or len(recs) == 1)
        self.entry, self.T, self.Bn, self.H, self.recs = entry, T, Bn, H, recs
        self.xchg, self.hT, self.h0, self.keep_gates = xchg and entry == "multi", hT, h0, keep_gates
        self.lib = _lib.load_library()
        self.kept = _Kept()
        self.tag = "%s T%d Bn%d H%d x%d" % (entry, T, Bn, H, len(recs))
        n1, n4 = T * Bn * H, T * Bn * 4 * H
        self.nx = T * ((Bn + 31) // 32) * 32 * H
        self.dev = []
        for d in recs:
            b = dict(Whh=self.kept.add("Whh", to_blocked(d["Whh"].T, H).T.contiguous().to(DEV)))
            b["gates"] = torch.cat([_bits(to_blocked(d["pre"], H).contiguous()).to(DEV), _poison32(TAIL)])
            b["gates_in"] = b["gates"][:n4].clone()
            if entry in ("layer", "steps"):
                assert d["c_prev"] is not None
                b["h0"] = self.kept.add("h0", d["h0"].contiguous().to(DEV)) if h0 else None
                b["h16"] = _poison16(Bn * H + TAIL)          # h0_16_scratch: the launch's own bf16 cast of h0
            else:
                b["h16"] = self.kept.add("h_prev16", d["h0"].to(torch.bfloat16).contiguous().to(DEV))
            b["c_prev"] = self.kept.add("c_prev", d["c_prev"].contiguous().to(DEV)) if d["c_prev"] is not None else None
            b["hseq"], b["cseq"], b["hT"], b["xchg"] = _poison16(n1 + TAIL), _poison32(n1 + TAIL), _poison32(Bn * H + TAIL), _poison16(self.nx + TAIL)
            self.dev.append(b)

    def launch(self, t0=0, Tc=None):
        """steps [t0, t0 + Tc) of the sequence; t0 > 0 carries the state of step t0 - 1 (multi / chunk)"""
        T, Bn, H = self.T, self.Bn, self.H
        Tc = T if Tc is None else Tc
        nrec, nrb = len(self.dev), (Bn + 31) // 32
        words = nrec * nrb * (Tc + 2)
        sync = torch.zeros(words + 4, dtype=torch.int32, device=DEV)
        so1, so4 = t0 * Bn * H, t0 * Bn * 4 * H
        if self.entry in ("multi", "chunk"):
            recs = (_lib.LstmFwdRec * nrec)()
            for r, b in zip(recs, self.dev):
                r.gates, r.Whh_blocked = b["gates"].data_ptr() + so4 * 4, b["Whh"].data_ptr()
                r.h_prev16 = b["h16"].data_ptr() if t0 == 0 else b["hseq"].data_ptr() + (so1 - Bn * H) * 2
                r.c_prev = _ptr(b["c_prev"]) if t0 == 0 else b["cseq"].data_ptr() + (so1 - Bn * H) * 4
                r.hseq16, r.cseq = b["hseq"].data_ptr() + so1 * 2, b["cseq"].data_ptr() + so1 * 4
                r.hT = b["hT"].data_ptr() if self.hT else None
                r.xchg = b["xchg"].data_ptr() + (t0 * nrb * 32 * H) * 2 if self.xchg else None
            if self.entry == "multi":
                _lib.check(self.lib.hsad_lstm_forward_chunk_multi(nrec, Tc, Bn, H, C.byref(recs), sync.data_ptr(), None, None))
            else:
                r = recs[0]
                _lib.check(self.lib.hsad_lstm_forward_chunk(Tc, Bn, H, r.gates, r.Whh_blocked, r.h_prev16, r.c_prev, r.hseq16, r.cseq, r.hT,
                                                            sync.data_ptr(), None))
        else:
            assert t0 == 0 and Tc == T
            b = self.dev[0]
            _lib.check(self.lib.hsad_lstm_layer_forward(T, Bn, H, b["gates"].data_ptr(), b["Whh"].data_ptr(), _ptr(b["h0"]), b["c_prev"].data_ptr(),
                                                        b["hseq"].data_ptr(), b["cseq"].data_ptr(), b["h16"].data_ptr(),
                                                        b["hT"].data_ptr() if self.hT else None,
                                                        sync.data_ptr() if self.entry == "layer" else None, self.keep_gates, None))
        torch.cuda.synchronize()
        assert int(sync[words].item()) == 0, self.tag + ": the launch's sticky timeout word is set"

    def outputs(self):
        T, Bn, H = self.T, self.Bn, self.H
        n1, n4 = T * Bn * H, T * Bn * 4 * H
        self.kept.assert_unchanged(self.tag)
        res = []
        for k, b in enumerate(self.dev):
            tag = "%s record %d" % (self.tag, k)
            c = {name: b[name].cpu() for name in ("gates", "gates_in", "hseq", "cseq", "hT", "xchg", "h16")}
            _clean(c["gates"][n4:], POISON32, tag + " gates past its end")
            _clean(c["hseq"][n1:], POISON16, tag + " hseq16 past its end")
            _clean(c["cseq"][n1:], POISON32, tag + " cseq past its end")
            _written(c["hseq"][:n1], POISON16, tag + " hseq16")
            _written(c["cseq"][:n1], POISON32, tag + " cseq")
            if self.hT:
                _clean(c["hT"][Bn * H:], POISON32, tag + " hT past its end")
                _written(c["hT"][:Bn * H], POISON32, tag + " hT")
            else:
                _clean(c["hT"], POISON32, tag + " hT (not given)")
            o = dict(hseq=c["hseq"][:n1].reshape(T, Bn, H), cseq=c["cseq"][:n1].reshape(T, Bn, H), hT=c["hT"][:Bn * H].reshape(Bn, H) if self.hT else None)
            if self.keep_gates:
                o["gates"] = c["gates"][:n4].reshape(T, Bn, 4 * H)
            else:
                assert torch.equal(c["gates"][:n4], c["gates_in"]), tag + ": keep_gates = 0 changed `gates`"
                o["gates"] = None
            if self.xchg:
                tiles = read_fwd_tiles(c["xchg"], T, Bn, H)
                assert torch.equal(tiles[:, :Bn], o["hseq"]), tag + ": the hand-off tiles and hseq16 differ"
                _clean(tiles[:, Bn:], POISON16, tag + " rows >= Bn of the hand-off tiles")
                _clean(c["xchg"][self.nx:], POISON16, tag + " xchg past its end")
            else:
                _clean(c["xchg"], POISON16, tag + " xchg (not given)")
            if self.entry in ("layer", "steps"):
                _clean(c["h16"][Bn * H:], POISON16, tag + " h0_16_scratch past its end")
                want = self.recs[k]["h0"].to(torch.bfloat16) if self.h0 else torch.zeros(Bn, H, dtype=torch.bfloat16)
                assert torch.equal(c["h16"][:Bn * H], _bits(want)), tag + ": h0_16_scratch is not the bf16 cast of h0"
            res.append(o)
        return res

    def check(self, out, kern):
        return check_seq(self.T, self.Bn, self.H, self.recs, out, kern, self.h0 or self.entry in ("multi", "chunk"), self.tag)


def check_seq(T, Bn, H, recs, out, kern, h0_given=True, tag=""):
    """outputs of the row-major entry points (bit tensors as SeqFwd.outputs returns them) against the teacher-forced reference"""
    ratios = {}
    for d, o in zip(recs, out):
        hseq, cseq = bf16_values(o["hseq"]), f32_values(o["cseq"])
        h0 = bf16_round(d["h0"].double()) if h0_given else torch.zeros(Bn, H, dtype=torch.float64)
        c0 = d["c_prev"].double() if d["c_prev"] is not None else torch.zeros(Bn, H, dtype=torch.float64)
        r = step64(d["pre"].double(), None, None, torch.cat([h0[None], hseq[:-1]]), d["Whh"].double(), torch.cat([c0[None], cseq[:-1]]))
        b = bounds(r)
        if o["gates"] is not None:
            ratio_into(ratios, kern + " gates", from_blocked(f32_values(o["gates"]), H), gates_nat(r), gate_bounds_nat(b))
        ratio_into(ratios, kern + " cseq", cseq, r["c"], b["c"])
        ratio_into(ratios, kern + " hseq16", hseq, r["h"], b["h16"])
        if o["hT"] is not None:
            ratio_into(ratios, kern + " hT", f32_values(o["hT"]), r["h"][-1], b["h32"][-1])
            assert torch.equal(_bits(f32_values(o["hT"]).float().to(torch.bfloat16)), o["hseq"][-1].reshape(-1)), tag + ": bf16(hT) is not the last hseq16 row"
    return ratios


# ---------------------------------------------------------------------------------------------------
# the harness: hsad_lstm_cell_fused / hsad_lstm_cell_fused_pair (gate16 rows)
# ---------------------------------------------------------------------------------------------------
class CellProblem:
    """device buffers of one cell; outs: which of 'c', 'h32', 'h16' are given; alias: c_out == c_prev"""

    def __init__(self, Bn, H, d, outs=("c", "h32", "h16"), alias=False):
        self.Bn, self.H, self.d, self.outs, self.alias = Bn, H, d, tuple(outs), alias
        self.kept = _Kept()
        self.x = self.kept.add("x16", d["x"].contiguous().to(DEV))
        self.h = self.kept.add("h_prev16", d["h_prev"].contiguous().to(DEV))
        self.W = self.kept.add("Wcat", to_gate16(d["Wcat"], H).contiguous().to(DEV))
        self.bias = self.kept.add("bias", to_gate16(d["bias"], H).contiguous().to(DEV))
        n = Bn * H
        if alias:
            assert "c" in outs
            self.c_prev = self.c = torch.cat([_bits(d["c_prev"].contiguous()).to(DEV), _poison32(TAIL)])
        else:
            self.c_prev = self.kept.add("c_prev", d["c_prev"].contiguous().to(DEV))
            self.c = _poison32(n + TAIL)
        self.h32, self.h16 = _poison32(n + TAIL), _poison16(n + TAIL)

    def ptrs(self):
        return (self.x.data_ptr(), self.h.data_ptr(), self.W.data_ptr(), self.bias.data_ptr(), self.c_prev.data_ptr(),
                self.c.data_ptr() if "c" in self.outs else None, self.h32.data_ptr() if "h32" in self.outs else None,
                self.h16.data_ptr() if "h16" in self.outs else None)

    def check(self, tag, kern, ratios):
        Bn, H, d = self.Bn, self.H, self.d
        n, Kx = Bn * H, d["Kx"]
        self.kept.assert_unchanged(tag)
        r, b = cell_reference(d)
        for name, buf, poison, val, ref, bnd in (("c", self.c, POISON32, f32_values, r["c"], b["c"]), ("h32", self.h32, POISON32, f32_values, r["h"], b["h32"]),
                                                 ("h16", self.h16, POISON16, bf16_values, r["h"], b["h16"])):
            v = buf.cpu()
            if name in self.outs:
                _clean(v[n:], poison, "%s %s past its end" % (tag, name))
                _written(v[:n], poison, "%s %s" % (tag, name))
                ratio_into(ratios, "%s %s" % (kern, name), val(v[:n]).reshape(Bn, H), ref, bnd)
            else:
                _clean(v, poison, "%s %s (not given)" % (tag, name))
        if "h32" in self.outs and "h16" in self.outs:
            assert torch.equal(_bits(self.h32[:n].view(torch.float32).to(torch.bfloat16)).cpu(), self.h16[:n].cpu()), tag + ": h_out16 is not bf16(h_out32)"


def cell_reference(d):
    """-> the step64 result and the clamped cell's bounds of a make_cell_inputs dict"""
    Kx = d["Kx"]
    r = step64(d["bias"].double(), d["x"][:, :Kx].double(), d["Wcat"][:, :Kx].double(), d["h_prev"].double(), d["Wcat"][:, Kx:].double(),
               d["c_prev"].double())
    return r, bounds(r, clamped=True)


def run_cell(P, variant=None):
    """hsad_lstm_cell_fused on one CellProblem; variant = (tile, pp) forced for the launch and restored to (0, 1)"""
    lib = _lib.load_library()
    d = P.d
    x, h, W, bias, cp, c, h32, h16 = P.ptrs()
    try:
        if variant is not None:
            _lib.check(lib.hsad_lstm_cell_set_variant(*variant))
        _lib.check(lib.hsad_lstm_cell_fused(P.Bn, P.H, d["Kx"], x, d["ldx"], h, W, bias, cp, c, h32, h16, None))
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.hsad_lstm_cell_set_variant(0, 1))


def run_cell_pair(Pa, Pb, variant=None):
    lib = _lib.load_library()
    a, b = Pa.ptrs(), Pb.ptrs()
    args = [v for pair in zip(a, b) for v in pair]
    try:
        if variant is not None:
            _lib.check(lib.hsad_lstm_cell_set_variant(*variant))
        _lib.check(lib.hsad_lstm_cell_fused_pair(Pa.Bn, Pa.H, Pa.d["Kx"], Pa.d["ldx"], *args, None))
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.hsad_lstm_cell_set_variant(0, 1))
