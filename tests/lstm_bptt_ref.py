"""Helper (not a test) of tests/test_lstm_bptt_ref_cpu.py and tests/test_lstm_bptt_kernels_gpu.py: a step-by-step fp64 reference of the
persistent BPTT launches of include/hsad.h (hsad_lstm_backward_fused -> lstm_fused_bwd_kernel<KB> / lstm_bptt_wide_kernel,
hsad_lstm_backward_chunk_multi, hsad_lstm_layer_backward) and the harness that calls those entry points directly.

The reference (plain torch in fp64, no project kernel).  One layer, one step, gate-blocked columns (r2d2.gate_block_perm):

    dh  = dO_t + dGnext16 WhhT^T [+ dGabove16_t WihT_above^T]          bf16 operands, summed in fp64
    tc  = tanh(c_t);  dct = dc + dh o (1 - tc^2);  dc <- dct f
    dG  = [dct g i (1 - i), dct c_{t-1} f (1 - f), dct i (1 - g^2), dh tc o (1 - o)]

and, next to it, the same expressions on absolute values: the magnitude M of the bound.

TEACHER FORCING.  The kernels publish every intermediate a later step or stage consumes as bf16 (fp32 for dO_stage).  The reference of
step t takes dGnext16 from the kernel's OWN output of step t + 1 (dG16, dGT16 or the hand-off tile -- they are asserted to hold the
same bits), the lower layer's dO from the kernel's own dO_stage, the sink from the kernel's own lower-layer dG.  Only the fp32 dc chain
is carried by the reference itself.  An error then belongs to the step and stage that made it.

THE BOUND, per element and step:  |got - ref| <= 2^-8 |ref| + (4H P + 16 T) 2^-23 M.
* 2^-8 |ref|: the one bf16 rounding of the result.  Half an ulp of an 8-bit significand is 2^-9 of the value at the top of a binade and
  2^-8 at its bottom, so across a binade 2^-9 of this term is slack and just above a power of two none is: the observed worst ratios of
  dG sit at 0.96-0.97 for that reason, in every kernel alike.
* (4H P + 16 T) 2^-23 M carries everything fp32: the accumulation of the P products of length 4H that enter dh (P = 1; P = 2 for a
  lower layer that computes the layer above's W_ih product inside its own recurrence: a sum of n terms in any order is within
  n 2^-24 sum|term|, 2^-23 with the MFMA's internal order unknown); 16 roundings per step along the dc chain, which the kernel carries in
  fp32 over T steps; the product chain of a gate (<= 6 roundings); and tanhf_ = 1 - 2 rcp(1 + exp(2c)): a few 2^-24 absolute in tc, which
  for |c| in [0.25, 3] is below 2^-13 relative in tc and in 1 - tc^2 -- against (4H + 16 T) 2^-23 >= 2^-13 at H = 256.
* dO_stage is fp32: the second term alone.  Bias sums: n_terms 2^-23 sum|term| (any order: the 32 x 32 kernel adds with float atomics).
Where the bound is 0 (an exact zero of M) the result must be a zero.

Canaries: every output buffer is longer than what the launch may write and pre-filled with a NaN bit pattern; the tail, the padding
columns of the transposed outputs and every input are compared bitwise after the launch; a payload element nobody wrote stays NaN."""
import ctypes as C

import numpy as np
import torch

from hanabi_sad_amd import _lib

DEV = "cuda:0"
POISON16 = 0x7FA5            # a bf16 NaN
POISON32 = 0x7FC00A5A        # an fp32 NaN
TAIL = 64                    # canary elements behind every vector
U23 = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------
def bf16_round(x):
    """fp64 -> the nearest bf16 (through fp32) -> fp64"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def split_gates(g, H):
    """[.., 4H] gate-blocked (column nb * 128 + gate * 32 + u) -> i, f, g, o as [.., H]"""
    v = g.reshape(*g.shape[:-1], H // 32, 4, 32)
    return [v[..., k, :].reshape(*g.shape[:-1], H) for k in range(4)]


def join_gates(parts, H):
    v = torch.stack([p.reshape(*p.shape[:-1], H // 32, 32) for p in parts], dim=-2)
    return v.reshape(*parts[0].shape[:-1], 4 * H)


def cell_backward64(dO, dGnext, WhhT, gates, c, c_prev, dc, dc_abs, above=None):
    """One layer, one step, everything fp64.  dO [Bn, H]; dGnext [Bn, 4H] (the values of the bf16 gradient of step t + 1); WhhT [H, 4H];
    gates [Bn, 4H] activated, gate-blocked; c, c_prev, dc, dc_abs [Bn, H]; above = (dG of the layer above at this step [Bn, 4H],
    WihT_above [H, 4H]) for a layer that forms that product inside its recurrence.  -> dG, M [Bn, 4H], dc, dc_abs (after the step)."""
    H = c.shape[-1]
    dh = dO + dGnext @ WhhT.T
    dh_abs = dO.abs() + dGnext.abs() @ WhhT.abs().T
    if above is not None:
        dh = dh + above[0] @ above[1].T
        dh_abs = dh_abs + above[0].abs() @ above[1].abs().T
    i, f, g, o = split_gates(gates, H)
    tc = torch.tanh(c)
    dct = dc + dh * o * (1 - tc * tc)
    dct_abs = dc_abs + dh_abs * o.abs() * (1 - tc * tc).abs()
    dG = join_gates([dct * g * i * (1 - i), dct * c_prev * f * (1 - f), dct * i * (1 - g * g), dh * tc * o * (1 - o)], H)
    M = join_gates([dct_abs * g.abs() * i.abs() * (1 - i).abs(), dct_abs * c_prev.abs() * f.abs() * (1 - f).abs(),
                    dct_abs * i.abs() * (1 - g * g).abs(), dh_abs * tc.abs() * o.abs() * (1 - o).abs()], H)
    return dG, M, dct * f, dct_abs * f.abs()


def layer_reference(forced, dO, WhhT, gates, c, c_before, dc0, above=None, tail=None):
    """A layer over T steps.  forced [T, Bn, 4H]: the gradient the recurrent term of step t reads at slot t + 1 (teacher forcing: the
    kernel's own bf16 output as fp64; free running: None -- the reference's own, unrounded); tail [Bn, 4H] = slot T (has_next) or None =
    zeros; dO [T, Bn, H] or None; above = (dG of the layer above [T, Bn, 4H], WihT_above).  -> ref, M [T, Bn, 4H], dc, dc_abs [Bn, H]."""
    T, Bn, H = c.shape
    ref = torch.zeros(T, Bn, 4 * H, dtype=torch.float64)
    M = torch.zeros_like(ref)
    dc, dc_abs = dc0.clone(), dc0.abs()
    zero = torch.zeros(Bn, H, dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            nxt = tail if tail is not None else torch.zeros(Bn, 4 * H, dtype=torch.float64)
        else:
            nxt = forced[t + 1] if forced is not None else ref[t + 1]
        cp = c[t - 1] if t > 0 else (c_before if c_before is not None else zero)
        ab = (above[0][t], above[1]) if above is not None else None
        ref[t], M[t], dc, dc_abs = cell_backward64(dO[t] if dO is not None else zero, nxt, WhhT, gates[t], c[t], cp, dc, dc_abs, ab)
    return ref, M, dc, dc_abs


def product_reference(dG, WT):
    """dG [.., 4H] x WT [H, 4H]^T in fp64 with its magnitude: a projection stage's dO, the sink's d x before rounding"""
    return dG @ WT.T, dG.abs() @ WT.abs().T


def bound(ref, M, H, T, products=1, rounded=True):
    return (2.0 ** -8 * ref.abs() if rounded else 0.0) + (4 * H * products + 16 * T) * U23 * M


def dc_bound(dc_abs, H, T, products=1):
    """the carried dc is fp32 and never rounded to bf16: no 2^-8 |ref| term.  2^-13 of the terms' magnitude for tanhf_'s relative error
    in 1 - tc^2 (the module docstring) next to the accumulation term on the same magnitude, which also holds the product chains"""
    return (2.0 ** -13 + (4 * H * products + 16 * T) * U23) * dc_abs


def worst_ratio(got, ref, bnd):
    """max of |got - ref| / bound; where the bound is 0 the result must be a zero (ratio 0, else inf); NaN anywhere -> inf"""
    err = (got - ref).abs()
    if torch.isnan(err).any():
        return float("inf")
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


# ---------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------
def pack_saved_gates(g, T, Bn, H):
    """[T, Bn, 4H] gate-blocked -> the fragment-major order of hsad_lstm_forward_fused (inverse of r2d2.unpack_saved_gates)"""
    v = g.reshape(T, Bn // 32, 2, 4, 4, H // 32, 4, 4, 8)        # t rb half lq r | nb j wave u8
    return v.permute(0, 1, 5, 7, 4, 3, 2, 8, 6).reshape(T, Bn, 4 * H).contiguous()   # t rb nb wave r lq half u8 j


def pack_saved_c(c, T, Bn, H):
    """[T, Bn, H] -> fragment-major (inverse of r2d2.unpack_saved_c); T = 1 packs c_before"""
    v = c.reshape(T, Bn // 32, 2, 4, 4, H // 32, 4, 8)           # t rb half lq r | nb wave u8
    return v.permute(0, 1, 5, 6, 3, 2, 7, 4).reshape(T, Bn, H).contiguous()          # t rb nb wave lq half u8 r


def read_tiles(x, T, Bn, H, rows):
    """hand-off tiles [T][Bn / rows][4H / 32 k blocks][rows][32 gate columns] (rows = 32: lstm_fused_bwd_kernel, lstm_seq_bwd_kernel;
    16: lstm_bptt_wide_kernel) -> [T, Bn, 4H]"""
    return x[:T * Bn * 4 * H].reshape(T, Bn // rows, 4 * H // 32, rows, 32).permute(0, 1, 3, 2, 4).reshape(T, Bn, 4 * H)


def write_tiles_like_the_kernel(dG, T, Bn, H, rows):
    """the tile buffer as the kernels' store loops fill it (lstm_fused_bwd.inc 'hand-off copy', lstm_bptt_wide.inc 'hand-off copy'),
    index formula for index formula: thread tid, trip it -> 8-byte piece c = tid + 256 it of the workgroup's 8 KB"""
    KB = 4 * H // 32
    nrb = Bn // rows
    out = np.full(T * Bn * 4 * H, -1, dtype=np.int64)
    src = dG.reshape(T, Bn, 4 * H)
    tid, it, e = np.meshgrid(np.arange(256), np.arange(4), np.arange(4), indexing="ij")
    c = tid + it * 256
    for t in range(T):
        for rb in range(nrb):
            if rows == 32:
                for nb in range(H // 32):
                    r, qq = (c >> 3) & 31, c & 7
                    dst = ((t * nrb + rb) * KB + 4 * nb) * 1024 + c * 4 + e
                    out[dst] = src[t, rb * 32 + r, nb * 128 + it * 32 + qq * 4 + e]
            else:
                for nb in range(H // 64):
                    sl, r, qq = c >> 7, (c >> 3) & 15, c & 7
                    dst = ((t * nrb + rb) * KB + 8 * nb) * 512 + c * 4 + e
                    out[dst] = src[t, rb * 16 + r, nb * 256 + sl * 32 + qq * 4 + e]
    return out


def read_transposed(xT, ld, T, Bn, ncol):
    """[ncol][ld] with element (column, t * Bn + row) -> [T, Bn, ncol]"""
    return xT[:ncol * ld].reshape(ncol, ld)[:, :T * Bn].T.reshape(T, Bn, ncol)


# ---------------------------------------------------------------------------------------------------
# inputs (CPU tensors; a test may edit them before the launch)
# ---------------------------------------------------------------------------------------------------
class Spec:
    def __init__(self, T, Bn, H, nnet=1, nlayer=2, mode="plain", dgt=False, frag=True, wide=False, sink_T=False, bias1=True,
                 colmap_perm=False, c_before=False, mask=True, seed=0):
        assert mode in ("plain", "split", "proj", "sink")
        self.T, self.Bn, self.H, self.nnet, self.nlayer = T, Bn, H, nnet, nlayer
        self.split, self.proj, self.sink = mode != "plain", mode in ("proj", "sink"), mode == "sink"
        self.dgt, self.frag, self.wide, self.sink_T, self.bias1, self.colmap_perm = dgt, frag, wide, sink_T, bias1, colmap_perm
        self.c_before, self.mask, self.seed, self.mode = c_before, mask, seed, mode

    def __repr__(self):
        return "Spec(%s)" % ", ".join("%s=%r" % kv for kv in sorted(vars(self).items()))


def make_layer_inputs(g, T, Bn, H, with_dO, with_above, with_sink, c_before, mask):
    """i, f, o in (0.02, 0.98), g in (-0.98, 0.98), |c| in [0.25, 3], weights randn / sqrt(H) as bf16, dO randn 0.1, dc_io randn 0.05"""
    def u(*s):
        return torch.rand(*s, generator=g, dtype=torch.float32)

    def n(*s):
        return torch.randn(*s, generator=g, dtype=torch.float32)

    def signed(x):
        return x * (torch.randint(0, 2, x.shape, generator=g).float() * 2 - 1)
    ifo = 0.02 + 0.96 * u(T, Bn, H // 32, 4, 32)
    gg = -0.98 + 1.96 * u(T, Bn, H // 32, 32)
    ifo[:, :, :, 2, :] = gg
    d = dict(gates=ifo.reshape(T, Bn, 4 * H).contiguous(), c=signed(0.25 + 2.75 * u(T, Bn, H)),
             WhhT=(n(H, 4 * H) / H ** 0.5).to(torch.bfloat16), dc0=n(Bn, H) * 0.05,
             c_before=signed(0.25 + 2.75 * u(Bn, H)) if c_before else None,
             dO=n(T, Bn, H) * 0.1 if with_dO else None,
             WihT_above=(n(H, 4 * H) / H ** 0.5).to(torch.bfloat16) if with_above else None,
             sink_WT=None, mask=None, tail=None)
    if with_sink:
        d["sink_WT"] = (n(H, 4 * H) / H ** 0.5).to(torch.bfloat16)
        if mask:
            d["mask"] = (n(T, Bn, H)).to(torch.bfloat16)
    return d


def make_inputs(s):
    g = torch.Generator().manual_seed(1000 + s.seed)
    inp = [[make_layer_inputs(g, s.T, s.Bn, s.H, k == 0, k > 0, s.sink and k == s.nlayer - 1, s.c_before, s.mask) for k in range(s.nlayer)]
           for _ in range(s.nnet)]
    for net in inp:
        for d in net:
            d["bias_old"] = torch.randn(4 * s.H, generator=g) * 3 + 0.5
            d["bias_old1"] = torch.randn(4 * s.H, generator=g) * 3 - 0.5
            d["sink_bias_old"] = torch.randn(s.H, generator=g) * 3 + 0.25
            d["colmap"] = torch.randperm(4 * s.H, generator=g).to(torch.int32) if s.colmap_perm else None
    return inp


# ---------------------------------------------------------------------------------------------------
# the harness: hsad_lstm_backward_fused
# ---------------------------------------------------------------------------------------------------
def _poison16(n):
    return torch.full((n,), POISON16, dtype=torch.int16, device=DEV)


def _poison32(n):
    return torch.full((n,), POISON32, dtype=torch.int32, device=DEV)


def _bits(t):
    """any tensor -> its bits as a flat integer tensor of the element size"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).reshape(-1)


def bf16_values(bits):
    """int16 bit patterns -> fp64 values"""
    return bits.view(torch.bfloat16).to(torch.float64)


class FusedLaunch:
    """Device buffers of a whole sequence and hsad_lstm_fused_bwd_rec records over a window [t0, t0 + Tc) of it."""

    def __init__(self, spec, inp):
        s = self.spec = spec
        self.inp = inp
        T, Bn, H = s.T, s.Bn, s.H
        self.lib = _lib.load_library()
        nrb = Bn // 32
        xb = T * nrb * 32 * 4 * H                       # hand-off buffers: sized as the learner sizes them
        self.ldT = T * Bn + 32
        self.keep_in, self.dev = [], []                  # (name, device tensor, bits before) / per (net, layer) dict of device buffers
        for net in inp:
            row = []
            for k, d in enumerate(net):
                b = {}
                gates, c = d["gates"], d["c"]
                cb = d["c_before"]
                if s.frag:
                    gates, c = pack_saved_gates(gates, T, Bn, H), pack_saved_c(c, T, Bn, H)
                    cb = pack_saved_c(cb, 1, Bn, H) if cb is not None else None
                for name, v in (("gates", gates), ("c", c), ("c_before", cb), ("WhhT", d["WhhT"]), ("dO", d["dO"]), ("WihT_above", d["WihT_above"]),
                                ("sink_WT", d["sink_WT"]), ("mask", d["mask"]), ("colmap", d["colmap"])):
                    b[name] = v.contiguous().to(DEV) if v is not None else None
                    if v is not None:
                        self.keep_in.append((name, b[name], _bits(b[name]).clone()))
                b["dc"] = torch.cat([_bits(d["dc0"].contiguous()).to(DEV), _poison32(TAIL)])
                b["dG16"] = _poison16((T + 2) * Bn * 4 * H)          # slot T: the tail, slot T + 1: canary
                b["xchg"] = _poison16(xb + TAIL)
                b["xout"] = _poison16(xb + TAIL)
                b["sink_xout"] = _poison16(xb + TAIL)
                b["dGT"] = _poison16(4 * H * self.ldT + TAIL)
                b["dO_stage"] = _poison32(T * Bn * H + TAIL)
                b["sink_out"] = _poison16(T * Bn * H + TAIL)
                b["sink_outT"] = _poison16(H * self.ldT + TAIL)
                b["bias0"] = torch.cat([_bits(d["bias_old"]).to(DEV), _poison32(TAIL)])
                b["bias1"] = torch.cat([_bits(d["bias_old1"]).to(DEV), _poison32(TAIL)])
                b["sink_bias"] = torch.cat([_bits(d["sink_bias_old"]).to(DEV), _poison32(TAIL)])
                row.append(b)
            self.dev.append(row)
        nint = (2 * s.nlayer - 1 if s.proj else s.nlayer) + (1 if s.sink else 0)
        self.R = 8 if s.wide else (2 * s.nnet * nint if s.split else s.nnet * s.nlayer)

    def set_tail(self, net, k, tail16):
        """slot T of dG16 (has_next of the sequence's last chunk)"""
        s = self.spec
        self.dev[net][k]["dG16"][s.T * s.Bn * 4 * s.H:(s.T + 1) * s.Bn * 4 * s.H] = _bits(tail16).to(DEV)

    def poison_outputs(self, dc_and_bias=True):
        """everything a launch writes back to NaN, the accumulated vectors back to their entry values (for a repeat launch)"""
        for net, row in zip(self.inp, self.dev):
            for d, b in zip(net, row):
                for name in ("dG16", "xchg", "xout", "sink_xout", "dGT", "sink_out", "sink_outT"):
                    b[name].fill_(POISON16)
                b["dO_stage"].fill_(POISON32)
                if dc_and_bias:
                    n = d["dc0"].numel()
                    b["dc"][:n] = _bits(d["dc0"].contiguous()).to(DEV)
                    b["bias0"][:4 * self.spec.H] = _bits(d["bias_old"]).to(DEV)
                    b["bias1"][:4 * self.spec.H] = _bits(d["bias_old1"]).to(DEV)
                    b["sink_bias"][:self.spec.H] = _bits(d["sink_bias_old"]).to(DEV)

    def records(self, t0, Tc, has_next, layout_steps):
        s = self.spec
        Bn, H = s.Bn, s.H
        recs = (_lib.LstmFusedBwdRec * (s.nnet * s.nlayer))()
        for n in range(s.nnet):
            for k in range(s.nlayer):
                b, r = self.dev[n][k], recs[n * s.nlayer + k]
                last = k == s.nlayer - 1
                r.WhhT_blocked = b["WhhT"].data_ptr()
                r.WihT_above_blocked = b["WihT_above"].data_ptr() if k > 0 else None
                r.gates = b["gates"].data_ptr() + t0 * Bn * 4 * H * 4
                r.cseq = b["c"].data_ptr() + t0 * Bn * H * 4
                if t0 > 0:
                    r.c_before = b["c"].data_ptr() + (t0 - 1) * Bn * H * 4
                else:
                    r.c_before = b["c_before"].data_ptr() if b["c_before"] is not None else None
                r.dO = b["dO"].data_ptr() + t0 * Bn * H * 4 if k == 0 else None
                r.dG16 = b["dG16"].data_ptr() + t0 * Bn * 4 * H * 2
                r.dc_io = b["dc"].data_ptr()
                r.has_next = has_next
                r.xchg = b["xchg"].data_ptr()
                r.saved_frag_major = 1 if s.frag else 0
                r.tail_is_zero = 0
                r.xout = b["xout"].data_ptr() if s.split and not last else None
                r.dO_stage = b["dO_stage"].data_ptr() + t0 * Bn * H * 4 if s.proj and k > 0 else None
                if s.sink and last:
                    r.sink_WT = b["sink_WT"].data_ptr()
                    r.sink_out16 = b["sink_out"].data_ptr() + t0 * Bn * H * 2
                    r.sink_mask16 = b["mask"].data_ptr() + t0 * Bn * H * 2 if b["mask"] is not None else None
                    r.sink_xout = b["sink_xout"].data_ptr()
                    r.sink_outT16 = b["sink_outT"].data_ptr() + t0 * Bn * 2 if s.sink_T else None
                    r.sink_ldT = self.ldT
                    r.sink_bias_grad = b["sink_bias"].data_ptr()
                if s.dgt:
                    assert t0 == 0 and not has_next      # (dGT16 replaces the row-major dG16 a following chunk would read)
                    r.dGT16 = b["dGT"].data_ptr()
                    r.ldT = self.ldT
                    r.bias_grad0 = b["bias0"].data_ptr()
                    r.bias_grad1 = b["bias1"].data_ptr() if s.bias1 else None
                    r.bias_col_map = b["colmap"].data_ptr() if b["colmap"] is not None else None
        recs[0].layout_steps = layout_steps
        recs[0].wide_blocks = 1 if s.wide else 0
        return recs

    def run(self, t0=0, Tc=None, has_next=0, layout_steps=0):
        """one launch over [t0, t0 + Tc); next_sync_scratch NULL; the sticky timeout word must read 0"""
        s = self.spec
        Tc = s.T if Tc is None else Tc
        TL = max(layout_steps, Tc)
        nrb = s.Bn // 32
        words = self.R * nrb * (TL + 2)
        sync = torch.zeros(max(words, 8 * nrb * (TL + 2)) + 4, dtype=torch.int32, device=DEV)      # (the learner's block: 8 nrb (T + 2) + 4)
        recs = self.records(t0, Tc, has_next, layout_steps)
        _lib.check(self.lib.hsad_lstm_backward_fused(s.nnet, s.nlayer, Tc, s.Bn, s.H, C.byref(recs), sync.data_ptr(), None, None))
        torch.cuda.synchronize()
        assert int(sync[words].item()) == 0, "%r: the launch's sticky timeout word is set" % s

    def assert_inputs_unchanged(self):
        for name, t, before in self.keep_in:
            assert torch.equal(_bits(t), before), "%r: the launch changed its input %s" % (self.spec, name)

    def outputs(self, window=None):
        """-> per (net, layer) dict of CPU bit tensors; canaries and untouched regions asserted on the way.  window = (t0, Tc) of the
        last launch when several launches covered the sequence: the hand-off buffers then hold that chunk's tiles."""
        s = self.spec
        T, Bn, H, ldT = s.T, s.Bn, s.H, self.ldT
        w0, wT = window if window is not None else (0, T)
        nw = wT * Bn * 4 * H
        n4, n1 = T * Bn * 4 * H, T * Bn * H
        res = []
        for n in range(s.nnet):
            row = []
            for k in range(s.nlayer):
                b = {name: v.cpu() for name, v in self.dev[n][k].items() if v is not None and name in (
                    "dc", "dG16", "xchg", "xout", "sink_xout", "dGT", "dO_stage", "sink_out", "sink_outT", "bias0", "bias1", "sink_bias")}
                last = k == s.nlayer - 1
                o = {}
                tag = "%r net %d layer %d: " % (s, n, k)

                def clean16(x, what):
                    assert bool((x == POISON16).all()), tag + what + " was written"

                def clean32(x, what):
                    assert bool((x == POISON32).all()), tag + what + " was written"
                clean16(b["dG16"][n4 + Bn * 4 * H:], "dG16 beyond slot T")
                o["tail"] = b["dG16"][n4:n4 + Bn * 4 * H].reshape(Bn, 4 * H)
                if s.dgt:
                    clean16(b["dG16"][:n4], "the row-major dG16 (a launch with dGT16)")
                    full = b["dGT"][:4 * H * ldT].reshape(4 * H, ldT)
                    clean16(full[:, T * Bn:], "dGT16 past column T Bn")
                    clean16(b["dGT"][4 * H * ldT:], "dGT16 past its end")
                    o["dG"] = read_transposed(b["dGT"], ldT, T, Bn, 4 * H).contiguous()
                else:
                    clean16(b["dGT"], "dGT16 (not given)")
                    o["dG"] = b["dG16"][:n4].reshape(T, Bn, 4 * H)
                # the hand-off tiles hold the bits of dG wherever a step publishes: t > 0, and t = 0 when a stage below reads it
                feeds = (not last) or s.sink
                clean16(b["xchg"][nw:], "xchg past its end")
                tiles = read_tiles(b["xchg"], wT, Bn, H, 16 if s.wide else 32)
                t_from = 0 if feeds else 1
                assert torch.equal(tiles[t_from:], o["dG"][w0 + t_from:w0 + wT]), tag + "hand-off tiles and dG differ"
                if not feeds:
                    clean16(tiles[0], "the hand-off tile of step 0 (nobody reads it)")
                o["tiles"] = tiles
                if not s.wide:
                    for name, used in (("xout", s.split and not last), ("sink_xout", s.sink and last)):
                        if used:
                            assert torch.equal(read_tiles(b[name], wT, Bn, H, 32), o["dG"][w0:w0 + wT]), tag + name + " and dG differ"
                            clean16(b[name][nw:], name + " past its end")
                        else:
                            clean16(b[name], name + " (not given)")
                if s.proj and k > 0:
                    clean32(b["dO_stage"][n1:], "dO_stage past its end")
                    o["dO_stage"] = b["dO_stage"][:n1].reshape(T, Bn, H)
                else:
                    clean32(b["dO_stage"], "dO_stage (not given)")
                if s.sink and last:
                    if s.sink_T:
                        clean16(b["sink_out"], "sink_out16 (a launch with sink_outT16)")
                        full = b["sink_outT"][:H * ldT].reshape(H, ldT)
                        clean16(full[:, T * Bn:], "sink_outT16 past column T Bn")
                        clean16(b["sink_outT"][H * ldT:], "sink_outT16 past its end")
                        o["sink"] = read_transposed(b["sink_outT"], ldT, T, Bn, H).contiguous()
                    else:
                        clean16(b["sink_outT"], "sink_outT16 (not given)")
                        clean16(b["sink_out"][n1:], "sink_out16 past its end")
                        o["sink"] = b["sink_out"][:n1].reshape(T, Bn, H)
                    clean32(b["sink_bias"][H:], "sink_bias_grad past H")
                    o["sink_bias"] = b["sink_bias"][:H]
                else:
                    clean16(b["sink_out"], "sink_out16 (not given)")
                    clean16(b["sink_outT"], "sink_outT16 (not given)")
                    assert torch.equal(b["sink_bias"][:H], _bits(self.inp[n][k]["sink_bias_old"])), tag + "sink_bias_grad (not given) changed"
                clean32(b["dc"][Bn * H:], "dc_io past its end")
                o["dc"] = b["dc"][:Bn * H].reshape(Bn, H)
                for name, old, used in (("bias0", "bias_old", s.dgt), ("bias1", "bias_old1", s.dgt and s.bias1)):
                    clean32(b[name][4 * H:], name + " past 4H")
                    if used:
                        o[name] = b[name][:4 * H]
                    else:
                        assert torch.equal(b[name][:4 * H], _bits(self.inp[n][k][old])), tag + name + " (not given) changed"
                row.append(o)
            res.append(row)
        return res


def f32_values(bits):
    return bits.view(torch.float32).to(torch.float64)


def check_layer(tag, d, got_dG_bits, H, T, dO64, above, tail64, ratios, key, products=1, exact_stats=None):
    """dG and the final dc of one layer against the teacher-forced reference -> the reference's (ref, M)"""
    got = bf16_values(got_dG_bits)
    ref, M, dc, dc_abs = layer_reference(got, dO64, d["WhhT"].double(), d["gates"].double(), d["c"].double(),
                                         d["c_before"].double() if d["c_before"] is not None else None, d["dc0"].double(), above, tail64)
    ratios[key + " dG"] = max(ratios.get(key + " dG", 0.0), worst_ratio(got, ref, bound(ref, M, H, T, products)))
    if exact_stats is not None:
        exact_stats.append(float((bf16_round(ref) == got).double().mean()))
    return ref, M, dc, dc_abs


def check_fused(spec, inp, out, tails=None):
    """every output of a launch (or of the launches that cover the sequence) against the reference -> {stage: worst err / bound},
    and the share of dG elements that equal the correctly rounded reference"""
    s = spec
    T, Bn, H = s.T, s.Bn, s.H
    kern = "wide" if s.wide else "32x32"
    ratios, exact = {}, []
    for n in range(s.nnet):
        for k in range(s.nlayer):
            d, o = inp[n][k], out[n][k]
            tag = "%r net %d layer %d: " % (s, n, k)
            tail64 = bf16_values(tails[n][k]) if tails is not None else None
            if s.wide:      # (the 16 x 64 blocking has no has_next and never touches the row-major dG16)
                assert bool((o["tail"] == POISON16).all()), tag + "dG16 slot T was written"
            elif tails is None:
                assert bool((o["tail"] == 0).all()), tag + "dG16 slot T is not zero after a launch without has_next"
            above, dO64, products = None, d["dO"].double() if d["dO"] is not None else None, 1
            if k > 0:
                dG_up = bf16_values(out[n][k - 1]["dG"])
                if s.proj:      # the projection stage's rows against the product of the kernel's own dG above; the layer takes them as they are
                    dO64 = f32_values(o["dO_stage"])
                    pref, pM = product_reference(dG_up, d["WihT_above"].double())
                    ratios[kern + " dO_stage"] = max(ratios.get(kern + " dO_stage", 0.0), worst_ratio(dO64, pref, bound(pref, pM, H, T, rounded=False)))
                else:
                    above, products = (dG_up, d["WihT_above"].double()), 2
            key = kern + (" top" if k == 0 else " lower")
            ref, M, dc, dc_abs = check_layer(tag, d, o["dG"], H, T, dO64, above, tail64, ratios, key, products, exact)
            got_dc = f32_values(o["dc"])
            ratios[key + " dc_io"] = max(ratios.get(key + " dc_io", 0.0), worst_ratio(got_dc, dc, dc_bound(dc_abs, H, T, products)))
            dG_own = bf16_values(o["dG"])
            if s.dgt:
                cm = d["colmap"].long() if d["colmap"] is not None else torch.arange(4 * H)
                terms = dG_own.reshape(T * Bn, 4 * H)
                for name, old in (("bias0", "bias_old"), ("bias1", "bias_old1")):
                    if name in o:
                        want = d[old].double().clone()
                        mag = d[old].double().abs()
                        want[cm] += terms.sum(0)
                        mag[cm] += terms.abs().sum(0)
                        ratios[kern + " bias"] = max(ratios.get(kern + " bias", 0.0),
                                                     worst_ratio(f32_values(o[name]), want, (T * Bn + 1) * U23 * mag))
            if s.sink and k == s.nlayer - 1:
                pref, pM = product_reference(dG_own, d["sink_WT"].double())
                on = (d["mask"].double() > 0) if d["mask"] is not None else torch.ones(T, Bn, H, dtype=torch.bool)
                want = torch.where(on, pref, torch.zeros_like(pref))
                got = bf16_values(o["sink"])
                ratios[kern + " sink"] = max(ratios.get(kern + " sink", 0.0),
                                             worst_ratio(got, want, torch.where(on, bound(pref, pM, H, T), torch.zeros_like(pref))))
                assert bool((o["sink"][~on] == 0).all()), tag + "a masked sink element is not +0"
                rows = got.reshape(T * Bn, H)
                want_b = d["sink_bias_old"].double() + rows.sum(0)
                mag = d["sink_bias_old"].double().abs() + rows.abs().sum(0)
                ratios[kern + " sink bias"] = max(ratios.get(kern + " sink bias", 0.0),
                                                  worst_ratio(f32_values(o["sink_bias"]), want_b, (T * Bn + 1) * U23 * mag))
    return ratios, min(exact)


def deterministic_bits(spec, out):
    """everything of a launch's outputs that is not summed by float atomics (the 32 x 32 kernel's bias sums are), for a bitwise repeat"""
    keep = []
    for row in out:
        for o in row:
            for name, v in sorted(o.items()):
                if spec.wide or name not in ("bias0", "bias1", "sink_bias"):
                    keep.append((name, v))
    return keep


# ---------------------------------------------------------------------------------------------------
# the harness: hsad_lstm_backward_chunk_multi / hsad_lstm_layer_backward (row-major activations, any Bn)
# ---------------------------------------------------------------------------------------------------
def run_seq_entry(entry, T, Bn, H, layers, with_sync=True):
    """entry 'multi': hsad_lstm_backward_chunk_multi over len(layers) independent records; 'layer': hsad_lstm_layer_backward (one record,
    sync_scratch given or NULL).  layers: make_layer_inputs dicts (dO given).  -> per record (dG bits [T, Bn, 4H], tail bits, dc bits or None)"""
    lib = _lib.load_library()
    nrec, nrb = len(layers), (Bn + 31) // 32
    n4 = T * Bn * 4 * H
    words = nrec * nrb * (T + 2)
    sync = torch.zeros(words + 4, dtype=torch.int32, device=DEV)
    bufs, keep = [], []
    for d in layers:
        b = {name: d[name].contiguous().to(DEV) for name in ("gates", "c", "WhhT", "dO")}
        b["c_before"] = d["c_before"].contiguous().to(DEV) if d["c_before"] is not None else None
        keep += [(name, v, _bits(v).clone()) for name, v in b.items() if v is not None]
        b["dG16"] = _poison16(n4 + Bn * 4 * H + TAIL)
        b["dc"] = torch.cat([_bits(d["dc0"].contiguous()).to(DEV), _poison32(TAIL)])
        bufs.append(b)
    if entry == "multi":
        recs = (_lib.LstmBwdRec * nrec)()
        for r, b in zip(recs, bufs):
            r.gates, r.cseq, r.WhhT_blocked, r.dO = b["gates"].data_ptr(), b["c"].data_ptr(), b["WhhT"].data_ptr(), b["dO"].data_ptr()
            r.c_before = b["c_before"].data_ptr() if b["c_before"] is not None else None
            r.dG16, r.dc_io = b["dG16"].data_ptr(), b["dc"].data_ptr()
            r.has_next, r.xchg, r.saved_frag_major, r.tail_is_zero = 0, None, 0, 0
        _lib.check(lib.hsad_lstm_backward_chunk_multi(nrec, T, Bn, H, C.byref(recs), sync.data_ptr(), None, None))
    else:
        b = bufs[0]
        _lib.check(lib.hsad_lstm_layer_backward(T, Bn, H, b["gates"].data_ptr(), b["c"].data_ptr(),
                                                b["c_before"].data_ptr() if b["c_before"] is not None else None, b["WhhT"].data_ptr(),
                                                b["dO"].data_ptr(), b["dG16"].data_ptr(), b["dc"].data_ptr(),
                                                sync.data_ptr() if with_sync else None, None))
    torch.cuda.synchronize()
    assert int(sync[words].item()) == 0, "the launch's sticky timeout word is set"
    for name, t, before in keep:
        assert torch.equal(_bits(t), before), "the launch changed its input %s" % name
    res = []
    for b in bufs:
        g = b["dG16"].cpu()
        assert bool((g[n4 + Bn * 4 * H:] == POISON16).all()), "dG16 was written beyond slot T"
        dc = b["dc"].cpu()
        assert bool((dc[Bn * H:] == POISON32).all()), "dc was written past its end"
        res.append((g[:n4].reshape(T, Bn, 4 * H), g[n4:n4 + Bn * 4 * H], dc[:Bn * H].reshape(Bn, H)))
    return res
