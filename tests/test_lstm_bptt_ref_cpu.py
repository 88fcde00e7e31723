"""CPU: the fp64 BPTT reference of tests/lstm_bptt_ref.py is itself held to something independent before the GPU tests lean on it.

* With rounding switched off (free running, no teacher forcing) its dG, dO and d x, chained over T = 4 and two stacked layers, are the
  gradients torch.autograd gives for an fp64 restatement of nn.LSTM (gate order i, f, g, o) -- on weights, biases, inputs, to 1e-12.
* The packers are the inverses of r2d2.unpack_saved_gates / unpack_saved_c.
* The tile reader inverts a tile written in Python from the kernels' own store-loop index formulas, for both blockings.
* The ctypes mirrors of hsad_lstm_fused_bwd_rec / hsad_lstm_bwd_rec have the C compiler's sizeof and field offsets."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from hanabi_sad_amd import _lib, r2d2
from tests import lstm_bptt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT_SRC = os.path.join(ROOT, "tests", "lstm_bptt", "bwd_rec_layout.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")


def relerr(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_the_unrounded_reference_is_autograd_of_an_fp64_lstm():
    T, Bn, H, F = 4, 3, 64, 32
    g = torch.Generator().manual_seed(5)

    def rn(*s):
        return torch.randn(*s, generator=g, dtype=torch.float64)
    x = rn(T, Bn, F).requires_grad_()
    Wih = [(rn(4 * H, F) / F ** 0.5).requires_grad_(), (rn(4 * H, H) / H ** 0.5).requires_grad_()]
    Whh = [(rn(4 * H, H) / H ** 0.5).requires_grad_() for _ in range(2)]
    bias = [rn(4 * H).requires_grad_() for _ in range(2)]
    c0 = [rn(Bn, H) for _ in range(2)]
    h0 = [rn(Bn, H) for _ in range(2)]
    RO, Rc = rn(T, Bn, H), [rn(Bn, H) * 0.3 for _ in range(2)]
    perm = r2d2.gate_block_perm(H, "cpu")
    # forward, nn.LSTM's arithmetic (torch/nn/modules/rnn.py): gates = x W_ih^T + h W_hh^T + b, chunks i f g o
    seq, saved, loss = x, [], 0.0
    for l in range(2):
        h, c = h0[l], c0[l]
        hs, acts, cs = [], [], []
        for t in range(T):
            pre = seq[t] @ Wih[l].T + h @ Whh[l].T + bias[l]
            i, f, gg, o = pre.chunk(4, dim=1)
            i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
            c = f * c + i * gg
            h = o * torch.tanh(c)
            hs.append(h)
            cs.append(c)
            acts.append(torch.cat([i, f, gg, o], dim=1)[:, perm])
        loss = loss + (c * Rc[l]).sum()         # a gradient that enters the last step through c: dc_io on entry
        saved.append(dict(gates=torch.stack(acts).detach(), c=torch.stack(cs).detach(), hprev=torch.stack([h0[l]] + hs[:-1]).detach()))
        seq = torch.stack(hs)
    loss = loss + (seq * RO).sum()
    loss.backward()
    # backward with the reference, top layer first, as the fused launch chains its stages
    WhhT = [Whh[l].detach()[perm].T.contiguous() for l in range(2)]
    WihT = [Wih[l].detach()[perm].T.contiguous() for l in range(2)]
    dG1, _, _, _ = R.layer_reference(None, RO, WhhT[1], saved[1]["gates"], saved[1]["c"], c0[1], Rc[1])
    dO0, _ = R.product_reference(dG1, WihT[1])
    dG0, _, _, _ = R.layer_reference(None, dO0, WhhT[0], saved[0]["gates"], saved[0]["c"], c0[0], Rc[0])
    dx, _ = R.product_reference(dG0, WihT[0])
    assert relerr(dx, x.grad) < 1e-12
    # the input sequence of layer 1 is layer 0's h: h_t = o_t tanh(c_t) from the saved activations
    h_below = [x.detach(), R.split_gates(saved[0]["gates"], H)[3] * torch.tanh(saved[0]["c"])]
    for l, dG in ((0, dG0), (1, dG1)):
        flat = dG.reshape(T * Bn, 4 * H)
        assert relerr(flat.sum(0), bias[l].grad[perm]) < 1e-12
        assert relerr(flat.T @ saved[l]["hprev"].reshape(T * Bn, H), Whh[l].grad[perm]) < 1e-12
        assert relerr(flat.T @ h_below[l].reshape(T * Bn, -1), Wih[l].grad[perm]) < 1e-12
    # the two-products-in-one-recurrence form (a lower layer without a projection stage) is the same chain
    dG0b, _, _, _ = R.layer_reference(None, None, WhhT[0], saved[0]["gates"], saved[0]["c"], c0[0], Rc[0], above=(dG1, WihT[1]))
    assert relerr(dG0b, dG0) < 1e-12


@pytest.mark.parametrize("T,Bn,H", [(2, 32, 256), (3, 96, 512)])
def test_packers_invert_the_unpackers(T, Bn, H):
    g = torch.arange(T * Bn * 4 * H, dtype=torch.float32).reshape(T, Bn, 4 * H)
    c = torch.arange(T * Bn * H, dtype=torch.float32).reshape(T, Bn, H)
    pg, pc = R.pack_saved_gates(g, T, Bn, H), R.pack_saved_c(c, T, Bn, H)
    assert not torch.equal(pg.reshape(-1), g.reshape(-1)) and not torch.equal(pc.reshape(-1), c.reshape(-1))
    assert torch.equal(r2d2.unpack_saved_gates(pg.reshape(-1), T, Bn, H), g)
    assert torch.equal(r2d2.unpack_saved_c(pc.reshape(-1), T, Bn, H), c)
    assert torch.equal(R.pack_saved_gates(r2d2.unpack_saved_gates(g.reshape(-1), T, Bn, H), T, Bn, H).reshape(-1), g.reshape(-1))
    assert torch.equal(R.pack_saved_c(r2d2.unpack_saved_c(c.reshape(-1), T, Bn, H), T, Bn, H).reshape(-1), c.reshape(-1))
    # a step's block stands alone: c_before is packed like one step of the sequence
    assert torch.equal(R.pack_saved_c(c[1:2], 1, Bn, H), pc[1:2])


def test_the_packed_order_is_the_one_the_kernels_index():
    """lstm_fused_bwd.inc / lstm_bptt_wide.inc: (row, unit) of the 32 x 32 blocking's lane sits at f32x4 index
    ((t nblk + blk) 1024 + fw 256 + r 64 + fl), fw = 2 wu + ((lane & 15) >> 3), fl = 16 (lane >> 4) + 8 wr + (lane & 7)"""
    T, Bn, H = 2, 64, 256
    g = torch.arange(T * Bn * 4 * H, dtype=torch.float32).reshape(T, Bn, 4 * H)
    c = torch.arange(T * Bn * H, dtype=torch.float32).reshape(T, Bn, H)
    pg, pc = R.pack_saved_gates(g, T, Bn, H).reshape(-1, 4), R.pack_saved_c(c, T, Bn, H).reshape(-1, 4)
    nrb, nun = Bn // 32, H // 32
    for t, rb, nb, wave, lane, r in ((0, 0, 0, 0, 0, 0), (1, 1, 7, 3, 63, 3), (1, 0, 5, 2, 37, 1), (0, 1, 2, 1, 24, 2)):
        wr, wu = wave >> 1, wave & 1
        fw, fl = wu * 2 + ((lane & 15) >> 3), (lane >> 4) * 16 + wr * 8 + (lane & 7)
        row, u = rb * 32 + wr * 16 + 4 * (lane >> 4) + r, nb * 32 + wu * 16 + (lane & 15)
        blk, nblk = rb * nun + nb, nrb * nun
        got = pg[(t * nblk + blk) * 1024 + fw * 256 + r * 64 + fl]
        assert got.tolist() == [float(g[t, row, nb * 128 + k * 32 + (u & 31)]) for k in range(4)]
        assert float(pc[(t * nblk + blk) * 256 + fw * 64 + fl][r]) == float(c[t, row, u])


@pytest.mark.parametrize("rows", [32, 16])
def test_the_tile_reader_inverts_the_kernels_store_loops(rows):
    T, Bn, H = 2, 64, 256 if rows == 32 else 512
    dG = torch.arange(T * Bn * 4 * H, dtype=torch.int64).reshape(T, Bn, 4 * H)
    tiles = torch.from_numpy(R.write_tiles_like_the_kernel(dG.numpy(), T, Bn, H, rows))
    assert int(tiles.min()) >= 0 and tiles.unique().numel() == tiles.numel()        # every element written exactly once
    assert torch.equal(R.read_tiles(tiles, T, Bn, H, rows), dG)
    assert not torch.equal(R.read_tiles(tiles, T, Bn, H, 48 - rows), dG)             # the other blocking is another order
    # transposed outputs: element (column, t Bn + row) with a row stride past T Bn
    ld = T * Bn + 32
    xT = torch.full((4 * H, ld), -1, dtype=torch.int64)
    xT[:, :T * Bn] = dG.reshape(T * Bn, 4 * H).T
    assert torch.equal(R.read_transposed(xT.reshape(-1), ld, T, Bn, 4 * H), dG)


def test_the_reference_bound_is_zero_only_where_the_result_is_an_exact_zero():
    ref = torch.tensor([1.0, 0.0, 0.0])
    M = torch.tensor([2.0, 0.0, 1.0])
    b = R.bound(ref, M, 256, 4)
    assert R.worst_ratio(torch.tensor([1.0, 0.0, 0.0]), ref, b) == 0.0
    assert R.worst_ratio(torch.tensor([1.0, -0.0, 0.0]), ref, b) == 0.0
    assert R.worst_ratio(torch.tensor([1.0, 1e-30, 0.0]), ref, b) == float("inf")
    assert R.worst_ratio(torch.tensor([float("nan"), 0.0, 0.0]), ref, b) == float("inf")
    assert 0.99 < R.worst_ratio(torch.tensor([1.0 + float(b[0]), 0.0, 0.0]), ref, b) < 1.01


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_ctypes_records_have_the_c_layout(tmp_path):
    exe = str(tmp_path / "bwd_rec_layout")
    cmd = ["gcc", "-std=c11", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + SAN + ["-I", os.path.join(ROOT, "include"), LAYOUT_SRC, "-o", exe]
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
    for name, mirror in (("hsad_lstm_fused_bwd_rec", _lib.LstmFusedBwdRec), ("hsad_lstm_bwd_rec", _lib.LstmBwdRec)):
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
