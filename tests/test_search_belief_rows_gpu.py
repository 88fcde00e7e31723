"""GPU: hsad_search_belief_rows -- the searcher's rows of the top LSTM layer's h as the bf16 operand of the belief head's GEMM --
against index_select + the tensor cast, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda:0"
INVALID = -1


def _s():
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


@pytest.mark.parametrize("G,P,H,pad", [(1, 2, 64, 0), (1, 2, 64, 8), (70, 3, 128, 0), (70, 3, 128, 24)])
def test_rows_equal_index_select_and_the_cast(G, P, H, pad):
    from hanabi_sad_amd import _lib
    lib = _lib.load_library()
    gen = torch.Generator().manual_seed(G * 1000 + H + pad)
    h = (torch.randn(G * P, H, generator=gen) * torch.logspace(-3, 3, G * P).unsqueeze(1)).to(DEV)
    h[0, :4] = torch.tensor([0.0, -0.0, 1.00390625, 1.01171875])      # two ties of the rounding: to even, down and up
    player = torch.from_numpy(np.arange(G) % P).to(torch.int32)
    if G > 4:
        player[3], player[G - 1], player[5] = -1, P, 7      # out of range: zero rows
    player = player.to(DEV)
    ldo = H + pad
    out = torch.full((G, ldo), 7.0, dtype=torch.bfloat16, device=DEV)
    before = h.clone()
    _lib.check(lib.hsad_search_belief_rows(h.data_ptr(), player.data_ptr(), G, P, H, out.data_ptr(), ldo, _s()))
    torch.cuda.synchronize()
    assert torch.equal(h, before), "the input was written"
    ok = (player >= 0) & (player < P)
    rows = torch.arange(G, device=DEV) * P + player.clamp(0, P - 1).long()
    want = h.index_select(0, rows).to(torch.bfloat16)
    want[~ok] = 0
    assert torch.equal(out[:, :H].view(torch.int16), want.view(torch.int16))
    assert bool((out[:, H:] == 7.0).all()), "a padding column was written"
    if G > 4:
        assert int((~ok).sum()) == 3 and not bool(out[3, :H].any()) and not bool(out[G - 1, :H].any())


def test_refusals_and_the_sampler_face():
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.belief import BeliefSampler
    lib = _lib.load_library()
    h = torch.zeros(6, 64, device=DEV)
    pl = torch.zeros(3, dtype=torch.int32, device=DEV)
    out = torch.zeros(3, 64, dtype=torch.bfloat16, device=DEV)
    f = lib.hsad_search_belief_rows
    assert f(None, pl.data_ptr(), 3, 2, 64, out.data_ptr(), 64, _s()) == INVALID
    assert f(h.data_ptr(), None, 3, 2, 64, out.data_ptr(), 64, _s()) == INVALID
    assert f(h.data_ptr(), pl.data_ptr(), 3, 2, 64, None, 64, _s()) == INVALID
    assert f(h.data_ptr(), pl.data_ptr(), 3, 2, 60, out.data_ptr(), 64, _s()) == INVALID      # H % 8
    assert f(h.data_ptr(), pl.data_ptr(), 3, 2, 64, out.data_ptr(), 56, _s()) == INVALID      # ldo < H
    assert f(h.data_ptr(), pl.data_ptr(), 0, 2, 64, out.data_ptr(), 64, _s()) == INVALID
    assert f(h.data_ptr() + 4, pl.data_ptr(), 2, 2, 64, out.data_ptr(), 64, _s()) == INVALID  # alignment
    # BeliefSampler.logits = rows, then the head's GEMM with its bias: against the float64 product of the bf16 operands
    gen = torch.Generator().manual_seed(3)
    sd = {"belief.weight": torch.randn(50, 64, generator=gen) * 0.3, "belief.bias": torch.randn(50, generator=gen), "hand_size": 2, "H": 64}
    bs = BeliefSampler(sd, DEV)
    assert (bs.hand_size, bs.H, bs.NZ, bs.NZp) == (2, 64, 50, 56)
    hh = torch.randn(6, 64, generator=gen).to(DEV)
    player = torch.tensor([1, 0, -1], dtype=torch.int32, device=DEV)
    z = bs.logits(hh, player)
    assert z.shape == (3, 56) and z.dtype == torch.float32
    x = torch.stack([hh[1], hh[2], torch.zeros(64, device=DEV)]).to(torch.bfloat16).double().cpu()
    w = sd["belief.weight"].to(torch.bfloat16).double()
    want = x @ w.t() + sd["belief.bias"].double()
    assert float((z[:, :50].double().cpu() - want).abs().max()) <= 64 * 2.0 ** -24 * float((x.abs() @ w.abs().t()).max() + 4)
    assert not bool(z[:, 50:].any())
    with pytest.raises(ValueError):
        bs.logits(hh[:, :32].contiguous(), player)
