"""One workgroup of a persistent LSTM launch made late on purpose (hsad_lstm_debug_stall, include/hsad.h).

The learner's three persistent recurrence launches -- lstm_fused_fwd_kernel (the forward), lstm_bptt_wide_kernel (the BPTT of one net at
H = 512, B <= 128) and lstm_fused_bwd_kernel (the 32 x 32 BPTT: VDN at B = 256, H = 256, set_fused bit 25) -- hand tiles between
workgroups through counters in memory and promise the same bits under every schedule.  Repeat runs only see the schedules the hardware
happens to produce; here the chosen workgroup sleeps 60 us (about 12 BPTT steps) behind one step's counter wait and in front of its
hand-off stores.  Loss, priorities and every gradient must be the bits of the same update without the stall, no wait may give up, and
the hook must have fired exactly once.  (The 32 x 32 launch adds its bias gradients -- and at 256 rows the input layer's split-K weight
gradient -- with float atomics in arrival order: there those are held to 1e-5, everything else to the bit.)

The learner reuses its dO and tile buffers, so a consumer that reads a row before its producer has written it finds the previous
update's value -- the right one, if that update ran on the same batch.  Every stalled update therefore runs right behind an update on a
DIFFERENT batch, and the expected bits are those of the same two-update sequence without the stall, on a fresh learner."""
import ctypes as C

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"
F, A, H, T = 838, 21, 512, 80
FWD, WIDE, B32 = 0, 1, 2              # HSAD_STALL_FWD / HSAD_STALL_BPTT_WIDE / HSAD_STALL_BPTT_32
STALL_US = 60
WIDE_FLAGS = 57 | (1 << 8)            # the default schedule: fused forward, four-stage BPTT launch (the wide blocking where the shape allows)
B32_FLAGS = WIDE_FLAGS | (1 << 25)    # ... in the 32 x 32 blocking


def _lib():
    from hanabi_sad_amd import _lib
    return _lib, _lib.load_library()


def fired(reset=True):
    m, lib = _lib()
    n = C.c_uint64(0)
    m.check(lib.hsad_lstm_debug_stall_fired(C.byref(n), 1 if reset else 0))
    return n.value


def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


def _batch(B, vdn, seed):
    """B sequences (IQL) or B games x 2 players (VDN, the layout of tests/test_vdn_gpu.py)"""
    from tests.test_r2d2_kernels_gpu import _rand_batch
    if not vdn:
        return _rand_batch(T, B, F, A, seed=seed)
    P = 2
    flat, weight = _rand_batch(T, B * P, F, A, seed=seed)
    v4 = lambda t: t.view(T, B, P, -1)
    seq_len = flat["seq_len"].view(B, P)[:, 0].contiguous()
    mask = (torch.arange(T, device=DEV).unsqueeze(1) < seq_len.unsqueeze(0)).float()
    legal = v4(flat["legal_move"]).clone()
    legal[..., 0] = 1
    batch = {"priv_s": v4(flat["priv_s"]) * mask.view(T, B, 1, 1), "legal_move": legal, "a": flat["a"].view(T, B, P),
             "reward": flat["reward"].view(T, B, P)[:, :, 0].contiguous() * mask,
             "bootstrap": (torch.arange(T, device=DEV).unsqueeze(1) + 3 < seq_len.unsqueeze(0)).float(), "seq_len": seq_len}
    return batch, weight[:B].contiguous()


class Shape:
    """one learner per batch shape (schedules switched with set_fused) and two batches; the expected bits per flag word"""

    def __init__(self, B, vdn):
        from hanabi_sad_amd.composite import CompositeLearner
        from tests.test_r2d2_kernels_gpu import _rand_net
        self.B, self.vdn, self.pw = B, vdn, 0.0 if vdn else 0.25
        self.rows = B * (2 if vdn else 1)
        self.W, self.Wt = _rand_net(F, H, A, seed=61), _rand_net(F, H, A, seed=62)
        self.other, self.batch = _batch(B, vdn, seed=101), _batch(B, vdn, seed=102)
        self.L = CompositeLearner(self.W, self.Wt, 3, 0.999, device=DEV)
        self.want = {}

    def update(self, L, batch):
        loss, prio = L.loss(batch[0], batch[1], self.pw)
        out = {"loss": loss.clone(), "priority": prio.clone()}
        out.update({k: v.clone() for k, v in L.grad.items()})
        return out

    def expected(self, flags):
        """the second update of (other batch, batch) on a fresh learner, no stall"""
        if flags not in self.want:
            from hanabi_sad_amd.composite import CompositeLearner
            fresh = CompositeLearner(self.W, self.Wt, 3, 0.999, device=DEV)
            fresh.set_fused(flags)
            self.update(fresh, self.other)
            self.want[flags] = self.update(fresh, self.batch)
            fresh.check_sync()
            fresh.close()
        return self.want[flags]


@pytest.fixture(scope="module")
def shape():
    made = {}

    def get(B, vdn=False):
        if (B, vdn) not in made:
            made[(B, vdn)] = Shape(B, vdn)
        return made[(B, vdn)]
    yield get
    for s in made.values():
        s.L.close()


def run_stalled(S, flags, kernel, rec, rb, nb, step, cross=False, atomics=False):
    m, lib = _lib()
    want = S.expected(flags)
    S.L.set_fused(flags)
    fired(reset=True)
    where = "kernel %d, record %d, row block %d, unit block %d, step %d%s" % (kernel, rec, rb, nb, step, ", cross-XCD exchange" if cross else "")
    try:
        if cross:
            m.check(lib.hsad_lstm_set_exchange_mode(1))
        S.update(S.L, S.other)        # a different batch first: what a too-early read finds is this update's value
        m.check(lib.hsad_lstm_debug_stall(kernel, rec, rb, nb, step, STALL_US))
        got = S.update(S.L, S.batch)
    finally:
        lib.hsad_lstm_debug_stall(-1, 0, 0, 0, 0, 0)
        lib.hsad_lstm_set_exchange_mode(0)
    n = fired()
    S.L.check_sync()
    assert n == 1, "the stall hook fired %d times (%s)" % (n, where)
    exact = lambda k: not atomics or k in ("loss", "priority") or k.startswith("lstm.weight")
    bad = {k: relerr(got[k], want[k]) for k in want if not torch.equal(got[k], want[k]) and (exact(k) or relerr(got[k], want[k]) > 1e-5)}
    assert not bad, "stalled workgroup (%s) changed the update: %s" % (where, bad)


@pytest.mark.parametrize("pos", ["first", "last"])
@pytest.mark.parametrize("step", [T - 1, T // 2, 1, 0])
@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_wide_bptt_gives_the_same_bits_with_one_workgroup_late(shape, stage, step, pos):
    """stages 0 top layer, 1 projection (dO of the lower layer), 2 lower layer, 3 sink (d x of the input layer); the first workgroup
    (row block 0, unit block 0) or the last (row block B / 16 - 1, unit block 7)"""
    S = shape(128)
    rb, nb = (0, 0) if pos == "first" else (S.rows // 16 - 1, 7)
    run_stalled(S, WIDE_FLAGS, WIDE, stage, rb, nb, step)


@pytest.mark.parametrize("step", [T - 1, T // 2, 1])
def test_wide_bptt_projection_stage_late_under_the_cross_xcd_exchange(shape, step):
    """the same hand-off with agent-scope counters and written-through tiles (hsad_lstm_set_exchange_mode(1))"""
    S = shape(128)
    run_stalled(S, WIDE_FLAGS, WIDE, 1, S.rows // 16 - 1, 7, step, cross=True)


@pytest.mark.parametrize("step", [T - 1, T // 2])
@pytest.mark.parametrize("vdn,rec", [(False, 0), (False, 1), (False, 2), (False, 3), (True, 0), (True, 1)])
def test_32x32_bptt_gives_the_same_bits_with_one_workgroup_late(shape, vdn, rec, step):
    """B = 128 under set_fused bit 25: internal records 0 top layer, 1 projection stage, 2 lower layer, 3 sink stage.  VDN at 128 games x 2
    players = 256 rows, where the 32 x 32 blocking is the default (the wide one takes at most 128 rows) and only the split placement fits
    the chip: records 0 top layer, 1 lower layer (its X stream through the written-through copy)"""
    S = shape(128, vdn)
    run_stalled(S, WIDE_FLAGS if vdn else B32_FLAGS, B32, rec, S.rows // 32 - 1, 15, step, atomics=True)


@pytest.mark.parametrize("step", [0, T // 2, T - 1])
@pytest.mark.parametrize("rec", [0, 1, 2, 3])
def test_fused_forward_gives_the_same_bits_with_one_workgroup_late(shape, rec, step):
    """records net * 2 + layer: the online net's two layers (0, 1), the target net's (2, 3), all four in one launch at B = 128"""
    S = shape(128)
    run_stalled(S, WIDE_FLAGS, FWD, rec, S.rows // 32 - 1, 9, step)


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("B", [32, 64, 96])
def test_wide_bptt_at_small_batches_gives_the_same_bits_with_one_workgroup_late(shape, B, stage):
    """B = 32 / 64 / 96 (selfplay --batchsize, VDN at batchsize 16 / 32): 2 / 4 / 6 row blocks, the other XCDs' workgroups return at once"""
    S = shape(B)
    run_stalled(S, WIDE_FLAGS, WIDE, stage, S.rows // 16 - 1, 7, T - 1)
