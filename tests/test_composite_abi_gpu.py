"""The COMPOSITE C-ABI entry points (include/hsad.h hsad_r2d2_*; csrc/hsad_agent.hip, csrc/hsad_learner.hip) -- the agent and the learner as single
library calls on plain pointers, what a C++ / pybind host binds.  Checked three ways:
  * against the REFERENCE's golden vectors (tests/golden/*.npz: act, compute_priority, loss, priorities, every gradient; IQL and
    VDN), with the tolerances measured for the bf16 kernels;
  * against the same schedule driven from Python (hanabi_sad_amd/r2d2.py) at the BASELINE shape: bit-equal loss, priorities and
    (deterministic, slab-reduced) LSTM weight gradients -- the library runs exactly the kernels in exactly the order the Python
    orchestration does -- and 1e-5-equal atomically accumulated ones;
  * in the loop: actor.DeviceActor on CompositeAgent writes the same replay as on the Python-orchestrated agent."""
import os

import numpy as np
import pytest
import torch

from tests import r2d2_torch_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def relerr(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


def maxerr(a, b):
    return float((torch.as_tensor(a).float().cpu() - torch.as_tensor(b).float().cpu()).abs().max())


def test_param_table_matches_the_reference_state_dict():
    from hanabi_sad_amd.composite import CNet, param_names
    from hanabi_sad_amd.r2d2 import PARAM_ORDER
    from hanabi_sad_amd.selfplay import init_weights
    assert param_names() == PARAM_ORDER
    W = init_weights(838, 64, 21, 5, 2)
    net = CNet(W, DEV)
    assert net.flat.numel() == sum(v.numel() for v in W.values())
    for k, v in W.items():
        assert torch.equal(net.w[k].cpu(), v)


@pytest.mark.parametrize("tag,pw", [("rl", 0.0), ("aux", 0.25)])
def test_composite_learner_against_reference_golden(tag, pw):
    from hanabi_sad_amd.composite import CompositeLearner
    z = np.load(os.path.join(GOLD, "r2d2_iql_sad_small.npz"))
    Won, Wtg = ref.weights_from_npz(z, "online_net."), ref.weights_from_npz(z, "target_net.")
    lr = CompositeLearner(Won, Wtg, int(z["meta"][8]), float(z["gamma"][0]), device=DEV)
    t = lambda k: torch.tensor(z[k]).to(DEV)
    batch = {k: t("loss." + k) for k in ("priv_s", "legal_move", "a", "reward", "bootstrap", "seq_len", "own_hand")}
    loss, prio = lr.loss(batch, t("loss.weight"), pw)
    assert maxerr(loss, z["loss.%s.loss" % tag]) <= 1.2e-3 and maxerr(prio, z["loss.%s.priority" % tag]) <= 1.5e-3
    for k, g in lr.grad.items():
        want = torch.tensor(z["loss.%s.grad.%s" % (tag, k)])
        if want.abs().max() == 0:
            assert g.abs().max() < 1e-6, k
        else:
            assert relerr(g, want) <= 8.5e-3, (k, relerr(g, want))


def test_composite_vdn_learner_and_priority_against_golden():
    from hanabi_sad_amd.composite import CNet, CompositeAgent, CompositeLearner
    z = np.load(os.path.join(GOLD, "r2d2_vdn_small.npz"))
    Won, Wtg = ref.weights_from_npz(z, "online_net."), ref.weights_from_npz(z, "target_net.")
    n, gamma = int(z["meta"][8]), float(z["gamma"][0])
    lr = CompositeLearner(Won, Wtg, n, gamma, device=DEV)
    batch = {k[5:]: torch.tensor(z[k]).to(DEV) for k in z.files if k.startswith("loss.") and k.count(".") == 1}
    loss, prio = lr.loss(batch, batch["weight"], 0.0)
    assert maxerr(loss, z["loss.rl.loss"]) <= 2.4e-3 and maxerr(prio, z["loss.rl.priority"]) <= 3e-3
    for k, g in lr.grad.items():
        want = torch.tensor(z["loss.rl.grad." + k])
        if float(want.norm()) >= 1e-7:
            assert relerr(g, want) <= 1.7e-2, k
    with pytest.raises(Exception):
        lr.loss(batch, batch["weight"], 0.25)
    P = z["act.priv_s"].shape[2]
    agent = CompositeAgent(CNet(Won, DEV), CNet(Wtg, DEV), n, gamma)
    f2 = lambda k: torch.tensor(z[k]).flatten(0, 2).to(DEV)

    def hid(hk, ck):
        f = lambda h: torch.tensor(h).reshape(h.shape[0] * h.shape[1], 2, -1).transpose(0, 1).contiguous().to(DEV)
        return {"h0": f(z[hk]), "c0": f(z[ck])}
    obs = {"priv_s": f2("act.priv_s"), "legal_move": f2("act.legal_move")}
    nobs = {"priv_s": f2("prio.next_priv_s"), "legal_move": f2("prio.next_legal_move")}
    p = agent.compute_priority(obs, f2("prio.a"), nobs, hid("act.h0", "act.c0"), hid("prio.next_h0", "prio.next_c0"),
                               torch.tensor(z["prio.reward"]).flatten().to(DEV), torch.tensor(z["prio.bootstrap"]).flatten().to(DEV),
                               num_player=P)
    assert maxerr(p, z["prio.out"].reshape(-1)) <= 3e-3


def test_composite_agent_against_golden_and_python_orchestration():
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.r2d2 import R2D2Agent, R2D2NetKernels
    z = np.load(os.path.join(GOLD, "r2d2_iql_sad_small.npz"))
    Won, Wtg = ref.weights_from_npz(z, "online_net."), ref.weights_from_npz(z, "target_net.")
    n, gamma = int(z["meta"][8]), float(z["gamma"][0])
    ca = CompositeAgent(CNet(Won, DEV), CNet(Wtg, DEV), n, gamma, seed=5)
    pa = R2D2Agent(R2D2NetKernels(Won, DEV), R2D2NetKernels(Wtg, DEV), n, gamma, seed=5)
    flat = lambda k: torch.tensor(z[k]).flatten(0, 1).to(DEV)

    def hid(hk, ck):
        f = lambda h: torch.tensor(h).reshape(h.shape[0] * h.shape[1], 2, -1).transpose(0, 1).contiguous().to(DEV)
        return {"h0": f(z[hk]), "c0": f(z[ck])}
    obs = {"priv_s": flat("act.priv_s"), "legal_move": flat("act.legal_move"), "eps": torch.zeros(flat("act.priv_s").shape[0], device=DEV)}
    rc, hc = ca.act(obs, hid("act.h0", "act.c0"), with_q=True)
    rp, hp = pa.act(obs, hid("act.h0", "act.c0"), with_q=True)
    for k in ("a", "greedy_a", "q_online_a", "q_target_greedy"):
        assert torch.equal(rc[k], rp[k]), k                       # same kernels, same order: bit-equal
    assert torch.equal(hc["h0"], hp["h0"]) and torch.equal(hc["c0"], hp["c0"])
    G = rc["a"].shape[0]
    assert maxerr(hc["h0"].transpose(0, 1), z["act.out_h0"].reshape(G, 2, -1)) <= 1e-3
    nobs = {"priv_s": flat("prio.next_priv_s"), "legal_move": flat("prio.next_legal_move")}
    args = (obs, flat("prio.a"), nobs, hid("act.h0", "act.c0"), hid("prio.next_h0", "prio.next_c0"), flat("prio.reward"), flat("prio.bootstrap"))
    pc, pp = ca.compute_priority(*args), pa.compute_priority(*args)
    assert torch.equal(pc, pp) and maxerr(pc, z["prio.out"].reshape(-1)) <= 1.5e-3
    obs["eps"] = torch.ones_like(obs["eps"])                       # exploration stream: same counter-based hash
    ca.counter = pa.counter = 9
    assert torch.equal(ca.act(obs, hid("act.h0", "act.c0"))[0]["a"], pa.act(obs, hid("act.h0", "act.c0"))[0]["a"])


@pytest.mark.parametrize("N", [2048, 4608])
def test_composite_act_on_the_fused_cell_path_equals_python_orchestration(N):
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.r2d2 import R2D2Agent, R2D2NetKernels
    from hanabi_sad_amd.selfplay import init_weights
    F, H, A = 838, 512, 21
    W, Wt = init_weights(F, H, A, 5, 1), init_weights(F, H, A, 5, 2)
    ca = CompositeAgent(CNet(W, DEV), CNet(Wt, DEV), 3, 0.999, seed=1)
    pa = R2D2Agent(R2D2NetKernels(W, DEV), R2D2NetKernels(Wt, DEV), 3, 0.999, seed=1)
    g = torch.Generator(device="cpu").manual_seed(N)
    obs = {"priv_s": (torch.rand(N, F, generator=g) < 0.15).float().to(DEV), "legal_move": (torch.rand(N, A, generator=g) < 0.5).float().to(DEV),
           "eps": torch.full((N,), 0.3, device=DEV)}
    obs["legal_move"][:, 0] = 1
    hid = {"h0": (torch.randn(2, N, H, generator=g) * 0.3).to(DEV), "c0": (torch.randn(2, N, H, generator=g) * 0.3).to(DEV)}
    for step in range(3):       # second / third step: the state carries its bf16 copy
        rc, hc = ca.act(obs, hid if step == 0 else hc_prev, with_q=True)
        rp, hp = pa.act(obs, hid if step == 0 else hp_prev, with_q=True)
        for k in ("a", "greedy_a", "q_online_a", "q_target_greedy"):
            assert torch.equal(rc[k], rp[k]), (step, k)
        assert torch.equal(hc["h0"], hp["h0"]) and torch.equal(hc["c0"], hp["c0"]) and torch.equal(hc["h0_16"], hp["h0_16"])
        hc_prev, hp_prev = hc, hp


@pytest.mark.parametrize("vdn", [False, True])
def test_composite_learner_equals_python_orchestration_bit_for_bit_at_the_baseline_shape(vdn):
    """configs[2]: F = 838, H = 512, T = 80, B = 128 (x 2 players for VDN): pipelined persistent recurrences, side-stream
    weight gradients, Adam -- three updates, parameters compared after each"""
    from hanabi_sad_amd.composite import CompositeLearner
    from hanabi_sad_amd.r2d2 import R2D2Learner, check_sync
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    F, A, H, T, B = (783, 21, 512, 80, 128) if vdn else (838, 21, 512, 80, 128)
    W, Wt = _rand_net(F, H, A, seed=3), _rand_net(F, H, A, seed=4)
    if vdn:
        P = 2
        flat, weight = _rand_batch(T, B * P, F, A)
        weight = weight[:B].contiguous()
        v4 = lambda t: t.view(T, B, P, -1)
        seq_len = flat["seq_len"].view(B, P)[:, 0].contiguous()
        batch = {"priv_s": v4(flat["priv_s"]).contiguous(), "legal_move": v4(flat["legal_move"]).contiguous(), "a": flat["a"].view(T, B, P),
                 "reward": flat["reward"].view(T, B, P)[:, :, 0].contiguous(),
                 "bootstrap": (torch.arange(T, device=DEV).unsqueeze(1) + 3 < seq_len.unsqueeze(0)).float(), "seq_len": seq_len}
        pw = 0.0
    else:
        batch, weight = _rand_batch(T, B, F, A)
        pw = 0.25
    cl = CompositeLearner(W, Wt, 3, 0.999, lr=1e-3, device=DEV)
    cl.set_fused(False)       # the Python orchestration runs the chunk-pipelined schedule
    pl = R2D2Learner(W, Wt, 3, 0.999, lr=1e-3, device=DEV)
    for it in range(3):
        lc, pc = cl.loss(batch, weight, pw)
        lp, pp = pl.loss(batch, weight, pw)
        torch.cuda.synchronize()
        if it == 0:
            assert torch.equal(lc, lp) and torch.equal(pc, pp)
        else:   # (the parameters differ in the last bits from here on -- see below -- and lr = 1e-3 amplifies that from update to update)
            # a single near-tie greedy flip moves one priority by O(0.1): percentiles, like the precision tests
            d = ((pc - pp).abs() / (1 + pp.abs())).flatten()
            assert torch.allclose(lc, lp, rtol=2e-2, atol=1e-2) and float(torch.quantile(d, 0.999)) < 1e-2 and float(d.max()) < 1.0
        for k in pl.grad:
            if it == 0 and k.startswith("lstm.weight"):
                # per-split slabs + one reduction pass: deterministic, so the two drivers must agree to the bit
                assert torch.equal(cl.grad[k], pl.grad[k]), k
            else:
                # split-K / column-sum ATOMICS (input layer, heads, biases): the fp32 summation order varies from run to run
                assert relerr(cl.grad[k], pl.grad[k]) < (1e-5 if it == 0 else 2e-3), (it, k, relerr(cl.grad[k], pl.grad[k]))
        gc, gp = cl.optimizer_step(), pl.optimizer_step()
        assert torch.allclose(gc, gp, rtol=1e-4)
        for k in pl.online.w:
            assert torch.allclose(cl.online.w[k], pl.online.w[k], rtol=0, atol=2e-5 * (it + 1)), (it, k)
        if it == 1:
            cl.sync_target_with_online()
            pl.sync_target_with_online()
    check_sync()
    cl.check_sync()


def test_bf16_observation_operands_give_the_same_bits_as_float32_inputs():
    """priv_s_bf16 (what hsad_env_bind_packed / the bit-field sampler hand over): a 0/1 observation is exact in bf16, so act()
    and the learner step must return the same bits as with the float32 tensor, minus the cast pass"""
    from hanabi_sad_amd.composite import CNet, CompositeAgent, CompositeLearner
    from hanabi_sad_amd.selfplay import init_weights
    from tests.test_r2d2_kernels_gpu import _rand_batch
    F, H, A, N = 838, 512, 21, 2048
    W, Wt = init_weights(F, H, A, 5, 1), init_weights(F, H, A, 5, 2)
    on, tg = CNet(W, DEV), CNet(Wt, DEV)
    assert on.Fp == 896
    g = torch.Generator(device="cpu").manual_seed(5)
    priv = (torch.rand(N, F, generator=g) < 0.15).float().to(DEV)
    p16 = torch.zeros(N, on.Fp, dtype=torch.bfloat16, device=DEV)
    p16[:, :F] = priv
    legal = (torch.rand(N, A, generator=g) < 0.5).float().to(DEV)
    legal[:, 0] = 1
    eps = torch.full((N,), 0.3, device=DEV)
    hid = {"h0": (torch.randn(2, N, H, generator=g) * 0.3).to(DEV), "c0": (torch.randn(2, N, H, generator=g) * 0.3).to(DEV)}
    r32, h32 = CompositeAgent(on, tg, 3, 0.999, seed=1).act({"priv_s": priv, "legal_move": legal, "eps": eps}, hid, with_q=True)
    r16, h16 = CompositeAgent(on, tg, 3, 0.999, seed=1).act({"priv_s_bf16": p16, "legal_move": legal, "eps": eps}, hid, with_q=True)
    for k in ("a", "greedy_a", "q_online_a", "q_target_greedy"):
        assert torch.equal(r32[k], r16[k]), k
    assert torch.equal(h32["h0"], h16["h0"]) and torch.equal(h32["c0"], h16["c0"])
    with pytest.raises(Exception):
        CompositeAgent(on, tg, 3, 0.999).act({"priv_s_bf16": p16[:, :F].contiguous(), "legal_move": legal, "eps": eps}, hid)

    T, B = 80, 128
    batch, weight = _rand_batch(T, B, F, A)
    batch["priv_s"] = (batch["priv_s"] > 0.8).float()
    b16 = dict(batch)
    del b16["priv_s"]
    b16["priv_s_bf16"] = torch.zeros(T, B, 1, 896, dtype=torch.bfloat16, device=DEV)
    b16["priv_s_bf16"][:, :, 0, :F] = batch["priv_s"]
    la = CompositeLearner(W, Wt, 3, 0.999, lr=1e-3, device=DEV)
    lb = CompositeLearner(W, Wt, 3, 0.999, lr=1e-3, device=DEV)
    l1, p1 = la.loss(batch, weight, 0.25)
    l2, p2 = lb.loss(b16, weight, 0.25)
    assert torch.equal(l1, l2) and torch.equal(p1, p2)
    for k in la.grad:
        if k.startswith("lstm.weight"):
            assert torch.equal(la.grad[k], lb.grad[k]), k
        else:
            assert relerr(la.grad[k], lb.grad[k]) < 1e-5, k
    la.check_sync()
    lb.check_sync()


def test_schedule_of_an_existing_learner_can_be_changed():
    """hsad_r2d2_learner_set_schedule after creation: hand-off buffers and counter blocks are sized for any chunk count (a learner
    created with 4 chunks and switched to 2 used to overrun its counter blocks: 884 ms updates that ended in the sticky time-out);
    the schedule only changes WHEN things run -- loss and priorities are bit-identical, no time-out"""
    from hanabi_sad_amd.composite import CompositeLearner
    from hanabi_sad_amd.selfplay import init_weights
    from tests.test_r2d2_kernels_gpu import _rand_batch
    F, H, A, T, B = 838, 512, 21, 80, 128
    W, Wt = init_weights(F, H, A, 5, 1), init_weights(F, H, A, 5, 2)
    batch, weight = _rand_batch(T, B, F, A)
    L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    L.set_fused(False)
    ref_loss, ref_prio = L.loss(batch, weight, 0.0)
    ref_g = {k: v.clone() for k, v in L.grad.items() if k.startswith("lstm.weight")}
    for chunks in (2, 8, 1, 5, 4):
        import ctypes as C
        from hanabi_sad_amd import _lib
        _lib.check(L.lib.hsad_r2d2_learner_set_schedule(L.h, chunks, 8))
        loss, prio = L.loss(batch, weight, 0.0)
        assert torch.equal(loss, ref_loss) and torch.equal(prio, ref_prio), chunks
        for k, v in ref_g.items():
            assert relerr(L.grad[k], v) < 1e-5, (chunks, k)
        L.check_sync()


def test_act_in_two_halves_equals_the_single_call():
    """hsad_r2d2_act(target = NULL, q_online_a) + hsad_r2d2_target_q == hsad_r2d2_act with both Q outputs, to the bit (fused-cell path
    with the carried bf16 state, and the small-batch path)"""
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.selfplay import init_weights
    F, H, A = 838, 512, 21
    W, Wt = init_weights(F, H, A, 5, 1), init_weights(F, H, A, 5, 2)
    on, tg = CNet(W, DEV), CNet(Wt, DEV)
    for N in (2048, 96):
        g = torch.Generator(device="cpu").manual_seed(N)
        priv = (torch.rand(N, F, generator=g) < 0.15).float().to(DEV)
        legal = (torch.rand(N, A, generator=g) < 0.5).float().to(DEV)
        legal[:, 0] = 1
        obs = {"priv_s": priv, "legal_move": legal, "eps": torch.full((N,), 0.3, device=DEV)}
        hid = {"h0": (torch.randn(2, N, H, generator=g) * 0.3).to(DEV), "c0": (torch.randn(2, N, H, generator=g) * 0.3).to(DEV)}
        one, two = CompositeAgent(on, tg, 3, 0.999, seed=1), CompositeAgent(on, tg, 3, 0.999, seed=1)
        for step in range(2):                      # second step: the state carries its bf16 copy
            r1, h1 = one.act(obs, hid if step == 0 else h1, with_q=True)
            hin = hid if step == 0 else h2
            r2, h2 = two.act(obs, hin, with_q=True, defer_target=True)
            assert r2["q_target_greedy"] is None
            tq = two.target_q(obs, hin, r2["greedy_a"])
            for k in ("a", "greedy_a", "q_online_a"):
                assert torch.equal(r1[k], r2[k]), (N, step, k)
            assert torch.equal(r1["q_target_greedy"], tq), (N, step)
            assert torch.equal(h1["h0"], h2["h0"]) and torch.equal(h1["c0"], h2["c0"])


def _expected_plan(flags, bchunks, n_cu, F, H, T, B, A=21, hand=5, layers=2, nfc=1, chunks=4, wgrad_split=8, num_player=1, grad=True):
    """What hsad_r2d2_learner_plan must report for a flag word of hsad_r2d2_learner_set_fused (bchunks: the last non-zero bits 8-15) at a
    shape on a device of n_cu CUs, from the documented conditions (include/hsad.h, DESIGN.md "Composite entry points") alone -- the library is
    not asked.  A stage of the fused BPTT launch needs its 16-workgroup groups on the chip: 2 (split) / 3 (projection) / 4 (sink) x H / 32
    workgroups per 32-row block; a fused forward launch needs a (net, row block)'s layers x H / 32 workgroups inside one of the 8 XCDs."""
    bit = lambda b: bool(flags >> b & 1)
    M, nrb, wpr = T * B, (B + 31) // 32, H // 32
    Mp, Fp, NH = -(-M // 64) * 64, -(-F // 64) * 64, A + 1 + 3 * hand
    pipe = layers == 2 and H in (256, 512) and B <= 512 and B % 8 == 0 and M % 64 == 0
    fwd_chunks = chunks if pipe else 1
    while fwd_chunks > 1 and (T % fwd_chunks or (T // fwd_chunks * B) % 64):
        fwd_chunks -= 1
    fits = []
    if bit(0) and T >= 2 and H in (256, 512) and B % 32 == 0 and T * B * H * 16 < 2 ** 32:
        fits = [(nn, g) for g in range(min(layers, 2), 0, -1) for nn in (2, 1) if g * wpr * ((nn * nrb + 7) // 8) <= n_cu // 8]
    nets, lay = fits[0] if fits else (0, 0)
    fwd_kind = 2 if nets else 1 if pipe else 0
    nbc = bchunks
    while nbc > 1 and (T % nbc or (T // nbc * B) % 64):
        nbc -= 1
    fused_bwd = pipe and bit(0) and not bit(1) and fwd_kind == 2 and B % 32 == 0 and 2 * wpr * ((nrb + 7) // 8) <= n_cu // 8
    split = proj = sink = dgt = group = chunk_input = False
    if fused_bwd:
        if 0 < (flags >> 16 & 0xff) < T:
            nbc = 2
        split = bit(3) and nrb * 2 * wpr <= n_cu
        proj = split and bit(4) and nrb * 3 * wpr <= n_cu
        sink = proj and bit(5) and nrb * 4 * wpr <= n_cu
        dgt = nbc == 1 and sink and not bit(6)
        group = dgt and nfc == 1 and not bit(7) and (4 * H) % 256 == 0 and H % 256 == 0 and Mp % 128 == 0 and Fp % 4 == 0
        chunk_input = nfc == 1 and nbc > 1 and M % 4 == 0 and H % 4 == 0 and wgrad_split > 1
    one = num_player == 1 and not bit(24) and M >= 128 and M % 128 == 0 and H % 16 == 0 and NH <= 64 and T <= 352
    e = dict(fwd_kind=fwd_kind, fwd_nets=nets, fwd_layers=lay, fwd_chunks=fwd_chunks, bwd_kind=2 if fused_bwd else 1 if pipe else 0,
             bptt_chunks=nbc if fused_bwd else fwd_chunks if pipe else 1, split=split, proj=proj, sink=sink, dgt_in_kernel=dgt, group=group,
             wide_requested=dgt and not bit(25), chunk_input=chunk_input, one_launch_heads=one,
             dO_in_loss_tail=one and grad and -(-NH // 64) * 64 == 64 and H % 32 == 0 and H <= (512 if T <= 128 else 256))
    return {k: int(v) for k, v in e.items()}


@pytest.mark.parametrize("F,H,T,B,pw", [(838, 512, 80, 128, 0.25), (838, 256, 24, 64, 0.0), (783, 512, 16, 256, 0.0)])
def test_fused_recurrences_equal_the_chunk_pipelined_schedule(F, H, T, B, pw):
    """default learner schedule -- hsad_lstm_forward_fused (projection inside the recurrence, both layers and both nets in one launch; B =
    256: one net per launch) and hsad_lstm_backward_fused (both layers in one launch, dO of the lower layer inside its recurrence; also
    in 2 time chunks with the weight gradients added up per chunk) -- vs the projection-GEMM + chunked-recurrence schedule of rounds 1-2:
    same operands, different fp32 summation orders -> agreement at the level of bf16 feedback noise; switching back and forth on a live
    learner reproduces each schedule's own bits.  What each mode RAN is read back (hsad_r2d2_learner_plan) and held to the plan the flag
    word and the shape resolve to on this device: a mode whose name promises a stage that the shape cannot hold (B = 256: 8 row blocks x
    3 groups x 16 workgroups = 384 > 256 CUs -- no projection, no sink stage, dG transposed behind the launch) still runs, as the degraded
    plan asserted here"""
    from hanabi_sad_amd.composite import CompositeLearner
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    A = 21
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    groups_fit = {k: (B + 31) // 32 * g * (H // 32) <= n_cu for k, g in (("split", 2), ("proj", 3), ("sink", 4))}
    bchunks = 1
    W, Wt = _rand_net(F, H, A, seed=13), _rand_net(F, H, A, seed=14)
    batch, weight = _rand_batch(T, B, F, A)
    L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    modes = {"fused": 1 | (1 << 8), "fused fwd + chunked bwd": 3, "fused, BPTT in 2 chunks": 1 | (2 << 8), "chunked": 0,   # (bits 8-15 = BPTT chunks; 0 keeps the last setting)
             "fused, split placement": 9 | (1 << 8), "fused, split placement, 2 chunks": 9 | (2 << 8),
             "fused, split placement + projection stage": 25 | (1 << 8), "fused, split + projection, 2 chunks": 25 | (2 << 8),
             "fused, split + projection + sink stage": 57 | (1 << 8), "fused, split + projection + sink, 2 chunks": 57 | (2 << 8),
             # (bit 25 off = default: the four-stage single-chunk launch in the 16-row x 64-unit blocking where the shape allows -- H = 512, B <= 128)
             "fused, split + projection + sink stage, 32 x 32 blocks": 57 | (1 << 8) | (1 << 25)}
    res = {}
    for rep in range(2):
        for name, flags in modes.items():
            L.set_fused(flags)
            loss, prio = L.loss(batch, weight, pw)
            torch.cuda.synchronize()
            bchunks = (flags >> 8 & 0xff) or bchunks
            plan = L.plan()
            assert plan == _expected_plan(flags, bchunks, n_cu, F, H, T, B), (name, plan)
            # the stages the mode's name promises: on when every group up to theirs fits the chip, else explicitly off
            assert plan["split"] == int("split" in name and groups_fit["split"]), (name, plan)
            assert plan["proj"] == int("projection" in name and groups_fit["split"] and groups_fit["proj"]), (name, plan)
            assert plan["sink"] == int("sink" in name and all(groups_fit.values())), (name, plan)
            assert plan["dgt_in_kernel"] == int(plan["sink"] and "2 chunks" not in name), (name, plan)
            got = (loss.clone(), prio.clone(), {k: v.clone() for k, v in L.grad.items()})
            if name in res:      # second visit: bit-identical to the first (counter blocks, ping-pong state survive the switch)
                assert torch.equal(got[0], res[name][0]) and torch.equal(got[1], res[name][1]), name
                for k in got[2]:
                    if k.startswith("lstm.weight"):
                        assert torch.equal(got[2][k], res[name][2][k]), (name, k)
            res[name] = got
    L.check_sync()
    lc, pc, gc = res["chunked"]
    for name in modes:
        lf, pf, gf = res[name]
        d = ((pf - pc).abs() / (1 + pc.abs())).flatten()
        assert float(torch.quantile(d, 0.999)) < 5e-3 and float(d.max()) < 1.0, name   # one near-tie greedy flip moves a priority by O(0.1)
        assert float(torch.quantile(((lf - lc).abs() / (1 + lc.abs())), 0.9)) < 1e-2, name
        for k in gc:
            assert relerr(gf[k], gc[k]) < 4e-3, (name, k, relerr(gf[k], gc[k]))
    # forward fused either way: the two BPTT schedules see the same activations -> their gradients agree much more closely
    for k in gc:
        assert relerr(res["fused"][2][k], res["fused fwd + chunked bwd"][2][k]) < 1e-3, k
        assert relerr(res["fused"][2][k], res["fused, BPTT in 2 chunks"][2][k]) < 1e-4, k
    # split placement (the two layers of a row block on different XCDs, second written-through hand-off copy): the same arithmetic in the
    # same order -> loss, priorities and the deterministic LSTM weight gradients are the SAME BITS as with both layers on one XCD
    # projection stage: dO of the lower layer is summed over the K split separately from the layer's own stream -- another fp32 order
    # (sink stage: d x of the input layer summed over the K split per wave instead of in the GEMM's k order, then rounded to bf16)
    for a, b in (("fused", "fused, split placement + projection stage"), ("fused, BPTT in 2 chunks", "fused, split + projection, 2 chunks"),
                 ("fused", "fused, split + projection + sink stage"), ("fused, BPTT in 2 chunks", "fused, split + projection + sink, 2 chunks")):
        assert torch.equal(res[a][0], res[b][0]) and torch.equal(res[a][1], res[b][1]), b
        for k in gc:
            assert relerr(res[a][2][k], res[b][2][k]) < 3e-4, (b, k, relerr(res[a][2][k], res[b][2][k]))    # (bf16 roundings of dG flip)
    # round 6: the 16-row x 64-unit blocking of the four-stage launch keeps every summation order of the 32 x 32 one: same loss, priorities,
    # LSTM and input-layer weight gradients bit for bit; the bias gradients are atomics over other partial sums (16-row instead of 32-row)
    a, b = "fused, split + projection + sink stage, 32 x 32 blocks", "fused, split + projection + sink stage"
    assert torch.equal(res[a][0], res[b][0]) and torch.equal(res[a][1], res[b][1]), b
    for k in gc:
        if k.startswith("lstm.weight"):
            assert torch.equal(res[a][2][k], res[b][2][k]), (b, k, relerr(res[a][2][k], res[b][2][k]))
        else:       # (atomics: bias gradients, split-K sums of the other layers -- the heads' gradients do not pass through the BPTT at all)
            assert relerr(res[a][2][k], res[b][2][k]) < (3e-4 if "bias" in k else 1e-5), (b, k, relerr(res[a][2][k], res[b][2][k]))
    for a, b in (("fused", "fused, split placement"), ("fused, BPTT in 2 chunks", "fused, split placement, 2 chunks")):
        assert torch.equal(res[a][0], res[b][0]) and torch.equal(res[a][1], res[b][1]), b
        for k in gc:
            if k.startswith("lstm.weight"):
                assert torch.equal(res[a][2][k], res[b][2][k]), (b, k)
            else:   # (atomics: the LSTM bias gradients are four per-row-block partial sums added in arrival order -- they cancel heavily)
                assert relerr(res[a][2][k], res[b][2][k]) < (3e-4 if k.startswith("lstm.bias") else 1e-5), (b, k, relerr(res[a][2][k], res[b][2][k]))


PLAN_SHAPES = [   # (H, B, T, lstm layers, fc layers, flag words in turn; None = the default word)
    (512, 128, 4, 2, 1, (None,)),                      # 256 CUs: every stage on, wide blocks asked for, grouped weight gradients, forward {2, 2}
    (512, 256, 4, 2, 1, (None,)),                      # 8 row blocks: split at exactly 256 workgroups, no projection -> no dgt_in_kernel, forward {1, 2}
    (256, 32, 4, 2, 1, (None,)),                       # all stages; the wide launch is for H = 512 (asked for, the launcher keeps 32 x 32)
    (256, 32, 4, 2, 1, (1 | (2 << 8), 0)),             # two BPTT chunks with chunk_input; then the pipelined forward and backward
    (128, 16, 3, 2, 1, (None,)),                       # plain forward and backward
    (256, 32, 1, 2, 1, (None,)),                       # one step: no fused forward
    (256, 32, 4, 3, 1, (None,)),                       # three LSTM layers: no pipeline, no grouped launch
    (256, 32, 4, 2, 2, (None,)),                       # two fc layers: fused BPTT without the grouped launch
]


@pytest.mark.parametrize("H,B,T,nl,nfc,words", PLAN_SHAPES)
def test_learner_plan_at_the_smallest_shapes_of_every_branch(H, B, T, nl, nfc, words):
    """plan_update at the smallest shape of each of its branches (A = 21, F = 128): one update per flag word, the plan read back and held to
    _expected_plan for this device's CU count; loss and priorities finite, a second evaluation the same bits, no timeout word set"""
    from hanabi_sad_amd.composite import CompositeLearner
    from hanabi_sad_amd.selfplay import init_weights
    from tests.test_r2d2_kernels_gpu import _rand_batch
    F, A = 128, 21
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    W, Wt = init_weights(F, H, A, 5, 51, nl, nfc), init_weights(F, H, A, 5, 52, nl, nfc)
    batch, weight = _rand_batch(T, B, F, A, seed=1000 * B + T)
    L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    bchunks = 1
    for flags in words:
        if flags is None:
            flags = CompositeLearner.FUSED_DEFAULT
        else:
            L.set_fused(flags)
        bchunks = (flags >> 8 & 0xff) or bchunks
        want = _expected_plan(flags, bchunks, n_cu, F, H, T, B, layers=nl, nfc=nfc)
        runs = []
        for rep in range(2):
            loss, prio = L.loss(batch, weight, 0.25)
            assert L.plan() == want, (flags, L.plan(), want)
            runs.append((loss.clone(), prio.clone()))
        L.check_sync()
        assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all(), flags
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), flags


@pytest.mark.parametrize("T", [2, 3, 5, 9, 33])
def test_short_sequences_run_the_persistent_launches_with_narrower_counter_strides(T):
    """round 6: the exchange counters of both persistent launches are one running word per row block, 128 bytes apart -- when the sequence
    is short the region (sized for one word per step) only holds a narrower stride (2 words at T = 2).  The 16-row x 64-unit BPTT launch
    against the 32 x 32 one (own counter layout, a word per step) on the same forward: same loss, priorities and LSTM weight gradients bit
    for bit, twice each (the second visit reuses the ping-pong counter blocks), and no timeout word set."""
    _wide_against_32x32(128, T, with_chunked=True)


@pytest.mark.parametrize("B,T", [(32, 2), (32, 80), (64, 17), (96, 2), (96, 80)])
def test_wide_bptt_at_small_batches_gives_the_bits_of_the_32x32_launch(B, T):
    """the wide launch takes every B that is a multiple of 32 up to 128 (selfplay --batchsize 32 / 64 / 96, VDN at batchsize 16 - 48): B / 16
    row blocks on as many XCDs -- the other XCDs' workgroups return at once --, bias_finish adds nrb partial rows and the counter stride
    shrinks with T * B / 32.  Same comparison as above; a 1 us stall hook on each launch proves which kernel ran.  (The four-stage launch
    needs T * B to be a multiple of 64: at B = 96 only even T reach it.)"""
    _wide_against_32x32(B, T, with_chunked=False)


@pytest.mark.parametrize("B,T", [(96, 3), (32, 5)])
def test_odd_row_blocks_and_odd_sequence_lengths_keep_the_counter_blocks_aligned(B, T):
    """the learner's counter blocks are nrb (T + 2) + 4 words: with an odd number of 32-row blocks and an odd T that is odd, and the next
    block -- whose first words a launch adds to with 64-bit atomics (the group handshake) -- lost its 8-byte alignment; the fused forward
    faulted at B = 96, T = 3.  Every block starts 16-byte aligned now: two updates, finite values, the same loss and priorities, no timeout.
    (T * B is no multiple of 64 here: the BPTT runs outside the four-stage launch and adds some gradients with float atomics.)"""
    from hanabi_sad_amd.composite import CompositeLearner
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    F, A, H = 838, 21, 512
    W, Wt = _rand_net(F, H, A, seed=45), _rand_net(F, H, A, seed=46)
    batch, weight = _rand_batch(T, B, F, A, seed=1000 * B + T)
    L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    res = []
    for rep in range(2):
        loss, prio = L.loss(batch, weight, 0.25)
        res.append([loss.clone(), prio.clone()] + [v.clone() for v in L.grad.values()])
    L.check_sync()
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.isfinite(a).all(), i
        assert torch.equal(a, b) if i < 2 else relerr(a, b) < 1e-5, (i, relerr(a, b))


def _wide_against_32x32(B, T, with_chunked):
    import ctypes as C
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.composite import CompositeLearner
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    lib = _lib.load_library()
    F, A, H = 838, 21, 512
    W, Wt = _rand_net(F, H, A, seed=41), _rand_net(F, H, A, seed=42)
    batch, weight = _rand_batch(T, B, F, A, seed=T if B == 128 else 1000 * B + T)
    L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    schedules = [("wide", 57 | (1 << 8), 1), ("32 x 32", 57 | (1 << 8) | (1 << 25), 2)] + ([("chunked", 0, -1)] if with_chunked else [])
    res = {}
    for rep in range(2):
        for name, flags, kernel in schedules:      # kernel: HSAD_STALL_BPTT_WIDE / HSAD_STALL_BPTT_32
            L.set_fused(flags)
            if kernel >= 0 and rep == 0:
                _lib.check(lib.hsad_lstm_debug_stall_fired(None, 1))
                _lib.check(lib.hsad_lstm_debug_stall(kernel, 0, 0, 0, 0, 1))
            try:
                loss, prio = L.loss(batch, weight, 0.25)
            finally:
                lib.hsad_lstm_debug_stall(-1, 0, 0, 0, 0, 0)
            torch.cuda.synchronize()
            if kernel >= 0 and rep == 0:
                n = C.c_uint64(0)
                _lib.check(lib.hsad_lstm_debug_stall_fired(C.byref(n), 1))
                assert n.value == 1, (B, T, name, "the launch did not run", n.value)
            got = (loss.clone(), prio.clone(), {k: v.clone() for k, v in L.grad.items()})
            if name in res:
                assert torch.equal(got[0], res[name][0]) and torch.equal(got[1], res[name][1]), (B, T, name)
                for k in got[2]:
                    if k.startswith("lstm.weight"):
                        assert torch.equal(got[2][k], res[name][2][k]), (B, T, name, k)
            res[name] = got
    L.check_sync()
    (lw, pw_, gw), (l3, p3, g3) = res["wide"], res["32 x 32"]
    assert torch.equal(lw, l3) and torch.equal(pw_, p3), (B, T)
    for k in gw:
        if k.startswith("lstm.weight"):
            assert torch.equal(gw[k], g3[k]), (B, T, k, relerr(gw[k], g3[k]))
        assert relerr(gw[k], g3[k]) < 3e-4, (B, T, k, relerr(gw[k], g3[k]))
        if with_chunked:
            assert relerr(gw[k], res["chunked"][2][k]) < 6e-3, (B, T, k, relerr(gw[k], res["chunked"][2][k]))     # another schedule: fp32 summation orders differ


def test_fused_recurrences_soak_every_evaluation_gives_the_same_bits():
    """stress target for the counter / hand-off protocols of the persistent fused launches (forward: 4 recurrences x 80 steps, BPTT: 2 x 80):
    a stale tile, a counter read too early or a lost wake-up changes bits (or trips the sticky timeout flag).  360 evaluations of the full-size
    update on the same weights and batch -- default placement, split placement, two time chunks, and the cross-XCD protocol forced on
    co-located groups -- must ALL reproduce the first evaluation's loss, priorities and (deterministic) LSTM weight gradients exactly."""
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.composite import CompositeLearner
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    lib = _lib.load_library()
    F, A, H, T, B = 838, 21, 512, 80, 128
    W, Wt = _rand_net(F, H, A, seed=21), _rand_net(F, H, A, seed=22)
    batch, weight = _rand_batch(T, B, F, A, seed=5)
    L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    ref_lp, ref_g = None, {}          # loss / priorities: one reference for everything; weight gradients: per chunk count / stage layout (partial
    try:                              # sums are added up in another order)
        for flags, cross, reps in ((1 | (1 << 8), 0, 150), (9 | (1 << 8), 0, 80), (9 | (2 << 8), 0, 50), (1 | (1 << 8), 1, 40), (9 | (1 << 8), 1, 40),
                                   (25 | (1 << 8), 0, 60), (57 | (1 << 8), 0, 120), (57 | (1 << 8), 1, 40),
                                   (57 | (1 << 8) | (1 << 25), 0, 40)):      # (bit 25: the 32 x 32 blocking of the four-stage launch -- same bits)
            _lib.check(lib.hsad_lstm_set_exchange_mode(cross))
            L.set_fused(flags)
            chunks = ((flags >> 8) & 0xff) + 100 * ((flags >> 4) & 3)      # (the projection / sink stages sum in another order)
            bad = torch.zeros((), dtype=torch.int64, device=DEV)
            for it in range(reps):
                loss, prio = L.loss(batch, weight, 0.25)
                got_lp, got_g = (loss, prio), (L.grad["lstm.weight_hh_l0"], L.grad["lstm.weight_ih_l1"])
                if ref_lp is None:
                    ref_lp = tuple(t.clone() for t in got_lp)
                if chunks not in ref_g:
                    ref_g[chunks] = tuple(t.clone() for t in got_g)
                # every evaluation is compared on the device; the host looks once per configuration
                for a, b in zip(got_lp + got_g, ref_lp + ref_g[chunks]):
                    bad += (a != b).any()
            assert int(bad) == 0, (hex(flags), cross)
    finally:
        lib.hsad_lstm_set_exchange_mode(0)
    L.check_sync()


def test_fused_recurrences_next_to_foreign_work_on_another_stream():
    """the persistent fused launches need every one of their workgroups resident (the four-stage BPTT launch: one per CU).  Foreign kernels on
    another stream -- what the rollout thread of the drop-in driver, or any co-tenant of the GPU, amounts to -- may hold CUs when a launch
    starts: its workgroups then arrive late, the others spin (bounded) and nothing may change but the time.  30 evaluations next to a
    stream of large matmuls: identical bits to the quiet evaluation, no sticky timeout."""
    from hanabi_sad_amd.composite import CompositeLearner
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    F, A, H, T, B = 838, 21, 512, 80, 128
    W, Wt = _rand_net(F, H, A, seed=31), _rand_net(F, H, A, seed=32)
    batch, weight = _rand_batch(T, B, F, A, seed=6)
    L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    loss, prio = L.loss(batch, weight, 0.25)
    ref = (loss.clone(), prio.clone(), L.grad["lstm.weight_hh_l0"].clone(), L.grad["lstm.weight_ih_l1"].clone())
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    a = torch.randn(8192, 8192, device=DEV, dtype=torch.bfloat16)
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for it in range(30):
        with torch.cuda.stream(side):
            for _ in range(3):
                a @ a                      # ~1 ms of full-chip work per launch, in flight while the learner's launches are issued
        loss, prio = L.loss(batch, weight, 0.25)
        for x, y in zip((loss, prio, L.grad["lstm.weight_hh_l0"], L.grad["lstm.weight_ih_l1"]), ref):
            bad += (x != y).any()
    torch.cuda.synchronize()
    assert int(bad) == 0
    L.check_sync()


@pytest.mark.slow          # (ten seconds by construction; the soak and the foreign-work tests above stay in the default set)
@pytest.mark.timeout(180)
def test_fused_recurrences_stress_ten_seconds_of_randomly_timed_foreign_kernels():
    """the spin protocols of the persistent fused launches (all-or-nothing co-residency, bounded spins, sticky timeout)
    under a co-tenant that is NOT phase-locked to them: a host thread issues full-chip kernels of random kind (8192^2 matmuls ~1 ms, 1 GB
    fills, bursts of small launches) on two other streams at random intervals for >= 10 s while full-size loss evaluations (forward
    launch: 256 workgroups x 80 steps, four-stage BPTT launch: 256 x 80) run back to back.  Every evaluation must reproduce the quiet
    evaluation's loss, priorities and LSTM weight gradients bit for bit, and hsad_lstm_sync_timed_out() must stay 0."""
    import random
    import threading
    import time
    from hanabi_sad_amd.composite import CompositeLearner
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    F, A, H, T, B = 838, 21, 512, 80, 128
    W, Wt = _rand_net(F, H, A, seed=41), _rand_net(F, H, A, seed=42)
    batch, weight = _rand_batch(T, B, F, A, seed=7)
    L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    loss, prio = L.loss(batch, weight, 0.25)
    ref = (loss.clone(), prio.clone(), L.grad["lstm.weight_hh_l0"].clone(), L.grad["lstm.weight_ih_l1"].clone())
    torch.cuda.synchronize()
    stop, issued = threading.Event(), [0]

    def foreign():
        rnd = random.Random(1234)
        streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
        a = torch.randn(8192, 8192, device=DEV, dtype=torch.bfloat16)
        big = torch.empty(1 << 28, device=DEV)                      # 1 GiB
        small = torch.zeros(4096, device=DEV)
        while not stop.is_set():
            with torch.cuda.stream(streams[rnd.randrange(2)]):
                kind = rnd.randrange(4)
                if kind == 0:
                    for _ in range(rnd.randrange(1, 4)):
                        a @ a
                elif kind == 1:
                    big.fill_(rnd.random())
                elif kind == 2:
                    for _ in range(rnd.randrange(5, 40)):
                        small.add_(1.0)
                else:
                    (a[:2048] @ a).relu_()
            issued[0] += 1
            time.sleep(rnd.random() * 0.003)
            if issued[0] % 64 == 0:
                for st in streams:
                    st.synchronize()                                 # (bounds the queue depth of the foreign streams)

    th = threading.Thread(target=foreign, daemon=True)
    th.start()
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    t0, evals = time.time(), 0
    try:
        while time.time() - t0 < 10.5:
            for _ in range(20):
                loss, prio = L.loss(batch, weight, 0.25)
                for x, y in zip((loss, prio, L.grad["lstm.weight_hh_l0"], L.grad["lstm.weight_ih_l1"]), ref):
                    bad += (x != y).any()
                evals += 1
            torch.cuda.synchronize()
    finally:
        stop.set()
        th.join()
    torch.cuda.synchronize()
    assert int(bad) == 0 and evals >= 200 and issued[0] >= 500, (int(bad), evals, issued[0])
    L.check_sync()                                                   # hsad_lstm_sync_timed_out() == 0


def test_a_timed_out_recurrence_fails_the_next_call_of_any_driver():
    """a persistent recurrence that gives up waiting leaves garbage, and only the repo's own driver polled the flag per
    epoch.  Now every update reports its sticky words to a pinned host word and hsad_r2d2_loss_fwd / _loss_bwd / _optimizer_step look at it
    first (no synchronisation): with a word set the way a timed-out launch sets it (fault-injection hook), the update in flight still
    returns -- its kernels are already enqueued -- and the NEXT call raises, also through the Python-orchestrated learner's own check."""
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.composite import CompositeLearner
    from hanabi_sad_amd import r2d2
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    F, A, H, T, B = 838, 21, 512, 16, 128
    W, Wt = _rand_net(F, H, A, seed=3), _rand_net(F, H, A, seed=4)
    batch, weight = _rand_batch(T, B, F, A)
    cl = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    cl.loss(batch, weight, 0.0)
    cl.optimizer_step()
    torch.cuda.synchronize()
    _lib.check(cl.lib.hsad_r2d2_learner_inject_timeout(cl.h, 1))
    cl.loss(batch, weight, 0.0)          # enqueued before anybody could know; its gather kernel reports the word
    torch.cuda.synchronize()
    with pytest.raises(_lib.HsadError, match="gave up waiting"):
        cl.optimizer_step()
    with pytest.raises(_lib.HsadError, match="gave up waiting"):
        cl.loss(batch, weight, 0.0)
    _lib.check(cl.lib.hsad_r2d2_learner_inject_timeout(cl.h, 0))
    cl.loss(batch, weight, 0.0)
    cl.optimizer_step()
    cl.check_sync()
    # the Python-orchestrated schedule: the same protocol over its torch-owned counter blocks
    pl = r2d2.R2D2Learner(W, Wt, 3, 0.999, device=DEV)
    pl.loss(batch, weight, 0.0)
    torch.cuda.synchronize()
    key, blk = next((k, b) for k, b in r2d2._SYNC.items() if k[0] == str(torch.device(DEV)) or k[0] == DEV)
    blk[key[3]] = 1
    try:
        pl.loss(batch, weight, 0.0)
        torch.cuda.synchronize()
        with pytest.raises(_lib.HsadError, match="timed out"):
            pl.loss(batch, weight, 0.0)
    finally:
        blk[key[3]] = 0
        r2d2.gather_timeouts(torch.device(DEV))
        torch.cuda.synchronize()
    pl.loss(batch, weight, 0.0)


@pytest.mark.parametrize("F,H,T,B,pw", [(838, 512, 80, 128, 0.25), (838, 512, 80, 128, 0.0), (838, 256, 24, 64, 0.25), (783, 512, 17, 128, 0.0)])
def test_the_two_launch_head_chain_gives_the_bits_of_the_four_launch_one(F, H, T, B, pw):
    """Between the two recurrences of an update: heads of both nets + the online dueling head in ONE launch (heads_q_kernel: the top layer's
    rows straight into MFMA fragments, q_head_kernel's row arithmetic on the rows a wave holds) and the loss tail with d loss / d o formed
    inside (loss_tail_kernel's MFMA section) -- against the GEMM pair -> q_head -> loss tail -> dO GEMM chain (set_fused bit 24).  Same MFMA,
    same k order, the same scalar arithmetic per row: loss, priorities, the LSTM's and the input layer's weight gradients the same bits (the float-atomic
    sums -- biases, the head layers' split-K products -- compared at 1e-5)."""
    from hanabi_sad_amd.composite import CompositeLearner
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    A = 21
    W, Wt = _rand_net(F, H, A, seed=31), _rand_net(F, H, A, seed=32)
    batch, weight = _rand_batch(T, B, F, A, seed=9)
    L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
    res = {}
    for rep in range(2):
        for name, flags in (("two launches", CompositeLearner.FUSED_DEFAULT), ("four launches", CompositeLearner.FUSED_DEFAULT | (1 << 24))):
            L.set_fused(flags)
            loss, prio = L.loss(batch, weight, pw)
            torch.cuda.synchronize()
            got = (loss.clone(), prio.clone(), {k: v.clone() for k, v in L.grad.items()})
            if name in res:
                assert torch.equal(got[0], res[name][0]) and torch.equal(got[1], res[name][1]), name
            res[name] = got
    L.check_sync()
    (l2, p2, g2), (l4, p4, g4) = res["two launches"], res["four launches"]
    assert torch.equal(l2, l4) and torch.equal(p2, p4)
    for k in g4:
        if k.startswith("lstm.weight") or k.startswith("net."):       # deterministic sums downstream of d loss / d o
            if "bias" not in k:
                assert torch.equal(g2[k], g4[k]), (k, relerr(g2[k], g4[k]))
        assert relerr(g2[k], g4[k]) < 1e-5, (k, relerr(g2[k], g4[k]))     # (bias sums and the head layers' split-K sums are float atomics)


def test_every_gradient_of_an_update_is_the_same_bits_run_to_run():
    """round 6: no float atomics left in the default update at the baseline shape -- the BPTT launch adds its per-row-block bias partial sums in
    row-block order (ticket), the heads' weight gradient is slabs + an ordered sum, their bias gradient one workgroup per column block, the
    five big weight gradients were slabs already.  Eight evaluations of the same update (a second learner object in between): loss, priorities
    and EVERY gradient tensor bit for bit."""
    from hanabi_sad_amd.composite import CompositeLearner
    from tests.test_r2d2_kernels_gpu import _rand_batch, _rand_net
    F, A, H, T, B = 838, 21, 512, 80, 128
    W, Wt = _rand_net(F, H, A, seed=31), _rand_net(F, H, A, seed=32)
    batch, weight = _rand_batch(T, B, F, A, seed=9)
    ref = None
    for who in range(2):
        L = CompositeLearner(W, Wt, 3, 0.999, device=DEV)
        for it in range(4):
            loss, prio = L.loss(batch, weight, 0.25)
            torch.cuda.synchronize()
            got = {"loss": loss.clone(), "priority": prio.clone()}
            got.update({k: v.clone() for k, v in L.grad.items()})
            if ref is None:
                ref = got
            for k in ref:
                assert torch.equal(got[k], ref[k]), (who, it, k, relerr(got[k], ref[k]))
        L.check_sync()
        L.close()
