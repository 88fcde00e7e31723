"""GPU: belief.BeliefHead end to end on tiny shapes -- a 64-unit trunk from init_weights, 16 games recorded from the `piers` bot, T the
rules' capacity: a fresh head scores the exact belief bit for bit, the weight and bias gradients are the float64 products of the same
o16 and dlogits within the bf16 GEMM's bound (tests/gemm_group.rounded_error's: (K + slabs) 2^-23 |A| |B|^T), two identical runs
give identical bits, 20 full-batch Adam steps bring the training NLL per card strictly below the exact belief's (the loss is convex
in the head and starts there), sample() after training yields only consistent hands, and a saved head reproduces the logits."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
GAMES, H, SEED = 16, 64, 77


@pytest.fixture(scope="module")
def setup():
    from hanabi_sad_amd import game_record as gr
    from hanabi_sad_amd.belief import BeliefHead
    from hanabi_sad_amd.clone import check_rules, records_from_teacher, sequences_from_records
    from hanabi_sad_amd.eval import env_dims
    from hanabi_sad_amd.rulebot import PRESETS
    from hanabi_sad_amd.selfplay import init_weights
    records = records_from_teacher([PRESETS["piers"]], GAMES, SEED, True, device=DEV, names=["piers"])
    r = check_rules(records)
    data = sequences_from_records(records, True, device=DEV, knowledge=True)
    assert data.T == gr.capacity(r) and data.n_rows == GAMES * r["players"]
    F, A = env_dims(r["players"], r["hand_size"], True)
    W = init_weights(F, H, A, r["hand_size"], 3)
    head = BeliefHead(W, r["hand_size"], DEV, lr=0.05)
    o16 = head.features(data.priv_s_bf16)
    batch = dict(o16=o16, pool=data.pool, compat=data.compat, cards=data.cards, seq_len=data.seq_len)
    return dict(records=records, data=data, W=W, head=head, batch=batch, weight=torch.ones(data.n_rows, device=DEV), rules=r)


def fresh(s):
    from hanabi_sad_amd.belief import BeliefHead
    return BeliefHead(s["W"], s["rules"]["hand_size"], DEV, lr=0.05)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def test_the_dataset_carries_the_knowledge_of_every_kept_step(setup):
    from tests import belief_head_ref as R
    d = setup["data"]
    T, N, Hs = d.T, d.n_rows, setup["rules"]["hand_size"]
    assert d.pool.shape == (T, N) and d.compat.shape == d.cards.shape == (T, N, Hs)
    valid = torch.arange(T, device=DEV).view(-1, 1) < d.seq_len.view(1, -1)
    assert not bool(d.pool[~valid].any()) and not bool(d.compat[~valid].any()) and bool((d.cards[~valid] == -1).all())
    cards, compat, pool = d.cards.cpu().numpy(), d.compat.cpu().numpy(), d.pool.cpu().numpy()
    v = valid.cpu().numpy()
    assert (cards[v][:, 0] >= 0).all()      # a live seat holds a card
    for t, n in zip(*np.nonzero(v)):
        if (t * 31 + n) % 37:      # a sample of the rows
            continue
        q = R.unpack_pool(pool[t, n])
        for i, c in enumerate(cards[t, n]):
            if c >= 0:
                assert (compat[t, n, i] >> c) & 1 and q[c] >= 1, (t, n, i)
    # the default leaves every existing result untouched
    from hanabi_sad_amd.clone import sequences_from_records
    plain = sequences_from_records(setup["records"], True, device=DEV)
    assert plain.pool is None and plain.compat is None and plain.cards is None
    assert torch.equal(plain.priv_s_bf16, d.priv_s_bf16) and torch.equal(plain.a, d.a) and torch.equal(plain.legal_move, d.legal_move)


def test_a_fresh_head_is_the_exact_belief(setup):
    head = fresh(setup)
    nll, st = head.loss(setup["batch"], setup["weight"], compute_grad=False)
    assert torch.equal(bits(st["nll"]), bits(st["nll0"])) and torch.equal(st["hits"], st["hits0"])
    assert int(st["bad"].sum()) == 0 and int(st["cards"].sum()) > 100 and float(st["nll0"].sum()) > 0


def test_the_gradients_are_the_float64_products_and_the_same_bits_run_to_run(setup):
    s = setup
    head = fresh(s)
    gen = torch.Generator().manual_seed(1)
    head.weight.copy_((torch.randn(head.NZ, H, generator=gen) * 0.3).to(DEV))
    head.bias.copy_((torch.randn(head.NZ, generator=gen) * 0.3).to(DEV))
    head.refresh()
    weight = (torch.rand(s["data"].n_rows, generator=gen) + 0.5).to(DEV)
    _, st = head.loss(s["batch"], weight)
    T, B = s["data"].T, s["data"].n_rows
    M = T * B
    k = head._buffers(T, B)
    dz = k["dz"][:M].double().cpu()
    o = s["batch"]["o16"].reshape(M, H).double().cpu()
    gw, gb = head.gw.double().cpu(), head.gb.double().cpu()
    want_w = dz.t() @ o
    bound_w = (k["Mp"] + head.wgrad_split) * 2.0 ** -23 * (dz.abs().t() @ o.abs()) + 2.0 ** -126
    assert float(((gw - want_w).abs() - bound_w).max()) <= 0.0
    assert float(want_w[:head.NZ].abs().max()) > 1e-3 and not bool(gw[head.NZ:].any())
    want_b = dz.sum(0)
    bound_b = (M + 2) * 2.0 ** -24 * dz.abs().sum(0) + 2.0 ** -126
    assert float(((gb - want_b).abs() - bound_b).max()) <= 0.0 and float(want_b.abs().max()) > 1e-3
    # the logits the tail saw are the head's GEMM of the same o16
    z = head.logits(s["batch"]["o16"].reshape(M, H)).double().cpu()
    zw = o @ head.w16.double().cpu().t() + head.b32.double().cpu()
    assert float((z - zw).abs().max()) <= 1e-3
    # a second head, the same calls: the same bits in every output and in the update
    other = fresh(s)
    other.weight.copy_(head.weight)
    other.bias.copy_(head.bias)
    other.refresh()
    _, st2 = other.loss(s["batch"], weight)
    for name in st:
        assert torch.equal(bits(st[name]), bits(st2[name])), name
    assert torch.equal(bits(head.gflat), bits(other.gflat))
    head.step()
    other.step()
    assert torch.equal(bits(head.flat), bits(other.flat)) and torch.equal(bits(head.w16), bits(other.w16))


def test_training_lowers_the_nll_below_the_exact_belief_and_samples_stay_consistent(setup, tmp_path):
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.belief import BeliefHead
    s = setup
    head = fresh(s)
    for _ in range(20):
        head.loss(s["batch"], s["weight"])
        head.step()
    _, st = head.loss(s["batch"], s["weight"], compute_grad=False)
    pc = st.per_card()
    print("training NLL per card after 20 steps: %.4f, exact belief %.4f; top-1 %.4f vs %.4f" % (pc["nll"], pc["nll0"], pc["top1"], pc["top1_0"]))
    assert pc["bad"] == 0 and pc["nll"] < pc["nll0"]
    # save / load: the same logits
    path = str(tmp_path / "belief.pthw")
    head.save(path)
    again = BeliefHead(s["W"], s["rules"]["hand_size"], DEV).load(path)
    o = s["batch"]["o16"][:3].reshape(-1, H)
    assert torch.equal(bits(head.logits(o)), bits(again.logits(o)))
    # sample() on live games: every hand consistent (the exact count of the result is >= 1, the deck is the pool less the hand)
    G = 70
    env = BatchedHanabiEnv(G, seed=5, eps_list=(0.0,), sad=True, device=DEV)
    env.rollout_random(12, 3)
    q = env.query()
    live = ((q[:, 14] == 1) & (q[:, 0] == 0))
    viewer = (torch.arange(G, device=DEV) % 2).to(torch.int32)
    pool0, _, cards0 = env.hand_knowledge()
    rows = torch.arange(G, device=DEV) * 2 + viewer.long()
    o16 = head.features(env.priv_s.view(1, G * 2, -1).float())[0][rows].contiguous()
    status, logp = head.sample(env, viewer, o16, torch.arange(G, dtype=torch.int64), 11)
    env.check_errors()
    assert torch.equal(status.bool(), live) and bool((logp[live] < 0).all())
    assert bool((env.hand_belief(viewer).total[live] >= 1).all())
    pool1, _, cards1 = env.hand_knowledge()
    idx = torch.arange(G, device=DEV)
    assert torch.equal(pool1[idx, viewer.long()], pool0[idx, viewer.long()])      # deck + hand is what it was: the hand came out of the pool
    assert int((cards1[idx, viewer.long()] != cards0[idx, viewer.long()]).any(1).sum()) >= 10
    env.close()
