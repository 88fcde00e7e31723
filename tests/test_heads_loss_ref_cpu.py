"""The float64 references of tests/heads_loss_ref.py checked on the CPU, before any kernel is held to them:
the hand-written gradient formulas against float64 autograd of the composite objective (1e-12), and the statistics of the restated
exploration hash over 2^20 (row, counter) pairs, each inside five standard deviations of its binomial / chi-square law."""
import math

import numpy as np
import pytest
import torch

from tests import heads_loss_ref as R

N_PAIRS = 1 << 20


def _batch(T, B, A, NP, seed):
    g = torch.Generator().manual_seed(seed)
    M = T * B
    heads = torch.randn(M, A + 1 + NP, generator=g, dtype=torch.float64)
    heads_t = torch.randn(M, A + 1, generator=g, dtype=torch.float64)
    legal = (torch.rand(M, A, generator=g) < 0.4).double()
    legal[:, A - 1] = (legal[:, :A - 1].sum(1) == 0).double()
    action = torch.randint(0, A, (M,), generator=g)
    own = torch.zeros(M, NP // 3, 3, dtype=torch.float64)
    kind = torch.randint(0, 4, (M, NP // 3), generator=g)          # 3 = empty slot
    for k in range(3):
        own[..., k] = (kind == k).double()
    own[::5] = 0                                                      # rows with an entirely empty mask
    reward = torch.randn(T, B, generator=g, dtype=torch.float64)
    boot = (torch.rand(T, B, generator=g) < 0.8).double()
    seq_len = torch.tensor([(T, T - 1, 1, 0)[b % 4] for b in range(B)], dtype=torch.float64)
    weight = torch.rand(B, generator=g, dtype=torch.float64) + 0.5
    return heads, heads_t, legal, action, own.view(M, NP), reward, boot, seq_len, weight


@pytest.mark.parametrize("T,B,A,NP,n,pw", [(7, 5, 21, 15, 3, 0.25), (4, 3, 49, 12, 1, 0.25), (3, 2, 12, 6, 5, 0.0), (9, 4, 33, 15, 2, 1.0)])
def test_hand_formulas_equal_float64_autograd(T, B, A, NP, n, pw):
    heads, heads_t, legal, action, own, reward, boot, seq_len, weight = _batch(T, B, A, NP, 100 + A)
    o = R.loss_objective(heads, heads_t, legal, action, reward, boot, seq_len, weight, own, T, B, A, n, 0.999, pw)
    td = o["td"]
    # d mean_b(w_b loss_b) / d qa = -clamp(err, -1, 1) mask w / B
    assert float((td["dqa"] - td["hand_dqa"]).abs().max()) <= 1e-12
    # the head gradient written out = autograd of the objective through duel_q
    hand = R.hand_head_grad(heads, legal, action, td["dqa"].reshape(-1), A, own, weight, pw / B, B)
    if pw == 0.0:
        hand[:, A + 1:] = 0
    assert float((hand - o["grad"]).abs().max()) <= 1e-12
    # head_grad (what hsad_heads_backward is held to) agrees with both
    g, _, _ = R.head_grad(heads, legal, action, td["dqa"].reshape(-1), A, own, weight, pw / B, B)
    assert float((g - o["grad"]).abs().max()) <= 1e-12
    # rows with an empty own-hand mask: zero cross-entropy and zero aux gradient, exactly
    empty = own.sum(1) == 0
    assert empty.any() and float(o["grad"][empty][:, A + 1:].abs().max()) == 0.0
    xs, steps = R.aux_xent(heads[:, A + 1:], own, T, B)
    assert float(steps.reshape(-1)[empty].abs().max()) == 0.0
    # masked steps: zero error and zero gradient
    assert float((td["err"] * (1 - td["mask"])).abs().max()) == 0.0 and float((td["dqa"] * (1 - td["mask"])).abs().max()) == 0.0
    # shift and cut of the n-step target: the last n steps bootstrap from nothing
    plain = (reward - o["qa"].view(T, B)) * td["mask"]
    assert torch.equal(td["err"][max(T - n, 0):], plain[max(T - n, 0):])


def test_greedy_takes_the_first_of_equal_scores_and_row_zero_without_a_legal_move():
    adv = torch.tensor([[1.0, 3.0, 3.0, -2.0], [-1.0, -5.0, -1.0, -7.0], [4.0, 4.0, 4.0, 4.0]], dtype=torch.float64)
    legal = torch.tensor([[1.0, 1, 1, 1], [0, 1, 1, 1], [0, 0, 0, 0]], dtype=torch.float64)
    assert R.greedy_of(adv, legal).tolist() == [1, 2, 0]
    assert R.duel_q(adv, torch.zeros(3, dtype=torch.float64), legal)["greedy"].tolist() == [1, 2, 0]


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -20), 0.0], dtype=np.float32)
    got = R.bf16_bits_to_f64(R.to_bf16_bits(x))
    assert got.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), 0.0]
    t = torch.randn(4096)
    assert np.array_equal(R.to_bf16_bits(t.numpy()), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


# ---- the restated hash: 2^20 (row, counter) pairs = 1024 rows x 1024 counters, seed fixed ----
@pytest.fixture(scope="module")
def draws():
    rows, counters = np.meshgrid(np.arange(1024), np.arange(1024), indexing="ij")
    u, low = R.act_hash(0x5EED, rows, counters)
    assert u.size == N_PAIRS and u.min() >= 0.0 and u.max() < 1.0
    return u, low


@pytest.mark.parametrize("eps", [0.05, 0.25, 1.0])
def test_hash_explores_with_probability_eps(draws, eps):
    u, _ = draws
    share = float((u < eps).mean())
    sd = math.sqrt(eps * (1 - eps) / N_PAIRS)            # binomial
    assert abs(share - eps) <= 5 * sd, (share, eps, sd)


@pytest.mark.parametrize("nlegal", [1, 2, 7, 21])
def test_hash_index_is_uniform_over_the_legal_moves(draws, nlegal):
    _, low = draws
    k = R.act_index(low, nlegal)
    assert k.min() >= 0 and k.max() < nlegal
    counts = np.bincount(k.ravel(), minlength=nlegal)
    expect = N_PAIRS / nlegal
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    dof = nlegal - 1
    assert chi2 <= dof + 5 * math.sqrt(2 * dof), (chi2, dof)        # chi-square: mean dof, variance 2 dof (0 <= 0 for one move)


@pytest.mark.parametrize("axis", ["counter", "row"])
def test_hash_draws_of_neighbours_are_uncorrelated(draws, axis):
    u, _ = draws
    a, b = (u[:, :-1], u[:, 1:]) if axis == "counter" else (u[:-1, :], u[1:, :])
    r = float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    assert abs(r) <= 5 / math.sqrt(a.size), r             # sample correlation of independent draws: sd 1 / sqrt(n)
    assert float((a == b).mean()) < 1e-4                  # and they are different draws


def test_hash_is_keyed_by_seed_row_and_counter():
    base = R.act_hash(5, np.arange(64), 9)[0]
    assert not np.array_equal(base, R.act_hash(6, np.arange(64), 9)[0])
    assert not np.array_equal(base, R.act_hash(5, np.arange(64), 10)[0])
    assert not np.array_equal(base[:-1], base[1:])
    # one known value, worked by hand with python integers
    def mix(z):
        m = (1 << 64) - 1
        z = (z + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)
    h = mix((mix(5 ^ ((0xD1342543DE82EF95 * 17) & ((1 << 64) - 1))) + 9) & ((1 << 64) - 1))
    u, low = R.act_hash(5, np.array([17]), 9)
    assert u[0] == ((h >> 40) & 0xFFFFFF) / 16777216.0 and int(low[0]) == h & 0xFFFFFFFF


def test_td_bounds_grow_with_the_operands_and_the_path():
    T, B = 300, 2
    g = torch.Generator().manual_seed(1)
    qa, tq, r = (torch.randn(T, B, generator=g, dtype=torch.float64) for _ in range(3))
    one = R.td(qa, tq, r, torch.ones(T, B), torch.tensor([300.0, 7.0]), 3, 0.999)
    big = R.td(8 * qa, 8 * tq, 8 * r, torch.ones(T, B), torch.tensor([300.0, 7.0]), 3, 0.999)
    assert (big["err_bound"] >= one["err_bound"]).all() and (big["loss_bound"] > one["loss_bound"]).all()
    assert float(one["err_bound"][7:, 1].abs().max()) == 0.0 and one["loss_bound"][0] > one["loss_bound"][1]
