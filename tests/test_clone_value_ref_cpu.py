"""The float64 reference of the cloning loss with the value term (tests/clone_value_ref.py): its case generator keeps what it promises
(the Huber kink is hit exactly where it is meant to be hit and kept at a distance everywhere else), its gradient is torch autograd of
policy_weight x masked log_softmax loss + value_weight x smooth_l1(q_act, ret) through the dueling head, and without the value term it is
tests/clone_loss_ref.py's clone_tail.  And hanabi_sad_amd.clone.returns_to_go against a scalar recursion.  All without a device."""
import numpy as np
import pytest
import torch

from hanabi_sad_amd import clone
from tests import clone_loss_ref as P
from tests import clone_value_ref as R

SHAPES = [(21, 37), (12, 19), (49, 62), (32, 48), (33, 49)]
CASES = [(1, 1), (5, 3), (97, 3), (5, 1), (97, 1)]


@pytest.mark.parametrize("A,ldh", SHAPES)
@pytest.mark.parametrize("T,B", CASES)
def test_the_case_generator_keeps_its_promises(A, ldh, T, B):
    c, mark = R.clone_value_case(A, ldh, T, B)
    base = P.clone_case(A, ldh, T, B)
    e = R.check_case(c, mark, T, B, A)
    # sequence 0's special rows are clone_case's
    for t in range(T):
        if (t + A) % 8 != 7:
            m = t * B
            assert torch.equal(c["heads"][m, :A], base["heads"][m, :A]) and torch.equal(c["legal"][m], base["legal"][m])
    for k in ("legal", "action", "seq_len", "weight"):
        assert torch.equal(c[k], base[k]), k
    grid = c["heads"][:, A] * 64
    assert torch.equal(grid, grid.round()) and float(c["heads"][:, A].abs().max()) <= 8.0
    if T == 97:      # every kind of marked row is there, more than once
        for k in R.MARKS:
            assert sum(1 for x in mark if x == k) >= 2, k
        ae = e.abs()
        assert int((ae == 1.0).sum()) >= 4 and int(((ae > 0) & (ae < 1)).sum()) >= 10 and int((ae > 1).sum()) >= 10


@pytest.mark.parametrize("A,ldh", SHAPES)
@pytest.mark.parametrize("T,B", CASES)
@pytest.mark.parametrize("pw,vw", [(1.0, 1.0), (0.0, 1.0), (1.0, 0.25)])
def test_reference_gradient_is_autograd_through_the_dueling_head(A, ldh, T, B, pw, vw):
    c, _ = R.clone_value_case(A, ldh, T, B)
    ref = R.clone_value_tail(c["heads"], c["legal"], c["action"], c["ret"], c["seq_len"], c["weight"], T, B, A, 64, pw, vw)
    # the restatement knows no bad rows (tests/test_clone_ref_cpu.py): they become rows that are multiplied by 0
    M = T * B
    t_of, b_of = torch.arange(M) // B, torch.arange(M) % B
    valid = t_of.double() < c["seq_len"].double()[b_of]
    bad = valid & ~ref["good"]
    assert torch.equal(ref["bad"], bad.view(T, B).sum(0)) and torch.equal(ref["steps"], (valid & ~bad).view(T, B).sum(0))
    h = c["heads"].double().clone().requires_grad_(True)
    legal, action = c["legal"].double().clone(), c["action"].clone()
    legal[bad] = 1.0
    action[bad] = 0
    keep = (valid & ~bad).double()
    z = h[:, :A].masked_fill((legal == 0) & valid[:, None], float("-inf"))
    xent = -torch.log_softmax(z, 1).gather(1, action.clamp(0, A - 1)[:, None])[:, 0] * keep
    al = h[:, :A] * c["legal"].double()
    q = h[:, A:A + 1] + al - al.mean(1, keepdim=True)
    qa = q.gather(1, action.clamp(0, A - 1)[:, None])[:, 0]
    target = torch.where(ref["good"], c["ret"].double(), qa.detach())
    hub = torch.nn.functional.smooth_l1_loss(qa, target, reduction="none") * keep
    loss, vloss = xent.view(T, B).sum(0), hub.view(T, B).sum(0)
    ((pw * loss + vw * vloss) * c["weight"].double()).mean().backward()
    assert torch.allclose(loss, ref["loss"], rtol=0, atol=1e-12 * max(1, T))
    assert torch.allclose(vloss, ref["vloss"], rtol=0, atol=1e-12 * max(1, T))
    assert torch.allclose(h.grad[:, :A + 1], ref["dheads"][:, :A + 1], rtol=0, atol=1e-14)
    assert not ref["dheads"][:, A + 1:].any() and not h.grad[:, A + 1:].any()
    assert torch.isfinite(ref["dheads"]).all() and torch.isfinite(ref["vloss"]).all()      # the NaN returns never show
    assert not ref["dheads"][ref["zero_row"]].any()
    # a single-legal row carries the value term alone
    alone = R.clone_value_tail(c["heads"], c["legal"], c["action"], c["ret"], c["seq_len"], c["weight"], T, B, A, 64, 0.0, vw)
    assert torch.equal(ref["dheads"][ref["single"]], alone["dheads"][ref["single"]])
    # the module's own restatement (what the learner test is modelled on) agrees where no row is bad
    if not bad.any():
        _, l2, v2 = R.objective(c["heads"].double(), c["legal"].double(), c["action"], c["ret"], c["seq_len"].double(), c["weight"].double(), T, B, A, pw, vw)
        assert torch.allclose(l2, ref["loss"], rtol=0, atol=1e-12 * T) and torch.allclose(v2, ref["vloss"], rtol=0, atol=1e-12 * T)


@pytest.mark.parametrize("A,ldh", SHAPES)
@pytest.mark.parametrize("T,B", [(5, 3), (97, 3)])
def test_without_the_value_term_it_is_clone_tail(A, ldh, T, B):
    c, _ = R.clone_value_case(A, ldh, T, B)
    args = (c["heads"], c["legal"], c["action"])
    old = P.clone_tail(*args, c["seq_len"], c["weight"], T, B, A, 64)
    new = R.clone_value_tail(*args, c["ret"], c["seq_len"], c["weight"], T, B, A, 64, 1.0, 0.0)
    for k in ("loss", "hits", "decisions", "bad", "dheads", "zero_row", "xent"):
        assert torch.equal(old[k], new[k]), k
    assert not new["vloss"].any()


def scalar_returns(rewards, n_moves, gamma):
    steps, G = len(rewards), len(n_moves)
    out = [[0.0] * G for _ in range(steps)]
    for j in range(G):
        run = 0.0
        for t in range(n_moves[j] - 1, -1, -1):
            run = rewards[t][j] + gamma * run
            out[t][j] = run
    return out


@pytest.mark.parametrize("gamma", [1.0, 0.999])
def test_returns_to_go_against_a_scalar_recursion(gamma):
    rng = np.random.RandomState(3)
    steps, n_moves = 23, [23, 7, 0, 1, 15, 22]
    rewards = rng.randint(0, 2, size=(steps, len(n_moves))).astype(np.float32)
    rewards[9:, 1] = 5.0            # whatever lies past a game's end is not read
    rewards[:, 2] = 9.0             # ... a game of no moves included
    got = clone.returns_to_go(rewards, n_moves, gamma)
    want = np.asarray(scalar_returns(rewards.tolist(), n_moves, gamma))
    assert got.dtype == np.float32 and got.shape == (steps, len(n_moves))
    for j, n in enumerate(n_moves):
        assert not got[n:, j].any()
    if gamma == 1.0:                # integer rewards: exact
        assert np.array_equal(got.astype(np.float64), want)
        assert got[0, 0] == rewards[:, 0].sum() and got[0, 1] == rewards[:7, 1].sum()
    else:                           # float64 inside, one rounding to float32
        assert np.array_equal(got, want.astype(np.float32))
