"""The float64 reference of the behaviour-cloning loss (tests/clone_loss_ref.py) against torch autograd of a masked log_softmax
restatement, and the host-side logic of hanabi_sad_amd/clone.py (split by game, fixed-size batches with padding rows, seat-name
matching, refusal of mixed rules) -- all without a device."""
import numpy as np
import pytest
import torch

from hanabi_sad_amd import clone
from hanabi_sad_amd import game_record as gr
from tests import clone_loss_ref as R

SHAPES = [(21, 37), (12, 19), (49, 62), (32, 48), (33, 49)]


@pytest.mark.parametrize("A,ldh", SHAPES)
@pytest.mark.parametrize("T,B", [(1, 1), (5, 3), (97, 3), (5, 1)])
def test_reference_gradient_is_autograd_of_masked_log_softmax(A, ldh, T, B):
    c = R.clone_case(A, ldh, T, B)
    ref = R.clone_tail(c["heads"], c["legal"], c["action"], c["seq_len"], c["weight"], T, B, A, 64)
    # the restatement knows no bad rows: they are taken out of its objective by shortening nothing -- their weight is removed row-wise
    t_of, b_of = torch.arange(T * B) // B, torch.arange(T * B) % B
    valid = t_of.double() < c["seq_len"].double()[b_of]
    act = c["action"]
    in_range = (act >= 0) & (act < A)
    bad = valid & ~(in_range & (c["legal"].gather(1, act.clamp(0, A - 1)[:, None])[:, 0] != 0))
    assert torch.equal(ref["bad"], bad.view(T, B).sum(0))
    h = c["heads"].double().clone().requires_grad_(True)
    legal = c["legal"].double().clone()
    action = act.clone()
    legal[bad] = 1.0            # a bad row becomes a row whose xent is multiplied by 0 below
    action[bad] = 0
    z = h[:, :A].masked_fill((legal == 0) & valid[:, None], float("-inf"))
    xent = -torch.log_softmax(z, 1).gather(1, action.clamp(0, A - 1)[:, None])[:, 0] * (valid & ~bad).double()
    loss = xent.view(T, B).sum(0)
    (loss * c["weight"].double()).mean().backward()
    assert torch.allclose(loss, ref["loss"], rtol=0, atol=1e-12 * max(1, T))
    assert torch.allclose(h.grad[:, :A], ref["dheads"][:, :A], rtol=0, atol=1e-14)
    assert not ref["dheads"][:, A:].any() and not h.grad[:, A:].any()
    # the module's own restatement (what the learner test differentiates) agrees where no row is bad
    if not bad.any():
        obj, l2 = R.masked_log_softmax_loss(c["heads"].double(), c["legal"], act, c["seq_len"].double(), c["weight"].double(), T, B, A)
        assert torch.allclose(l2, ref["loss"], rtol=0, atol=1e-12 * max(1, T))


@pytest.mark.parametrize("A,ldh", SHAPES)
def test_single_legal_and_past_seq_len_rows_are_exact_zeros(A, ldh):
    T, B = 97, 3
    c = R.clone_case(A, ldh, T, B)
    ref = R.clone_tail(c["heads"], c["legal"], c["action"], c["seq_len"], c["weight"], T, B, A, 64)
    single = [t * B for t in range(T) if (t + A) % 8 == 0]
    assert len(single) >= 12
    for m in single:
        assert ref["xent"].view(-1)[m] == 0.0 and not ref["dheads"][m].any() and bool(ref["zero_row"][m])
    past = [t * B + b for b in range(B) for t in range(T) if t >= c["seq_len"][b]]
    assert len(past) > T
    for m in past:
        assert ref["xent"].view(-1)[m] == 0.0 and not ref["dheads"][m].any()
    assert torch.isfinite(ref["dheads"]).all() and torch.isfinite(ref["loss"]).all()
    # counters: decisions are the valid, not bad rows with >= 2 legal actions; a hit needs the FIRST maximum
    assert int(ref["decisions"][2]) == 0 and int(ref["hits"][2]) == 0 and int(ref["bad"][2]) == 0
    tie_second = [t * B for t in range(T) if (t + A) % 8 == 5]
    tie_first = [t * B for t in range(T) if (t + A) % 8 == 6]
    hit = (ref["multi"] & (ref["p"].argmax(1) == c["action"]))
    assert all(not bool(hit[m]) for m in tie_second) and all(bool(hit[m]) for m in tie_first)


# ---- hanabi_sad_amd/clone.py without a device -------------------------------------------------------------------------------------
RULES = dict(players=2, hand_size=5, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3, bomb=0)


def fake_dataset(n_game=10, P=2, T=6, F=5, A=4):
    N = n_game * P
    game = torch.arange(n_game).repeat_interleave(P)
    seat = torch.arange(P).repeat(n_game)
    return clone.CloneDataset(priv_s=torch.arange(T * N * F, dtype=torch.float32).view(T, N, F), priv_s_bf16=None,
                              legal_move=torch.ones(T, N, A), a=torch.zeros(T, N, dtype=torch.int64),
                              seq_len=torch.arange(1, N + 1, dtype=torch.float32).clamp(max=T), game=game, seat=seat, truncated=0)


def test_split_is_by_game():
    ds = fake_dataset()
    train, held = ds.split(0.3, seed=4)
    gt, gh = set(train.game.tolist()), set(held.game.tolist())
    assert len(gh) == 3 and len(gt) == 7 and not (gt & gh) and gt | gh == set(range(10))
    assert train.n_rows == 14 and held.n_rows == 6          # both seats of a game go together
    again = ds.split(0.3, seed=4)
    assert torch.equal(again[1].game, held.game) and not torch.equal(ds.split(0.3, seed=5)[1].game, held.game)
    # the rows are the source's rows
    j = int(held.game[0]) * 2 + int(held.seat[0])
    assert torch.equal(held.priv_s[:, 0], ds.priv_s[:, j]) and held.seq_len[0] == ds.seq_len[j]
    with pytest.raises(ValueError):
        ds.split(1.0, seed=0)


def test_batches_have_a_fixed_row_count_and_pad_with_weightless_rows():
    ds = fake_dataset()                     # 20 rows
    got = list(ds.batches(8, seed=2))
    assert len(got) == 3 and clone.padding_rows(20, 8) == 4 and clone.padding_rows(16, 8) == 0
    seen = []
    for k, (batch, weight, index) in enumerate(got):
        assert batch["priv_s"].shape == (6, 8, 5) and batch["legal_move"].shape == (6, 8, 4) and batch["a"].shape == (6, 8)
        assert weight.shape == (8,) and batch["seq_len"].shape == (8,)
        real = index >= 0
        assert int(real.sum()) == (8 if k < 2 else 4)
        assert torch.equal(weight, real.float()) and not batch["seq_len"][~real].any()
        assert not batch["priv_s"][:, ~real].any() and not batch["legal_move"][:, ~real].any()
        for c, j in enumerate(index.tolist()):
            if j >= 0:
                assert torch.equal(batch["priv_s"][:, c], ds.priv_s[:, j]) and batch["seq_len"][c] == ds.seq_len[j]
        seen += index[real].tolist()
    assert sorted(seen) == list(range(20)) and seen != list(range(20))
    assert [i.tolist() for _, _, i in ds.batches(8, seed=2)] == [i.tolist() for _, _, i in got]
    assert [i.tolist() for _, _, i in ds.batches(8, seed=3)] != [i.tolist() for _, _, i in got]


def rec(seats, rules=RULES):
    return gr.GameRecord(rules, list(range(10)), [], meta={"seats": seats})


def test_seat_selection_by_index_and_by_name():
    recs = [rec(["piers", "cautious"]), rec(["cautious", "piers"]), rec(["piers", "piers"])]
    assert clone.select_seats(recs, None).tolist() == [[True, True]] * 3
    assert clone.select_seats(recs, [1]).tolist() == [[False, True]] * 3
    assert clone.select_seats(recs, "piers").tolist() == [[True, False], [False, True], [True, True]]
    with pytest.raises(ValueError, match="no seat"):
        clone.select_seats(recs, "iggi")
    with pytest.raises(ValueError, match="seat names"):
        clone.select_seats([gr.GameRecord(RULES, list(range(10)), [])], "piers")
    with pytest.raises(ValueError):
        clone.select_seats(recs, [2])


def test_records_of_different_rules_are_refused():
    other = dict(RULES, colors=3)
    with pytest.raises(ValueError, match="different rules"):
        clone.check_rules([rec(["a", "b"]), rec(["a", "b"], other)])
    assert clone.check_rules([rec(["a", "b"])] * 2) == RULES
    with pytest.raises(ValueError):
        clone.check_rules([])


def test_sequence_lengths_cut_at_max_len():
    lens, cut = clone.sequence_lengths([3, 9, 5], 5)
    assert lens.tolist() == [3, 5, 5] and cut == 1
    lens, cut = clone.sequence_lengths([3, 9, 5], None, capacity=80)
    assert lens.tolist() == [3, 9, 5] and cut == 0
    assert np.asarray(lens).dtype == np.int64
