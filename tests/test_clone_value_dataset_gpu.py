"""CloneDataset.ret: the returns sequences_from_records(gamma=...) collects from env.reward while it steps the recorded games, held to the
plain-Python replay of the same records (GameRecord.position), to returns_to_go, and to the dataset without returns; and one end-to-end
run of the driver with the value term.  Records of `piers` playing itself: Hanabi-Small (2 colours, hands of 2, 3 information tokens,
1 life) and the standard game, 8 games each, bomb 0.

The env's reward, as read in the step tail of csrc/hsad_env.hip: reward = score_after - score_before with score = 0 if (no life is left
and bomb) else the sum of the fireworks.  With bomb 0 that is the score step of the move at every move, the last one included -- a game
lost on its last life keeps its fireworks -- so the test expects the fireworks step of the Python replay everywhere."""
import re

import numpy as np
import pytest
import torch

from hanabi_sad_amd import clone
from hanabi_sad_amd import game_record as gr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
SMALL = dict(colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1)
FULL = dict(colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3)
CASES = {"small": (2, 2, SMALL), "standard": (2, 5, FULL)}
_RECORDS, _DATA = {}, {}


def records_of(case):
    if case not in _RECORDS:
        from hanabi_sad_amd.rulebot import PRESETS
        P, hand, rules = CASES[case]
        _RECORDS[case] = clone.records_from_teacher([PRESETS["piers"]], 8, 21, 1, num_player=P, bomb=0, device=DEV, hand_size=hand, **rules)
        assert len(_RECORDS[case]) == 8 and all(r.rules["bomb"] == 0 for r in _RECORDS[case])
    return _RECORDS[case]


def data_of(case, gamma):
    """the uncut dataset (computed once per case and gamma, shared, never written)"""
    if (case, gamma) not in _DATA:
        _DATA[case, gamma] = clone.sequences_from_records(records_of(case), True, device=DEV, gamma=gamma)
    return _DATA[case, gamma]


def score_steps(rec):
    """the score step of every move by the plain-Python replay of the rules"""
    score = [sum(rec.position(k).fireworks) for k in range(rec.n_moves + 1)]
    return np.diff(np.asarray(score, dtype=np.float64))


def test_undiscounted_returns_step_by_the_score_of_the_python_replay():
    scoring = deck_ends = rows = 0
    for case in CASES:
        P = CASES[case][0]
        records = records_of(case)
        data = data_of(case, 1.0)
        assert data.ret.shape == (data.T, data.n_rows) == (gr.capacity(records[0].rules), len(records) * P) and data.ret.dtype == torch.float32
        ret = data.ret.cpu().numpy().astype(np.float64)
        for n in range(data.n_rows):
            g = int(data.game[n])
            rec = records[g]
            k = rec.n_moves
            assert int(data.seq_len[n]) == k
            step = score_steps(rec)
            togo = np.append(ret[:k, n], 0.0)
            assert np.array_equal(togo[:-1] - togo[1:], step), (case, g)
            assert ret[0, n] == rec.score if k else True       # (bomb 0: the whole return is the final score)
            assert not ret[k:, n].any()                        # past seq_len: 0
            scoring += int((step > 0).sum())
            deck_ends += int(rec.end == gr.ENDS["deck"])
            rows += k
        # every seat's row of a game carries the same returns
        assert torch.equal(data.ret[:, 0::P], data.ret[:, 1::P])
    assert rows > 0 and scoring >= 1, "no scoring move among the checked rows"
    assert deck_ends >= 1, "no game that ends by the deck among the checked rows"


@pytest.mark.parametrize("case", sorted(CASES))
def test_discounted_returns_are_returns_to_go_of_the_same_rewards(case):
    records = records_of(case)
    gamma = 0.999
    data = data_of(case, gamma)
    P = CASES[case][0]
    steps = max(r.n_moves for r in records)
    rewards = np.zeros((steps, len(records)), dtype=np.float32)
    for g, rec in enumerate(records):
        rewards[:rec.n_moves, g] = score_steps(rec)
    want = clone.returns_to_go(rewards, [r.n_moves for r in records], gamma)                 # [steps, G] float32
    got = data.ret.cpu().numpy()
    assert not got[steps:].any()
    game = data.game.cpu().numpy()
    # float64 inside, one rounding to fp32: the same bits
    assert np.array_equal(got[:steps], want[:, game])
    assert float(np.abs(got[:steps] - data_of(case, 1.0).ret.cpu().numpy()[:steps]).max()) > 0      # (and the discount does something)


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_cut_game_keeps_the_return_of_the_whole_game(case):
    records = records_of(case)
    whole = data_of(case, 0.999)
    n = sorted(r.n_moves for r in records)
    cut_at = n[len(n) // 2] - 1
    assert 0 < cut_at < n[-1]
    short = clone.sequences_from_records(records, True, max_len=cut_at, device=DEV, gamma=0.999)
    assert short.T == cut_at and short.truncated == sum(k > cut_at for k in n) >= 1
    assert torch.equal(short.seq_len, whole.seq_len.clamp(max=cut_at))
    assert torch.equal(short.ret.view(torch.int32), whole.ret[:cut_at].contiguous().view(torch.int32))       # bit-equal on the kept steps
    # the observations are those of the uncut dataset
    keep = (torch.arange(cut_at, device=DEV).view(-1, 1) < short.seq_len.view(1, -1))
    assert torch.equal(short.priv_s_bf16, whole.priv_s_bf16[:cut_at] * keep.unsqueeze(2)) and torch.equal(short.a, torch.where(keep, whole.a[:cut_at], short.a))


@pytest.mark.parametrize("case", sorted(CASES))
def test_without_a_gamma_the_dataset_is_what_it_was(case):
    records = records_of(case)
    plain = clone.sequences_from_records(records, True, device=DEV)
    also = clone.sequences_from_records(records, True, device=DEV, gamma=None)
    with_ret = data_of(case, 0.999)
    assert plain.ret is None and also.ret is None
    for other in (also, with_ret):          # ... and the returns change no other field
        assert other.priv_s is None and plain.priv_s is None
        for k in ("priv_s_bf16", "legal_move", "a", "seq_len", "game", "seat"):
            x, y = getattr(plain, k), getattr(other, k)
            assert x.dtype == y.dtype and torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y), k
        assert plain.truncated == other.truncated
    cut = clone.sequences_from_records(records, True, max_len=10, device=DEV)
    assert cut.ret is None and cut.T == 10


def test_the_driver_fits_the_value_and_writes_a_net_that_loads(tmp_path, capsys):
    """small variant, 64 games, 3 epochs with --value_weight 1: the held-out value loss per step falls, clone.pthw loads into NetPartner"""
    import os
    from hanabi_sad_amd.actor import NetPartner
    from hanabi_sad_amd.eval import env_dims
    argv = ["--teacher", "piers", "--num_game", "64", "--num_epoch", "3", "--value_weight", "1", "--sad", "1", "--hand_size", "2", "--colors", "2",
            "--max_information_tokens", "3", "--max_life_tokens", "1", "--max_len", "40", "--batchsize", "16", "--rnn_hid_dim", "256", "--lr", "1e-3",
            "--num_eval_game", "8", "--save_dir", str(tmp_path), "--train_device", DEV]
    assert clone.main(argv) == 0
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("epoch ")]
    assert len(lines) == 3, out
    held = [float(re.search(r"held-out value loss per step ([0-9.eE+-]+)", ln).group(1)) for ln in lines]
    train = [float(re.search(r", value loss per step ([0-9.eE+-]+)", ln).group(1)) for ln in lines]
    print("value loss per step, held out: %s, training: %s" % (held, train))
    assert held[2] < held[0], held
    partner = NetPartner(os.path.join(str(tmp_path), "clone.pthw"), name="cloned")
    F, A = env_dims(2, 2, True, **SMALL)
    assert partner.dims() == (F, A)
    net = partner.make_net(torch.device(DEV))
    assert (net.F, net.A) == (F, A)
    net.close()
