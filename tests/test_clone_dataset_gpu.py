"""hanabi_sad_amd.clone.sequences_from_records against the paths it is built from: without SAD every row (t, seat) is bit for bit the row of
game_record.replay(records, stop=t); with SAD the rows are those of a second env this test steps itself from replay(stop=0) with
env.step(a, greedy_a) (the path tests/test_env_parity_gpu.py pins to the oracle).  2 and 3 players, the standard game and a small variant,
8 recorded games each."""
import numpy as np
import pytest
import torch

from hanabi_sad_amd import clone
from hanabi_sad_amd import game_record as gr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
FULL = dict(colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3)
SMALL = dict(colors=3, ranks=4, max_information_tokens=5, max_life_tokens=2)
CASES = {"p2-standard": (2, 5, FULL), "p3-standard": (3, 5, FULL), "p2-small": (2, 3, SMALL), "p3-small": (3, 3, SMALL)}
_RECORDS = {}


def records_of(case):
    """8 games of piers and cautious taking turns on the seats (recorded once per case, shared by the tests)"""
    if case not in _RECORDS:
        from hanabi_sad_amd.rulebot import PRESETS
        P, hand, rules = CASES[case]
        _RECORDS[case] = clone.records_from_teacher([PRESETS["piers"], PRESETS["cautious"]], 8, 21, 1, num_player=P, device=DEV, hand_size=hand, **rules)
        assert len(_RECORDS[case]) == 8
    return _RECORDS[case]


def new_env(records, sad):
    from hanabi_sad_amd import BatchedHanabiEnv
    r = records[0].rules
    env = BatchedHanabiEnv(len(records), players=r["players"], hand_size=r["hand_size"], bomb=r["bomb"], eps_list=[0.0], max_len=-1, sad=sad, device=DEV,
                           colors=r["colors"], ranks=r["ranks"], max_information_tokens=r["max_information_tokens"], max_life_tokens=r["max_life_tokens"])
    env.reset()
    return env


def same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_common(data, records, P, keep=None):
    G = len(records)
    A = data.legal_move.shape[2]
    keep = np.ones((G, P), bool) if keep is None else keep
    flat = np.nonzero(keep.reshape(-1))[0]
    assert data.game.tolist() == (flat // P).tolist() and data.seat.tolist() == (flat % P).tolist()
    a, lens = data.a.cpu().numpy(), data.seq_len.cpu().numpy()
    for n, row in enumerate(flat):
        g, p = divmod(int(row), P)
        k = min(records[g].n_moves, data.T)
        assert lens[n] == k
        want = np.full(data.T, A - 1, np.int64)
        for t in range(k):
            if t % P == p:
                want[t] = records[g].moves[t]
        assert a[:, n].tolist() == want.tolist(), (g, p)
        assert not data.legal_move[k:, n].any() and not (data.priv_s if data.priv_s is not None else data.priv_s_bf16)[k:, n].any()
        # inside the sequence: the mover's recorded move is legal, the other seats may only pass
        legal = data.legal_move[:k, n].cpu().numpy()
        assert all(legal[t, want[t]] == 1.0 for t in range(k))
        assert all(legal[t].sum() == 1.0 for t in range(k) if t % P != p)


@pytest.mark.parametrize("case", sorted(CASES))
def test_without_sad_the_rows_are_those_of_replay_at_every_move(case):
    P, hand, rules = CASES[case]
    records = records_of(case)
    data = clone.sequences_from_records(records, False, device=DEV, bf16=False)
    G, T = len(records), gr.capacity(records[0].rules)
    assert data.T == T and data.n_rows == G * P and data.truncated == 0 and data.priv_s_bf16 is None
    check_common(data, records, P)
    env = new_env(records, False)
    longest = max(r.n_moves for r in records)
    for t in range(longest):
        gr.replay(records, stop=[t] * G, env=env)
        live = torch.tensor([t < r.n_moves for r in records], device=DEV)
        rows = live.repeat_interleave(P)
        assert same(data.priv_s[t][rows], env.priv_s.view(G * P, -1)[rows]), t
        assert same(data.legal_move[t][rows], env.legal_move.view(G * P, -1)[rows]), t
    env.close()
    # the bf16 rows are the same bits, zero-padded to the net's row length
    d16 = clone.sequences_from_records(records, False, device=DEV, bf16=True)
    F = data.priv_s.shape[2]
    assert d16.priv_s is None and d16.priv_s_bf16.shape[2] == (F + 63) // 64 * 64 and d16.priv_s_bf16.dtype == torch.bfloat16
    assert torch.equal(d16.priv_s_bf16[..., :F].float(), data.priv_s) and not d16.priv_s_bf16[..., F:].any()
    assert torch.equal(d16.legal_move, data.legal_move) and torch.equal(d16.a, data.a)


@pytest.mark.parametrize("case", sorted(CASES))
def test_with_sad_the_rows_are_those_of_an_env_stepped_with_the_record(case):
    P, hand, rules = CASES[case]
    records = records_of(case)
    data = clone.sequences_from_records(records, True, device=DEV, bf16=False)
    G = len(records)
    check_common(data, records, P)
    env = new_env(records, True)
    gr.replay(records, stop=[0] * G, env=env)
    A = env.A
    assert data.priv_s.shape[2] == env.F > clone.sequences_from_records(records[:1], False, device=DEV, bf16=False).priv_s.shape[2]
    for t in range(max(r.n_moves for r in records)):
        live = torch.tensor([t < r.n_moves for r in records], device=DEV)
        rows = live.repeat_interleave(P)
        assert same(data.priv_s[t][rows], env.priv_s.view(G * P, -1)[rows]), t
        assert same(data.legal_move[t][rows], env.legal_move.view(G * P, -1)[rows]), t
        a = np.full((G, P), A - 1, np.int64)
        ga = a.copy()
        for g, r in enumerate(records):
            if t < r.n_moves:
                a[g, t % P], ga[g, t % P] = r.moves[t], r.greedy[t]
        env.step(torch.from_numpy(a).to(DEV), torch.from_numpy(ga).to(DEV))
    env.close()


def test_seat_filter_and_max_len():
    case = "p3-standard"
    P = CASES[case][0]
    records = records_of(case)
    whole = clone.sequences_from_records(records, True, device=DEV, bf16=False)
    # by name: the seats piers played (pool member p % 2 on seat p: seats 0 and 2)
    keep = clone.select_seats(records, "piers")
    assert keep.tolist() == [[True, False, True]] * len(records)
    part = clone.sequences_from_records(records, True, seats="piers", device=DEV, bf16=False)
    check_common(part, records, P, keep)
    rows = torch.from_numpy(np.nonzero(keep.reshape(-1))[0]).to(DEV)
    assert same(part.priv_s, whole.priv_s[:, rows]) and same(part.legal_move, whole.legal_move[:, rows]) and torch.equal(part.a, whole.a[:, rows])
    one = clone.sequences_from_records(records, True, seats=[1], device=DEV, bf16=False)
    assert one.seat.tolist() == [1] * len(records) and same(one.priv_s, whole.priv_s[:, 1::P])
    # max_len shorter than some games: they are cut and counted, the kept part is unchanged
    n = sorted(r.n_moves for r in records)
    cut_at = n[len(n) // 2] - 1
    short = clone.sequences_from_records(records, True, max_len=cut_at, device=DEV, bf16=False)
    assert short.T == cut_at and short.truncated == sum(k > cut_at for k in n) >= len(n) // 2
    check_common(short, records, P)
    assert same(short.priv_s, whole.priv_s[:cut_at] * (torch.arange(cut_at, device=DEV).view(-1, 1, 1) < short.seq_len.view(1, -1, 1)))
    assert torch.equal(short.seq_len, whole.seq_len.clamp(max=cut_at))
    with pytest.raises(ValueError, match="different rules"):
        clone.sequences_from_records([records[0], records_of("p2-small")[0]], True, device=DEV)
