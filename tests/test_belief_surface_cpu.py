"""The learned belief's Python face without a GPU (hanabi_sad_amd/belief.py, the knowledge fields of clone.CloneDataset): what is
refused before any device work, the dataset plumbing on synthetic tensors, the saved head's format, the command line's errors."""
import numpy as np
import pytest
import torch

from hanabi_sad_amd import belief
from hanabi_sad_amd.clone import CloneDataset


def test_argument_refusals():
    assert belief.check_head_args(5, 512) == (5, 512) and belief.check_head_args(2, 64) == (2, 64)
    for hs, H in ((0, 64), (6, 64), (5, 0), (5, 96), (5, 63)):
        with pytest.raises(ValueError):
            belief.check_head_args(hs, H)
    assert [belief.padded_logits(h) for h in (5, 4, 2)] == [128, 104, 56]
    T, B, Hs, H = 3, 2, 4, 64
    good = dict(o16=torch.zeros(T, B, H, dtype=torch.bfloat16), pool=torch.zeros(T, B, dtype=torch.int64),
                compat=torch.zeros(T, B, Hs, dtype=torch.int32), cards=torch.full((T, B, Hs), -1, dtype=torch.int32), seq_len=torch.zeros(B))
    assert belief.check_batch(good, Hs) == (T, B)
    for key, bad in (("o16", good["o16"].float()), ("o16", good["o16"][0]), ("pool", good["pool"].int()), ("pool", good["pool"][:2]),
                     ("compat", good["compat"].long()), ("cards", good["cards"][:, :, :3]), ("seq_len", good["seq_len"].double()),
                     ("seq_len", torch.zeros(B + 1))):
        with pytest.raises(ValueError, match=key):
            belief.check_batch(dict(good, **{key: bad}), Hs)
    for key in good:
        with pytest.raises(ValueError, match=key):
            belief.check_batch({k: v for k, v in good.items() if k != key}, Hs)
    with pytest.raises(ValueError):
        belief.check_batch(good, 5)
    # no CPU path: a head on the CPU is an error, not a slow head
    from hanabi_sad_amd import HsadError
    from hanabi_sad_amd.selfplay import init_weights
    W = init_weights(838, 64, 21, 5, 0)
    with pytest.raises(HsadError):
        belief.BeliefHead(W, 5, "cpu")
    with pytest.raises(ValueError):
        belief.BeliefHead(W, 6, "cpu")
    if not torch.cuda.is_available():
        with pytest.raises((HsadError, RuntimeError, AssertionError)):
            belief.BeliefHead(W, 5, "cuda:0")
    with pytest.raises(HsadError, match="architecture"):
        belief.BeliefHead(init_weights(838, 64, 21, 5, 0, num_lstm_layer=1), 5, "cuda:0")


def synthetic(T=4, N=6, A=5, Hs=3):
    g = torch.Generator().manual_seed(0)
    seq_len = torch.tensor([4.0, 2.0, 3.0, 1.0, 4.0, 2.0])
    return CloneDataset(torch.rand(T, N, 7, generator=g), None, torch.ones(T, N, A), torch.randint(0, A, (T, N), generator=g), seq_len,
                        torch.tensor([0, 0, 1, 1, 2, 2]), torch.tensor([0, 1, 0, 1, 0, 1]), 0, None, None,
                        pool=torch.randint(1, 1 << 40, (T, N), generator=g), compat=torch.randint(1, 1 << 25, (T, N, Hs), generator=g).int(),
                        cards=torch.randint(0, 25, (T, N, Hs), generator=g).int())


def test_the_knowledge_fields_travel_through_take_split_and_batches():
    d = synthetic()
    rows = torch.tensor([4, 1, 3])
    t = d.take(rows)
    for name in ("pool", "compat", "cards"):
        assert torch.equal(getattr(t, name), getattr(d, name)[:, rows]) and getattr(t, name).dtype == getattr(d, name).dtype
    train, held = d.split(0.34, 3)
    assert train.n_rows + held.n_rows == d.n_rows and held.n_rows == 2
    held_game = int(held.game[0])
    sel = d.game == held_game
    assert torch.equal(held.pool, d.pool[:, sel]) and torch.equal(held.cards, d.cards[:, sel]) and torch.equal(train.compat, d.compat[:, ~sel])
    seen = []
    for batch, weight, index in d.batches(4, 1):
        assert batch["pool"].shape == (d.T, 4) and batch["pool"].dtype == torch.int64
        assert batch["compat"].shape == batch["cards"].shape == (d.T, 4, 3) and batch["cards"].dtype == torch.int32
        for k, i in enumerate(index.tolist()):
            if i >= 0:
                assert torch.equal(batch["pool"][:, k], d.pool[:, i]) and torch.equal(batch["compat"][:, k], d.compat[:, i])
                assert torch.equal(batch["cards"][:, k], d.cards[:, i])
                seen.append(i)
            else:      # a padding column: weight 0, seq_len 0 -- never read
                assert float(weight[k]) == 0.0 and float(batch["seq_len"][k]) == 0.0 and not bool(batch["pool"][:, k].any())
    assert sorted(seen) == list(range(d.n_rows))
    # without the fields nothing changes
    plain = CloneDataset(d.priv_s, None, d.legal_move, d.a, d.seq_len, d.game, d.seat)
    assert plain.pool is None and plain.take(rows).cards is None
    assert all("pool" not in b for b, _, _ in plain.batches(4, 1))
    with pytest.raises(ValueError, match="knowledge"):
        next(belief.belief_batches(plain, torch.zeros(d.T, d.n_rows, 64, dtype=torch.bfloat16), 4, 1))
    o16 = torch.arange(d.T * d.n_rows * 2, dtype=torch.float32).view(d.T, d.n_rows, 2).to(torch.bfloat16)
    for (b, w), (_, _, index) in zip(belief.belief_batches(d, o16, 4, 1), d.batches(4, 1)):
        assert set(b) == {"o16", "pool", "compat", "cards", "seq_len"}
        assert torch.equal(b["o16"], o16[:, index.clamp(min=0)]) and torch.equal(w, (index >= 0).float())


def test_the_saved_head_round_trips_and_is_held_to_its_shape(tmp_path):
    g = torch.Generator().manual_seed(1)
    sd = {"belief.weight": torch.randn(100, 64, generator=g), "belief.bias": torch.randn(100, generator=g), "hand_size": 4, "H": 64}
    path = str(tmp_path / "belief.pthw")
    torch.save(sd, path)
    back = torch.load(path, map_location="cpu")
    assert belief.check_state(back) == (4, 64) and belief.check_state(back, 4, 64) == (4, 64)
    assert torch.equal(back["belief.weight"], sd["belief.weight"]) and torch.equal(back["belief.bias"], sd["belief.bias"])
    for bad in (dict(sd, hand_size=5), dict(sd, H=128), {k: v for k, v in sd.items() if k != "belief.bias"}, dict(sd, hand_size=0),
                dict(sd, **{"belief.bias": sd["belief.bias"][:-1]})):
        with pytest.raises(ValueError):
            belief.check_state(bad)
    with pytest.raises(ValueError, match="saved head"):
        belief.check_state(sd, 5, 64)
    with pytest.raises(ValueError, match="saved head"):
        belief.check_state(sd, 4, 128)


def test_command_line_errors(tmp_path):
    from hanabi_sad_amd.checkpoint import save_weights
    from hanabi_sad_amd.selfplay import init_weights
    blueprint = str(tmp_path / "b.pthw")
    save_weights(init_weights(838, 64, 21, 5, 0), blueprint)
    games = str(tmp_path / "g.jsonl")
    open(games, "w").close()
    for argv, text in (([], "--blueprint"), (["--blueprint", str(tmp_path / "none.pthw"), "--teacher", "piers"], "no such weight file"),
                       (["--blueprint", blueprint], "either --games"), (["--blueprint", blueprint, "--games", games, "--teacher", "piers"], "either --games"),
                       (["--blueprint", blueprint, "--teacher", "piers", "--lr", "0"], "--lr"),
                       (["--blueprint", blueprint, "--teacher", "piers", "--lr", "nan"], "--lr"),
                       (["--blueprint", blueprint, "--teacher", "piers", "--holdout", "1"], "--holdout"),
                       (["--blueprint", blueprint, "--games", str(tmp_path / "none.jsonl")], "no such file"),
                       (["--blueprint", blueprint, "--teacher", "nobody"], "no rule-bot preset")):
        with pytest.raises(SystemExit) as e:
            belief.main(argv)
        assert text in str(e.value), (argv, str(e.value))
    args = belief.parse_args(["--blueprint", "x", "--teacher", "piers", "a.pthw"])
    assert args.teacher == ["piers", "a.pthw"] and args.lr == 1e-3 and args.holdout == 0.1 and args.sad == 1
    assert np.isfinite(args.eps)
