"""Search distillation end to end on Hanabi-Small (2 colours, hands of 2, 3 information tokens, 1 life; 2 players, sad = 1), 8 deals,
4 worlds per action, a random-weight net: search.play_with_search(records=True) writes the searched games and their action values down
without changing the play; the values are those of a separate search of the same position; clone.search_targets /
sequences_from_records(targets=...) turn them into the dataset's target rows; one epoch over it finds no bad row; and the command line
(--blueprint ... --target_temperature) runs through and leaves a weight file that loads."""
import os

import numpy as np
import pytest
import torch

from tests.search_fixtures import CONFIGS

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"
RULES = {k: v for k, v in CONFIGS["small"].items() if k not in ("players", "hand_size")}
P, HAND = CONFIGS["small"]["players"], CONFIGS["small"]["hand_size"]
GAMES, WORLDS, SEED, SEARCH_SEED, SAD, TAU = 8, 4, 301, 77, True, 0.5


def weights(seed=3):
    from hanabi_sad_amd.eval import env_dims
    from hanabi_sad_amd.selfplay import init_weights
    F, A = env_dims(P, HAND, SAD, **RULES)
    return init_weights(F, 64, A, HAND, seed), F, A


@pytest.fixture(scope="module")
def played():
    from hanabi_sad_amd.search import play_with_search
    W, F, A = weights()
    kw = dict(worlds=WORLDS, search_seed=SEARCH_SEED, num_player=P, hand_size=HAND, device=DEV, **RULES)
    plain = play_with_search(W, GAMES, SEED, 0, SAD, **kw)
    rec = play_with_search(W, GAMES, SEED, 0, SAD, records=True, **kw)
    return W, A, plain, rec


def test_recording_changes_nothing_and_the_records_are_the_games_played(played):
    from hanabi_sad_amd.game_record import GameFilter
    from hanabi_sad_amd.search import play_with_search
    W, A, plain, rec = played
    assert plain.records is None and plain.search_values is None
    assert rec.scores == plain.scores and torch.equal(rec.deviations, plain.deviations) and len(rec.trace) == len(plain.trace)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(rec.trace, plain.trace))
    assert len(rec.records) == GAMES == len(rec.search_values)
    chosen = torch.stack([c for c, _ in rec.trace]).numpy()          # [moves, G]
    blueprint = torch.stack([b for _, b in rec.trace]).numpy()
    searched_moves = 0
    for k, (r, v) in enumerate(zip(rec.records, rec.search_values)):
        r.validate()
        assert r.meta["game"] == k and r.meta["deal_seed"] == SEED + k and r.meta["worlds"] == WORLDS and r.meta["search_seed"] == SEARCH_SEED
        assert r.score == rec.scores[k] and r.rules["colors"] == 2 and r.rules["hand_size"] == HAND
        n = r.n_moves
        assert v.shape == (n, A) and v.dtype == np.float32
        # every seat searches: the move made is search's choice, the greedy move the blueprint's
        assert (chosen[:n, k] >= 0).all() and list(r.moves) == chosen[:n, k].tolist() and list(r.greedy) == blueprint[:n, k].tolist()
        assert (chosen[n:, k] == -1).all()
        game = r._replay(0)                                          # the plain-Python rules GameRecord.position(t) replays with
        for t in range(n):
            legal = np.array([game.illegal(u) is None for u in range(A - 1)] + [False])
            finite = np.isfinite(v[t])
            assert not (finite & ~legal).any(), (k, t)
            assert finite[r.moves[t]] and finite[r.greedy[t]] and (v[t][finite] >= 0).all() and (v[t][finite] <= 10).all()
            searched_moves += 1
            game.apply(r.moves[t])
    assert searched_moves >= GAMES
    assert int(rec.deviations.sum()) == sum(int(m != g) for r in rec.records for m, g in zip(r.moves, r.greedy))
    # one seat searching: the other seat's moves have all-NaN rows and the blueprint's move; a filter takes the place of True
    seat0 = play_with_search(W, GAMES, SEED, 0, SAD, worlds=WORLDS, search_seed=SEARCH_SEED, num_player=P, hand_size=HAND, device=DEV, searcher=0,
                             records=GameFilter.parse("moves>=1"), **RULES)
    assert len(seat0.records) == len(seat0.search_values) == GAMES
    for r, v in zip(seat0.records, seat0.search_values):
        r.validate()
        assert r.score == seat0.scores[r.meta["game"]] and v.shape == (r.n_moves, A)
        assert np.isnan(v[1::2]).all() and np.isfinite(v[0::2]).any(1).all()
        assert list(r.moves[1::2]) == list(r.greedy[1::2])


def test_the_values_of_move_0_are_those_of_a_separate_search(played):
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd.eval import _acting_agent
    from hanabi_sad_amd.search import move_seed, policy_action_values
    W, A, _, rec = played
    agent = _acting_agent(W, "bf16", DEV)
    root = BatchedHanabiEnv(GAMES, players=P, hand_size=HAND, seed=SEED, bomb=0, eps_list=[0.0], max_len=-1, sad=SAD, device=DEV, **RULES)
    try:
        root.reset()
        hid = agent.get_h0(GAMES * P)
        sv = policy_action_values(root, agent, hid, WORLDS, move_seed(SEARCH_SEED, 0), capacity=min(4096, GAMES * (A - 1) * WORLDS))
        want = sv.values.cpu().numpy()
    finally:
        root.close()
    got = np.stack([v[0] for v in rec.search_values])
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(got[np.isfinite(got)], want[np.isfinite(want)])
    assert np.isfinite(got).sum(1).min() >= 2


def test_the_dataset_carries_the_search_targets_and_an_epoch_finds_no_bad_row(played):
    from hanabi_sad_amd import clone
    from hanabi_sad_amd.composite import CompositeLearner
    from hanabi_sad_amd.game_record import capacity
    W, A, _, rec = played
    records, values = rec.records, rec.search_values
    tg = clone.search_targets(records, values, TAU)
    for r, v, t in zip(records, values, tg):      # search_targets is soft_targets on the finite set plus the move made
        legal = np.isfinite(v)
        legal[np.arange(r.n_moves), r.moves] = True
        assert np.array_equal(t, clone.soft_targets(v, legal, np.asarray(r.moves), TAU))
        assert np.abs(t.astype(np.float64).sum(1) - 1).max() <= A * 2.0 ** -23 and not t[~np.isfinite(v)].any()
    ds = clone.sequences_from_records(records, SAD, device=DEV, targets=tg)
    plain = clone.sequences_from_records(records, SAD, device=DEV)
    assert plain.target is None and ds.priv_s is None and plain.priv_s is None
    for k in ("priv_s_bf16", "legal_move", "a", "seq_len", "game", "seat"):
        x, y = getattr(ds, k), getattr(plain, k)
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y), k
    T = capacity(records[0].rules)
    assert ds.target.shape == (T, GAMES * P, A) and ds.target.dtype == torch.float32
    target = ds.target.cpu().numpy()
    noop = np.zeros(A, dtype=np.float32)
    noop[A - 1] = 1.0
    for j, r in enumerate(records):
        n = r.n_moves
        for t in range(n):
            for seat in range(P):
                want = tg[j][t] if seat == t % P else noop
                assert np.array_equal(target[t, j * P + seat], want), (j, t, seat)
        assert not target[n:, j * P:(j + 1) * P].any()
    # no target row carries mass on an illegal action of the position the env replays
    assert not bool(((ds.legal_move == 0) & (ds.target != 0)).any())
    W2, _, _ = weights(seed=9)
    lr = CompositeLearner(W2, W2, 1, 0.999, device=DEV)
    first = clone.run_epoch(lr, ds, 8, 1, True)           # raises if any row was counted bad
    for batch, weight, _ in ds.batches(8, 1):
        _, stats = lr.clone_loss(batch, weight, compute_grad=False)
        assert int(stats["bad"].sum()) == 0 and int(stats["decisions"].sum()) > 0
    kl = first[0] - clone.target_entropy(ds) / first[2]
    print("epoch 0: loss per decision %.4f over %d decisions, KL per decision %.4f" % (first[0], first[2], kl))
    assert first[2] > 0 and kl > -1e-3
    # a target row that is no distribution over the position's legal actions is found by the update
    broken = [t.copy() for t in tg]
    broken[0][0] = 0.0
    illegal = int(torch.nonzero(ds.legal_move[0, 0] == 0)[0, 0])
    broken[0][0, illegal] = 1.0
    bad_ds = clone.sequences_from_records(records, SAD, device=DEV, targets=broken)
    from hanabi_sad_amd._lib import HsadError
    with pytest.raises(HsadError, match="target rows"):
        clone.run_epoch(lr, bad_ds, 8, 1, False)
    lr.close()


def test_the_command_line_distils_a_search_into_a_weight_file(tmp_path):
    from hanabi_sad_amd import clone
    from hanabi_sad_amd.checkpoint import load_weights, save_weights
    W, F, A = weights()
    blueprint = str(tmp_path / "blueprint.pthw")
    save_weights(W, blueprint)
    out = str(tmp_path / "out")
    rc = clone.main(["--blueprint", blueprint, "--search_worlds", str(WORLDS), "--target_temperature", str(TAU), "--num_game", str(GAMES), "--num_epoch", "1",
                     "--sad", "1", "--num_player", str(P), "--hand_size", str(HAND), "--colors", "2", "--ranks", "5", "--max_information_tokens", "3",
                     "--max_life_tokens", "1", "--rnn_hid_dim", "64", "--batchsize", "8", "--num_eval_game", "8", "--holdout", "0.25",
                     "--seed", str(SEED), "--train_device", DEV, "--save_dir", out])
    assert rc == 0
    got = load_weights(os.path.join(out, "clone.pthw"))
    assert set(got) == set(W)
    assert all(torch.isfinite(v.float()).all() for v in got.values())
    assert os.path.exists(os.path.join(out, "games.jsonl")) and os.path.exists(os.path.join(out, "clone_epoch0.pthw"))
