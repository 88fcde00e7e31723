"""The pipelined persistent rollout builds its observation rows in registers at fixed bit positions and places them with one
shifted write (csrc/hsad_obs_row.h; env_rollout_pipe_kernel<2,5>, <3,5>, <4,4>, <5,4>), where every other kernel scatters field by
field (build_rows).  Here the two meet on the device: an env on the pipelined path and a twin on the launch-per-iteration path
(chunk 0, env_kernel: the scatter form), compared byte for byte after every launch.

* G = 69: one full 64-game workgroup and one of 5 games, 128 threads; the last row of the full workgroup ends on the last word of
  the LDS bit rows.
* chunks 1, 2 and 7: both row copies, a first `all` stream per launch, odd and even last iterations.
* every instance, SAD and colour shuffle on and off; max_len 3, so that games end and restart inside the launches.
* hand-set positions (position.Position) at the extremes of the row's sections: empty and full deck, a colour's discards at full
  width, information 0 and 8, life 1 and 3, fireworks 0 and 5, a short hand, cards fully hinted and cards nothing is known of,
  every type of last move.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, the actions and the exported state planes.  The header itself is
held to the scatter form, word for word and without a device, in test_obs_row_cpu.py."""
import pytest
import torch

from hanabi_sad_amd import position

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda:0"
EPS = [0.1 ** (1 + 7 * i / 79) for i in range(80)]
SEED, PSEED = 977, 53
G = 69
LAUNCHES = 4
CHUNKS = (1, 2, 7)
INSTANCES = [(2, 5), (3, 5), (4, 4), (5, 4)]


def make(players, hand_size, sad, shuffle, chunk, max_len=3):
    from hanabi_sad_amd import BatchedHanabiEnv
    e = BatchedHanabiEnv(G, players=players, hand_size=hand_size, sad=sad, shuffle_color=shuffle, seed=SEED, eps_list=EPS,
                         max_len=max_len, device=DEV, track_deck_history=False, games_per_workgroup=64, threads_per_workgroup=128)
    assert e.games_per_workgroup == 64 and e.threads_per_workgroup == 128
    e.set_rollout_chunk(chunk)
    return e


def outputs(e):
    torch.cuda.synchronize()
    e.check_errors()
    out = {"priv_s": e.priv_s, "legal_move": e.legal_move, "own_hand": e.own_hand, "eps": e.eps, "reward": e.reward,
           "terminal": e.terminal, "a": e.a, "greedy_a": e.greedy_a, "state": e.export_state()}
    return {k: v.clone() for k, v in out.items()}


def assert_same(ref, got, what):
    assert ref.keys() == got.keys()
    for k in ref:
        assert torch.equal(ref[k], got[k]), "%s: %s differs" % (what, k)


_REFS = {}


def reference(players, hand_size, sad, shuffle):
    """the twin: one launch per iteration (env_kernel, the scatter build); its outputs after every iteration count a launch of one of
    CHUNKS ends on, computed once per configuration, and whether any game ended before the last of them"""
    key = (players, hand_size, sad, shuffle)
    if key not in _REFS:
        e = make(players, hand_size, sad, shuffle, 0)
        wanted = {c * k for c in CHUNKS for k in range(1, LAUNCHES + 1)}
        snaps, ended = {}, 0
        for it in range(1, max(wanted) + 1):
            e.rollout_random(1, PSEED)
            if it in wanted:
                snaps[it] = outputs(e)
            if it < max(wanted):
                ended += int(e.terminal.sum().item())
        _REFS[key] = (snaps, ended)
    return _REFS[key]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("sad", [False, True])
@pytest.mark.parametrize("players,hand_size", INSTANCES)
def test_rows_are_those_of_the_scatter_build_after_every_launch(players, hand_size, sad, shuffle, chunk):
    snaps, ended = reference(players, hand_size, sad, shuffle)
    assert ended >= G            # max_len 3: every game has ended, and restarted in the iteration after, well before the last launch
    e = make(players, hand_size, sad, shuffle, chunk)
    for k in range(1, LAUNCHES + 1):
        e.rollout_random(chunk, PSEED)       # one launch of `chunk` iterations
        assert_same(snaps[chunk * k], outputs(e), "<%d,%d> sad=%s shuffle=%s chunk %d, launch %d"
                    % (players, hand_size, sad, shuffle, chunk, k))


# ---- hand-set positions at the extremes of the sections ---------------------------------------------------------------------
RULES = dict(players=2, hand_size=5, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3)
PERMS = [[2, 0, 4, 1, 3], [4, 3, 2, 1, 0]]
COPIES = [3, 2, 2, 2, 1]


def hinted(c, r):
    return position.Card(c, r, colours=1 << c, ranks=1 << r, hinted_colour=c, hinted_rank=r)


def extreme_positions():
    out = []
    # the end of a game: deck empty, three fireworks complete and two at 0, every card of colour 4 discarded (its thermometers at
    # full width), no information token, one life, one hand a card short; seat 0's cards fully hinted, nothing known of seat 1's
    disc = [(c, r) for c in range(3) for r, n in enumerate(COPIES) for _ in range(n - 1)]
    disc += [(4, r) for r, n in enumerate(COPIES) for _ in range(n)] + [(3, 0)]
    out.append(position.Position(RULES, [[hinted(3, r) for r in range(5)], [(3, 0), (3, 1), (3, 2), (3, 3)]], fireworks=[5, 5, 5, 0, 0],
                                 discards=disc, info=0, life=1, mover=0, turns_to_play=1, num_step=0, perms=PERMS,
                                 last_move=dict(type="hint_rank", player=1, target_offset=1, value=4, reveal_mask=16)))
    # the start of one: full deck, nothing played or discarded, every token, no last move
    hands = [[(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)], [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)]]
    out.append(position.Position(RULES, hands, perms=PERMS))
    # in between, one per remaining type of last move, at the widest values of its fields
    mid = dict(fireworks=[1, 2, 3, 4, 0], discards=[(4, 0), (4, 0), (4, 4), (0, 1)], info=4, life=2, perms=PERMS)
    hands = [[(0, 2), hinted(1, 3), (2, 4), (3, 4), (4, 1)], [(0, 4), (1, 4), (4, 3), hinted(4, 2), (0, 3)]]
    out.append(position.Position(RULES, hands, mover=1, last_move=dict(type="play", player=0, card_index=4, colour=4, rank=4, scored=1,
                                                                       info_token=1), **mid))
    out.append(position.Position(RULES, hands, mover=0, last_move=dict(type="discard", player=1, card_index=4, colour=4, rank=4,
                                                                       info_token=1), **mid))
    out.append(position.Position(RULES, hands, mover=0, last_move=dict(type="hint_colour", player=1, target_offset=1, value=4,
                                                                       reveal_mask=31), **mid))
    return out


def test_hand_set_positions_at_the_section_extremes():
    flags = dict(max_len=80, shuffle_color=True)
    records = [p.to_record() for p in extreme_positions()]
    for r in records:
        assert position.validate(r, RULES, flags) == 0, position.explain(position.validate(r, RULES, flags))
    states = torch.tensor([records[g % len(records)].tolist() for g in range(G)], dtype=torch.int32)
    seeds = torch.arange(G, dtype=torch.int32) + 31           # the same position under different moves
    envs = {}
    for chunk in (0,) + CHUNKS:
        e = make(2, 5, True, True, chunk, max_len=80)
        status = e.import_state(states, seeds=seeds)
        assert not status.any().item(), status
        envs[chunk] = e
    ref = {}
    twin = envs[0]
    for it in range(1, 2 * max(CHUNKS) + 1):     # the first rows built are those after the move out of the position
        twin.rollout_random(1, PSEED)
        ref[it] = outputs(twin)
    for chunk in CHUNKS:
        for k in (1, 2):
            envs[chunk].rollout_random(chunk, PSEED)
            assert_same(ref[chunk * k], outputs(envs[chunk]), "positions, chunk %d, launch %d" % (chunk, k))
