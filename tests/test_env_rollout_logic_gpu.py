"""The logic wave's shortened reset, deal and policy paths (csrc/hsad_env.hip: the wrapped window fetch, the straight deal of a
restart from the look-ahead and the window, csrc/hsad_deal_fast.h's pick and select, the policy keys carried through a launch of
env_rollout_pipe_kernel<2,5>) against the paths they did not touch:

* the pipelined rollout with the fast deal (deal_mode 0) equals, byte for byte and after every launch, a launch-per-iteration env on
  the literal fp64 deal (deal_mode 1) with the same seeds.  A draw leaves the fast band with probability 2^-35, so the two agree
  unless the fast path is wrong.  Shapes: two players with a full and a one-game workgroup, SAD and the colour shuffle on and off;
  five players in 32-game workgroups (the window of more than 32 words); three and four players.  Every game must restart at least
  twice inside launches, or the reset path would not be what is compared.
* the sampled actions equal a plain-Python restatement of the hash and the k-th legal bit, on the legal moves read before the launch.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, a, greedy_a and the exported state."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
EPS = [0.1 ** (1 + 7 * i / 79) for i in range(80)]
SEED, PSEED = 4242, 91
BLOCKS = (57, 46)
CHUNKS = (7, 20)

# name: (games, players, hand, sad, shuffle_color, games per workgroup, seed).  The seeds are chosen on the CPU oracle's games (which
# the kernels reproduce): with them every game restarts at least twice inside launches at both chunks; three players do not with 4242
SHAPES = {
    "2p": (65, 2, 5, False, False, 64, SEED), "2p-sad": (65, 2, 5, True, False, 64, SEED), "2p-shuffle": (65, 2, 5, False, True, 64, SEED),
    "2p-sad-shuffle": (65, 2, 5, True, True, 64, SEED), "5p-gpw32": (33, 5, 4, False, True, 32, SEED), "3p": (64, 3, 5, False, True, 64, 7),
    "4p": (64, 4, 4, True, False, 64, SEED),
}


def make(shape, chunk, deal_mode):
    from hanabi_sad_amd import BatchedHanabiEnv
    G, P, H, sad, sc, gpw, seed = SHAPES[shape] if isinstance(shape, str) else shape
    e = BatchedHanabiEnv(G, players=P, hand_size=H, sad=sad, shuffle_color=sc, seed=seed, eps_list=EPS, max_len=80, device=DEV,
                         track_deck_history=False, deal_mode=deal_mode, games_per_workgroup=gpw, threads_per_workgroup=128)
    assert e.games_per_workgroup == gpw and e.threads_per_workgroup == 128
    e.set_rollout_chunk(chunk)
    return e


def outputs(e):
    torch.cuda.synchronize()
    e.check_errors()
    out = {"priv_s": e.priv_s, "legal_move": e.legal_move, "own_hand": e.own_hand, "eps": e.eps, "reward": e.reward,
           "terminal": e.terminal, "a": e.a, "greedy_a": e.greedy_a, "state": e.export_state()}
    return {k: v.clone() for k, v in out.items()}


def launches(chunk):
    """iterations of every launch of the blocks at this chunk, in order"""
    out = []
    for n in BLOCKS:
        out += [chunk] * (n // chunk) + ([n % chunk] if n % chunk else [])
    return out


_REFS = {}


def reference(shape):
    """the literal deal, one launch per iteration: the outputs after every iteration count at which a launch of either chunk ends,
    and terminal after every iteration.  Computed once per shape."""
    if shape not in _REFS:
        ends = set()
        for chunk in CHUNKS:
            ends.update(np.cumsum(launches(chunk)).tolist())
        e = make(shape, 0, 1)
        snaps, term = {}, []
        for it in range(1, sum(BLOCKS) + 1):
            e.rollout_random(1, PSEED)
            term.append(e.terminal.clone())
            if it in ends:
                snaps[it] = outputs(e)
        _REFS[shape] = (snaps, torch.stack(term).cpu().numpy().astype(bool))
    return _REFS[shape]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pipelined_fast_deal_equals_the_literal_deal_after_every_launch(shape, chunk):
    snaps, term = reference(shape)
    # a game restarts in iteration j when iteration j - 1 ended it; inside a launch unless j is the launch's first iteration
    first = np.zeros(term.shape[0], dtype=bool)
    first[np.cumsum([0] + launches(chunk))[:-1]] = True
    inside = (term[:-1] & ~first[1:, None]).sum(axis=0)
    print("%s chunk %d: restarts inside launches per game: min %d, mean %.1f" % (shape, chunk, inside.min(), inside.mean()))
    assert inside.min() >= 2, "a game that restarted fewer than twice inside launches"
    e = make(shape, chunk, 0)
    done = 0
    for n in launches(chunk):
        e.rollout_random(n, PSEED)          # one launch
        done += n
        got, ref = outputs(e), snaps[done]
        for k in ref:
            assert torch.equal(ref[k], got[k]), "%s chunk %d: %s differs after %d iterations" % (shape, chunk, k, done)


M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def policy_hash(seed, game, counter, stream):
    k = mix64(seed ^ mix64((game * 0xD1342543DE82EF95 + stream) & M64))
    return mix64((k + counter) & M64) >> 32


def kth_legal(legal_row, h):
    uids = [u for u, v in enumerate(legal_row) if v]
    return uids[h % len(uids)]


def test_policy_equals_the_restated_hash_on_the_legal_moves_before_the_launch():
    """64 games, 30 launches of one iteration; a second env runs the same iterations three to a launch in the pipelined kernel (the
    carried keys and counter) and must hold the same actions whenever both stand at the same iteration"""
    G, P = 64, 2
    shape = (G, P, 5, True, False, 64, SEED)
    e, pipe = make(shape, 0, 0), make(shape, 3, 0)
    checked = 0
    for it in range(30):
        torch.cuda.synchronize()
        legal = e.legal_move.cpu().numpy()
        fresh = e.terminal.cpu().numpy().astype(bool) if it else np.ones(G, dtype=bool)   # restarts first: its legal moves are not these
        e.rollout_random(1, PSEED)
        torch.cuda.synchronize()
        e.check_errors()
        a, ga = e.a.cpu().numpy(), e.greedy_a.cpu().numpy()
        for g in np.flatnonzero(~fresh):
            for p in range(P):
                assert a[g, p] == kth_legal(legal[g, p], policy_hash(PSEED, int(g), it, 2 * p)), (it, g, p)
                assert ga[g, p] == kth_legal(legal[g, p], policy_hash(PSEED, int(g), it, 2 * p + 1)), (it, g, p)
                checked += 1
        if it % 3 == 2:
            pipe.rollout_random(3, PSEED)
            torch.cuda.synchronize()
            pipe.check_errors()
            assert torch.equal(pipe.a, e.a) and torch.equal(pipe.greedy_a, e.greedy_a), it
    assert checked >= G * P * 20      # most games are in mid-play at most iterations
