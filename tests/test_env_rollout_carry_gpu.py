"""What the pipelined persistent rollout (env_rollout_pipe_kernel) carries from one iteration of a launch to the next instead of
reading it back from global memory (LogicCarry, csrc/hsad_env.hip): each lane's act counter, in a register from the launch's
prologue to its last iteration, and the legal masks the policy reads, which build_rows leaves in the lane's own column of the
mt19937 prefetch window in LDS.  The eps list is read from its LDS copy with an LDS instruction.

* bit identity against the launch-per-iteration rollout (chunk 0) and the single-phase persistent kernel (HSAD_ENV_PIPE=0) over
  chunk lengths (1: prologue load and epilogue store with nothing carried; 2, 3: one or two carried iterations), partial workgroups,
  every (players, hand) instantiation in 32- and 64-game workgroups, SAD, colour shuffle, deck history and the delta stream on / off,
* games that restart every few iterations: lanes that recompute their masks (and use their window column) next to lanes that read
  the stored ones, in every wave and iteration,
* launch edges against the other entry points (step with policy_random, reset, export, fork): a counter or a mask that is not
  written back, or read stale, at the edge of a launch shows in the next call's actions,
* LDS bytes per workgroup (hsad_env_rollout_lds_bytes) and resident workgroups per CU (hsad_env_rollout_resident_workgroups: the
  runtime's occupancy query for the kernel the env launches) of every configuration this file runs are what they were before the
  masks had a home in LDS (the window column costs nothing): constants read once on the parent commit.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, the sampled actions a / greedy_a and the exported state."""
import os
import weakref

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
EPS = [0.1 ** (1 + 7 * i / 79) for i in range(80)]
SEED, PSEED = 4242, 91


_TRACKED = weakref.WeakSet()          # the envs made with deck history


def make(G, players=2, hand_size=5, sad=False, shuffle_color=False, gpw=64, chunk=0, delta=True, max_len=80, seed=SEED, pipe=True,
         track=False):
    from hanabi_sad_amd import BatchedHanabiEnv
    old = os.environ.get("HSAD_ENV_PIPE")
    os.environ["HSAD_ENV_PIPE"] = "1" if pipe else "0"   # read when the env is created
    try:
        e = BatchedHanabiEnv(G, players=players, hand_size=hand_size, sad=sad, shuffle_color=shuffle_color, seed=seed, eps_list=EPS,
                             max_len=max_len, device=DEV, track_deck_history=track, games_per_workgroup=gpw,
                             threads_per_workgroup=128)
    finally:
        if old is None:
            del os.environ["HSAD_ENV_PIPE"]
        else:
            os.environ["HSAD_ENV_PIPE"] = old
    assert e.games_per_workgroup == gpw and e.threads_per_workgroup == 128
    e.set_rollout_chunk(chunk)
    e.set_rollout_delta(delta)
    if track:
        _TRACKED.add(e)
    return e


def outputs(e):
    torch.cuda.synchronize()
    e.check_errors()
    out = {"priv_s": e.priv_s, "legal_move": e.legal_move, "own_hand": e.own_hand, "eps": e.eps, "reward": e.reward,
           "terminal": e.terminal, "a": e.a, "greedy_a": e.greedy_a, "state": e.export_state()}
    if e in _TRACKED:
        out["deck_history"], out["deck_history_count"] = e.deck_history()
    return {k: v.clone() for k, v in out.items()}


def assert_same(ref, got, what):
    assert ref.keys() == got.keys()
    for k in ref:
        assert torch.equal(ref[k], got[k]), "%s: %s differs" % (what, k)


def run(e, blocks):
    for n in blocks:
        e.rollout_random(n, PSEED)
    return outputs(e)


# what the tests below build their envs with, besides SHAPES: the residency test at the end pins every one of them
BASE_KW = dict()
HISTORY_KW = dict(track=True, shuffle_color=True)
RESTART_KW = {m: dict(max_len=m, sad=True, shuffle_color=True) for m in (3, 5)}
EDGE_KW = dict(sad=True, shuffle_color=True)
BLOCKS = (45, 28)        # at chunk 20: launches of 20 + 20 + 5, then 20 + 8
_REFS = {}


def reference(G, blocks=BLOCKS, **kw):
    """the launch-per-iteration rollout of the same games: computed once per configuration"""
    key = (G, blocks, tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = run(make(G, **kw), blocks)
    return _REFS[key]


def check_all_schedules(G, chunk, blocks=BLOCKS, **kw):
    ref = reference(G, blocks, **kw)
    what = "G=%d chunk=%d %s" % (G, chunk, kw)
    for delta in (True, False):
        assert_same(ref, run(make(G, chunk=chunk, delta=delta, **kw), blocks), what + " pipelined, delta=%s" % delta)
    assert_same(ref, run(make(G, chunk=chunk, pipe=False, **kw), blocks), what + " single-phase")


@pytest.mark.parametrize("G", [192, 100])            # three workgroups; a partial last workgroup (36 games)
@pytest.mark.parametrize("chunk", [1, 2, 3, 7, 20])
def test_chunk_lengths(G, chunk):
    check_all_schedules(G, chunk, **BASE_KW)


SHAPES = [  # (players, hand, games per workgroup, sad, colour shuffle): every instantiation in both workgroup shapes, and per
            # instantiation every combination of SAD and colour shuffle
    (2, 5, 64, True, False), (2, 5, 64, False, True), (2, 5, 32, True, True), (2, 5, 32, False, False),
    (3, 5, 32, True, False), (3, 5, 32, False, True), (3, 5, 64, True, True), (3, 5, 64, False, False),
    (4, 4, 64, True, False), (4, 4, 64, False, True), (4, 4, 32, True, True), (4, 4, 32, False, False),
    (5, 4, 32, True, False), (5, 4, 32, False, True), (5, 4, 64, True, True), (5, 4, 64, False, False),
]


@pytest.mark.parametrize("G", [192, 100])
@pytest.mark.parametrize("P,H,gpw,sad,shuffle", SHAPES)
def test_every_instantiation_sad_and_colour_shuffle(G, P, H, gpw, sad, shuffle):
    check_all_schedules(G, 20, players=P, hand_size=H, sad=sad, shuffle_color=shuffle, gpw=gpw)


def test_deck_history_tracked():
    check_all_schedules(100, 7, **HISTORY_KW)


@pytest.mark.parametrize("max_len", [3, 5])
def test_games_restart_every_few_iterations(max_len):
    """Every game ends by its max_len-th move and restarts in the iteration after, so in 40 iterations it restarts at least
    40 / max_len - 1 >= 7 times, and only a restart in the first iteration of a 7-iteration launch (iterations 0, 7, 14, ...: at most
    six of them) is not inside a launch: the bound below holds for any seed; it is asserted on what the games did.  Games that start
    together end together, so game j starts from a fork of a game that has already made 1 + j % max_len moves: every wave then has
    lanes that restart next to lanes that do not in every iteration."""
    G, chunk, n = 192, 7, 40
    kw = RESTART_KW[max_len]
    srcs = []
    for k in range(max_len):
        src = make(G, seed=SEED + 7, **kw)
        src.rollout_random(1 + k, PSEED + 1)
        idx = torch.arange(G, dtype=torch.int32)
        idx[idx % max_len != k] = -1
        srcs.append((src, idx))

    def staggered(**mk):
        e = make(G, **kw, **mk)
        for src, idx in srcs:
            e.fork_from(src, idx)
        return e

    r = staggered()
    term = []
    for _ in range(n):
        r.rollout_random(1, PSEED)
        term.append(r.terminal.clone())
    ref = outputs(r)
    term = torch.stack(term).cpu().numpy().astype(bool)                     # [iteration, game]
    inside = np.array([(i + 1) % chunk != 0 for i in range(n - 1)])         # the restart in iteration i + 1 is not a launch's first
    restarts_inside = (term[:n - 1] & inside[:, None]).sum(axis=0)
    mixed = np.mean([(t.reshape(-1, 64).any(axis=1) & ~t.reshape(-1, 64).all(axis=1)).mean() for t in term])
    print("restarts inside launches per game: min %d median %d; share of (wave, iteration) with both kinds of lane %.2f"
          % (restarts_inside.min(), np.median(restarts_inside), mixed))
    assert (restarts_inside >= 2).sum() > G // 2
    assert mixed > 0.9
    for delta in (True, False):
        assert_same(ref, run(staggered(chunk=chunk, delta=delta), (n,)), "max_len %d, delta=%s" % (max_len, delta))
    assert_same(ref, run(staggered(chunk=chunk, pipe=False), (n,)), "max_len %d, single-phase" % max_len)


def test_launch_edges_against_the_other_entry_points():
    """(step() takes no finished game, so every policy_random + step is preceded by reset(), which restarts the games that have
    ended and those only: the masks and counters of the running games still cross the edge from the rollout untouched)"""
    G = 100
    kw = EDGE_KW
    src = make(G, seed=SEED + 1, **kw)
    src.rollout_random(6, PSEED + 1)
    idx = torch.full((G,), -1, dtype=torch.int32)
    idx[[3, 64, 70, 99]] = torch.tensor([5, 5, 90, 0], dtype=torch.int32)
    envs = {"chunk 0": make(G, **kw), "pipelined": make(G, chunk=20, **kw), "pipelined, full stream": make(G, chunk=20, delta=False, **kw),
            "single-phase": make(G, chunk=20, pipe=False, **kw)}

    def step_with_policy(e):
        e.reset()                       # (restarts the games that have ended, and those only: step() takes no finished game)
        a, g = e.policy_random(PSEED)
        e.step(a, g)

    calls = [("rollout 3", lambda e: e.rollout_random(3, PSEED)), ("policy + step", step_with_policy), ("policy + step", step_with_policy),
             ("rollout 4", lambda e: e.rollout_random(4, PSEED)), ("reset", lambda e: e.reset()),
             ("rollout 5", lambda e: e.rollout_random(5, PSEED)), ("export", lambda e: e.export_state()),
             ("fork", lambda e: e.fork_from(src, idx)), ("rollout 2", lambda e: e.rollout_random(2, PSEED)),
             ("policy + step", step_with_policy), ("rollout 1", lambda e: e.rollout_random(1, PSEED))]
    for k, (name, call) in enumerate(calls):
        outs = {}
        for what, e in envs.items():
            call(e)
            outs[what] = outputs(e)
        for what in envs:
            assert_same(outs["chunk 0"], outs[what], "after call %d (%s), %s" % (k, name, what))


# Every configuration this file runs: SHAPES and the named ones above, each with the delta stream asked for and not.
def shape_kw(P, H, gpw, sad, shuffle):
    return dict(players=P, hand_size=H, gpw=gpw, sad=sad, shuffle_color=shuffle)


def config_key(kw):
    d = dict(players=2, hand_size=5, gpw=64, sad=False, shuffle_color=False, max_len=80, track=False)
    d.update(kw)
    return (d["players"], d["hand_size"], d["gpw"], d["sad"], d["shuffle_color"], d["max_len"], d["track"])


KEY_NAMES = ("players", "hand_size", "gpw", "sad", "shuffle_color", "max_len", "track")
CONFIG_KEYS = sorted({config_key(kw) for kw in [shape_kw(*sh) for sh in SHAPES] + [BASE_KW, HISTORY_KW, EDGE_KW] + list(RESTART_KW.values())})


def residency(key):
    """((LDS bytes, delta stream active, resident workgroups per CU) with the delta stream asked for, (bytes, resident) without)"""
    e = make(192, chunk=20, delta=True, **dict(zip(KEY_NAMES, key)))
    on = (int(e.lib.hsad_env_rollout_lds_bytes(e.h)), bool(e.rollout_delta_active()), int(e.lib.hsad_env_rollout_resident_workgroups(e.h)))
    e.set_rollout_delta(False)
    return on, (int(e.lib.hsad_env_rollout_lds_bytes(e.h)), int(e.lib.hsad_env_rollout_resident_workgroups(e.h)))


# residency(key) as read once on the parent of the change that gave the masks their home in LDS (the parent built with the same
# hsad_env_rollout_resident_workgroups query: hipOccupancyMaxActiveBlocksPerMultiprocessor of the kernel the env launches)
# PARENT-BEGIN
PARENT = {(2, 5, 32, False, False, 80, False): ((25472, True, 4), (19184, 4)),
 (2, 5, 32, True, True, 80, False): ((27104, True, 4), (20384, 4)),
 (2, 5, 64, False, False, 80, False): ((38256, True, 4), (25712, 4)),
 (2, 5, 64, False, True, 80, False): ((39024, True, 4), (26480, 4)),
 (2, 5, 64, False, True, 80, True): ((39024, True, 4), (26480, 4)),
 (2, 5, 64, True, False, 80, False): ((40016, True, 4), (26592, 4)),
 (2, 5, 64, True, True, 3, False): ((40784, True, 4), (27360, 4)),
 (2, 5, 64, True, True, 5, False): ((40784, True, 4), (27360, 4)),
 (2, 5, 64, True, True, 80, False): ((40784, True, 4), (27360, 4)),
 (3, 5, 32, False, True, 80, False): ((42256, False, 3), (42256, 3)),
 (3, 5, 32, True, False, 80, False): ((40384, False, 4), (40384, 4)),
 (3, 5, 64, False, False, 80, False): ((53248, False, 3), (53248, 3)),
 (3, 5, 64, True, True, 80, False): ((57168, False, 2), (57168, 2)),
 (4, 4, 32, False, False, 80, False): ((48320, False, 3), (48320, 3)),
 (4, 4, 32, True, True, 80, False): ((52816, False, 3), (52816, 3)),
 (4, 4, 64, False, True, 80, False): ((70976, False, 2), (70976, 2)),
 (4, 4, 64, True, False, 80, False): ((69216, False, 2), (69216, 2)),
 (5, 4, 32, False, True, 80, False): ((68816, False, 2), (68816, 2)),
 (5, 4, 32, True, False, 80, False): ((65392, False, 2), (65392, 2)),
 (5, 4, 64, False, False, 80, False): ((148256, True, 1), (93040, 1)),
 (5, 4, 64, True, True, 80, False): ((157600, True, 1), (100016, 1))}
CONFIGS1 = (128, 64, True, 38256, 4)      # the same for 65,536 two-player games as the library sizes them (bench.py's env)
# PARENT-END


def test_every_configuration_of_this_file_is_pinned():
    assert sorted(PARENT) == CONFIG_KEYS and len(CONFIG_KEYS) >= len(SHAPES) + 4


@pytest.mark.parametrize("key", CONFIG_KEYS)
def test_lds_and_resident_workgroups_are_the_parents(key):
    got = residency(key)
    print("residency %s: %s" % (key, got))
    assert got == PARENT[key]


def configs1_residency():
    from hanabi_sad_amd import BatchedHanabiEnv
    e = BatchedHanabiEnv(65536, seed=SEED, eps_list=EPS, max_len=80, device=DEV, track_deck_history=False)
    e.set_rollout_chunk(50)
    return (e.threads_per_workgroup, e.games_per_workgroup, bool(e.rollout_delta_active()), int(e.lib.hsad_env_rollout_lds_bytes(e.h)),
            int(e.lib.hsad_env_rollout_resident_workgroups(e.h)))


def test_configs1_keeps_four_workgroups_per_cu():
    got = configs1_residency()
    print("configs[1]", got)
    assert got == CONFIGS1 and got[:3] == (128, 64, True) and got[4] == 4
