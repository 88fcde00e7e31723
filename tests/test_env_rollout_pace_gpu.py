"""Pacing of the persistent rollout (pace_delay in csrc/hsad_env.hip): workgroups ahead of the launch's mean progress delay their
observation stream.  It may change timing only, so everything here is an equality:

* pace on = pace off = launch per iteration, bit for bit, at the smallest shapes where the host's tracking of the counter base
  (carried over launches of 5, 5, 3 and 5, 4 iterations and over two calls), the partial last workgroup and the hand-off of the
  delay through LDS can go wrong,
* a hostile base (every workgroup far ahead, far behind, half of them ahead) changes nothing, and the delays are capped,
* reset, step, a launch-per-iteration rollout, a reseed and a second env leave the device word equal to the host's record,
* so does switching the pacing off and on between calls.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, a, greedy_a and the exported state."""
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda:0"
EPS = [0.1 ** (1 + 7 * i / 79) for i in range(80)]
SEED, PSEED = 4242, 91
G65 = 4096 + 37          # 65 workgroups of 64 games, the last one partial
BLOCKS, CHUNK = (13, 9), 5


def make(G, chunk=CHUNK, pace=True, pipe=True, seed=SEED, **kw):
    from hanabi_sad_amd import BatchedHanabiEnv
    old = {k: os.environ.get(k) for k in ("HSAD_ENV_PIPE", "HSAD_ENV_PACE")}
    os.environ["HSAD_ENV_PIPE"] = "1" if pipe else "0"     # both read when the env is created
    os.environ["HSAD_ENV_PACE"] = "1" if pace else "0"
    try:
        e = BatchedHanabiEnv(G, seed=seed, eps_list=EPS, max_len=80, device=DEV, track_deck_history=False, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
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


def assert_word(e, expect=None):
    word, base = e.debug_pace_word()
    assert word == base, "device word %d, host base %d" % (word, base)
    if expect is not None:
        assert base == expect, "host base %d, expected %d" % (base, expect)


def run(e, blocks=BLOCKS):
    for n in blocks:
        e.rollout_random(n, PSEED)
    return outputs(e)


def paced_iterations(n, chunk=CHUNK):
    """iterations of an n-iteration call that run in persistent launches: a last launch of one iteration is an ordinary one"""
    return n - (1 if n % chunk == 1 else 0)


def n_blocks(e):
    return (e.G + e.games_per_workgroup - 1) // e.games_per_workgroup


SHAPES = {  # name: (games, constructor arguments)
    "65_blocks_2p_hand5": (G65, dict(games_per_workgroup=64, threads_per_workgroup=128)),
    "one_block_32_games": (32, dict(games_per_workgroup=32, threads_per_workgroup=128)),
    "5p_hand4_sad_shuffle": (2048 + 37, dict(players=5, hand_size=4, sad=True, shuffle_color=True, games_per_workgroup=32,
                                             threads_per_workgroup=128)),
}


@pytest.fixture(scope="module")
def unpaced():
    """per shape: outputs of the launch-per-iteration rollout (the reference of every test of that shape)"""
    cache = {}

    def get(name):
        if name not in cache:
            G, kw = SHAPES[name]
            cache[name] = run(make(G, chunk=0, pace=False, **kw))
        return cache[name]
    return get


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("pipe", [True, False])
def test_pace_on_off_and_per_iteration_are_bit_identical(unpaced, shape, pipe):
    G, kw = SHAPES[shape]
    ref = unpaced(shape)
    off = make(G, pace=False, pipe=pipe, **kw)
    assert_same(ref, run(off), "%s, pace off" % shape)
    assert_word(off, 0)                                  # an unpaced launch never touches the word
    on = make(G, pace=True, pipe=pipe, **kw)
    assert on.threads_per_workgroup == 128
    assert_same(ref, run(on), "%s, pace on" % shape)
    assert_word(on, n_blocks(on) * sum(BLOCKS))          # launches of 5, 5, 3 and 5, 4: only workgroups with games count


def timed_launch(e, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    e.rollout_random(n, PSEED)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3       # us


@pytest.mark.parametrize("bias", [10 ** 9, -10 ** 9, "half"])
def test_hostile_bias_changes_nothing_and_delays_are_capped(unpaced, bias):
    shape = "65_blocks_2p_hand5"
    G, kw = SHAPES[shape]
    ref = unpaced(shape)
    e = make(G, pace=True, **kw)
    nb = n_blocks(e)
    # +-10^9: leads no launch could produce.  "half": every lead reads half an iteration too high; workgroups in step see leads of
    # (-0.5, 0.5] in their order of arrival, so the half that arrives first looks ahead of the mean
    e.debug_pace_bias(nb // 2 if bias == "half" else bias)
    assert_same(ref, run(e), "bias %s" % bias)
    assert_word(e, nb * sum(BLOCKS))
    if bias == 10 ** 9:
        # a 10-iteration launch under that lie, and under the worst lie a launch still believes (every workgroup 9 iterations
        # ahead from the first iteration on: every delay at its cap): sleeps are bounded per iteration and depend on no other
        # workgroup, so neither takes longer than the unpaced launch plus twice 10 caps
        e.set_rollout_chunk(10)
        cap = e.rollout_pace_cap_us()
        assert 0 < cap <= 100
        off = make(G, pace=False, **kw)
        run(off)                                                      # the unpaced twin: the same launches throughout
        off.set_rollout_chunk(10)
        timed_launch(off, 10), timed_launch(e, 10)                    # warm both
        t_off = min(timed_launch(off, 10) for _ in range(3))
        t_far = min(timed_launch(e, 10) for _ in range(3))
        assert_same(outputs(off), outputs(e), "after the timed launches, bias +10^9")
        e.debug_pace_bias(9 * nb)
        t_nine = min(timed_launch(e, 10) for _ in range(3))
        t_off = min([t_off] + [timed_launch(off, 10) for _ in range(3)])
        print("10-iteration launch: unpaced %.1f us, bias +1e9 %.1f us, bias 9 iterations %.1f us, cap %d us" % (t_off, t_far, t_nine, cap))
        assert t_far < t_off + 2 * 10 * cap
        assert t_nine < t_off + 2 * 10 * cap
        assert_same(outputs(off), outputs(e), "after the timed launches, bias of 9 iterations")


def test_mixed_use_keeps_word_and_base_consistent():
    G, kw = SHAPES["65_blocks_2p_hand5"]
    envs = {pace: make(G, pace=pace, **kw) for pace in (True, False)}
    other = make(1024 + 5, pace=True, seed=7, games_per_workgroup=64, threads_per_workgroup=128)   # a second env: its own word
    nb, nb_other = n_blocks(envs[True]), n_blocks(other)
    expect = 0
    for step in ("rollout 7", "reset", "rollout 5", "step", "per-iteration 4", "rollout 6", "reseed", "reset", "rollout 11"):
        for pace, e in envs.items():
            what, _, n = step.partition(" ")
            if what == "rollout":
                e.set_rollout_chunk(CHUNK)
                e.rollout_random(int(n), PSEED)
            elif what == "per-iteration":
                e.set_rollout_chunk(0)
                e.rollout_random(int(n), PSEED)
            elif what == "reset":
                e.reset()
            elif what == "reseed":
                e.reseed(99, 16)
            else:
                e.reset()                                   # finished games restart before actions are chosen for them
                a, ga = e.policy_random(PSEED + 1)
                e.step(a.clone(), ga.clone())
        what, _, n = step.partition(" ")
        if what == "rollout":
            expect += nb * paced_iterations(int(n))
            other.rollout_random(3, PSEED)
            assert_word(other, nb_other * 3 * (1 + ["rollout 7", "rollout 5", "rollout 6", "rollout 11"].index(step)))
        assert_word(envs[True], expect)
        assert_word(envs[False], 0)
        assert_same(outputs(envs[False]), outputs(envs[True]), "after %s" % step)


def test_run_time_switch_keeps_word_base_and_results_consistent(unpaced):
    shape = "65_blocks_2p_hand5"
    G, kw = SHAPES[shape]
    e = make(G, pace=True, **kw)
    nb = n_blocks(e)
    e.set_rollout_pace(False)
    e.rollout_random(4, PSEED)
    assert_word(e, 0)
    e.set_rollout_pace(True)
    e.rollout_random(9, PSEED)                          # launches of 5 and 4
    assert_word(e, nb * 9)
    e.set_rollout_pace(False)
    e.rollout_random(3, PSEED)
    assert_word(e, nb * 9)
    e.set_rollout_pace(True)
    e.rollout_random(6, PSEED)                          # 5 and a single iteration, which never takes a persistent kernel
    assert_word(e, nb * 14)
    assert sum(BLOCKS) == 4 + 9 + 3 + 6
    assert_same(unpaced(shape), outputs(e), "pace switched off and on")
