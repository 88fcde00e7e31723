"""Wave priority in the pipelined persistent rollout (hsad_env_set_rollout_prio, HSAD_ENV_PRIO; include/hsad.h): at the top of every
iteration each wave of env_rollout_pipe_kernel sets its priority to (role ? 2 * is_stream_wave : 0) + (alternation ?
(iteration ^ hardware wave slot) & 1 : 0).  Priority decides which of the two waves of a SIMD issues first and nothing else, so

* every mode 0-3 gives, byte for byte, what mode 0 gives and what the launch-per-iteration rollout of the same games gives, after
  every call and for every bound output: for every pipelined instance (<2,5>, <3,5>, <4,4>, <5,4> and the generic one), with SAD
  and colour shuffle on and off, with one full workgroup plus one of five games (G = 69) and with four (G = 256), in calls of 1, 2
  and 7 iterations per launch (both iteration parities) and in a call of three chained launches, with games that restart inside
  the launches,
* hsad_env_rollout_prio returns what was set, and 0 wherever the pipelined kernel does not run,
* the mode bits ride in EnvParams::delta and cost neither LDS nor residency: hsad_env_rollout_lds_bytes and
  hsad_env_rollout_resident_workgroups are the values tests/test_env_rollout_carry_gpu.py holds.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, the sampled actions a / greedy_a and the exported state."""
import pytest
import torch

from tests.test_env_rollout_carry_gpu import CONFIGS1, PARENT

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
EPS = [0.1 ** (1 + 7 * i / 79) for i in range(80)]
SEED, PSEED = 977, 23
MAX_LEN = 5                      # every game ends by its fifth move: restarts in every launch of 7 iterations
MODES = (0, 1, 2, 3)
# (iterations per launch, iterations of the call): launches of 1; one launch of 2; one of 7; three chained launches of 7
CALLS = ((1, 3), (2, 2), (7, 7), (7, 21))
INSTANCES = [(2, 5), (3, 5), (4, 4), (5, 4), (2, 4)]         # the four fixed shapes and one that runs the generic instance


def make(G, players, hand_size, sad, shuffle, **kw):
    from hanabi_sad_amd import BatchedHanabiEnv
    kw.setdefault("threads_per_workgroup", 128)
    kw.setdefault("games_per_workgroup", 64)
    return BatchedHanabiEnv(G, players=players, hand_size=hand_size, sad=sad, shuffle_color=shuffle, seed=SEED, eps_list=EPS,
                            max_len=MAX_LEN, device=DEV, track_deck_history=False, **kw)


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


@pytest.mark.parametrize("G", [69, 256])
@pytest.mark.parametrize("sad,shuffle", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("P,H", INSTANCES)
def test_every_mode_is_bit_identical(P, H, sad, shuffle, G):
    twin = make(G, P, H, sad, shuffle)           # one launch per iteration
    twin.set_rollout_chunk(0)
    envs = {}
    for mode in MODES:
        e = make(G, P, H, sad, shuffle)
        e.set_rollout_prio(mode)
        assert e.rollout_prio() == mode
        envs[mode] = e
    restarts = 0
    for chunk, n in CALLS:
        for _ in range(n):                       # the twin, iteration by iteration: its terminal flags count the restarts to come
            twin.rollout_random(1, PSEED)
            if chunk > 1:
                restarts += int(twin.terminal.sum().item())
        ref = outputs(twin)
        outs = {}
        for mode, e in envs.items():
            e.set_rollout_chunk(chunk)
            e.rollout_random(n, PSEED)
            outs[mode] = outputs(e)
        what = "P=%d H=%d sad=%s shuffle=%s G=%d, %d iterations in launches of %d" % (P, H, sad, shuffle, G, n, chunk)
        for mode in MODES:
            assert_same(outs[0], outs[mode], what + ", mode %d against mode 0" % mode)
            assert_same(ref, outs[mode], what + ", mode %d against the launch-per-iteration twin" % mode)
    # 30 iterations in persistent launches, a game of at most five moves: every game restarted inside them several times
    assert restarts >= 4 * G, restarts


def test_prio_reads_zero_where_the_pipelined_kernel_does_not_run():
    pipelined = make(69, 2, 5, False, False)
    elsewhere = {"256-thread workgroups": dict(threads_per_workgroup=256), "knowledge_mode 1": dict(knowledge_mode=1),
                 "a variant": dict(colors=4)}
    others = {what: make(69, 2, 5, False, False, **kw) for what, kw in elsewhere.items()}
    twins = {what: make(69, 2, 5, False, False, **kw) for what, kw in elsewhere.items()}   # never told a mode
    assert pipelined.rollout_prio() in MODES      # the default
    for mode in MODES:
        pipelined.set_rollout_prio(mode)
        assert pipelined.rollout_prio() == mode
        for what, e in others.items():
            e.set_rollout_prio(mode)
            assert e.rollout_prio() == 0, what
            for x in (e, twins[what]):            # and the switch changes nothing there
                x.set_rollout_chunk(7)
                x.rollout_random(7, PSEED)
            assert_same(outputs(twins[what]), outputs(e), "%s, mode %d" % (what, mode))
    for bad in (-1, 4):
        with pytest.raises(Exception):
            pipelined.set_rollout_prio(bad)
    assert pipelined.rollout_prio() == MODES[-1]


PINNED = sorted(k for k in PARENT if k[2] == 64 and k[5] == 80 and not k[6])


@pytest.mark.parametrize("key", PINNED)
def test_lds_and_resident_workgroups_are_the_pinned_ones(key):
    P, H, gpw, sad, shuffle = key[:5]
    e = make(256, P, H, sad, shuffle)
    e.set_rollout_chunk(20)
    for mode in MODES:
        e.set_rollout_prio(mode)
        e.set_rollout_delta(True)
        on = (int(e.lib.hsad_env_rollout_lds_bytes(e.h)), bool(e.rollout_delta_active()), int(e.lib.hsad_env_rollout_resident_workgroups(e.h)))
        e.set_rollout_delta(False)
        off = (int(e.lib.hsad_env_rollout_lds_bytes(e.h)), int(e.lib.hsad_env_rollout_resident_workgroups(e.h)))
        assert (on, off) == PARENT[key], "mode %d" % mode


def test_configs1_keeps_its_lds_bytes_and_four_workgroups_per_cu():
    from hanabi_sad_amd import BatchedHanabiEnv
    e = BatchedHanabiEnv(65536, seed=SEED, eps_list=EPS, max_len=80, device=DEV, track_deck_history=False)
    e.set_rollout_chunk(50)
    for mode in MODES:
        e.set_rollout_prio(mode)
        got = (e.threads_per_workgroup, e.games_per_workgroup, bool(e.rollout_delta_active()), int(e.lib.hsad_env_rollout_lds_bytes(e.h)),
               int(e.lib.hsad_env_rollout_resident_workgroups(e.h)))
        assert got == CONFIGS1 and got[3] == 38256 and got[4] == 4, "mode %d: %s" % (mode, got)
