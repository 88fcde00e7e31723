"""The pipelined persistent rollout (env_rollout_pipe_kernel: a logic wave and a stream wave, the rows of iteration k - 1 streamed
while the logic of iteration k runs) against the single-phase persistent rollout (env_rollout_kernel, HSAD_ENV_PIPE=0) and the
launch-per-iteration rollout, bit for bit:

* configs[1] at full size (65,536 two-player games): chunks 2, 3, 7, 20 and 50, over a rollout whose length is not a multiple of
  the chunk and which is split over two calls, so that games finish and restart across launch boundaries (chunk 1 is the
  launch-per-iteration reference itself: a one-iteration launch never takes a persistent kernel),
* every (players, hand) instantiation, in 32- and 64-game and 128- and 256-thread workgroups (the 256-thread shapes keep the
  single-phase schedule: the equality holds either way),
* the packed device-consumer outputs (bit words, bf16 rows) written by the stream wave.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, the sampled actions a / greedy_a and the exported state."""
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = "cuda:0"
EPS = [0.1 ** (1 + 7 * i / 79) for i in range(80)]
SEED, PSEED = 4242, 91


def make(G, players=2, hand_size=5, sad=False, shuffle_color=False, gpw=0, threads=0, chunk=0, pipe=True):
    from hanabi_sad_amd import BatchedHanabiEnv
    old = os.environ.get("HSAD_ENV_PIPE")
    os.environ["HSAD_ENV_PIPE"] = "1" if pipe else "0"   # read when the env is created
    try:
        e = BatchedHanabiEnv(G, players=players, hand_size=hand_size, sad=sad, shuffle_color=shuffle_color, seed=SEED, eps_list=EPS,
                             max_len=80, device=DEV, track_deck_history=False, games_per_workgroup=gpw, threads_per_workgroup=threads)
    finally:
        if old is None:
            del os.environ["HSAD_ENV_PIPE"]
        else:
            os.environ["HSAD_ENV_PIPE"] = old
    e.set_rollout_chunk(chunk)
    return e


def outputs(e):
    torch.cuda.synchronize()
    e.check_errors()
    out = {"priv_s": e.priv_s, "legal_move": e.legal_move, "own_hand": e.own_hand, "eps": e.eps, "reward": e.reward,
           "terminal": e.terminal, "a": e.a, "greedy_a": e.greedy_a, "state": e.export_state()}
    for k in ("priv_bits", "legal_bits", "own_bits", "priv_s_bf16"):
        if getattr(e, k, None) is not None:
            out[k] = getattr(e, k)
    return {k: v.clone() for k, v in out.items()}


def assert_same(ref, got, what):
    assert ref.keys() == got.keys()
    for k in ref:
        assert torch.equal(ref[k], got[k]), "%s: %s differs" % (what, k)


def run(e, blocks):
    for n in blocks:
        e.rollout_random(n, PSEED)
    return outputs(e)


@pytest.mark.parametrize("chunk", [2, 3, 7, 20, 50])
def test_configs1_full_size_pipelined_equals_single_phase_and_per_iteration(chunk):
    blocks = (57, 46)      # 103 iterations: not a multiple of any chunk > 1; games end and restart across launches and calls
    ref = run(make(65536), blocks)
    for pipe in (True, False):
        e = make(65536, chunk=chunk, pipe=pipe)
        assert e.threads_per_workgroup == 128 and e.games_per_workgroup == 64
        assert_same(ref, run(e, blocks), "chunk %d, %s schedule" % (chunk, "pipelined" if pipe else "single-phase"))
        del e
        torch.cuda.empty_cache()


def test_configs1_full_size_games_restart_inside_the_persistent_launches():
    # the comparison above means something only if games finish inside launches: after 103 random-policy iterations every game has
    # finished at least once (max_len = 80 ends every game by its 80th move at the latest)
    e = make(65536, chunk=50)
    e.rollout_random(103, PSEED)
    torch.cuda.synchronize()
    st = e.export_state().cpu()
    assert (st[:, 74] >= 0).all(), "some game never finished"          # last score: -1 until the first game of the slot ended


def test_configs1_four_workgroups_fit_the_lds_of_a_cu():
    # what a persistent launch of configs[1] requests per workgroup, from the library's own sizing: all 1,024 workgroups resident
    e = make(65536, chunk=50)
    lds = int(e.lib.hsad_env_rollout_lds_bytes(e.h))
    assert 0 < lds and 4 * lds <= 160 * 1024, lds


SHAPES = [  # (players, hand, sad, shuffle_color, games per workgroup, threads per workgroup)
    (2, 5, True, True, 64, 128), (2, 5, False, False, 32, 128), (2, 5, True, False, 64, 256), (2, 5, False, True, 32, 256),
    (3, 5, True, True, 64, 128), (3, 5, False, False, 32, 256),
    (4, 4, True, True, 32, 128), (4, 4, False, True, 64, 256),
    (5, 4, True, True, 32, 128), (5, 4, False, True, 64, 128), (5, 4, True, True, 32, 256),
    (2, 4, True, True, 64, 128), (3, 3, False, True, 32, 128),   # the generic <0, 0> instances
]


@pytest.mark.parametrize("P,H,sad,sc,gpw,threads", SHAPES)
def test_every_instantiation_pipelined_equals_single_phase_and_per_iteration(P, H, sad, sc, gpw, threads):
    G, blocks, chunk = 3 * 4096 + 37, (41, 30), 13        # a partial last workgroup; 71 iterations in launches of 13
    kw = dict(players=P, hand_size=H, sad=sad, shuffle_color=sc, gpw=gpw, threads=threads)
    ref = run(make(G, **kw), blocks)
    for pipe in (True, False):
        e = make(G, chunk=chunk, pipe=pipe, **kw)
        assert e.games_per_workgroup == gpw and e.threads_per_workgroup == threads
        assert_same(ref, run(e, blocks), "P=%d H=%d gpw=%d threads=%d pipe=%s" % (P, H, gpw, threads, pipe))


@pytest.mark.parametrize("keep_float32", [True, False])
def test_packed_outputs_from_the_stream_wave(keep_float32):
    G, blocks = 8192, (33, 20)
    envs = []
    for chunk, pipe in ((0, True), (9, True), (9, False)):
        e = make(G, sad=True, shuffle_color=True, chunk=chunk, pipe=pipe)
        e.enable_packed(bf16_row_len=(e.F + 63) // 64 * 64, keep_float32=keep_float32)
        envs.append(e)
    outs = []
    for e in envs:
        for n in blocks:
            e.rollout_random(n, PSEED)
        torch.cuda.synchronize()
        e.check_errors()
        o = {k: getattr(e, k).clone() for k in ("priv_bits", "legal_bits", "own_bits", "priv_s_bf16", "legal_move", "own_hand",
                                                "eps", "reward", "terminal", "a", "greedy_a")}
        if keep_float32:
            o["priv_s"] = e.priv_s.clone()
        o["state"] = e.export_state()
        outs.append(o)
    assert_same(outs[0], outs[1], "packed, pipelined")
    assert_same(outs[0], outs[2], "packed, single-phase")
