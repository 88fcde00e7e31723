"""The delta stream of the pipelined persistent rollout (env_rollout_pipe_kernel with EnvParams::delta: within one launch every
observation stream after the first stores only the 128-byte lines of priv_s whose bits changed; include/hsad.h,
hsad_env_set_rollout_delta):

* bit identity of delta on against delta off (the full stream) and against the launch-per-iteration rollout, over chunks, partial
  workgroups, every (players, hand) instantiation, SAD, colour shuffle, the packed outputs and games that restart inside a launch,
* no dependence on what priv_s held before a launch (a NaN sentinel),
* the number of lines each workgroup stores in each stream equals, exactly, the number of 32-float units that differ between the CPU
  oracle's consecutive observations,
* four workgroups of configs[1] still fit a CU's LDS, and the env falls back to the full stream where the float32 observation is
  off or the second copy of the rows would cost a resident workgroup.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, the sampled actions a / greedy_a and the exported state."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
EPS = [0.1 ** (1 + 7 * i / 79) for i in range(80)]
SEED, PSEED = 4242, 91


def make(G, players=2, hand_size=5, sad=False, shuffle_color=False, gpw=64, chunk=0, delta=True, max_len=80, seed=SEED):
    from hanabi_sad_amd import BatchedHanabiEnv
    e = BatchedHanabiEnv(G, players=players, hand_size=hand_size, sad=sad, shuffle_color=shuffle_color, seed=seed, eps_list=EPS,
                         max_len=max_len, device=DEV, track_deck_history=False, games_per_workgroup=gpw, threads_per_workgroup=128)
    assert e.games_per_workgroup == gpw and e.threads_per_workgroup == 128
    e.set_rollout_chunk(chunk)
    e.set_rollout_delta(delta)
    if not delta:
        assert not e.rollout_delta_active()
    return e


def outputs(e):
    torch.cuda.synchronize()
    e.check_errors()
    out = {"legal_move": e.legal_move, "own_hand": e.own_hand, "eps": e.eps, "reward": e.reward,
           "terminal": e.terminal, "a": e.a, "greedy_a": e.greedy_a, "state": e.export_state()}
    for k in ("priv_s", "priv_bits", "legal_bits", "own_bits", "priv_s_bf16"):
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


BLOCKS = (45, 28)        # at chunk 20: launches of 20 + 20 + 5, then 20 + 8
_REFS = {}


def reference(G, blocks=BLOCKS, **kw):
    """the launch-per-iteration rollout of the same games: computed once per configuration"""
    key = (G, blocks, tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = run(make(G, **kw), blocks)
    return _REFS[key]


@pytest.mark.parametrize("G", [192, 100])            # three workgroups; a partial last workgroup (36 games)
@pytest.mark.parametrize("chunk", [2, 3, 7, 20, 50])
def test_delta_on_equals_delta_off_and_per_iteration(G, chunk):
    ref = reference(G)
    for delta in (True, False):
        e = make(G, chunk=chunk, delta=delta)
        assert e.rollout_delta_active() == delta
        assert_same(ref, run(e, BLOCKS), "G=%d chunk=%d delta=%s" % (G, chunk, delta))


SHAPES = [  # (players, hand, sad, games per workgroup)
    (2, 5, True, 64), (2, 5, False, 32), (3, 5, True, 32), (3, 5, False, 64), (4, 4, True, 64), (4, 4, False, 32),
    (5, 4, True, 32), (5, 4, False, 64),
]


@pytest.mark.parametrize("G", [192, 100])
@pytest.mark.parametrize("P,H,sad,gpw", SHAPES)
def test_every_instantiation_sad_and_colour_shuffle(G, P, H, sad, gpw):
    kw = dict(players=P, hand_size=H, sad=sad, shuffle_color=True, gpw=gpw)
    ref = reference(G, **kw)
    for delta in (True, False):
        # (whether delta is active for a shape is the library's residency rule: the results may not depend on it)
        assert_same(ref, run(make(G, chunk=20, delta=delta, **kw), BLOCKS), "P=%d H=%d sad=%s gpw=%d delta=%s" % (P, H, sad, gpw, delta))


@pytest.mark.parametrize("keep_float32", [True, False])
def test_packed_outputs_bound(keep_float32):
    G = 192
    outs = []
    for chunk, delta in ((0, True), (20, True), (20, False)):
        e = make(G, shuffle_color=True, chunk=chunk, delta=delta)
        e.enable_packed(bf16_row_len=(e.F + 63) // 64 * 64, keep_float32=keep_float32)
        # without the float32 observation there is nothing to skip: the full-stream path, and no second copy in LDS
        assert e.rollout_delta_active() == (delta and keep_float32)
        outs.append(run(e, BLOCKS))
        assert ("priv_s" in outs[-1]) == keep_float32 and "priv_bits" in outs[-1] and "priv_s_bf16" in outs[-1]
    assert_same(outs[0], outs[1], "packed, delta on")
    assert_same(outs[0], outs[2], "packed, delta off")


def test_games_restart_inside_the_launches():
    # max_len 5: every game ends by its fifth move, so most games restart at least three times inside a 20-iteration launch
    G = 192
    ref = reference(G, max_len=5)
    assert (ref["state"][:, 74] >= 0).all(), "some game never finished"
    for delta in (True, False):
        e = make(G, chunk=20, delta=delta, max_len=5)
        assert e.rollout_delta_active() == delta
        assert_same(ref, run(e, BLOCKS), "max_len 5, delta=%s" % delta)


@pytest.mark.parametrize("G,n", [(192, 9), (100, 2)])
def test_no_dependence_on_earlier_contents_of_priv_s(G, n):
    """the first stream of a launch writes every line: a sentinel left in priv_s before a launch of >= 2 iterations is gone after it"""
    on, off = make(G, chunk=20, delta=True), make(G, chunk=20, delta=False)
    assert on.rollout_delta_active()
    for e in (on, off):
        e.rollout_random(7, PSEED)
    torch.cuda.synchronize()
    on.priv_s.fill_(float("nan"))
    for e in (on, off):
        e.rollout_random(n, PSEED)      # one launch of n iterations
    got, ref = outputs(on), outputs(off)
    assert not torch.isnan(got["priv_s"]).any()
    assert_same(ref, got, "after a NaN fill")


def test_lines_stored_equal_the_oracles_changed_lines_exactly():
    from hanabi_sad_amd import _lib
    from oracle.oracle import OracleVecEnv
    G, n, warm, seed, pseed = 128, 12, 7, 777, 3
    e = make(G, chunk=n, delta=True, seed=seed)
    assert e.rollout_delta_active()
    ref = OracleVecEnv(G, seed, players=2, hand_size=5, eps_list=EPS, max_len=80)
    e.rollout_random(warm, pseed)
    ref.rollout(warm, pseed)
    nwg = G // 64
    buf = torch.zeros(nwg * n * 16, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    _lib.check(e.lib.hsad_env_debug_trace(e.h, buf.data_ptr(), n))
    e.rollout_random(n, pseed)                    # one traced launch of n iterations
    torch.cuda.synchronize()
    _lib.check(e.lib.hsad_env_debug_trace(e.h, None, 0))
    e.check_errors()
    s = buf.view(nwg, n, 16).cpu().numpy()
    obs = []
    for _ in range(n):
        ref.rollout(1, pseed)
        obs.append(ref.priv_s.copy())
    assert np.array_equal(e.priv_s.cpu().numpy(), obs[-1])
    units = 64 * 2 * e.F // 32                    # a workgroup's range is a whole number of 32-float units
    assert units * 32 == 64 * 2 * e.F
    # the stream of the rows of iteration i: phase A of iteration i + 1 (slot 13), the last one in the epilogue (slots 14 + 15)
    stored = np.concatenate([s[:, 1:, 13], (s[:, n - 1, 14] + s[:, n - 1, 15])[:, None]], axis=1)
    expect = np.zeros((nwg, n), np.int64)
    expect[:, 0] = units                          # the first stream of the launch stores everything
    for i in range(1, n):
        expect[:, i] = (obs[i] != obs[i - 1]).reshape(nwg, units, 32).any(axis=2).sum(axis=1)
    print("lines stored per workgroup and stream:\n%s\nexpected:\n%s" % (stored, expect))
    assert (expect[:, 1:] < units).all() and (expect[:, 1:] > 0).all()
    assert np.array_equal(stored, expect)


def test_configs1_keeps_four_workgroups_per_cu_and_uses_the_delta_stream():
    from hanabi_sad_amd import BatchedHanabiEnv
    e = BatchedHanabiEnv(65536, seed=SEED, eps_list=EPS, max_len=80, device=DEV, track_deck_history=False)
    e.set_rollout_chunk(50)
    assert e.threads_per_workgroup == 128 and e.games_per_workgroup == 64
    assert e.rollout_delta_active()
    lds = int(e.lib.hsad_env_rollout_lds_bytes(e.h))
    assert 0 < lds and 4 * lds <= 160 * 1024, lds
    e.set_rollout_delta(False)
    assert not e.rollout_delta_active() and 0 < int(e.lib.hsad_env_rollout_lds_bytes(e.h)) < lds


def test_falls_back_to_the_full_stream_where_the_second_copy_costs_residency():
    # five players in 32-game workgroups: 68.8 KB of LDS per workgroup (rows 27.6 KB, state planes, the 113-word mt19937 window per
    # lane), two workgroups in a CU's 160 KB; with a second copy of the rows 96.4 KB, one.  (64-game workgroups of this game are
    # alone on a CU either way, 97.6 and 152.9 KB, and keep the delta stream.)
    kw = dict(players=5, hand_size=4, sad=False, shuffle_color=True, gpw=32)
    e = make(192, chunk=20, delta=True, **kw)
    assert not e.rollout_delta_active()
    assert_same(reference(192, **kw), run(e, BLOCKS), "fallback shape")
