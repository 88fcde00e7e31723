"""The chain of the launches of one hsad_env_rollout_random call (hsad_env_set_rollout_chain; include/hsad.h).  A persistent call of
more than one launch issues its launches back to back on one stream, so launch 2, 3, ... finds in priv_s exactly the rows its
predecessor's epilogue streamed.  With the chain on, the predecessor copies those bit rows to a buffer of the env and the follower
loads them as the `prev` of its first stream, which then stores only what changed instead of every line.  Nothing is carried from
one call to the next: the first launch of every call streams in full.

* bit identity, after every call, against the same env with the chain off and against the launch-per-iteration rollout (chunk 0):
  calls of 2-4 launches with odd and even chunk lengths (both parities of the row copy handed over), a shorter last launch and a
  last launch of a single iteration (which runs without the delta stream, so its predecessor hands nothing over); partial
  workgroups, 32-game workgroups, every (players, hand) instantiation, SAD, colour shuffle, both units, the direct form of the
  delta stream, pacing, and games that restart inside every launch,
* nothing crosses a call: a NaN fill of priv_s, a reset() and a step() between two calls, and a change of the chunk length,
* what the first stream of a chained launch stored equals, exactly, the CPU oracle's count of changed 16-float units between the
  predecessor's last observation and the follower's first (and is not "everything"),
* the chain is inactive wherever the delta stream is, and those envs compute what they did.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, the sampled actions a / greedy_a and the exported state."""
import os

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
EPS = [0.1 ** (1 + 7 * i / 79) for i in range(80)]
SEED, PSEED = 4242, 91
MODES = (1,)                     # the chain modes the library has besides 0
# (chunk, n_iter) of the calls one env runs in turn: launches of 2+2+2, 3+3+3, 7+7+6, 7+7+1 (no hand-over into the last), 2+2+1
CALLS = ((2, 6), (3, 9), (7, 20), (7, 15), (2, 5))


def make(G, players=2, hand_size=5, sad=False, shuffle_color=False, gpw=64, chain=0, max_len=80, seed=SEED, unit=None, compact=True,
         pace=None, threads=128, **rules):
    from hanabi_sad_amd import BatchedHanabiEnv
    e = BatchedHanabiEnv(G, players=players, hand_size=hand_size, sad=sad, shuffle_color=shuffle_color, seed=seed, eps_list=EPS,
                         max_len=max_len, device=DEV, track_deck_history=False, games_per_workgroup=gpw,
                         threads_per_workgroup=threads, **rules)
    assert e.games_per_workgroup == gpw and e.threads_per_workgroup == threads
    e.set_rollout_chain(chain)
    if unit is not None:
        e.set_rollout_unit(unit)
    e.set_rollout_compact(compact)
    if pace is not None:
        e.set_rollout_pace(pace)
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


def run_calls(e, per_iteration=False, calls=CALLS):
    """the outputs after every call"""
    outs = []
    for chunk, n in calls:
        e.set_rollout_chunk(0 if per_iteration else chunk)
        e.rollout_random(n, PSEED)
        outs.append(outputs(e))
    return outs


_REFS = {}


def reference(G, **kw):
    """the launch-per-iteration twin of the same games, after every call: computed once per configuration"""
    key = (G, tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = run_calls(make(G, **kw), per_iteration=True)
    return _REFS[key]


def check_equal(G, expect_active=None, ref_kw=None, **kw):
    """chain on (every mode) == chain off == launch per iteration, after every call of CALLS"""
    ref = reference(G, **(kw if ref_kw is None else ref_kw))
    off = make(G, chain=0, **kw)
    assert off.rollout_chain_active() == 0
    runs = [("chain 0", run_calls(off))]
    for mode in MODES:
        e = make(G, chain=mode, **kw)
        active = e.rollout_chain_active()
        assert active == (mode if e.rollout_delta_active() else 0)
        if expect_active is not None:
            assert (active != 0) == expect_active
        runs.append(("chain %d" % mode, run_calls(e)))
    for name, outs in runs:
        for (chunk, n), r, o in zip(CALLS, ref, outs):
            assert_same(r, o, "%s, G=%d %s, call of %d at chunk %d" % (name, G, kw, n, chunk))


@pytest.mark.parametrize("G,gpw", [(69, 64), (200, 32)])   # a full 64-game workgroup and one of 5 games; seven 32-game workgroups, the last of 8
def test_chained_calls_equal_unchained_and_per_iteration(G, gpw):
    check_equal(G, expect_active=True, gpw=gpw)


SHAPES = [  # (players, hand, sad, games per workgroup): every fixed instance and the generic one
    (2, 5, True, 64), (3, 5, False, 64), (3, 5, True, 32), (4, 4, True, 64), (4, 4, False, 32), (5, 4, False, 64), (5, 4, True, 32),
    (2, 4, True, 64), (3, 3, False, 32),
]


@pytest.mark.parametrize("P,H,sad,gpw", SHAPES)
def test_every_instantiation_sad_and_colour_shuffle(P, H, sad, gpw):
    # (whether the delta stream, and with it the chain, is active for a shape is the library's residency rule: check_equal holds
    # the chain to it, and the results may not depend on it)
    check_equal(100, players=P, hand_size=H, sad=sad, shuffle_color=True, gpw=gpw)


@pytest.mark.parametrize("kw", [dict(unit=128), dict(unit=64), dict(compact=False), dict(pace=True), dict(pace=True, unit=128)],
                         ids=lambda kw: "-".join("%s%s" % kv for kv in kw.items()))
def test_units_direct_form_and_pacing(kw):
    # none of these switches changes a result: one launch-per-iteration reference serves them all
    check_equal(69, expect_active=True, ref_kw=dict(sad=True), sad=True, **kw)


def test_games_restart_inside_every_launch():
    # max_len 2: every game ends by its second move, so every launch of two iterations or more restarts every game
    ref = reference(69, max_len=2)
    assert (ref[0]["state"][:, 74] >= 0).all(), "some game never finished"
    check_equal(69, expect_active=True, max_len=2)


def test_nothing_crosses_a_call():
    """the first launch of a call never reads the buffer the call before left: whatever happens to priv_s or the games between two
    calls, the chained env equals the unchained one"""
    G = 69
    for mode in MODES:
        on, off = make(G, chain=mode), make(G, chain=0)
        assert on.rollout_chain_active() == mode

        def call(chunk, n, what):
            for e in (on, off):
                e.set_rollout_chunk(chunk)
                e.rollout_random(n, PSEED)
            got = outputs(on)
            assert not torch.isnan(got["priv_s"]).any(), what
            assert_same(outputs(off), got, "mode %d, %s" % (mode, what))

        call(3, 9, "first call")
        on.priv_s.fill_(float("nan"))
        call(3, 9, "after a NaN fill of priv_s")
        on.priv_s.fill_(float("nan"))
        call(2, 6, "after a NaN fill, at another chunk length than the one that last wrote the buffer")
        for e in (on, off):
            e.reset()
        call(2, 6, "after reset()")
        call(7, 20, "another chunk length")
        for e in (on, off):
            e.reset()                             # (step() wants no finished game)
            a, g = e.policy_random(PSEED + 1)
            e.step(a, g)
        call(7, 15, "after one step()")
        for e in (on, off):
            e.reset()
        on.priv_s.fill_(float("nan"))
        call(3, 7, "after reset() and a NaN fill")


@pytest.mark.parametrize("mode", MODES)
def test_first_stream_of_a_chained_launch_stores_the_oracles_changed_units_exactly(mode):
    from hanabi_sad_amd import _lib
    from oracle.oracle import OracleVecEnv
    G, n, warm, seed, pseed = 128, 6, 7, 777, 3
    e = make(G, chain=mode, seed=seed)
    assert e.rollout_chain_active() == mode and e.rollout_unit() == 64
    ref = OracleVecEnv(G, seed, players=2, hand_size=5, eps_list=EPS, max_len=80)
    e.set_rollout_chunk(n)
    e.rollout_random(warm, pseed)
    ref.rollout(warm, pseed)
    nwg = G // 64
    buf = torch.zeros(nwg * n * 16, dtype=torch.int64, device=DEV)
    ubuf = torch.zeros(nwg * n, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    _lib.check(e.lib.hsad_env_debug_trace(e.h, buf.data_ptr(), n))
    _lib.check(e.lib.hsad_env_debug_units(e.h, ubuf.data_ptr()))
    e.rollout_random(2 * n, pseed)                # two launches of n iterations: the trace holds the second, the chained one
    torch.cuda.synchronize()
    _lib.check(e.lib.hsad_env_debug_units(e.h, None))
    _lib.check(e.lib.hsad_env_debug_trace(e.h, None, 0))
    e.check_errors()
    obs = []
    for _ in range(2 * n):
        ref.rollout(1, pseed)
        obs.append(ref.priv_s.copy())
    assert np.array_equal(e.priv_s.cpu().numpy(), obs[-1])
    units = 64 * 2 * e.F // 16                    # a workgroup's range is a whole number of 16-float units
    assert units * 16 == 64 * 2 * e.F
    # record k of the units buffer: the stream of the rows of iteration k - 1 of the traced launch (phase A of iteration k)
    stored = ubuf.view(nwg, n).cpu().numpy()[:, 1:]
    expect = np.stack([(obs[n + k] != obs[n + k - 1]).reshape(nwg, units, 16).any(axis=2).sum(axis=1) for k in range(n - 1)], axis=1)
    print("units stored per workgroup and stream of the chained launch:\n%s\nexpected:\n%s" % (stored, expect))
    assert (expect < units).all() and (expect > 0).all()      # never "every unit", which is what an unchained launch stores first
    # column 0: the rows of the launch's iteration 0 against the predecessor's last rows, which came through the buffer
    assert np.array_equal(stored, expect)


def test_chain_is_inactive_wherever_the_delta_stream_is():
    G = 100
    cases = []
    e = make(G, chain=1)
    e.enable_packed(bf16_row_len=(e.F + 63) // 64 * 64, keep_float32=False)
    r = make(G, chain=0)
    r.enable_packed(bf16_row_len=(r.F + 63) // 64 * 64, keep_float32=False)
    cases.append(("packed outputs only", e, r))
    cases.append(("knowledge_mode 1", make(G, chain=1, knowledge_mode=1), make(G, chain=0, knowledge_mode=1)))
    cases.append(("variant", make(G, chain=1, colors=4, ranks=4), make(G, chain=0, colors=4, ranks=4)))
    cases.append(("256 threads", make(G, chain=1, threads=256), make(G, chain=0, threads=256)))
    old = os.environ.get("HSAD_ENV_DELTA")
    os.environ["HSAD_ENV_DELTA"] = "0"            # read when the env is created
    try:
        cases.append(("HSAD_ENV_DELTA=0", make(G, chain=1), make(G, chain=0)))
    finally:
        if old is None:
            del os.environ["HSAD_ENV_DELTA"]
        else:
            os.environ["HSAD_ENV_DELTA"] = old
    for what, e, r in cases:
        assert not e.rollout_delta_active() and e.rollout_chain_active() == 0, what
        got, ref = run_calls(e, calls=CALLS[:2]), run_calls(r, per_iteration=True, calls=CALLS[:2])
        for o, p in zip(got, ref):
            assert_same(p, o, what)
    # and switching the delta stream off on an env whose chain was active switches the chain off with it
    e = make(G, chain=1)
    assert e.rollout_chain_active() == 1
    e.set_rollout_delta(False)
    assert e.rollout_chain_active() == 0
