"""Half-line units of the compacted delta stream (stream_bits_f32_compact<NT, 16> in csrc/hsad_env.hip; include/hsad.h,
hsad_env_set_rollout_unit): the stream wave decides "changed" per 64-byte half line of priv_s (16 bits of the LDS bit rows) and
stores sixteen whole halves per wave-store.

* bit identity of unit 64 against unit 128, the direct form and the full stream after every launch, over chunks of both parities,
  a one-game last workgroup (a partial last word) and every instantiation the compacted form is active for,
* games that restart several times inside a launch,
* no dependence on what priv_s held before a launch and not a byte written outside priv_s,
* the traced unit counts (hsad_env_debug_units) equal, exactly, the number of 16-float units that differ between the CPU oracle's
  consecutive observations, and slot 13 keeps counting the 32-float units,
* the switch: rollout_unit() follows it, is 128 wherever the compacted form is not active, and costs neither LDS nor residency.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, the sampled actions a / greedy_a and the exported state."""
import numpy as np
import pytest
import torch

from tests.test_env_rollout_compact_gpu import GUARD, SHAPES, bind_guarded, run_in_step
from tests.test_env_rollout_compact_gpu import make as make_compact
from tests.test_env_rollout_delta_gpu import DEV, EPS, PSEED, assert_same, outputs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
BLOCKS = (45, 28)


def make(G, unit=64, compact=True, delta=True, **kw):
    e = make_compact(G, compact=compact, delta=delta, **kw)
    e.set_rollout_unit(unit)
    assert e.rollout_unit() == (unit if e.rollout_compact_active() else 128)
    return e


def four_forms(G, **kw):
    """unit 64 first (the reference of run_in_step), then unit 128, the direct form and the full stream"""
    envs = [make(G, unit=64, **kw), make(G, unit=128, **kw), make(G, compact=False, **kw), make(G, delta=False, **kw)]
    assert envs[0].rollout_unit() == 64 and [e.rollout_unit() for e in envs[1:]] == [128, 128, 128]
    return envs


@pytest.mark.parametrize("G", [65, 100, 192])        # a second workgroup of one game; a partial one of 36; three full ones
@pytest.mark.parametrize("chunk", [2, 3, 7, 20])
def test_all_four_forms_agree_after_every_launch(G, chunk):
    run_in_step(four_forms(G, chunk=chunk), (chunk, chunk, chunk) + BLOCKS, "G=%d chunk=%d" % (G, chunk))


@pytest.mark.parametrize("P,H,sad,gpw", SHAPES)
def test_every_instantiation_with_the_compacted_form(P, H, sad, gpw):
    envs = four_forms(100, players=P, hand_size=H, sad=sad, shuffle_color=True, gpw=gpw, chunk=20)
    run_in_step(envs, BLOCKS, "P=%d H=%d sad=%s gpw=%d" % (P, H, sad, gpw))


def test_games_restart_inside_the_launches():
    # max_len 5: every game ends by its fifth move, so most games restart at least three times inside a 20-iteration launch
    envs = four_forms(192, chunk=20, max_len=5)
    run_in_step(envs, BLOCKS, "max_len 5")
    assert (outputs(envs[0])["state"][:, 74] >= 0).all(), "some game never finished"


@pytest.mark.parametrize("G,n", [(65, 9), (65, 2), (100, 3)])
def test_nan_fill_is_gone_and_nothing_outside_priv_s_is_written(G, n):
    on, off = make(G, unit=64, chunk=20), make(G, chunk=20, delta=False)
    assert on.rollout_unit() == 64
    buf = bind_guarded(on)
    for e in (on, off):
        e.rollout_random(7, PSEED)
    torch.cuda.synchronize()
    on.priv_s.fill_(float("nan"))
    for e in (on, off):
        e.rollout_random(n, PSEED)      # one launch of n iterations
    got, ref = outputs(on), outputs(off)
    assert not torch.isnan(got["priv_s"]).any()
    assert_same(ref, got, "after a NaN fill")
    # the guards hold the bit pattern they were given, every word of them
    nan_bits = torch.full((GUARD,), float("nan"), dtype=torch.float32, device=DEV).view(torch.int32)
    assert torch.equal(buf[:GUARD].view(torch.int32), nan_bits), "written in front of priv_s"
    assert torch.equal(buf[GUARD + on.priv_s.numel():].view(torch.int32), nan_bits), "written behind priv_s"


def test_units_stored_equal_the_oracles_changed_units_exactly():
    from hanabi_sad_amd import _lib
    from oracle.oracle import OracleVecEnv
    from tests.test_env_rollout_delta_gpu import make as make_delta
    G, n, warm, seed, pseed = 128, 12, 7, 777, 3     # the inputs of the delta suite's oracle-count test
    e = make_delta(G, chunk=n, delta=True, seed=seed)
    e.set_rollout_unit(64)
    assert e.rollout_unit() == 64
    ref = OracleVecEnv(G, seed, players=2, hand_size=5, eps_list=EPS, max_len=80)
    e.rollout_random(warm, pseed)
    ref.rollout(warm, pseed)
    nwg = G // 64
    buf = torch.zeros(nwg * n * 16, dtype=torch.int64, device=DEV)
    ubuf = torch.full((nwg * n,), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    _lib.check(e.lib.hsad_env_debug_trace(e.h, buf.data_ptr(), n))
    _lib.check(e.lib.hsad_env_debug_units(e.h, ubuf.data_ptr()))
    e.rollout_random(n, pseed)                    # one traced launch of n iterations
    torch.cuda.synchronize()
    _lib.check(e.lib.hsad_env_debug_units(e.h, None))
    _lib.check(e.lib.hsad_env_debug_trace(e.h, None, 0))
    e.check_errors()
    s = buf.view(nwg, n, 16).cpu().numpy()
    u = ubuf.view(nwg, n).cpu().numpy()
    obs = []
    for _ in range(n):
        ref.rollout(1, pseed)
        obs.append(ref.priv_s.copy())
    assert np.array_equal(e.priv_s.cpu().numpy(), obs[-1])
    lines = 64 * 2 * e.F // 32                    # a workgroup's range is a whole number of 32-float units
    assert lines * 32 == 64 * 2 * e.F
    # the stream of the rows of iteration i is phase A of iteration i + 1: record i + 1.  Record 0 has no stream (nothing is
    # written to it), record 1 is the first stream of the launch, which stores every line in the direct form and counts lines.
    assert (u[:, 0] == -1).all()
    assert (u[:, 1] == lines).all() and (s[:, 1, 13] == lines).all()
    expect16 = np.zeros((nwg, n - 2), np.int64)
    expect32 = np.zeros((nwg, n - 2), np.int64)
    for i in range(1, n - 1):                     # streams 1 .. n - 2 (the last stream is the epilogue's, by lines)
        diff = obs[i] != obs[i - 1]
        expect16[:, i - 1] = diff.reshape(nwg, 2 * lines, 16).any(axis=2).sum(axis=1)
        expect32[:, i - 1] = diff.reshape(nwg, lines, 32).any(axis=2).sum(axis=1)
    got16, got32 = u[:, 2:], s[:, 2:, 13]
    print("half lines stored per workgroup and stream:\n%s\nexpected:\n%s\nlines with any change (slot 13):\n%s\nexpected:\n%s"
          % (got16, expect16, got32, expect32))
    assert (expect16 > 0).all() and (expect16 < 2 * lines).all(), "vacuous: a stream with no or with every half line changed"
    assert (expect32 > 0).all() and (expect32 < lines).all(), "vacuous: a stream with no or with every line changed"
    assert np.array_equal(got16, expect16)
    assert np.array_equal(got32, expect32)
    # the epilogue's stream goes by lines, as before
    last = (obs[n - 1] != obs[n - 2]).reshape(nwg, lines, 32).any(axis=2).sum(axis=1)
    assert np.array_equal(s[:, n - 1, 14] + s[:, n - 1, 15], last)


def test_switch_follows_the_compacted_form_and_costs_no_lds():
    from hanabi_sad_amd import BatchedHanabiEnv, _lib
    e = BatchedHanabiEnv(65536, seed=4242, eps_list=EPS, max_len=80, device=DEV, track_deck_history=False)
    e.set_rollout_chunk(50)
    res = lambda: (int(e.lib.hsad_env_rollout_lds_bytes(e.h)), int(e.lib.hsad_env_rollout_resident_workgroups(e.h)))
    assert e.rollout_compact_active()
    e.set_rollout_unit(64)
    assert e.rollout_unit() == 64
    at64 = res()
    e.set_rollout_unit(128)
    assert e.rollout_unit() == 128
    assert res() == at64 and at64 == (38256, 4)
    e.set_rollout_unit(64)
    e.set_rollout_compact(False)
    assert e.rollout_unit() == 128                # the direct form goes by lines
    e.set_rollout_compact(True)
    e.set_rollout_delta(False)
    assert e.rollout_unit() == 128
    e.set_rollout_delta(True)
    assert e.rollout_unit() == 64
    with pytest.raises(_lib.HsadError):
        e.set_rollout_unit(32)
    assert e.rollout_unit() == 64
    # a shape the delta stream is not active for: lines
    f = make_compact(192, players=5, hand_size=4, shuffle_color=True, gpw=32, chunk=20)
    f.set_rollout_unit(64)
    assert not f.rollout_compact_active() and f.rollout_unit() == 128
