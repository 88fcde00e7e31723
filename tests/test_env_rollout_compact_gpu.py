"""The compacted form of the delta stream of the pipelined persistent rollout (EnvParams::compact, stream_bits_f32_compact in
csrc/hsad_env.hip; include/hsad.h, hsad_env_set_rollout_compact): the stream wave lists the changed lines of priv_s first, in place in
the LDS copy it has just compared, and stores from the list.

* bit identity of compact on against compact off (the direct form) and against delta off (the full stream), after every launch, over
  chunks of both parities, a one-game last workgroup (a partial last word), and every pipelined instantiation the delta stream is
  active for, the five-player 64-game workgroups included (the largest word index),
* no dependence on what priv_s held before a launch and not a byte written outside priv_s (a NaN fill between guard regions),
* the traced line counts (slot 13; 14 / 15 in the epilogue) equal the direct form's exactly, per workgroup and stream,
* the switch follows the delta stream's, and costs neither LDS nor a resident workgroup.

Compared: priv_s, legal_move, own_hand, eps, reward, terminal, the sampled actions a / greedy_a and the exported state."""
import pytest
import torch

from tests.test_env_rollout_delta_gpu import DEV, EPS, PSEED, assert_same, make as make_delta, outputs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
BLOCKS = (45, 28)


def make(G, compact=True, delta=True, **kw):
    e = make_delta(G, delta=delta, **kw)
    e.set_rollout_compact(compact)
    assert e.rollout_compact_active() == (bool(compact) and e.rollout_delta_active())
    return e


def run_in_step(envs, blocks, what):
    """every env runs the same blocks; after every rollout call (its launches done) all outputs equal the first env's"""
    for n in blocks:
        outs = []
        for e in envs:
            e.rollout_random(n, PSEED)
            outs.append(outputs(e))
        for i, o in enumerate(outs[1:], 1):
            assert_same(outs[0], o, "%s, after a block of %d, env %d" % (what, n, i))


@pytest.mark.parametrize("G", [65, 100, 192])        # a second workgroup of one game; a partial one of 36; three full ones
@pytest.mark.parametrize("chunk", [2, 3, 7, 20])
def test_compact_equals_direct_form_and_full_stream_after_every_launch(G, chunk):
    envs = [make(G, chunk=chunk, delta=False), make(G, chunk=chunk, compact=False), make(G, chunk=chunk, compact=True)]
    assert not envs[0].rollout_compact_active() and not envs[1].rollout_compact_active() and envs[2].rollout_compact_active()
    # blocks of one chunk each: every launch is compared; then a block of several launches and a shorter last one
    run_in_step(envs, (chunk, chunk, chunk) + BLOCKS, "G=%d chunk=%d" % (G, chunk))


SHAPES = [  # (players, hand, sad, games per workgroup): the shapes of the delta test the delta stream is active for
    (2, 5, True, 64), (2, 5, False, 32), (5, 4, False, 64), (5, 4, True, 64),
]


@pytest.mark.parametrize("P,H,sad,gpw", SHAPES)
def test_every_instantiation_with_the_delta_stream(P, H, sad, gpw):
    kw = dict(players=P, hand_size=H, sad=sad, shuffle_color=True, gpw=gpw, chunk=20)
    envs = [make(100, delta=False, **kw), make(100, compact=False, **kw), make(100, compact=True, **kw)]
    assert envs[1].rollout_delta_active() and envs[2].rollout_compact_active()
    run_in_step(envs, BLOCKS, "P=%d H=%d sad=%s gpw=%d" % (P, H, sad, gpw))


GUARD = 4096   # floats in front of and behind priv_s


def bind_guarded(e):
    """priv_s as a view into a larger buffer with a NaN guard on either side"""
    from hanabi_sad_amd import _lib
    n = e.priv_s.numel()
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + n].view(e.priv_s.shape)
    assert view.data_ptr() % 16 == 0
    view.copy_(e.priv_s)
    e.priv_s = view
    _lib.check(e.lib.hsad_env_bind_outputs(e.h, e.priv_s.data_ptr(), e.legal_move.data_ptr(), e.own_hand.data_ptr(), e.eps.data_ptr(),
                                           e.reward.data_ptr(), e.terminal.data_ptr()))
    return buf


@pytest.mark.parametrize("G,n", [(65, 9), (65, 2), (100, 3)])
def test_nan_fill_is_gone_and_nothing_outside_priv_s_is_written(G, n):
    on, off = make(G, chunk=20, compact=True), make(G, chunk=20, delta=False)
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


def traced_counts(e, n):
    from hanabi_sad_amd import _lib
    nwg = (e.G + e.games_per_workgroup - 1) // e.games_per_workgroup
    buf = torch.zeros(nwg * n * 16, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    _lib.check(e.lib.hsad_env_debug_trace(e.h, buf.data_ptr(), n))
    e.rollout_random(n, PSEED)                    # one traced launch of n iterations
    torch.cuda.synchronize()
    _lib.check(e.lib.hsad_env_debug_trace(e.h, None, 0))
    e.check_errors()
    s = buf.view(nwg, n, 16).cpu()
    return s[:, :, 13:16].clone()


@pytest.mark.parametrize("G", [65, 192])
def test_traced_line_counts_equal_the_direct_forms(G):
    n = 12
    direct, compact = make(G, chunk=n, compact=False), make(G, chunk=n, compact=True)
    for e in (direct, compact):
        e.rollout_random(7, PSEED)
    want, got = traced_counts(direct, n), traced_counts(compact, n)
    print("lines per workgroup, iteration and slot 13 / 14 / 15, direct form:\n%s\ncompacted:\n%s" % (want, got))
    assert (want[:, 2:, 0] > 0).all(), "a delta stream that stored nothing: the comparison would be vacuous"
    assert torch.equal(want, got)
    assert_same(outputs(direct), outputs(compact), "traced launch")


def test_switch_follows_the_delta_stream_and_costs_no_lds():
    from hanabi_sad_amd import BatchedHanabiEnv
    e = BatchedHanabiEnv(65536, seed=4242, eps_list=EPS, max_len=80, device=DEV, track_deck_history=False)
    e.set_rollout_chunk(50)
    res = lambda: (int(e.lib.hsad_env_rollout_lds_bytes(e.h)), int(e.lib.hsad_env_rollout_resident_workgroups(e.h)))
    assert e.rollout_delta_active() and e.rollout_compact_active()      # on by default wherever the delta stream is
    on = res()
    e.set_rollout_compact(False)
    assert e.rollout_delta_active() and not e.rollout_compact_active()
    assert res() == on and on[1] == 4
    e.set_rollout_compact(True)
    e.set_rollout_delta(False)
    assert not e.rollout_delta_active() and not e.rollout_compact_active()
    e.set_rollout_delta(True)
    assert e.rollout_compact_active()
    # a shape the delta stream is not active for (the second copy would cost a resident workgroup): no compacted form either
    f = make(192, players=5, hand_size=4, shuffle_color=True, gpw=32, chunk=20)
    assert not f.rollout_delta_active() and not f.rollout_compact_active()
