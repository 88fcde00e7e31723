"""GPU: hsad_env_playout_random (BatchedHanabiEnv.playout_random) plays every live game to its end in one launch, without streaming
observations, on exactly the trajectory of policy_random + step; a finished game is never touched again."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import search_fixtures as SF
from tests.test_env_fork_gpu import DEV, make_env

pytestmark = pytest.mark.gpu
G = 65
Q_TERM, Q_SCORE, Q_NUM_STEP, Q_DRAWS = 0, 2, 6, 13


def _drain(env):
    """the twin hands its finished games the noop, which the step refuses and notes (as eval.py does): only those notes may appear"""
    from hanabi_sad_amd import _lib
    n, g, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(env.lib.hsad_env_error_count(env.h, C.byref(n), C.byref(g), C.byref(c)))
    assert n.value == 0 or c.value == 3
    return n.value


def _twin_step(twin, pseed):
    """one iteration of the reference loop on the twin: policy, finished games parked on the noop, step"""
    live = twin.query()[:, Q_TERM] == 0
    a, ga = twin.policy_random(pseed)
    a, ga = a.clone(), ga.clone()
    noop = torch.full_like(a, twin.A - 1)
    twin.step(torch.where(live.unsqueeze(1), a, noop).contiguous(), torch.where(live.unsqueeze(1), ga, noop).contiguous())
    parked = _drain(twin)
    assert parked == int((~live).sum())
    return live, a, ga


@pytest.mark.parametrize("config,sad,sc,km,gpw", [("full", True, True, 0, 64), ("small", False, False, 1, 32), ("c3r4", True, False, 0, 32)],
                         ids=lambda x: str(x))
def test_playout_is_the_policy_step_loop_without_restarts(config, sad, sc, km, gpw):
    pseed = 4711
    env, twin, once = (make_env(config, sad, sc, km, G, gpw, 8400) for _ in range(3))
    for e in (env, twin, once):
        e.reset()
    # iteration by iteration first: the sampled actions are those of the policy kernel
    for it in range(6):
        a, ga = env.playout_random(1, pseed)
        live, ta, tga = _twin_step(twin, pseed)
        assert torch.equal(a[live], ta[live]) and torch.equal(ga[live], tga[live]), "actions differ at iteration %d" % it
        assert torch.equal(env.export_state(), twin.export_state()), "state differs at iteration %d" % it
        assert torch.equal(env.terminal, twin.terminal)
    # then to the end in one launch
    env.playout_random(250, pseed)
    once.playout_random(250, pseed)
    for _ in range(100):
        if bool((twin.query()[:, Q_TERM] == 1).all()):
            break
        _twin_step(twin, pseed)
    q, tq = env.query(), twin.query()
    assert bool((q[:, Q_TERM] == 1).all()) and bool((tq[:, Q_TERM] == 1).all())
    assert torch.equal(q, tq), "scores, steps or draws consumed differ from the twin's"
    assert torch.equal(env.export_state(), twin.export_state())
    assert torch.equal(once.export_state(), twin.export_state()) and torch.equal(once.query(), tq)
    assert torch.equal(env.terminal, torch.ones_like(env.terminal))
    (dh, n), (tdh, tn) = env.deck_history(), twin.deck_history()
    assert torch.equal(n, tn) and torch.equal(dh, tdh)
    env.check_errors()     # no error: finished games were left alone, not stepped
    once.check_errors()
    # a second call is a no-op: nothing restarts, no counter moves
    state, a0, g0 = env.export_state(), env.a.clone(), env.greedy_a.clone()
    env.playout_random(10, pseed)
    assert torch.equal(env.export_state(), state) and torch.equal(env.query(), q)
    assert torch.equal(env.a, a0) and torch.equal(env.greedy_a, g0)
    env.check_errors()
    # the policy counters of live games advanced once per step, those of finished games not at all: after a reset both envs,
    # which finished their games at different calls, still sample the same actions
    env.reset()
    once.reset()
    a1, _ = env.policy_random(3)
    a2, _ = once.policy_random(3)
    assert torch.equal(a1, a2)


def test_playout_stops_at_max_iter_and_leaves_policy_and_step_usable():
    env, twin = (make_env("full", False, False, 0, G, 64, 8500) for _ in range(2))
    env.reset()
    twin.reset()
    env.playout_random(7, 5)
    for _ in range(7):
        _twin_step(twin, 5)
    assert torch.equal(env.export_state(), twin.export_state())
    assert int(env.query()[:, Q_NUM_STEP].max()) == 7
    # the masks the policy reads are current although the rows are not
    a, ga = env.policy_random(5)
    ta, tga = twin.policy_random(5)
    live = twin.query()[:, Q_TERM] == 0
    assert torch.equal(a[live], ta[live])
