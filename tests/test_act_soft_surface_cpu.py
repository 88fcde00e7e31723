"""CPU: the host surface of softmax-policy acting -- how play_seatings / cross_play / evaluate read their `temperature` argument (all
before any device work), NetPartner(temperature=), the ctypes signatures of the new declarations of include/hsad.h, the command lines,
and, for the inputs of tests/test_act_sample_kernel_gpu.py, how many sampled rows lie within the margin of a boundary (a property of
the reference and u alone)."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import act_sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def weights(F=838, A=21):
    import torch
    return {"net.0.weight": torch.zeros(4, F), "fc_a.weight": torch.zeros(A, 4)}


def test_temperature_broadcast_and_refusals():
    from hanabi_sad_amd.eval import pool_temperatures
    assert pool_temperatures(None, 3) is None and pool_temperatures(0, 3) is None and pool_temperatures([0, 0.0, 0], 3) is None
    t = pool_temperatures(0.5, 3)
    assert t.dtype == np.float32 and t.tolist() == [0.5, 0.5, 0.5]
    assert pool_temperatures([0, 1, 0.25], 3).tolist() == [0.0, 1.0, 0.25]
    assert pool_temperatures(np.float32(2.0), 2).tolist() == [2.0, 2.0]
    for bad, text in (([1, 0], "one per pool member"), ([[1, 0, 0]], "one per pool member"), ([0, -1, 0], ">= 0"), (-0.5, ">= 0"),
                      ([0, float("nan"), 0], "finite"), (float("inf"), "finite")):
        with pytest.raises(ValueError, match=text):
            pool_temperatures(bad, 3)


def test_play_seatings_refuses_before_any_device_work():
    """device "cuda:99" does not exist: a call that got as far as the device would fail with another error"""
    from hanabi_sad_amd.eval import cross_play, evaluate, play_seatings
    from hanabi_sad_amd.rulebot import PRESETS

    class Other:                    # an agent of another family (obl.OBLAgent, rela.ContractAgent, the fp32 R2D2Agent): act / get_h0 only
        def act(self, obs, hid):
            raise AssertionError("never reached")

        def get_h0(self, n):
            raise AssertionError("never reached")
    kw = dict(device="cuda:99")
    with pytest.raises(ValueError, match=r"pool member 1 \(theirs\) cannot play at temperature 0.5"):
        play_seatings([weights(), Other(), PRESETS["piers"]], [(0, 1)], 4, 1, 0, True, temperature=[0, 0.5, 0], names=["w", "theirs", "piers"], **kw)
    with pytest.raises(ValueError, match=r"pool member 0 \(model0\) cannot play at temperature 1"):
        play_seatings([weights()], [(0, 0)], 4, 1, 0, True, temperature=1.0, precision="fp32", **kw)
    with pytest.raises(ValueError, match="one per pool member"):
        cross_play([weights(), PRESETS["piers"]], 4, 1, 0, True, temperature=[1, 1, 1], **kw)
    with pytest.raises(ValueError, match=">= 0"):
        cross_play([weights(), PRESETS["piers"]], 4, 1, 0, True, temperature=-1, **kw)
    with pytest.raises(ValueError, match="4096 moves"):
        play_seatings([weights()], [(0, 0)], 4, 1, 0, True, temperature=1.0, max_steps=5000, **kw)
    with pytest.raises(ValueError, match="cannot play at temperature"):
        evaluate(Other(), 4, 1, 0, True, temperature=1.0, **kw)
    with pytest.raises(ValueError, match=">= 0"):
        evaluate(weights(), 4, 1, 0, True, temperature=-1.0, **kw)
    # a rule bot ignores its entry: the refusal names no bot
    from hanabi_sad_amd.eval import check_pool_temperatures
    check_pool_temperatures([PRESETS["piers"], weights()], np.float32([3, 1]), ["piers", "w"], "bf16")


def test_sample_keys_are_injective_over_a_call():
    import torch
    from hanabi_sad_amd.eval import SAMPLE_KEY_STEPS, sample_key_base
    deals, seats = torch.arange(5000, 5300).repeat_interleave(5), torch.arange(5).repeat(300)
    base = sample_key_base(deals, seats)
    keys = (base.view(-1, 1) + torch.tensor([0, 1, SAMPLE_KEY_STEPS - 1])).reshape(-1)
    assert keys.dtype == torch.int64 and len(torch.unique(keys)) == keys.numel()


def test_net_partner_round_trips_its_temperature():
    from hanabi_sad_amd.actor import NetPartner
    assert NetPartner(weights()).temperature == 0.0
    assert NetPartner(weights(), name="x", skip_connect=False, temperature=0.75).temperature == 0.75
    assert list(inspect.signature(NetPartner.__init__).parameters)[1:] == ["source", "name", "skip_connect", "temperature"]
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            NetPartner(weights(), temperature=bad)
    from hanabi_sad_amd import selfplay
    args = selfplay.parse_args(["--partner", "piers", "--partner_temperature", "0.5"]) if hasattr(selfplay, "parse_args") else None
    if args is not None:
        assert args.partner_temperature == 0.5


def test_keywords_of_the_callers():
    from hanabi_sad_amd import clone, eval as ev
    from hanabi_sad_amd.composite import CompositeAgent
    assert inspect.signature(ev.evaluate).parameters["temperature"].default == 0.0
    assert inspect.signature(ev.evaluate).parameters["sample_seed"].default == 0
    assert inspect.signature(ev.play_seatings).parameters["temperature"].default is None
    assert inspect.signature(ev.play_seatings).parameters["sample_seed"].default == 0
    assert inspect.signature(clone.records_from_teacher).parameters["temperature"].default is None
    assert inspect.signature(clone.records_from_teacher).parameters["sample_seed"].default == 0
    assert inspect.signature(CompositeAgent.act).parameters["sample_seed"].default is None
    a = clone.parse_args(["--games", "x", "--eval_temperature", "1", "--teacher_temperature", "0.5"])
    assert (a.eval_temperature, a.teacher_temperature) == (1.0, 0.5)
    from hanabi_sad_amd import eval_model
    b = eval_model.parse_args(["--temperature", "1", "0.5", "--sample_seed", "3"])
    assert b.temperature == [1.0, 0.5] and b.sample_seed == 3 and eval_model.parse_args([]).temperature is None
    # refusals of the command lines, before anything is loaded
    for flag in ("--eval_temperature", "--teacher_temperature"):
        with pytest.raises(SystemExit, match="not negative"):
            clone.main(["--games", "nowhere.jsonl", flag, "-1"])
    with pytest.raises(SystemExit, match="not negative"):
        eval_model.main(["--paper", "sad", "--weight", "nowhere.pthw", "--temperature", "1", "-0.5"])
    with pytest.raises(SystemExit, match="no --search_worlds"):
        eval_model.main(["--paper", "op", "--idx", "0", "--search_worlds", "4", "--temperature", "1"])


def test_the_new_declarations_have_ctypes_signatures():
    from hanabi_sad_amd import _lib
    header = open(os.path.join(ROOT, "include", "hsad.h")).read()
    for name, n_args in (("hsad_act_sample_q", 16), ("hsad_r2d2_act_soft", 21), ("hsad_actor_set_partner_temperature", 3)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, flags=re.M)
        assert m, "%s is not declared in include/hsad.h" % name
        assert len(m.group(1).split(",")) == n_args
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == n_args, name
    # where the 64-bit seeds and the float sit
    import ctypes as C
    assert _lib.SIGNATURES["hsad_act_sample_q"][1][6] is C.c_uint64 and _lib.SIGNATURES["hsad_r2d2_act_soft"][1][8] is C.c_uint64
    assert _lib.SIGNATURES["hsad_actor_set_partner_temperature"][1][2] is C.c_float


def test_few_rows_of_the_gpu_inputs_lie_near_a_boundary():
    from tests.test_act_sample_kernel_gpu import SHAPES, expected_rows, make_inputs
    for N, A, ldh in SHAPES:
        heads, legal, eps, temp, key = make_inputs(N, A, ldh)
        for k in (None, key):
            sampled = near = 0
            for m, (kind, u) in expected_rows(heads, legal, eps, temp, k, A).items():
                _, idx, cdf = R.pick(heads[m, :A], legal[m], temp[m], u)
                if kind == "sample" and len(idx) > 1:
                    sampled += 1
                    near += bool(np.abs(cdf[:-1] - u).min() <= R.MARGIN)
            print("N %d A %d %s: %d of %d sampled rows within the margin" % (N, A, "keyed" if k is not None else "unkeyed", near, sampled))
            assert near <= sampled // 100 and (sampled > N // 4 or N == 1)
