"""sampler="learned" without a GPU: the refusals of search.PolicySearch / policy_action_values / play_with_search / mc_action_values
(all ValueError, all before anything touches the device), eval_model's argument errors, belief.BeliefSampler on bad state dicts, and
that the header, the ctypes table and the Python surface carry the two new entry points."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "hsad_env_determinize_belief_worlds": "int hsad_env_determinize_belief_worlds(hsad_env* env, const int32_t* viewer, const float* logits, int ldz, "
                                          "int n_rows, const int32_t* row, const int64_t* group, const int32_t* world, int n_worlds, uint64_t seed, "
                                          "float* logp_out, float* logp0_out, int32_t* status_out, void* stream);",
    "hsad_search_belief_rows": "int hsad_search_belief_rows(const float* h_top, const int32_t* player, int G, int P, int H, void* out_bf16, int ldo, "
                               "void* stream);",
}


def head_state(H=64, hand_size=5):
    return {"belief.weight": torch.zeros(25 * hand_size, H), "belief.bias": torch.zeros(25 * hand_size), "hand_size": hand_size, "H": H}


def fake_agent(H=64, skip=False):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    return NS(online=NS(H=H, L=2, skip=skip), get_h0=boom, act=boom)


def fake_env(H=5):
    class Env:
        def __getattr__(self, name):
            raise AssertionError("the env was touched (%s)" % name)
    e = Env()
    e.__dict__["H"] = H
    return e


def test_header_ctypes_table_and_callers_carry_the_entry_points():
    from hanabi_sad_amd import _lib, belief, env, eval_model, search
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hsad.h")).read(), flags=re.S)
    for name, want in DECLARED.items():
        found = re.findall(r"\bint\s+%s\s*\([^;]*\);" % name, txt)
        assert len(found) == 1 and re.sub(r"\s+", " ", found[0]) == want, name
        restype, argtypes = _lib.SIGNATURES[name]
        args = want[want.index("(") + 1:want.rindex(")")].split(", ")
        assert restype is C.c_int and argtypes == [C.c_void_p if "*" in a else (C.c_uint64 if a.startswith("uint64_t") else C.c_int) for a in args], name
    assert search.SAMPLERS == ("rejection", "stratified", "learned")
    for fn in (search.PolicySearch.search, search.policy_action_values):
        assert inspect.signature(fn).parameters["hid_next"].default is None
    for fn in (search.PolicySearch.__init__, search.policy_action_values, search.play_with_search):
        assert inspect.signature(fn).parameters["belief"].default is None
    assert list(inspect.signature(env.BatchedHanabiEnv.determinize_belief_worlds).parameters)[1:] == ["viewer", "logits", "row", "group", "world",
                                                                                                    "n_worlds", "seed"]
    assert hasattr(belief.BeliefSampler, "logits")
    sv = search.SearchValues(torch.zeros(1, 2, 3, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    assert sv.belief_logp is None and sv.belief_logp0 is None
    args = eval_model.parse_args(["--search_sampler", "learned", "--search_belief", "x.pthw"])
    assert args.search_sampler == "learned" and args.search_belief == "x.pthw"
    assert eval_model.parse_args([]).search_belief is None
    # the header of the uniforms names its stream, and no other sampler's
    text = open(os.path.join(ROOT, "hanabi_sad_amd", "csrc", "hsad_belief_world.h")).read()
    assert re.search(r"BW_STREAM = 67;", text)


def test_policy_search_refuses_before_any_device_work(tmp_path):
    from hanabi_sad_amd import search
    env, agent = fake_env(5), fake_agent(64)
    with pytest.raises(ValueError, match="needs belief"):
        search.PolicySearch(env, agent, 64, sampler="learned")
    for sampler in ("rejection", "stratified"):
        with pytest.raises(ValueError, match="takes none"):
            search.PolicySearch(env, agent, 64, sampler=sampler, belief=head_state())
    with pytest.raises(ValueError, match="sampler must be one of"):
        search.PolicySearch(env, agent, 64, sampler="belief", belief=head_state())
    with pytest.raises(ValueError, match="trunk of width 128"):
        search.PolicySearch(env, agent, 64, sampler="learned", belief=head_state(H=128))
    with pytest.raises(ValueError, match="hands of 4"):
        search.PolicySearch(env, agent, 64, sampler="learned", belief=head_state(hand_size=4))
    with pytest.raises(ValueError, match="skip_connect"):
        search.PolicySearch(env, fake_agent(64, skip=True), 64, sampler="learned", belief=head_state())
    # an object with a head's shape (a BeliefSampler, a BeliefHead) is checked alike
    with pytest.raises(ValueError, match="trunk of width 256"):
        search.PolicySearch(env, agent, 64, sampler="learned", belief=NS(hand_size=5, H=256, logits=None))
    # what is no head at all
    with pytest.raises(ValueError, match="not a belief head"):
        search.PolicySearch(env, agent, 64, sampler="learned", belief={"belief.weight": torch.zeros(125, 64)})
    with pytest.raises(ValueError, match="no such file"):
        search.PolicySearch(env, agent, 64, sampler="learned", belief=str(tmp_path / "missing.pthw"))
    with pytest.raises(ValueError):
        search.PolicySearch(env, agent, 64, sampler="learned", belief=3.5)
    path = str(tmp_path / "head.pthw")
    torch.save(head_state(H=128), path)
    with pytest.raises(ValueError, match="trunk of width 128"):
        search.PolicySearch(env, agent, 64, sampler="learned", belief=path)
    # the one-call faces pass the arguments on
    with pytest.raises(ValueError, match="needs belief"):
        search.policy_action_values(env, agent, None, 8, 1, sampler="learned")
    with pytest.raises(ValueError, match="takes none"):
        search.policy_action_values(env, agent, None, 8, 1, belief=head_state())
    with pytest.raises(ValueError, match="needs belief"):
        search.play_with_search(agent, 2, 1, 0, False, worlds=4, sampler="learned", device="cuda:0")
    with pytest.raises(ValueError, match="takes none"):
        search.play_with_search(agent, 2, 1, 0, False, worlds=4, sampler="stratified", belief=head_state(), device="cuda:0")
    with pytest.raises(ValueError, match="hands of 4"):
        search.play_with_search(agent, 2, 1, 0, False, worlds=4, sampler="learned", belief=head_state(hand_size=4), device="cuda:0")


def test_mc_action_values_has_no_learned_sampler():
    from hanabi_sad_amd import search
    with pytest.raises(ValueError, match="no learned sampler"):
        search.mc_action_values(fake_env(), 8, 1, sampler="learned")


def test_belief_sampler_refuses_bad_state_dicts_before_the_device(tmp_path):
    from hanabi_sad_amd.belief import BeliefSampler
    good = head_state()
    for drop in ("belief.weight", "belief.bias", "hand_size", "H"):
        with pytest.raises(ValueError, match="not a belief head"):
            BeliefSampler({k: v for k, v in good.items() if k != drop}, "cuda:0")
    with pytest.raises(ValueError):
        BeliefSampler(dict(good, **{"belief.weight": torch.zeros(125, 32)}), "cuda:0")      # the shapes disagree with H
    with pytest.raises(ValueError):
        BeliefSampler(dict(good, H=96, **{"belief.weight": torch.zeros(125, 96)}), "cuda:0")      # no multiple of 64
    with pytest.raises(ValueError):
        BeliefSampler(dict(good, hand_size=6, **{"belief.weight": torch.zeros(150, 64), "belief.bias": torch.zeros(150)}), "cuda:0")
    with pytest.raises(ValueError):
        BeliefSampler(dict(good, **{"belief.bias": torch.zeros(100)}), "cuda:0")
    with pytest.raises(ValueError):
        BeliefSampler([1, 2, 3], "cuda:0")
    path = str(tmp_path / "weights.pthw")
    torch.save({"fc_a.weight": torch.zeros(3, 3)}, path)
    with pytest.raises(ValueError, match="not a belief head"):
        BeliefSampler(path, "cuda:0")


def test_eval_model_argument_errors(tmp_path):
    from hanabi_sad_amd import eval_model
    base = ["--paper", "op", "--method", "sad", "--idx", "0", "--search_worlds", "4"]
    with pytest.raises(SystemExit, match="go together"):
        eval_model.main(base + ["--search_sampler", "learned"])
    with pytest.raises(SystemExit, match="go together"):
        eval_model.main(base + ["--search_belief", "x.pthw"])
    with pytest.raises(SystemExit, match="go together"):
        eval_model.main(base + ["--search_sampler", "stratified", "--search_belief", "x.pthw"])
    with pytest.raises(SystemExit, match="no such file"):
        eval_model.main(base + ["--search_sampler", "learned", "--search_belief", str(tmp_path / "missing.pthw")])
    path = str(tmp_path / "weights.pthw")
    torch.save({"fc_a.weight": torch.zeros(3, 3)}, path)
    with pytest.raises(SystemExit, match="not a belief head"):
        eval_model.main(base + ["--search_sampler", "learned", "--search_belief", path])
    junk = str(tmp_path / "junk.pthw")
    with open(junk, "wb") as fh:
        fh.write(b"not a torch file")
    with pytest.raises(SystemExit, match="search_belief"):
        eval_model.main(base + ["--search_sampler", "learned", "--search_belief", junk])
    with pytest.raises(SystemExit):      # argparse: no such sampler
        eval_model.parse_args(["--search_sampler", "belief"])
