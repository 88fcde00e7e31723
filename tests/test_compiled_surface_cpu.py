"""The compiled `rela` / `hanalearn` modules (bindings/*.cc -> build/*.so) carry every member the reference's bindings register, without a GPU:
the names below are those of cpp/pybind.cc:24-37 and rela/pybind.cc:17-91, written out here with their line citations.  FFTransition
behaves like the Python face's (hanabi_sad_amd/rela.py) on small CPU tensors, and RNNPrioritizedReplay.get refuses before anything was added.
The modules are imported in a subprocess whose sys.path puts build/ first, as a reference driver does."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# cpp/pybind.cc:24-37, in registration order
HANABI_ENV = ["feature_size",          # :24
              "num_action",            # :25
              "reset",                 # :26
              "step",                  # :27
              "terminated",            # :28
              "get_current_player",    # :29
              "move_is_legal",         # :30
              "last_score",            # :31
              "hand_feature_size",     # :32
              "deck_history",          # :33
              "get_score",             # :34
              "get_life",              # :35
              "get_info",              # :36
              "get_fireworks"]         # :37
FF_TRANSITION = ["obs", "action", "reward", "terminal", "bootstrap", "next_obs"]                     # rela/pybind.cc:18-23
RNN_TRANSITION = ["obs", "h0", "action", "reward", "terminal", "bootstrap", "seq_len"]              # rela/pybind.cc:26-32
RNN_REPLAY = ["size", "num_add", "sample", "update_priority", "get"]                                # rela/pybind.cc:54-58
CONTEXT = ["push_env_thread", "start", "pause", "resume", "terminate", "terminated"]                # rela/pybind.cc:64-69
R2D2_ACTOR = ["num_act"]                                                                           # rela/pybind.cc:82
BATCH_RUNNER = ["start", "stop", "update_model"]                                                   # rela/pybind.cc:87-89
MODULE_FUNCTIONS = ["aggregate_priority"]                                                          # rela/pybind.cc:92

DRIVER = r'''
import sys
build, root = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, build)
import torch
import rela, hanalearn
assert rela.__file__.endswith(".so") and hanalearn.__file__.endswith(".so"), (rela.__file__, hanalearn.__file__)
from hanabi_sad_amd import rela as pyrela
names = %r
missing = []
for cls, members in ((hanalearn.HanabiEnv, names["HanabiEnv"]), (rela.FFTransition, names["FFTransition"]),
                     (rela.RNNTransition, names["RNNTransition"]), (rela.RNNPrioritizedReplay, names["RNNPrioritizedReplay"]),
                     (rela.Context, names["Context"]), (rela.R2D2Actor, names["R2D2Actor"]), (rela.BatchRunner, names["BatchRunner"])):
    missing += ["%%s.%%s" %% (cls.__name__, m) for m in members if not hasattr(cls, m)]
missing += [f for f in names["module"] if not hasattr(rela, f)]
assert not missing, missing

# FFTransition: readwrite fields, constructor, index, to_dict -- against the Python face on the same tensors
g = torch.Generator().manual_seed(5)
obs = {"priv_s": torch.rand(4, 7, generator=g), "legal_move": torch.rand(4, 3, generator=g)}
action = {"a": torch.arange(4)}
next_obs = {"priv_s": torch.rand(4, 7, generator=g)}
reward, terminal, bootstrap = torch.rand(4, generator=g), torch.tensor([0, 1, 0, 1], dtype=torch.bool), torch.rand(4, generator=g)
c = rela.FFTransition(obs, action, reward, terminal, bootstrap, next_obs)
p = pyrela.FFTransition(obs, action, reward, terminal, bootstrap, next_obs)
e = rela.FFTransition()
assert e.obs == {} and e.action == {} and e.next_obs == {} and e.reward is None
for f in names["FFTransition"]:
    assert getattr(c, f) is getattr(p, f), f
    setattr(e, f, getattr(c, f))
    assert getattr(e, f) is getattr(c, f), f

def same(x, y):
    if isinstance(x, dict):
        return isinstance(y, dict) and list(x) == list(y) and all(same(x[k], y[k]) for k in x)
    if isinstance(x, torch.Tensor):
        return isinstance(y, torch.Tensor) and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    return x == y

for i in range(4):
    ci, pi = c.index(i), p.index(i)
    for f in names["FFTransition"]:
        assert same(getattr(ci, f), getattr(pi, f)), (i, f)
assert same(c.to_dict(), p.to_dict()), (list(c.to_dict()), list(p.to_dict()))
assert same(e.to_dict(), p.to_dict())

# RNNTransition: all seven fields readwrite
t = rela.RNNTransition(obs, action, reward, terminal, bootstrap, torch.ones(4))
for f in names["RNNTransition"]:
    v = {"x": torch.zeros(1)} if f in ("obs", "h0", "action") else torch.zeros(2)
    setattr(t, f, v)
    assert getattr(t, f) is v, f

# get() before anything was added: a RuntimeError naming the cause (no GPU touched)
r = rela.RNNPrioritizedReplay(64, 1, 0.9, 0.6, 3)
try:
    r.get(0)
except RuntimeError as err:
    assert "nothing has been added" in str(err), str(err)
else:
    raise AssertionError("get(0) on an empty replay did not raise")
print("ok")
'''


def test_compiled_modules_carry_every_reference_member_and_ff_transition_matches_the_python_face(tmp_path):
    import __graft_entry__ as ge
    ge.build_bindings()
    names = {"HanabiEnv": HANABI_ENV, "FFTransition": FF_TRANSITION, "RNNTransition": RNN_TRANSITION, "RNNPrioritizedReplay": RNN_REPLAY,
             "Context": CONTEXT, "R2D2Actor": R2D2_ACTOR, "BatchRunner": BATCH_RUNNER, "module": MODULE_FUNCTIONS}
    assert (len(HANABI_ENV), len(FF_TRANSITION), len(RNN_TRANSITION), len(RNN_REPLAY), len(CONTEXT), len(BATCH_RUNNER)) == (14, 6, 7, 5, 6, 3)
    out = subprocess.run([sys.executable, "-c", DRIVER % (names,), os.path.join(ROOT, "build"), ROOT], cwd=str(tmp_path), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]
