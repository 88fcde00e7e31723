"""The compiled `rela` / `hanalearn` modules (bindings/*.cc -> build/*.so) against the Python face (hanabi_sad_amd/rela.py, hanalearn.py) on
one GPU: single-game stepping, replay.get / sample(.., "cpu") in the shape of the reference's tools/action_matrix.py, skip-connection models
of the Other-Play zoo, models behind the act / get_h0 contract in evaluation loops (alone and in cross-play), and the lifetimes of the
actors' step counts and the loop's end flag.

Every driver runs in a subprocess (this file run as a script) with build/ and the repository root in front of the inherited PYTHONPATH
(compiled face) or the repository root alone in front of it (Python face, whose rela / hanalearn packages re-export hanabi_sad_amd).  A
driver that dies by a signal or its time limit fails its test and every later one in this file without starting anything more on the GPU."""
import gc
import json
import os
import subprocess
import sys
import threading
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")
DEV = "cuda:0"
SMALL_PARAMS = {"players": "2", "colors": "2", "ranks": "5", "hand_size": "2", "max_information_tokens": "3",
                "max_life_tokens": "1", "seed": "4", "bomb": "0", "observation_type": "1", "random_start_player": "0"}   # test_env_variants_gpu.py:158-159
SKIP_GAMES = 64          # enough games that the zoo models' scores see the skip connection (asserted below)
CONTRACT_GAMES = 32


class ProbeAgent(nn.Module):
    """a model behind the act / get_h0 contract that is NOT the R2D2Net shape (no online_net.*): fc -> fc (+ skip) -> an LSTM cell ->
    advantage head, greedy and deterministic.  act: {priv_s [S,E,F], legal_move [S,E,A], eps [S,E], h0/c0 [S,E,L,H]} ->
    {a, greedy_a [S,E], h0, c0 [S,E,L,H]} (replies on the CPU, like the reference's TorchScript agents); L = 1"""

    def __init__(self, F, A, H=32):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(F, H), nn.Linear(H, H)
        self.wx, self.wh = nn.Linear(H, 4 * H), nn.Linear(H, 4 * H, bias=False)
        self.adv = nn.Linear(H, A)
        self.H, self.shapes = H, []

    def get_h0(self, n):
        z = torch.zeros(1, n, self.H, device=self.adv.weight.device)
        return {"h0": z, "c0": z.clone()}

    def act(self, d):
        S, E = d["priv_s"].shape[:2]
        self.shapes.append({k: list(v.shape) for k, v in d.items()})
        h0 = d["h0"].flatten(0, 2)           # [S*E, H] (one layer)
        c0 = d["c0"].flatten(0, 2)
        x = torch.relu(self.fc1(d["priv_s"].flatten(0, 1)))
        x = x + torch.relu(self.fc2(x))
        i, f, g, o = (self.wx(x) + self.wh(h0)).chunk(4, 1)
        c = torch.sigmoid(f) * c0 + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        adv = self.adv(h)
        legal = d["legal_move"].flatten(0, 1)
        greedy = ((1 + adv - adv.min()) * legal).argmax(1)
        shp = (S, E, 1, self.H)
        return {"a": greedy.view(S, E).cpu(), "greedy_a": greedy.view(S, E).cpu(), "h0": h.reshape(shp).cpu(), "c0": c.reshape(shp).cpu()}


# ------------------------------------------------------------------------------------------------------------------------------------
# drivers (run as `python tests/test_compiled_surface_gpu.py <face> <what> <out.json>`)
# ------------------------------------------------------------------------------------------------------------------------------------
class TinyAgent:
    """stands in for the reference's R2D2Agent: what BatchRunner needs is state_dict() with online_net.* / target_net.*"""

    def __init__(self, in_dim, hid, out_dim, hand, seed):
        from hanabi_sad_amd.selfplay import init_weights
        W = init_weights(in_dim, hid, out_dim, hand, seed)
        self.sd = {"online_net." + k: v for k, v in W.items()}
        self.sd.update({"target_net." + k: v.clone() for k, v in W.items()})

    def state_dict(self):
        return self.sd


def create_envs(hanalearn, num_env, seed, num_player, hand_size, bomb, eps, max_len, sad):
    params = lambda i: {"players": str(num_player), "hand_size": str(hand_size), "seed": str(seed + i), "bomb": str(bomb)}
    return [hanalearn.HanabiEnv(params(i), eps, max_len, sad, False, False, False) for i in range(num_env)]


def wait_terminated(context, limit=120):
    t0 = time.time()
    while not context.terminated():
        assert time.time() - t0 < limit, "evaluation did not finish"
        time.sleep(0.02)


def drive_single():
    """both faces in this process: the compiled hanalearn.HanabiEnv and hanabi_sad_amd.hanalearn.HanabiEnv, same params, same moves"""
    import numpy as np
    import hanalearn
    from hanabi_sad_amd import hanalearn as pyhl
    configs = [("2p", {"players": "2"}, False, False),
               ("2p-sad-shuffle-bomb", {"players": "2", "bomb": "1"}, True, True),
               ("5p-hand4-sad", {"players": "5", "hand_size": "4"}, True, False),
               ("small", dict(SMALL_PARAMS), False, False)]
    getters = ("terminated", "get_current_player", "get_score", "get_life", "get_info", "last_score", "get_fireworks")
    report = {}
    for name, base, sad, shuffle_color in configs:
        steps = 0
        for seed in (3, 11):
            params = dict(base, seed=str(seed))
            c = hanalearn.HanabiEnv(params, [0.0], 80, sad, False, shuffle_color, False)
            p = pyhl.HanabiEnv(params, [0.0], 80, sad, False, shuffle_color, False)
            assert (c.feature_size(), c.num_action(), c.hand_feature_size()) == (p.feature_size(), p.num_action(), p.hand_feature_size()), name
            A = c.num_action()
            rng = np.random.default_rng(seed * 1000 + len(name))

            def same_obs(oc, op, where):
                assert list(oc) == list(op), (where, list(oc), list(op))
                for k in oc:
                    x, y = oc[k], op[k]
                    assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape and str(x.device) == str(y.device), (where, k)
                    assert torch.equal(x, y), (where, k)

            def same_queries(where):
                for g in getters:
                    assert getattr(c, g)() == getattr(p, g)(), (where, g)
                for u in range(A):
                    assert c.move_is_legal(u) == p.move_is_legal(u), (where, u)

            for episode in range(2):          # the second reset() follows a finished game
                oc, op = c.reset(), p.reset()
                same_obs(oc, op, (name, seed, episode, "reset"))
                same_queries((name, seed, episode, "reset"))
                terminal = False
                while not terminal:
                    legal = oc["legal_move"].cpu().numpy()
                    a = torch.tensor([int(rng.choice(np.flatnonzero(legal[q]))) for q in range(legal.shape[0])], dtype=torch.int64)
                    act = {"a": a}
                    if sad:
                        act["greedy_a"] = torch.tensor([int(rng.choice(np.flatnonzero(legal[q]))) for q in range(legal.shape[0])],
                                                       dtype=torch.int64)
                    oc, rc, tc = c.step(act)
                    op, rp, tp = p.step(act)
                    where = (name, seed, episode, steps)
                    same_obs(oc, op, where)
                    assert type(rc) is float and type(tc) is bool and rc == rp and tc == tp, (where, rc, rp, tc, tp)
                    same_queries(where)
                    terminal = tc
                    steps += 1
                assert c.deck_history() == p.deck_history(), (name, seed, episode)
                assert len(c.deck_history()) > 0
            # an illegal move raises on the compiled face and the process goes on
            oc = c.reset()
            legal = oc["legal_move"].cpu().numpy()
            cur = c.get_current_player()
            bad = int(np.flatnonzero(legal[cur] == 0)[0])
            a = torch.tensor([bad if q == cur else A - 1 for q in range(legal.shape[0])], dtype=torch.int64)
            try:
                c.step({"a": a, "greedy_a": a} if sad else {"a": a})
            except RuntimeError as e:
                assert "illegal" in str(e), str(e)
            else:
                raise AssertionError("an illegal move did not raise")
            assert not c.terminated() and c.get_current_player() == cur
        report[name] = steps
    return report


def drive_replay(rela, hanalearn, compiled):
    """tools/action_matrix.py:31-107, call order: VDN actors of one game per thread, multi_step 1, priority exponent 0, eps [0]; wait for
    N sequences, pause, two sample(10, "cpu") / update_priority(w.cpu()) rounds, then get(i).action["a"][t][p] / get(i).seq_len"""
    import hashlib
    import numpy as np
    N, capacity, num_thread, max_len = 256, 4096, 100, 80
    games = create_envs(hanalearn, num_thread, 1, 2, 5, 0, [0], max_len, True)
    agent = TinyAgent(games[0].feature_size(), 64, games[0].num_action(), 5, 9)
    runner = rela.BatchRunner(agent, DEV, 100, ["act", "compute_priority"])
    replay = rela.RNNPrioritizedReplay(capacity, 1, 0, 1, 0)
    actors = [rela.R2D2Actor(runner, 1, 1, 0.99, 0.9, max_len, 2, replay) for _ in range(num_thread)]
    context = rela.Context()
    for t in range(num_thread):
        env = hanalearn.HanabiVecEnv()
        env.append(games[t])
        context.push_env_thread(hanalearn.HanabiThreadLoop(actors[t], env, False))
    runner.start()
    context.start()
    t0 = time.time()
    while replay.size() < N:
        assert time.time() - t0 < 120, replay.size()
        time.sleep(0.01)
    context.pause()
    size = replay.size()
    assert N <= size < capacity, size

    def tensors_of(data, w):
        t = dict(data.obs, **data.action)
        t.update(reward=data.reward, terminal=data.terminal, bootstrap=data.bootstrap, seq_len=data.seq_len, weight=w)
        return t
    shapes = []
    for _ in range(2):
        data, w = replay.sample(10, "cpu")
        t = tensors_of(data, w)
        if compiled:          # (the Python face hands the batch over on the replay's device whatever it is asked for)
            assert all(v.device.type == "cpu" for v in t.values()), {k: str(v.device) for k, v in t.items()}
        shapes.append({k: [str(v.dtype)] + list(v.shape) for k, v in t.items()})
        replay.update_priority(w.cpu())
    data, w = replay.sample(10, DEV)          # a device sample's layout, for comparison
    t = tensors_of(data, w)
    assert all(v.device.type == "cuda" for v in t.values())
    device_shapes = {k: [str(v.dtype)] + list(v.shape) for k, v in t.items()}
    replay.update_priority(w)
    p0_p1 = np.zeros((20, 20))
    digests, pad_bad = [], 0
    for i in range(N):
        epsd = replay.get(i)
        action = epsd.action["a"]
        for t in range(int(epsd.seq_len.item()) - 1):
            if t % 2 == 0:
                a0, a1 = int(action[t][0].item()), int(action[t + 1][1].item())
            else:
                a0, a1 = int(action[t][1].item()), int(action[t + 1][0].item())
            p0_p1[a0][a1] += 1
        fields = dict(("obs." + k, v) for k, v in epsd.obs.items())
        fields.update(("action." + k, v) for k, v in epsd.action.items())
        fields.update(reward=epsd.reward, terminal=epsd.terminal, bootstrap=epsd.bootstrap, seq_len=epsd.seq_len)
        digests.append({k: "%s %s %s" % (str(v.dtype), list(v.shape), hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest())
                        for k, v in fields.items()})
        L = int(epsd.seq_len.item())
        pad_bad += int(any(bool(v[L:].any()) for v in epsd.obs.values()))          # padLike (rela/transition.cc:29-40): zero observations,
        pad_bad += int(not bool(epsd.terminal[L:].all())) + int(bool(epsd.bootstrap[L:].any()))   # terminal = 1, bootstrap = 0
    context.terminate()
    return {"size": size, "shapes": shapes, "device_shapes": device_shapes, "digests": digests, "p0_p1": p0_p1.astype(int).tolist(),
            "pad_bad": pad_bad}


def zoo_agent(path, skip):
    from hanabi_sad_amd.checkpoint import load_weights
    from hanabi_sad_amd.torch_r2d2 import R2D2Agent
    W = load_weights(path)
    nl = sum(1 for k in W if k.startswith("lstm.weight_ih_l"))
    nfc = 2 if "net.2.weight" in W else 1
    hid, in_dim = W["net.0.weight"].shape
    agent = R2D2Agent(False, 3, 0.999, 0.9, DEV, in_dim, hid, W["fc_a.weight"].shape[0], nl, W["pred.weight"].shape[0] // 3, False,
                      num_fc_layer=nfc, skip_connect=skip)
    agent.online_net.load_state_dict(W)
    agent.sync_target_with_online()
    return agent, W


def compiled_eval(rela, hanalearn, runners, num_game, seed, sad, lifetimes=False):
    """eval.py:25-66 shape: one vector env and thread loop per game, one actor per seat (runners[p] plays seat p)"""
    games = create_envs(hanalearn, num_game, seed, 2, 5, 0, [0.0], -1, sad)
    context, loops, actors = rela.Context(), [], []
    for g in games:
        env = hanalearn.HanabiVecEnv()
        env.append(g)
        seat = [rela.R2D2Actor(r, 1) for r in runners]
        actors += seat
        loops.append(hanalearn.HanabiThreadLoop(seat, env, True))
        context.push_env_thread(loops[-1])
    seen, errors = [], []

    def reader():          # Context.terminated() polled from another thread while the loop runs
        try:
            t0 = time.time()
            while not context.terminated():
                assert time.time() - t0 < 120
                seen.append(False)
                time.sleep(0.001)
            seen.append(True)
        except Exception as e:          # noqa: BLE001 (reported to the driver's thread)
            errors.append(repr(e))
    th = threading.Thread(target=reader) if lifetimes else None
    context.start()
    if th is not None:
        th.start()
    wait_terminated(context)
    if th is not None:
        th.join(timeout=60)
        assert not th.is_alive() and not errors and seen and seen[-1], (errors, seen[-5:])
    context.terminate()
    scores = [g.last_score() for g in games]
    out = {"scores": scores}
    if lifetimes:
        before = [a.num_act() for a in actors]
        assert all(n > 0 for n in before)
        del context, loops, games, env, g
        gc.collect()
        out["num_act_kept"] = [a.num_act() for a in actors] == before
    return out


def drive_skip():
    import rela
    import hanalearn
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.eval import evaluate
    out = {}
    for m in ("M3", "M9"):
        path = os.path.join(ROOT, "tests", "golden", "op_zoo", "models", "op", "sad", m + ".pthw")
        agent, W = zoo_agent(path, True)
        runner = rela.BatchRunner(agent, DEV, 1000, ["act"])
        runner.update_model(agent)          # keeps the architecture (skip connection) the runner was built with
        got = compiled_eval(rela, hanalearn, [runner, runner], SKIP_GAMES, 1000, False)["scores"]
        ref = {}
        for skip in (True, False):
            net = CNet(W, DEV, skip_connect=skip)
            ref[skip] = evaluate(CompositeAgent(net, net, 1, 0.99), SKIP_GAMES, 1000, 0, False, device=DEV)[2]
        out[m] = {"compiled": got, "python_skip": ref[True], "python_noskip": ref[False]}
    return out


def drive_contract(rela, hanalearn, compiled):
    torch.manual_seed(11)
    probe_env = hanalearn.HanabiEnv({"players": "2", "seed": "1"}, [0.0], -1, True, False, False, False)
    F, A = probe_env.feature_size(), probe_env.num_action()
    model = ProbeAgent(F, A).to(DEV)
    crunner = rela.BatchRunner(model, DEV, 1000, ["act"])
    krunner = rela.BatchRunner(TinyAgent(F, 64, A, 5, 21), DEV, 1000, ["act"])
    out = {}
    out["solo"] = compiled_eval(rela, hanalearn, [crunner, crunner], CONTRACT_GAMES, 300, True, lifetimes=compiled)
    out["solo_first_call"] = model.shapes[0]
    model.shapes.clear()
    out["cross"] = compiled_eval(rela, hanalearn, [crunner, krunner], CONTRACT_GAMES, 700, True, lifetimes=compiled)
    out["cross_first_call"] = model.shapes[0]
    if compiled:
        crunner.update_model(ProbeAgent(F, A).to(DEV))          # a contract runner takes another model's weights
        replay = rela.RNNPrioritizedReplay(1024, 1, 0.9, 0.6, 0)
        env = hanalearn.HanabiVecEnv()
        env.append(probe_env)
        loop = hanalearn.HanabiThreadLoop(rela.R2D2Actor(crunner, 1, 1, 0.99, 0.9, 80, 2, replay), env, False)
        ctx = rela.Context()
        try:
            ctx.push_env_thread(loop)
        except RuntimeError as e:
            out["train_refused"] = str(e)
        ctx.terminate()
    return out


def _main():
    face, what, out_path = sys.argv[1], sys.argv[2], sys.argv[3]
    import rela
    import hanalearn
    compiled = face == "compiled"
    # the extension modules' classes are pybind11 types; the Python face's are plain classes
    assert ("pybind11" in repr(type(rela.Context))) == compiled and ("pybind11" in repr(type(hanalearn.HanabiEnv))) == compiled, \
        (rela.__file__, repr(type(rela.Context)))
    if compiled:
        assert rela.__file__.startswith(BUILD) and hanalearn.__file__.startswith(BUILD), (rela.__file__, hanalearn.__file__)
    if what == "single":
        res = drive_single()
    elif what == "replay":
        res = drive_replay(rela, hanalearn, compiled)
    elif what == "skip":
        res = drive_skip()
    else:
        res = drive_contract(rela, hanalearn, compiled)
    with open(out_path, "w") as f:
        json.dump(res, f)
    print("driver %s %s OK" % (face, what), flush=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------------------------------------------
if __name__ != "__main__":
    import pytest

    pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
    _STOPPED = []          # a driver died by a signal or hit its time limit: nothing more starts on the GPU from this file

    def _run(face, what, tmp_path, timeout=300):
        if _STOPPED:
            pytest.fail("an earlier driver of this file ended with status %d: not starting another GPU process" % _STOPPED[0])
        env = dict(os.environ, HSAD_QUIET="1")
        front = [BUILD, ROOT] if face == "compiled" else [ROOT]
        env["PYTHONPATH"] = os.pathsep.join(front + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        out_path = str(tmp_path / ("%s_%s.json" % (face, what)))
        t0 = time.time()
        p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), face, what, out_path],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True)
        print("%s %s driver: %.1f s, exit %d" % (face, what, time.time() - t0, p.returncode))
        if p.returncode < 0 or p.returncode >= 124:        # (timeout: 124 / 137 on its limit, 128 + N when the driver died by signal N)
            _STOPPED.append(p.returncode)
            pytest.fail("%s %s driver ended by a signal or the time limit (%d): %s" % (face, what, p.returncode, p.stderr[-4000:]))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        with open(out_path) as f:
            return json.load(f)

    def _modules_built():
        import glob
        assert glob.glob(os.path.join(BUILD, "rela*.so")) and glob.glob(os.path.join(BUILD, "hanalearn*.so")), \
            "build/rela*.so / build/hanalearn*.so missing: run python -c 'import __graft_entry__ as g; g.build()'"

    def test_single_game_members_are_bit_equal_to_the_python_face(tmp_path):
        _modules_built()
        rep = _run("compiled", "single", tmp_path)
        print("steps compared per configuration:", rep)
        assert set(rep) == {"2p", "2p-sad-shuffle-bomb", "5p-hand4-sad", "small"} and all(n > 0 for n in rep.values())

    def test_replay_get_and_cpu_sample_match_the_python_face_in_the_action_matrix_call_order(tmp_path):
        _modules_built()
        c = _run("compiled", "replay", tmp_path)
        p = _run("python", "replay", tmp_path)
        for r in (c, p):
            assert r["pad_bad"] == 0
        for s in c["shapes"]:
            assert s == c["device_shapes"], (s, c["device_shapes"])
        assert c["device_shapes"] == p["device_shapes"]
        assert len(c["digests"]) == len(p["digests"]) == 256
        for i, (x, y) in enumerate(zip(c["digests"], p["digests"])):
            assert x == y, (i, {k: (x.get(k), y.get(k)) for k in set(x) | set(y) if x.get(k) != y.get(k)})
        assert c["p0_p1"] == p["p0_p1"] and sum(map(sum, c["p0_p1"])) > 0

    def test_skip_connection_models_evaluate_like_the_python_face(tmp_path):
        _modules_built()
        r = _run("compiled", "skip", tmp_path)
        for m in ("M3", "M9"):
            x = r[m]
            print(m, "mean compiled %.3f, python skip %.3f, python without skip %.3f" % tuple(
                sum(x[k]) / len(x[k]) for k in ("compiled", "python_skip", "python_noskip")))
            assert x["python_skip"] != x["python_noskip"], "%s: %d games cannot see the skip connection" % (m, SKIP_GAMES)
            assert x["compiled"] == x["python_skip"], m

    def test_contract_model_evaluates_alone_and_in_cross_play_like_the_python_face(tmp_path):
        _modules_built()
        c = _run("compiled", "contract", tmp_path)
        p = _run("python", "contract", tmp_path)
        assert c["solo"]["scores"] == p["solo"]["scores"]
        assert c["cross"]["scores"] == p["cross"]["scores"]
        assert c["solo_first_call"] == p["solo_first_call"] and c["solo_first_call"]["priv_s"] == [1, 2 * CONTRACT_GAMES, 838]
        assert c["cross_first_call"] == p["cross_first_call"] and c["cross_first_call"]["h0"] == [1, CONTRACT_GAMES, 1, 32]
        # lifetimes: num_act() keeps its value after the Context and the loops are gone; a reader thread saw terminated() turn True
        assert c["solo"]["num_act_kept"] and c["cross"]["num_act_kept"]
        assert "Python face" in c.get("train_refused", ""), c.get("train_refused")


if __name__ == "__main__":
    _main()
