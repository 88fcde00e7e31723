"""GPU: game variants (HLE's colors / ranks / max_information_tokens / max_life_tokens) on the HIP env kernels, bit-exact against
the variant restatement (tests/variant_oracle) step by step, through the C ABI, both hanalearn faces, the random-policy rollout and a
short training run (modelled on test_env_parity_gpu.py)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.oracle import policy_random
from tests.test_env_parity_gpu import EPS, _bits, _cmp
from tests.variant_oracle.variant_oracle import VariantEnv, VariantVecEnv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1)
VARIANTS = {
    "small": dict(players=2, hand_size=2, **SMALL),
    "very_small": dict(players=2, hand_size=2, colors=1, ranks=5, max_information_tokens=3, max_life_tokens=1),
    "c3r4": dict(players=3, hand_size=4, colors=3, ranks=4, max_information_tokens=6, max_life_tokens=2),
    "r1": dict(players=2, hand_size=3, colors=4, ranks=1, max_information_tokens=2, max_life_tokens=3),
    "p4": dict(players=4, hand_size=3, colors=4, ranks=3, max_information_tokens=5, max_life_tokens=2),
    "tokens": dict(players=2, hand_size=5, colors=5, ranks=5, max_information_tokens=4, max_life_tokens=2),
}
# variant x (sad, shuffle_color, knowledge_mode, bomb, max_len)
GRID = [(v, sad, sc, km, bomb) for v in sorted(VARIANTS) for (sad, sc, km, bomb) in
        ((False, False, 0, 0), (True, True, 0, 1), (True, False, 1, 0), (False, True, 1, 1))]


def _cmp_packed(dev, r_priv, r_legal, r_own, it):
    F, A, O = r_priv.shape[-1], r_legal.shape[-1], r_own.shape[-1]
    for name, t, ref, n in (("priv_bits", dev.priv_bits, r_priv, F), ("legal_bits", dev.legal_bits.unsqueeze(-1), r_legal, A),
                            ("own_bits", dev.own_bits.unsqueeze(-1), r_own, O)):
        got, rest = _bits(t, n)
        assert np.array_equal(got, ref) and not rest.any(), "%s differs at iteration %d" % (name, it)
    b16 = dev.priv_s_bf16.float().cpu().numpy()
    assert np.array_equal(b16[..., :F], r_priv) and not b16[..., F:].any(), "priv_s_bf16 differs at iteration %d" % it


def _run_parity(cfg, G, iters, gpw=0, threads=0, seed=7100, pseed=29):
    from hanabi_sad_amd import BatchedHanabiEnv
    dev = BatchedHanabiEnv(G, seed=seed, eps_list=EPS, device="cuda:0", games_per_workgroup=gpw, threads_per_workgroup=threads, **cfg)
    refs = [VariantEnv(seed=seed + g, eps_list=EPS, **cfg) for g in range(G)]
    P, F, A, H = dev.P, dev.F, dev.A, dev.H
    assert (F, A, dev.max_deck_size()) == (refs[0].F, refs[0].A, refs[0].deck)
    assert dev.hand_feature_size() == H * cfg["colors"] * cfg["ranks"]
    assert dev.rules() == {k: cfg[k] for k in ("colors", "ranks", "max_information_tokens", "max_life_tokens")}
    packed = cfg["knowledge_mode"] == 0
    if packed:
        dev.enable_packed((F + 63) // 64 * 64, keep_float32=True)
    r_priv, r_legal = np.zeros((G, P, F), np.float32), np.zeros((G, P, A), np.float32)
    r_own, r_eps = np.zeros((G, P, 3 * H), np.float32), np.zeros((G, P), np.float32)
    r_rew, r_term = np.zeros((G,), np.float32), np.zeros((G,), np.uint8)
    r_a, r_g = np.zeros((G, P), np.int64), np.zeros((G, P), np.int64)
    counters = np.zeros((G,), np.int64)
    n_reset = n_term = 0
    for it in range(iters):
        dev.reset()
        for g, e in enumerate(refs):
            if e.terminated():
                o = e.reset()
                n_reset += 1
                r_priv[g], r_legal[g], r_own[g], r_eps[g] = o["priv_s"], o["legal_move"], o["own_hand"], o["eps"]
        for name, d, r in (("reset priv_s", dev.priv_s, r_priv), ("reset legal_move", dev.legal_move, r_legal),
                           ("reset own_hand", dev.own_hand, r_own), ("reset eps", dev.eps, r_eps)):
            _cmp(name, d, r, it)
        a, ga = dev.policy_random(pseed)
        for g in range(G):
            r_a[g], r_g[g] = policy_random(r_legal[g], pseed, g, int(counters[g]))
            counters[g] += 1
        _cmp("policy a", a, r_a, it)
        dev.step(a, ga)
        for g, e in enumerate(refs):
            o, r, t = e.step(r_a[g], r_g[g])
            r_priv[g], r_legal[g], r_own[g], r_eps[g] = o["priv_s"], o["legal_move"], o["own_hand"], o["eps"]
            r_rew[g], r_term[g] = r, t
            n_term += int(t)
        dev.check_errors()
        for e in refs:
            e.terminated()
        for name, d, r in (("step priv_s", dev.priv_s, r_priv), ("step legal_move", dev.legal_move, r_legal),
                           ("step own_hand", dev.own_hand, r_own), ("step eps", dev.eps, r_eps),
                           ("step reward", dev.reward, r_rew), ("step terminal", dev.terminal, r_term)):
            _cmp(name, d, r, it)
        if packed:
            _cmp_packed(dev, r_priv, r_legal, r_own, it)
        _cmp("state dump", dev.export_state(), np.stack([e.export_state() for e in refs]), it)
        q = dev.query().cpu().numpy()
        assert (q[:, 2] == np.array([e.get("score") for e in refs])).all()
    assert n_reset > G and n_term > 0
    dh, cnt = dev.deck_history()
    dh, cnt = dh.cpu().numpy(), cnt.cpu().numpy()
    for g, e in enumerate(refs):
        assert cnt[g] == len(e.deck_history()) and list(dh[g, :cnt[g]]) == e.deck_history()


@pytest.mark.parametrize("v,sad,sc,km,bomb", GRID, ids=lambda x: str(x))
def test_variant_bit_parity(v, sad, sc, km, bomb):
    cfg = dict(VARIANTS[v], sad=sad, shuffle_color=sc, knowledge_mode=km, bomb=bomb, max_len=40 if bomb else 80)
    _run_parity(cfg, G=37, iters=50)


@pytest.mark.parametrize("threads", [128, 256], ids=lambda t: "t%d" % t)
@pytest.mark.parametrize("gpw", [32, 64], ids=lambda g: "gpw%d" % g)
@pytest.mark.parametrize("v", ["small", "c3r4"])
def test_variant_bit_parity_kernel_shapes(v, gpw, threads):
    cfg = dict(VARIANTS[v], sad=True, shuffle_color=True, knowledge_mode=0, bomb=0, max_len=80)
    _run_parity(cfg, G=70, iters=40, gpw=gpw, threads=threads)


@pytest.mark.parametrize("shape", [(0, 0), (64, 128)], ids=lambda s: "gpw%d_t%d" % s)
@pytest.mark.parametrize("chunk_iters", [0, 9])
@pytest.mark.parametrize("v", ["small", "p4", "r1"])
def test_variant_rollout_random_matches_restatement(v, chunk_iters, shape):
    """hsad_env_rollout_random, one launch per iteration and persistent launches (variants run the single-phase kernel), in the
    automatic kernel shape (32-game, 256-thread workgroups at this G) and in the production one (64 games, 128 threads)"""
    from hanabi_sad_amd import BatchedHanabiEnv
    cfg = dict(VARIANTS[v], sad=True, shuffle_color=True, max_len=80)
    G, iters, seed, pseed = 64 * 3 + 5, 45, 515, 3
    gpw, threads = shape
    dev = BatchedHanabiEnv(G, seed=seed, eps_list=EPS, device="cuda:0", games_per_workgroup=gpw, threads_per_workgroup=threads, **cfg)
    if gpw:
        assert (dev.games_per_workgroup, dev.threads_per_workgroup) == (gpw, threads)
    dev.set_rollout_chunk(chunk_iters)
    ref = VariantVecEnv(G, seed, eps_list=EPS, **cfg)
    for chunk in range(3):
        dev.rollout_random(iters // 3, pseed)
        ref.rollout(iters // 3, pseed)
        torch.cuda.synchronize()
        dev.check_errors()
        for name, d, r in (("priv_s", dev.priv_s, ref.priv_s), ("legal_move", dev.legal_move, ref.legal),
                           ("own_hand", dev.own_hand, ref.own_hand), ("reward", dev.reward, ref.reward),
                           ("terminal", dev.terminal, ref.terminal)):
            _cmp(name, d, r, chunk)
    for e in ref.envs:
        e.terminated()
    _cmp("state dump", dev.export_state(), np.stack([e.export_state() for e in ref.envs]), 0)


@pytest.mark.parametrize("bad", [dict(colors=6), dict(colors=0), dict(ranks=6), dict(max_information_tokens=9),
                                 dict(max_information_tokens=0), dict(max_life_tokens=4), dict(max_life_tokens=0),
                                 dict(colors=1, ranks=1, hand_size=2), dict(colors=1, ranks=2, players=5, hand_size=1)],
                         ids=lambda b: "_".join("%s%d" % kv for kv in sorted(b.items())))
def test_create_rules_refuses_what_the_game_cannot_hold(bad):
    """the library's own checks (hsad_env_create_rules), reached without any Python-side validation: rules out of bounds, and a
    deal larger than the deck (1 colour x 1 rank = 3 cards < 2 x 2; 1 x 2 = 4 cards < 5 x 1)"""
    from hanabi_sad_amd import BatchedHanabiEnv, HsadError
    kw = dict(players=2, hand_size=5)
    kw.update(bad)
    with pytest.raises(HsadError):
        BatchedHanabiEnv(4, device="cuda:0", **kw)


SMALL_PARAMS = {"players": "2", "colors": "2", "ranks": "5", "hand_size": "2", "max_information_tokens": "3",
                "max_life_tokens": "1", "seed": "4", "bomb": "0", "observation_type": "1", "random_start_player": "0"}


def test_hanalearn_ctypes_face_runs_hanabi_small():
    from hanabi_sad_amd import hanalearn
    e = hanalearn.HanabiEnv(SMALL_PARAMS, [0.0], 80, False, False, False, False)
    assert (e.feature_size(), e.num_action(), e.hand_feature_size()) == (191, 12, 20)
    assert hanalearn.HanabiEnv(SMALL_PARAMS, [0.0], 80, True, False, False, False).feature_size() == 222
    ref = VariantEnv(players=2, hand_size=2, seed=4, eps_list=[0.0], max_len=80, **SMALL)
    o, r_o = e.reset(), ref.reset()
    for n in range(30):
        for k in ("priv_s", "legal_move", "own_hand"):
            assert np.array_equal(o[k].cpu().numpy(), r_o[k]), (n, k)
        if ref.terminated():
            break
        a, ga = policy_random(r_o["legal_move"], 1, 0, n)
        o, r, t = e.step({"a": torch.tensor(a), "greedy_a": torch.tensor(ga)})
        r_o, rr, rt = ref.step(a, ga)
        assert (r, t) == (rr, rt)
    for key, val in (("colors", "6"), ("max_life_tokens", "0"), ("observation_type", "0"), ("random_start_player", "1")):
        with pytest.raises(ValueError, match=key):
            hanalearn.HanabiEnv(dict(SMALL_PARAMS, **{key: val}), [0.0], 80, False, False, False, False)


RSP_VALUES = ("0", "false", "False", "FALSE", " false", "1", "true", "True")


def test_hanalearn_compiled_face_reports_the_variant_sizes():
    build = os.path.join(ROOT, "build")
    assert glob.glob(os.path.join(build, "hanalearn*.so")), "build/hanalearn*.so missing: run __graft_entry__.build()"
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import hanalearn\nassert hanalearn.__file__.endswith('.so')\n"
            "p = %r\n"
            "e = hanalearn.HanabiEnv(p, [0.0], 80, False, False, False, False)\n"
            "print(e.feature_size(), e.num_action(), e.hand_feature_size())\n"
            "print(hanalearn.HanabiEnv(dict(p), [0.0], 80, True, False, False, False).feature_size())\n"
            "for v in %r:\n"
            "    try:\n        hanalearn.HanabiEnv(dict(p, random_start_player=v), [0.0], 80, False, False, False, False)\n"
            "        print('rsp accepted', repr(v))\n"
            "    except ValueError:\n        print('rsp refused', repr(v))\n"
            "for k, v in (('colors', '6'), ('max_information_tokens', '9'), ('observation_type', '0'), ('random_start_player', 'true')):\n"
            "    try:\n        hanalearn.HanabiEnv(dict(p, **{k: v}), [0.0], 80, False, False, False, False).feature_size()\n"
            "        print('accepted', k)\n"
            "    except ValueError as ex:\n        assert k in str(ex), ex\n"
            "print('refusals OK')\n") % (ROOT, build, SMALL_PARAMS, RSP_VALUES)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert lines[0] == "191 12 20" and lines[1] == "222" and "refusals OK" in out.stdout, out.stdout
    # random_start_player: the compiled face accepts exactly what the Python face (hanalearn.game_rules) accepts
    from hanabi_sad_amd.hanalearn import game_rules
    for v in RSP_VALUES:
        try:
            game_rules(dict(SMALL_PARAMS, random_start_player=v))
            want = "rsp accepted %r" % v
        except ValueError:
            want = "rsp refused %r" % v
        assert want in lines, (want, out.stdout)


def test_selfplay_iql_updates_and_eval_on_hanabi_small():
    from hanabi_sad_amd.eval import evaluate
    from hanabi_sad_amd.selfplay import Trainer, parse_args
    tr = Trainer(parse_args(["--num_game", "256", "--sad", "1", "--seed", "5", "--burn_in_frames", "200", "--replay_buffer_size", "4096",
                             "--batchsize", "32", "--rnn_hid_dim", "64", "--hand_size", "2", "--colors", "2",
                             "--max_information_tokens", "3", "--max_life_tokens", "1"]), "cuda:0")
    assert (tr.env.F, tr.env.A) == (222, 12)
    tr.act_step(60)
    sizes, losses = [tr.replay.size()], []
    for _ in range(6):
        tr.act_step(4)
        loss, _ = tr.learner_update()
        losses.append(float(loss.detach().float()))
        sizes.append(tr.replay.size())
    tr.join_rollout()
    torch.cuda.synchronize()
    tr.env.check_errors()
    tr.replay.check_errors()
    assert all(np.isfinite(losses)) and sizes[-1] > sizes[0] > 0
    score, perfect, scores, num_perfect = evaluate(tr.learner.online.w, 64, 31, 0, True, hand_size=2, device="cuda:0", **SMALL)
    assert all(0 <= s <= 10 for s in scores) and 0 <= score <= 10
    assert num_perfect == sum(s == 10 for s in scores) and perfect == num_perfect / 64   # perfect = every firework of the variant


class _PlayFirstCard:
    """acting agent for eval.evaluate: plays the first card whenever that is legal, else the first legal move"""

    def __init__(self, hand_size):
        self.play = hand_size   # uid of "play card 0"

    def get_h0(self, n):
        return {}

    def act(self, obs, hid):
        legal = obs["legal_move"]
        pref = legal.clone()
        pref[:, self.play] *= 2.0
        a = pref.argmax(1)
        return {"a": a, "greedy_a": a}, hid


def test_eval_counts_perfect_games_of_the_variant():
    """one colour of one rank: the three cards are all the rank-0 card, so the first play completes the only firework and the game
    ends at C * R = 1, a perfect score, which evaluate must count as perfect"""
    from hanabi_sad_amd.eval import evaluate
    rules = dict(colors=1, ranks=1, max_information_tokens=8, max_life_tokens=3)
    score, perfect, scores, num_perfect = evaluate(_PlayFirstCard(1), 16, 11, 0, False, hand_size=1, device="cuda:0", **rules)
    assert scores == [1] * 16 and score == 1.0
    assert num_perfect == 16 and perfect == 1.0
