"""GPU: the cross-play tournament (eval.play_seatings / cross_play, hsad_env_reseed, the seat kernels of csrc/hsad_eval.hip, the
eval_model command and selfplay --eval_partner).

The yardstick throughout is what the code base could do before: one small env per pairing, stepped in lock-step with each
seat's agent acting on `priv_s[:, p].contiguous()` (hanalearn.HanabiThreadLoop.step), and `eval.evaluate` for self-play.  A
row's result depends on no other row of a batch (the project's identical-bits tests), and every batch here stays under the
1,024-row switch inside hsad_r2d2_act, so the tournament must reproduce those scores game for game."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ZOO = os.path.join(GOLD, "op_zoo")
DEV = "cuda:0"
SEED, DEALS = 11, 16


def _lowest_legal(legal_move):
    """lowest legal uid of every row: a function of the observation only"""
    A = legal_move.shape[-1]
    weight = torch.arange(A, 0, -1, device=legal_move.device, dtype=torch.float32)
    return (legal_move * weight).argmax(-1).contiguous()


def _lockstep(agents_by_seat, n, seed, sad, **env_kw):
    """the per-pairing path: n games, seat p played by agents_by_seat[p] on its own rows -> scores [n]"""
    from hanabi_sad_amd import BatchedHanabiEnv
    P = len(agents_by_seat)
    env = BatchedHanabiEnv(n, players=P, seed=seed, bomb=0, eps_list=[0.0], max_len=-1, sad=sad, device=DEV, track_deck_history=False,
                           **env_kw)
    hids = [ag.get_h0(n) for ag in agents_by_seat]
    env.reset()
    eps = torch.zeros(n, device=DEV)
    for _ in range(200):
        done = env.query()[:, 0] == 1
        if bool(done.all()):
            break
        a, g = [], []
        for p, ag in enumerate(agents_by_seat):
            obs = {"priv_s": env.priv_s[:, p].contiguous(), "legal_move": env.legal_move[:, p].contiguous(), "eps": eps}
            reply, hids[p] = ag.act(obs, hids[p])
            a.append(reply["a"])
            g.append(reply["greedy_a"])
        a, g = torch.stack(a, 1), torch.stack(g, 1)
        noop = torch.full_like(a, env.A - 1)
        env.step(torch.where(done.unsqueeze(1), noop, a).contiguous(), torch.where(done.unsqueeze(1), noop, g).contiguous())
    else:
        raise AssertionError("yardstick games did not finish")
    scores = env.query()[:, 5].cpu().numpy().astype(np.int64)
    env.close()
    return scores


def _yardstick(pool, seatings, n, seed, sad, **env_kw):
    return np.stack([_lockstep([pool[k] for k in s], n, seed, sad, **env_kw) for s in seatings])


# ------------------------------------------------------------------------------------------------------------------
# 4. reseed
# ------------------------------------------------------------------------------------------------------------------
def _advance(env):
    env.reset()                     # (re)starts the games that ended, as the actor loop does
    a = _lowest_legal(env.legal_move)
    env.step(a, a)


def _snapshot(env, lo, hi):
    return [env.export_state()[lo:hi], env.priv_s[lo:hi], env.reward[lo:hi], env.terminal[lo:hi]]


@pytest.mark.parametrize("gpw", [32, 64])
def test_reseed_repeats_deals_with_a_period_and_reseeds_in_place(gpw):
    from hanabi_sad_amd import BatchedHanabiEnv
    s = 77
    kw = dict(players=2, bomb=0, eps_list=[0.0, 0.1, 0.2, 0.4], max_len=80, sad=True, shuffle_color=True, device=DEV,
              games_per_workgroup=gpw)
    env = BatchedHanabiEnv(120, seed=5, **kw)
    assert env.games_per_workgroup == gpw
    env.rollout_random(3, 9)        # the object has history: reseed must wipe it
    fresh = BatchedHanabiEnv(40, seed=s, **kw)
    env.reseed(s, period=40)
    restarted = 0
    for step in range(30):
        _advance(env)
        _advance(fresh)
        want = _snapshot(fresh, 0, 40)
        for grp in range(3):        # the groups straddle the 32- and 64-game workgroup boundaries
            got = _snapshot(env, 40 * grp, 40 * grp + 40)
            for name, x, y in zip(("state", "priv_s", "reward", "terminal"), got, want):
                assert torch.equal(x, y), (step, grp, name)
        assert torch.equal(env.eps[:40], env.eps[40:80]) and torch.equal(env.eps[:40], fresh.eps)
        restarted += int(fresh.terminal.sum())
    assert restarted > 0            # games ended and were dealt again from the continuing generators
    env.check_errors()
    # the same object, next chunk of deals without a wrap == a new object with that seed
    fresh120 = BatchedHanabiEnv(120, seed=s + 40, **kw)
    env.reseed(s + 40, 0)
    for step in range(12):
        _advance(env)
        _advance(fresh120)
        for name, x, y in zip(("state", "priv_s", "reward", "terminal"), _snapshot(env, 0, 120), _snapshot(fresh120, 0, 120)):
            assert torch.equal(x, y), (step, name)
    assert not torch.equal(env.export_state()[:40], env.export_state()[40:80])
    env.check_errors()


# ------------------------------------------------------------------------------------------------------------------
# 5. seat kernels against torch indexing
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_env():
    """128 two-player SAD games (256 rows) somewhere in the middle of play, some of them finished, with all three observation forms"""
    from hanabi_sad_amd import BatchedHanabiEnv
    env = BatchedHanabiEnv(128, players=2, seed=3, bomb=0, eps_list=[0.0], max_len=-1, sad=True, device=DEV, track_deck_history=False)
    env.enable_packed(bf16_row_len=896, keep_float32=True)
    env.reset()
    for it in range(200):
        done = env.query()[:, 0] == 1
        if int(done.sum()) >= 8:
            break
        a, g = env.policy_random(1234)
        noop = torch.full_like(a, env.A - 1)
        env.step(torch.where(done.unsqueeze(1), noop, a).contiguous(), torch.where(done.unsqueeze(1), noop, g).contiguous())
    done = env.query()[:, 0] == 1
    assert 8 <= int(done.sum()) <= 120, "the fixture needs finished and running games side by side"
    return env, done


@pytest.mark.parametrize("n", [1, 63, 64, 200])
def test_seat_gather_and_scatter_against_indexing(mixed_env, n):
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.r2d2 import cast_pad_bf16
    env, done = mixed_env
    lib, st = env.lib, env._stream()
    N, F, A, Kp = env.G * env.P, env.F, env.A, 896
    gen = torch.Generator().manual_seed(100 + n)
    rows = torch.randperm(N, generator=gen)[:n].to(torch.int32).to(DEV)
    if n > 1:
        assert bool((rows % 2 == 0).any()) and bool((rows % 2 == 1).any())        # both seats
    idx = rows.long()
    src16, src32, legal = env.priv_s_bf16.view(N, Kp), env.priv_s.view(N, F), env.legal_move.view(N, A)
    assert float(src32.sum()) > 0

    def gather(kind, src, dtype, width):
        out = torch.full((n, width), 7, dtype=dtype, device=DEV)
        lg = torch.full((n, A), 7.0, device=DEV)
        _lib.check(lib.hsad_seat_gather(rows.data_ptr(), n, N, kind, src.data_ptr(), F, Kp, legal.data_ptr(), A, out.data_ptr(),
                                        lg.data_ptr(), st))
        assert torch.equal(lg.view(torch.int32), legal[idx].view(torch.int32))
        return out
    got = gather(0, src16, torch.bfloat16, Kp)
    assert torch.equal(got.view(torch.int16), src16[idx].view(torch.int16))
    got = gather(1, src32, torch.bfloat16, Kp)
    assert torch.equal(got.view(torch.int16), cast_pad_bf16(src32[idx].contiguous(), Kp).view(torch.int16))
    assert torch.equal(got.view(torch.int16), src16[idx].view(torch.int16))       # and the env's own bf16 rows are that cast
    got = gather(2, src32, torch.float32, F)
    assert torch.equal(got.view(torch.int32), src32[idx].view(torch.int32))

    a = torch.full((env.G, env.P), -7, dtype=torch.int64, device=DEV)
    g = torch.full((env.G, env.P), -9, dtype=torch.int64, device=DEV)
    a_src = torch.arange(n, dtype=torch.int64, device=DEV) % (A - 1)
    g_src = (a_src + 1) % (A - 1)
    _lib.check(lib.hsad_seat_scatter(env.h, rows.data_ptr(), n, a_src.data_ptr(), g_src.data_ptr(), a.data_ptr(), g.data_ptr(), st))
    want_a, want_g = torch.full((N,), -7, dtype=torch.int64, device=DEV), torch.full((N,), -9, dtype=torch.int64, device=DEV)
    fin = done[idx // env.P]
    want_a[idx] = torch.where(fin, torch.full_like(a_src, A - 1), a_src)
    want_g[idx] = torch.where(fin, torch.full_like(g_src, A - 1), g_src)
    assert torch.equal(a.view(N), want_a) and torch.equal(g.view(N), want_g)      # listed rows only; noop where the game is over


def test_seating_stats_against_query(mixed_env):
    from hanabi_sad_amd import _lib
    env, done = mixed_env
    for per in (128, 32, 1):
        S = env.G // per
        stats = torch.full((S, 4), -1, dtype=torch.int64, device=DEV)
        open_ = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        _lib.check(env.lib.hsad_seating_stats(env.h, per, stats.data_ptr(), open_.data_ptr(), env._stream()))
        q = env.query().cpu().numpy().astype(np.int64)
        fin, sc = (q[:, 0] == 1) & (q[:, 14] == 1), q[:, 5]
        want = np.stack([(sc * fin).reshape(S, per).sum(1), (sc * sc * fin).reshape(S, per).sum(1),
                         ((sc == 25) & fin).reshape(S, per).sum(1), fin.reshape(S, per).sum(1)], 1)
        assert np.array_equal(stats.cpu().numpy(), want)
        assert int(open_.cpu()[0]) == int((~fin).sum())
    with pytest.raises(_lib.HsadError):          # 128 games are no whole number of 48-game seatings
        _lib.check(env.lib.hsad_seating_stats(env.h, 48, stats.data_ptr(), open_.data_ptr(), env._stream()))


# ------------------------------------------------------------------------------------------------------------------
# 6 / 7 / 10. the tournament equals the per-pair path
# ------------------------------------------------------------------------------------------------------------------
def _zoo(precision):
    from hanabi_sad_amd.checkpoint import load_op_model
    return [load_op_model("sad", idx, None, DEV, root=ZOO, precision=precision)[0] for idx in (0, 3, 6, 9)]


PAIRS4 = [(i, j) for i in range(4) for j in range(4)]


@pytest.fixture(scope="module")
def zoo_bf16():
    """pool, its per-pair yardstick [16, DEALS] and the tournament's result over the same deals"""
    from hanabi_sad_amd.eval import play_seatings
    pool = _zoo("bf16")
    want = _yardstick(pool, PAIRS4, DEALS, SEED, False)
    res = play_seatings(pool, PAIRS4, DEALS, SEED, 0, False, device=DEV)
    return pool, want, res


def test_tournament_scores_equal_the_per_pair_runs(zoo_bf16):
    from hanabi_sad_amd.eval import evaluate
    pool, want, res = zoo_bf16
    # the yardstick alone is no vacuous one: pairings differ and points are scored
    assert want.max() > 0 and any(not np.array_equal(want[0], w) for w in want[1:])
    assert res.scores.shape == (16, DEALS) and res.scores.dtype == np.int64
    differing = [(s, d, int(res.scores[s, d]), int(want[s, d])) for s in range(16) for d in range(DEALS) if res.scores[s, d] != want[s, d]]
    assert not differing, "(seating, deal, tournament, per-pair): %s" % differing
    for i in range(4):              # the diagonal is self-play over the deals evaluate() plays
        assert res.scores[i * 4 + i].tolist() == evaluate(pool[i], DEALS, SEED, 0, False, device=DEV)[2], i


def test_tournament_fp32_equals_the_per_pair_runs():
    from hanabi_sad_amd.checkpoint import load_op_model
    from hanabi_sad_amd.eval import play_seatings
    pool = [load_op_model("sad", idx, None, DEV, root=ZOO, precision="fp32")[0] for idx in (0, 9)]
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    want = _yardstick(pool, pairs, DEALS, SEED, False)
    res = play_seatings(pool, pairs, DEALS, SEED, 0, False, precision="fp32", device=DEV)
    assert want.max() > 0
    assert np.array_equal(res.scores, want)


def test_chunked_run_gives_the_same_scores(zoo_bf16):
    from hanabi_sad_amd.eval import play_seatings
    pool, want, res = zoo_bf16
    chunked = play_seatings(pool, PAIRS4, DEALS, SEED, 0, False, device=DEV, games_per_launch=16 * 7)      # 7 + 7 + 2 deals
    assert np.array_equal(chunked.scores, res.scores)
    assert np.array_equal(chunked.totals, res.totals)


def test_statistics_are_numpy_on_the_scores(zoo_bf16):
    from hanabi_sad_amd.eval import cross_play
    pool, want, res = zoo_bf16
    sc = res.scores
    assert np.array_equal(res.totals, np.stack([sc.sum(1), (sc * sc).sum(1), (sc == 25).sum(1), np.full(16, DEALS)], 1))
    assert np.abs(res.mean - sc.mean(1)).max() <= 1e-9
    assert np.abs(res.sem - np.std(sc, axis=1) / np.sqrt(DEALS)).max() <= 1e-9
    assert np.array_equal(res.perfect, (sc == 25).mean(1))
    xp = cross_play(pool, DEALS, SEED, 0, False, device=DEV)
    assert np.array_equal(xp.scores, sc.reshape(4, 4, DEALS))
    assert xp.mean.shape == (4, 4) and np.abs(xp.mean - sc.mean(1).reshape(4, 4)).max() <= 1e-9
    assert np.abs(xp.sem - (np.std(sc, axis=1) / np.sqrt(DEALS)).reshape(4, 4)).max() <= 1e-9
    assert np.abs(xp.row_mean - sc.mean(1).reshape(4, 4).mean(1)).max() <= 1e-9
    assert np.array_equal(xp.perfect, (sc == 25).mean(1).reshape(4, 4))


# ------------------------------------------------------------------------------------------------------------------
# 8. three players      9. mixed families
# ------------------------------------------------------------------------------------------------------------------
def test_three_player_seatings_equal_the_per_seat_runs():
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.eval import env_dims, play_seatings
    from hanabi_sad_amd.selfplay import init_weights
    F, A = env_dims(3, 5, False)
    pool = []
    for seed in (1, 2):
        net = CNet(init_weights(F, 64, A, 5, seed), DEV)
        pool.append(CompositeAgent(net, net, 1, 0.99))
    seatings = [(0, 0, 1), (1, 0, 0), (0, 1, 0), (1, 1, 1)]
    want = _yardstick(pool, seatings, 8, SEED, False)
    res = play_seatings(pool, seatings, 8, SEED, 0, False, device=DEV)
    assert want.max() > 0
    assert np.array_equal(res.scores, want)


def test_mixed_model_families_share_a_tournament():
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.eval import play_seatings
    from hanabi_sad_amd.obl import OBLAgent, OBLNetKernels
    from hanabi_sad_amd.selfplay import init_weights
    z = np.load(os.path.join(GOLD, "obl_small.npz"))
    obl = OBLAgent(OBLNetKernels({k[2:]: torch.tensor(z[k]) for k in z.files if k.startswith("w.")}, DEV, "bf16"))
    net = CNet(init_weights(838, 64, 21, 5, 4), DEV)
    pool = [obl, CompositeAgent(net, net, 1, 0.99)]
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    want = _yardstick(pool, pairs, 8, SEED, True)        # the OBL agent reads the float32 SAD observation
    res = play_seatings(pool, pairs, 8, SEED, 0, True, device=DEV)
    assert want.max() > 0
    assert np.array_equal(res.scores, want)


# ------------------------------------------------------------------------------------------------------------------
# 11. the command      12. selfplay --eval_partner
# ------------------------------------------------------------------------------------------------------------------
def _run_eval_model(*flags):
    cmd = [sys.executable, "-m", "hanabi_sad_amd.eval_model", "--paper", "op", "--method", "sad", "--root", os.path.join("tests", "golden", "op_zoo"),
           "--num_game", "8", "--device", DEV] + list(flags)
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)     # a fresh child process
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_eval_model_command_prints_the_matrix_and_the_one_line_form():
    from hanabi_sad_amd.eval import cross_play, parse_cross_play_table
    xp = cross_play(_zoo("bf16"), 8, 1, 0, False, device=DEV)
    text = _run_eval_model("--idx", "0", "3", "6", "9", "--cross_play")
    table = text[text.index("self-play & cross-play of SAD"):]
    title, names, mean, row_mean = parse_cross_play_table(table)
    assert names == ["M0", "M3", "M6", "M9"]
    want = np.array([[float("%.2f" % v) for v in r] for r in xp.mean])
    assert np.array_equal(mean, want)
    assert np.array_equal(row_mean, np.array([float("%.2f" % v) for v in xp.row_mean]))
    lines = table.splitlines()
    assert lines[1] == "-" * len(lines[2]) and lines[2].split() == ["name", "M0", "M3", "M6", "M9", "mean"]
    line = [l for l in _run_eval_model("--idx1", "0", "--idx2", "3").splitlines() if l.startswith("score:")]
    assert line == ["score: %f +/- %f ; perfect:  %s" % (xp.mean[0, 1], xp.sem[0, 1], xp.perfect[0, 1])]


def test_selfplay_logs_cross_play_with_fixed_partners(tmp_path):
    from hanabi_sad_amd import selfplay
    from hanabi_sad_amd.checkpoint import agent_from_file, load_weights
    from hanabi_sad_amd.eval import play_seatings
    save_dir, partner = str(tmp_path / "xp"), os.path.join(GOLD, "ref_small.pthw")
    argv = ["--save_dir", save_dir, "--num_game", "64", "--rnn_hid_dim", "64", "--batchsize", "16", "--replay_buffer_size", "2048",
            "--burn_in_frames", "64", "--max_len", "40", "--num_epoch", "2", "--epoch_len", "5", "--num_eval_game", "48",
            "--load_model", partner, "--seed", "7", "--eval_partner", partner]
    old = sys.stdout
    try:
        selfplay.main(argv)
    finally:
        sys.stdout = old
    log = open(os.path.join(save_dir, "train.log")).read()
    found = re.findall(r"^xplay: mean ([0-9.]+) \(as seat 0: ([0-9.]+), as seat 1: ([0-9.]+)\)$", log, flags=re.M)
    assert len(found) == 2                                            # one line per epoch
    # the top-k saver writes every epoch's weights to slot 0 while its list fills: model0.pthw is epoch 1's online net
    w = load_weights(os.path.join(save_dir, "model0.pthw"))
    seed = (9917 + 1 * 999999) % 7777777
    res = play_seatings([w, agent_from_file(partner, DEV)], [[0, 1], [1, 0]], 48, seed, 0, True, device=DEV)
    mean, s0, s1 = (float(v) for v in found[1])
    assert abs(mean - res.mean.mean()) <= 5.1e-5 and abs(s0 - res.mean[0]) <= 5.1e-5 and abs(s1 - res.mean[1]) <= 5.1e-5
