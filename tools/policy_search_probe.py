"""Records for DESIGN §3g, blueprint-policy search: seconds per search.policy_action_values call on one root batch of the full
2-player game, jobs/s, env-steps/s of the search loop, the mean fraction of games still live per iteration (the case for or against
compacting finished games out of the act batch), the three glue kernels' times, and the same call of mc_action_values (random
playouts) as the yardstick.  --replay adds the replay stage (PolicySearch(replay=True)): its seconds alone at several move
depths -- the cost grows with the move number -- and the whole search with it.  Host clock around a device synchronise, median of
the repeats.  --sampler chooses how the worlds' hands are drawn in every search timed here (rejection: hsad_env_determinize;
stratified: hsad_env_determinize_exact); the determinise call of both samplers and hsad_env_hand_belief are also timed alone on the
search env.  --rounds a,b,c (summing to --worlds) adds the search in rounds on the same root in the same process: the jobs it
played per round against pairs x worlds, its seconds per search next to the flat search's, and the time of one hsad_search_round
call on the search's own score table.  One JSON line.

    python tools/policy_search_probe.py [--roots 64] [--worlds 8] [--capacity 4096] [--hid 512] [--repeats 5] [--replay]
                                        [--sampler rejection|stratified] [--rounds 2,2,4] [--prune_z 2.0]
"""
import argparse
import json
from fractions import Fraction
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hanabi_sad_amd import BatchedHanabiEnv, _lib  # noqa: E402
from hanabi_sad_amd.search import GameLog, PolicySearch, mc_action_values, search_jobs, world_seed  # noqa: E402


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=64)
    ap.add_argument("--worlds", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--hid", type=int, default=512)
    ap.add_argument("--moves", type=int, default=10, help="lock-step greedy moves before the root position")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sad", type=int, default=1)
    ap.add_argument("--replay", action="store_true", help="also time the replay stage per move depth and the search with replay")
    ap.add_argument("--sampler", choices=["rejection", "stratified"], default="rejection")
    ap.add_argument("--rounds", type=lambda s: tuple(int(x) for x in s.split(",")), default=None,
                    help="world counts per round (sum = --worlds): also time the search in rounds against the flat search")
    ap.add_argument("--prune_z", type=float, default=2.0)
    args = ap.parse_args()
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.eval import env_dims
    from hanabi_sad_amd.selfplay import init_weights
    dev, G, P = "cuda:0", args.roots, 2
    F, A = env_dims(P, 5, bool(args.sad))
    net = CNet(init_weights(F, args.hid, A, 5, 1), dev)          # a random net of the zoo's shape: timing does not ask for a trained one
    agent = CompositeAgent(net, net, 1, 0.99)
    root = BatchedHanabiEnv(G, players=P, seed=1, bomb=0, eps_list=[0.0], max_len=-1, sad=bool(args.sad), device=dev, track_deck_history=bool(args.replay))
    root.reset()
    hid = agent.get_h0(G * P)
    log = GameLog(G, P, dev)
    depths = sorted({d for d in (args.moves // 4, args.moves // 2, args.moves) if d >= 1}) if args.replay else []
    snaps = {}
    for move in range(args.moves):
        obs = {"priv_s": root.priv_s.view(G * P, F), "legal_move": root.legal_move.view(G * P, A), "eps": root.eps.view(G * P)}
        reply, hid = agent.act(obs, hid)
        log.append(reply["a"], reply["greedy_a"])
        root.step(reply["a"].view(G, P).contiguous(), reply["greedy_a"].view(G, P).contiguous())
        if move + 1 in depths:
            snaps[move + 1] = BatchedHanabiEnv(G, players=P, seed=1, bomb=0, eps_list=[0.0], max_len=-1, sad=bool(args.sad), device=dev,
                                               track_deck_history=True)
            snaps[move + 1].fork_from(root, torch.arange(G, dtype=torch.int32))
        log.observed(root)
    hid = {"h0": hid["h0"], "c0": hid["c0"]}
    ps = PolicySearch(root, agent, args.capacity, sampler=args.sampler)
    res = {"roots": G, "worlds": args.worlds, "capacity": args.capacity, "hid": args.hid, "sad": args.sad, "repeats": args.repeats,
           "sampler": args.sampler}
    sv = ps.search(root, hid, args.worlds, 0)                       # warm-up (first launch of each kernel)
    jobs = int(sv.totals[..., 2].sum())
    res["jobs"] = jobs
    ms, steps, live, live_steps = [], [], [], []
    for r in range(args.repeats):
        ms += timed(lambda: ps.search(root, hid, args.worlds, 1 + r), 1)
        steps.append(ps.iterations * args.capacity)                 # every slot is stepped every iteration, finished or not
        live.append(sum(ps.open_games) / max(1, len(ps.open_games)) / args.capacity)
        live_steps.append(sum(ps.open_games))                       # games still running after each step: the steps that moved a game
    res["search_ms"], res["loop_iterations"] = ms, ps.iterations
    res["jobs_per_s"] = [jobs / m * 1e3 for m in ms]
    res["slot_steps_per_s"] = [s / m * 1e3 for s, m in zip(steps, ms)]
    res["live_env_steps_per_s"] = [s / m * 1e3 for s, m in zip(live_steps, ms)]
    res["live_fraction_per_iteration"] = live
    if args.rounds is not None:
        rkw = dict(rounds=args.rounds, prune_z=args.prune_z)
        sv = ps.search(root, hid, args.worlds, 0, **rkw)            # warm-up
        rms, rjobs = [], []
        for r in range(args.repeats):                               # the seeds of the flat searches timed above
            rms += timed(lambda: ps.search(root, hid, args.worlds, 1 + r, **rkw), 1)
            rjobs.append(list(ps.round_jobs))
        res["rounds"], res["prune_z"], res["rounds_flat_jobs"] = list(args.rounds), args.prune_z, jobs
        res["rounds_jobs"], res["rounds_jobs_total"] = rjobs, [sum(j) for j in rjobs]
        res["rounds_search_ms"], res["rounds_search_ms_median"] = rms, statistics.median(rms)
        # one hsad_search_round call on the last search's table: every (game, action) a pair, illegal actions all-absent rows
        A_ = root.A
        table = sv.world_scores.reshape(G * A_, args.worlds).contiguous()
        first = (torch.arange(G + 1, device=dev) * A_).to(torch.int32)
        bp_pair = (torch.arange(G, device=dev) * A_ + sv.blueprint_a.clamp(min=0)).to(torch.int32)
        alive = torch.ones(G * A_, dtype=torch.uint8, device=dev)
        leader = torch.zeros(G, dtype=torch.int32, device=dev)
        raw = torch.zeros(G * A_, 2, dtype=torch.int64, device=dev)
        pr, pb = torch.zeros(G * A_, 3, dtype=torch.int64, device=dev), torch.zeros(G * A_, 3, dtype=torch.int64, device=dev)
        z2 = Fraction(args.prune_z * args.prune_z).limit_denominator(1024)
        call = lambda: _lib.check(ps.lib.hsad_search_round(table.data_ptr(), G * A_, args.worlds, first.data_ptr(), G, bp_pair.data_ptr(),
                                                           z2.numerator, z2.denominator, 2, alive.data_ptr(), leader.data_ptr(), raw.data_ptr(),
                                                           pr.data_ptr(), pb.data_ptr(), ps.env._stream()))
        call()
        res["round_kernel_ms"] = timed(call, args.repeats)
        res["round_kernel_ms_median"] = statistics.median(res["round_kernel_ms"])
    res["mc_action_values_ms"] = timed(lambda: mc_action_values(root, args.worlds, 3, capacity=args.capacity, sampler=args.sampler), args.repeats)
    # the three glue kernels alone, on the search env as the last chunk left it
    env, lib, st = ps.env, ps.lib, ps.env._stream()
    cap = args.capacity
    src = torch.randint(0, G, (cap,), device=dev).to(torch.int32)
    L, H = ps.h.shape[0], ps.h.shape[2]
    h16 = ps.h16.data_ptr() if ps.h16 is not None else None
    a = torch.zeros(cap * P, dtype=torch.int64, device=dev)
    player = torch.zeros(cap, dtype=torch.int32, device=dev)
    override = torch.zeros(cap, dtype=torch.int64, device=dev)
    job = (torch.arange(cap, device=dev) // args.worlds).to(torch.int32)
    n_job = int(job.max()) + 1
    stats = torch.zeros(n_job, 3, dtype=torch.int64, device=dev)
    calls = {
        "fork_state_ms": lambda: _lib.check(lib.hsad_search_fork_state(src.data_ptr(), cap, G, P, L, H, hid["h0"].data_ptr(), hid["c0"].data_ptr(),
                                                                       ps.h.data_ptr(), ps.c.data_ptr(), h16, st)),
        "actions_ms": lambda: _lib.check(lib.hsad_search_actions(env.h, a.data_ptr(), a.data_ptr(), player.data_ptr(), override.data_ptr(),
                                                                 env.a.data_ptr(), env.greedy_a.data_ptr(), st)),
        "job_stats_ms": lambda: _lib.check(lib.hsad_search_job_stats(env.h, job.data_ptr(), n_job, stats.data_ptr(), st)),
    }
    for name, fn in calls.items():
        fn()
        res[name] = timed(fn, args.repeats)
    # the determinise call of both samplers and the belief kernel, on forks of the root in the search env (every slot a world)
    q = root.query()
    cur = torch.where(q[:, 0] == 0, q[:, 1], torch.full_like(q[:, 1], -1)).to(torch.int32)
    viewer = cur[src.to(torch.int64)].contiguous()
    wkey = torch.arange(cap, device=dev, dtype=torch.int64)
    stratum = (torch.arange(cap, device=dev) % args.worlds).to(torch.int32)
    det = {"determinize_observe_ms": lambda: env.determinize(viewer, wkey, 7),
           "determinize_exact_observe_ms": lambda: env.determinize_exact(viewer, wkey, 7, stratum=stratum, n_strata=args.worlds),
           "hand_belief_ms": lambda: env.hand_belief(viewer)}
    for name, fn in det.items():
        ms = []
        for r in range(args.repeats + 1):
            env.fork_from(root, src)
            ms += timed(fn, 1)
        res[name] = ms[1:]                                          # the first call is the warm-up
        res[name + "_median"] = statistics.median(res[name])
    res["chosen_determinize_ms_median"] = res["determinize_exact_observe_ms_median" if args.sampler == "stratified" else "determinize_observe_ms_median"]
    for k in ("search_ms", "jobs_per_s", "slot_steps_per_s", "live_env_steps_per_s", "live_fraction_per_iteration", "mc_action_values_ms", "fork_state_ms", "actions_ms",
              "job_stats_ms"):
        res[k + "_median"] = statistics.median(res[k])
    ps.close()
    if args.replay:
        rp = PolicySearch(root, agent, args.capacity, replay=True, sampler=args.sampler)
        rp.search(root, hid, args.worlds, 0, log=log)               # warm-up: builds the world envs
        res["search_replay_ms"] = timed(lambda: rp.search(root, hid, args.worlds, 1, log=log), args.repeats)
        res["search_replay_ms_median"] = statistics.median(res["search_replay_ms"])
        # the replay stage alone at several move depths: forks of the root taken on the way, each with the log up to there
        res["replay_ms_by_depth"], res["replay_ms_per_move"] = {}, {}
        for depth, snap in sorted(snaps.items()):
            part = GameLog(G, P, dev)
            for t in range(depth):
                part.append(log.a[t], log.greedy_a[t])
                part._s[t].copy_(log.sad[t])
            pairs, cur = search_jobs(snap)
            games = np.unique(pairs[:, 0])
            seed_of = np.zeros((G, args.worlds), dtype=np.int32)
            for g in games:
                seed_of[g] = [world_seed(1, int(g), w) for w in range(args.worlds)]
            ms = timed(lambda: rp._replay(snap, part, games, cur, args.worlds, 1, seed_of), args.repeats)
            res["replay_ms_by_depth"][str(depth)] = statistics.median(ms)
            res["replay_ms_per_move"][str(depth)] = statistics.median(ms) / depth
            snap.close()
        rp.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
