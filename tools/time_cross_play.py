"""Developer tool: how long does a cross-play matrix take as ONE tournament batch (eval.cross_play) against the way the code base
had before -- one small env per ordered pairing, stepped in lock-step with each seat's agent acting on its own rows
(hanalearn.HanabiThreadLoop.step)?

Workload: twelve randomly initialised nets of the Other-Play zoo's shape (H = 512, three of each architecture class: default,
skip connection, two fc layers, both), 838 inputs, SAD env, 1,000 deals -> a 12 x 12 matrix = 144 pairings.  Both ways run in
the same process, alternating, `--repeat` times each after a warm-up of every shape; a host clock around work that ends in a
device synchronise.  Writes the times, their spread, the ratio and the number of games whose score differs between the two ways
(the two run hsad_r2d2_act in different row regimes: see DESIGN.md) as JSON.

    python tools/time_cross_play.py --out profiles/cross_play_timing.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_pool(K, hid, device):
    from hanabi_sad_amd.checkpoint import op_model_arch
    from hanabi_sad_amd.composite import CNet, CompositeAgent
    from hanabi_sad_amd.selfplay import init_weights
    pool = []
    for k in range(K):
        nfc, skip = op_model_arch(k * 12 // K)
        net = CNet(init_weights(838, hid, 21, 5, 100 + k, num_fc_layer=nfc), device, skip_connect=skip)
        pool.append(CompositeAgent(net, net, 1, 0.99))
    return pool


def lockstep_pair(ag0, ag1, n, seed, device):
    from hanabi_sad_amd import BatchedHanabiEnv
    env = BatchedHanabiEnv(n, players=2, seed=seed, bomb=0, eps_list=[0.0], max_len=-1, sad=True, device=device, track_deck_history=False)
    agents, hids = (ag0, ag1), [ag0.get_h0(n), ag1.get_h0(n)]
    env.reset()
    eps = torch.zeros(n, device=device)
    for _ in range(200):
        done = env.query()[:, 0] == 1
        if bool(done.all()):
            break
        cols = []
        for p, ag in enumerate(agents):
            obs = {"priv_s": env.priv_s[:, p].contiguous(), "legal_move": env.legal_move[:, p].contiguous(), "eps": eps}
            reply, hids[p] = ag.act(obs, hids[p])
            cols.append(reply["greedy_a"])
        a = torch.stack(cols, 1)
        a = torch.where(done.unsqueeze(1), torch.full_like(a, env.A - 1), a).contiguous()
        env.step(a, a)
    scores = env.query()[:, 5].cpu().numpy().astype(np.int64)
    env.close()
    return scores


def per_pair_matrix(pool, n, seed, device):
    K = len(pool)
    return np.stack([lockstep_pair(pool[i], pool[j], n, seed, device) for i in range(K) for j in range(K)]).reshape(K, K, n)


def timed(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0, out


def main():
    from hanabi_sad_amd.eval import cross_play
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=12)
    ap.add_argument("--hid", type=int, default=512)
    ap.add_argument("--deals", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join("profiles", "cross_play_timing.json"))
    args = ap.parse_args()
    pool = make_pool(args.models, args.hid, args.device)
    tour = lambda: cross_play(pool, args.deals, args.seed, 0, True, device=args.device)
    pairs = lambda: per_pair_matrix(pool, args.deals, args.seed, args.device)
    timed(tour, args.device)            # warm-up of every shape
    timed(pairs, args.device)
    t_tour, t_pair = [], []
    for _ in range(args.repeat):
        dt, xp = timed(tour, args.device)
        t_tour.append(dt)
        dt, ref = timed(pairs, args.device)
        t_pair.append(dt)
    differing = int((xp.scores != ref).sum())
    rows_per_model = 2 * args.models * args.deals
    res = {
        "workload": {"models": args.models, "hid_dim": args.hid, "deals": args.deals, "pairings": args.models ** 2, "sad": True,
                     "in_dim": 838, "device": torch.cuda.get_device_name(args.device)},
        "tournament_s": t_tour, "per_pair_s": t_pair,
        "tournament_median_s": float(np.median(t_tour)), "per_pair_median_s": float(np.median(t_pair)),
        "tournament_spread_s": float(max(t_tour) - min(t_tour)), "per_pair_spread_s": float(max(t_pair) - min(t_pair)),
        "ratio_per_pair_over_tournament": float(np.median(t_pair) / np.median(t_tour)),
        "games": int(ref.size), "games_with_differing_score": differing,
        "rows_per_act": {"tournament": rows_per_model, "per_pair": args.deals},
        "mean_score": {"tournament": float(xp.scores.mean()), "per_pair": float(ref.mean())},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
