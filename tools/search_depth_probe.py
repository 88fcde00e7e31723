"""Depth-limited search, measured (profiles/search_depth_probe.json), all in one process and on one root batch per net: 64 two-player
games (sad = 1) three blueprint moves into the game, 8 worlds per legal action, capacity 4,096.  Per depth in None, 0, 1, 2, 4, 8:
  - the time of one searched move (PolicySearch.search, the search env kept across calls, the same seed every time so that every
    repeat plays the same worlds): a host clock around a call that ends in a device synchronise, the depths interleaved repeat by
    repeat, the median with the spread.  depth=None is the full playout -- the code path the search has always had -- in the same run;
  - the act calls issued (PolicySearch.acts), the env steps and the share of worlds cut at the horizon;
  - with keep_world_values, the mean and the RMS of (bootstrapped value - full-playout score) per world OF THE SAME WORLD: a world's
    hands depend on (seed, game, world) only and both searches run in the same acting regime, so the two play the same game up to the
    horizon.  Worlds that end within the depth differ by 0 and are part of the average; `cut_share` says how many did not.
Two nets: a random 512-unit net (times only: its Q calibrates nothing, and its games are short) and a clone of the rule bot `piers`
fitted in this script with `clone --teacher piers --value_weight 1` (times and calibration: its games have the usual length and its
Q was fitted to the returns of recorded games).  Single runs; nothing here says whether a bounded search plays as well as the full
one.  One JSON line (and --out FILE).  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hanabi_sad_amd import BatchedHanabiEnv                  # noqa: E402
from hanabi_sad_amd.composite import CNet, CompositeAgent    # noqa: E402
from hanabi_sad_amd.search import PolicySearch               # noqa: E402
from hanabi_sad_amd.selfplay import init_weights             # noqa: E402

DEPTHS = (None, 0, 1, 2, 4, 8)
NOT_PLAYED = 0xFFFF


def make_root(agent, games, moves, dev):
    root = BatchedHanabiEnv(games, players=2, seed=17, bomb=0, eps_list=[0.0], max_len=-1, sad=True, device=dev, track_deck_history=False)
    root.reset()
    N = games * root.P
    hid = agent.get_h0(N)
    for _ in range(moves):
        obs = {"priv_s": root.priv_s.view(N, root.F), "legal_move": root.legal_move.view(N, root.A), "eps": torch.zeros(N, device=dev)}
        reply, hid = agent.act(obs, hid)
        root.step(reply["a"].view(games, root.P).contiguous(), reply["greedy_a"].view(games, root.P).contiguous())
    return root, {"h0": hid["h0"].contiguous(), "c0": hid["c0"].contiguous()}


def name_of(depth):
    return "none" if depth is None else str(depth)


def probe(agent, args, dev, calibrate):
    root, hid = make_root(agent, args.root_games, args.root_moves, dev)
    live = int((root.query()[:, 0] == 0).sum())
    searches = {d: PolicySearch(root, agent, args.capacity, depth=d, horizon_value="mover") for d in DEPTHS}
    info, ms = {}, {d: [] for d in DEPTHS}
    for rep in range(args.repeats + 1):                # repeat 0 warms up and is not kept
        for d, ps in searches.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sv = ps.search(root, hid, args.worlds, args.seed)
            torch.cuda.synchronize()
            if rep:
                ms[d].append((time.perf_counter() - t0) * 1e3)
            jobs = int(sv.totals[..., 2].sum())
            info[d] = dict(jobs=jobs, chunks=-(-jobs // args.capacity), act_calls=ps.acts, env_steps=ps.iterations,
                           cut_share=None if d is None else float(sv.cut.sum()) / max(jobs, 1), nonfinite=sv.nonfinite)
    out = {"root_games": args.root_games, "live_root_games": live, "root_moves": args.root_moves}
    full_ms = statistics.median(ms[None])
    for d in DEPTHS:
        out[name_of(d)] = dict(info[d], ms_median=statistics.median(ms[d]), ms_min=min(ms[d]), ms_max=max(ms[d]),
                               speedup_over_full=full_ms / statistics.median(ms[d]))
    if calibrate:
        full = searches[None].search(root, hid, args.worlds, args.seed, keep_world_values=True).world_values.cpu().numpy().astype(np.int64)
        for hv in ("mover", "team"):
            for d in DEPTHS[1:]:
                ps = searches[d]
                ps.horizon_value = hv
                sv = ps.search(root, hid, args.worlds, args.seed, keep_world_values=True)
                wv = sv.world_values.cpu().numpy().astype(np.int64)
                both = (wv != NOT_PLAYED) & (full != NOT_PLAYED)
                diff = wv[both] / 256.0 - full[both]
                out[name_of(d)]["calibration_" + hv] = dict(worlds=int(both.sum()), cut_share=float(sv.cut.sum()) / max(int(both.sum()), 1),
                                                            mean_diff=float(diff.mean()), rms_diff=float(np.sqrt((diff * diff).mean())),
                                                            mean_full_score=float(full[both].mean()), mean_value=float((wv[both] / 256.0).mean()))
                ps.horizon_value = "mover"
    for ps in searches.values():
        ps.close()
    root.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_games", type=int, default=64)
    ap.add_argument("--root_moves", type=int, default=3)
    ap.add_argument("--worlds", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--clone_games", type=int, default=2000)
    ap.add_argument("--clone_epochs", type=int, default=12)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "worlds": args.worlds, "capacity": args.capacity, "repeats": args.repeats, "hidden": 512,
           "depths": [name_of(d) for d in DEPTHS],
           "note": "ms per PolicySearch.search call (host loop and the final synchronise included), depths interleaved repeat by repeat; "
                   "'none' is the full playout in the same run; calibration: bootstrapped value - full-playout score of the same world, "
                   "in points, over all worlds (those that ended within the depth differ by 0); single runs, no claim about playing "
                   "strength"}
    probe_root = BatchedHanabiEnv(1, players=2, seed=0, bomb=0, eps_list=[0.0], max_len=-1, sad=True, device=dev, track_deck_history=False)
    F, A = probe_root.F, probe_root.A
    probe_root.close()
    net = CNet(init_weights(F, 512, A, 5, 1), dev)
    out["random_net"] = probe(CompositeAgent(net, net, 1, 0.99), args, dev, calibrate=False)
    # the calibrated net: a clone of `piers` whose Q was fitted to the recorded returns
    from hanabi_sad_amd import clone
    from hanabi_sad_amd.checkpoint import load_weights
    tmp = tempfile.mkdtemp()
    clone.main(["--teacher", "piers", "--value_weight", "1", "--num_game", str(args.clone_games), "--num_epoch", str(args.clone_epochs),
                "--lr", "5e-4", "--sad", "1", "--save_dir", tmp, "--num_eval_game", "200", "--train_device", dev])
    net = CNet(load_weights(os.path.join(tmp, "clone.pthw")), dev)
    out["clone_of_piers"] = dict(probe(CompositeAgent(net, net, 1, 0.99), args, dev, calibrate=True),
                                 clone=dict(teacher="piers", value_weight=1.0, games=args.clone_games, epochs=args.clone_epochs))
    line = json.dumps(out, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
