"""Times of snapshot, restore and import_state for a batch of games, with hsad_env_fork on the same games as the yardstick (each of
them ends in the same observe pass).  One JSON line; no figure is claimed anywhere.

    python tools/position_probe.py [--games 65536] [--repeats 5] [--sad 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hanabi_sad_amd import BatchedHanabiEnv  # noqa: E402


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
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sad", type=int, default=1)
    args = ap.parse_args()
    G, dev = args.games, "cuda:0"
    kw = dict(players=2, hand_size=5, sad=bool(args.sad), eps_list=(0.0,), device=dev)
    src = BatchedHanabiEnv(G, seed=1, **kw)
    dst = BatchedHanabiEnv(G, seed=2, **kw)
    src.reset()
    src.rollout_random(12, 3)
    dst.reset()
    idx = torch.arange(G, device=dev, dtype=torch.int32)
    seeds = torch.arange(G, device=dev, dtype=torch.int32)
    res = {"games": G, "sad": args.sad, "repeats": args.repeats, "record_bytes": src.snapshot_record_bytes()}
    snap = src.snapshot()
    states = src.export_state()
    live = (src.terminal == 0).nonzero().view(-1)
    dst.fork_from(src, idx)            # warm-up: the first launch of each kernel
    dst.restore(snap)
    dst.import_state(states[live], live, seeds=seeds[live])
    dst.check_errors()
    res["fork_observe_ms"] = timed(lambda: dst.fork_from(src, idx), args.repeats)
    res["snapshot_ms"] = timed(lambda: src.snapshot(), args.repeats)
    res["restore_observe_ms"] = timed(lambda: dst.restore(snap), args.repeats)
    # (the wrapper's scatter into the [G, words] / take form is part of what a caller pays)
    res["import_observe_ms"] = timed(lambda: dst.import_state(states[live], live, seeds=seeds[live]), args.repeats)
    res["imported_games"] = int(live.numel())
    dst.check_errors()
    for k in ("fork_observe_ms", "snapshot_ms", "restore_observe_ms", "import_observe_ms"):
        res[k[:-3] + "_median_ms"] = round(statistics.median(res[k]), 4)
        res[k] = [round(v, 4) for v in res[k]]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
