"""Records for DESIGN §3g: fork + observe time, the playout's env-steps/s without the observation stream, the sampler's mean tries,
next to hsad_env_step on the same games; with --sampler stratified also the time of hsad_env_determinize_exact + observe on the same
states (8 strata), and in either case the time of hsad_env_hand_belief; with --playout NAME (a preset of hanabi_sad_amd.rulebot) the
env-steps/s of hsad_env_playout_rule next to hsad_env_playout_random's from the same states.  One JSON line.

    python tools/search_probe.py [--games 65536] [--repeats 5] [--sampler rejection|stratified] [--playout cautious|piers|flawed|random]
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
from hanabi_sad_amd.rulebot import PRESETS  # noqa: E402


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
    ap.add_argument("--sampler", choices=["rejection", "stratified"], default="rejection")
    ap.add_argument("--playout", choices=sorted(PRESETS), default=None)
    args = ap.parse_args()
    G, dev = args.games, "cuda:0"
    kw = dict(players=2, hand_size=5, sad=bool(args.sad), eps_list=(0.0,), device=dev)
    src = BatchedHanabiEnv(G, seed=1, **kw)
    dst = BatchedHanabiEnv(G, seed=2, track_deck_history=False, **kw)
    src.rollout_random(12, 3)
    idx = torch.randperm(G, device=dev, generator=torch.Generator(device=dev).manual_seed(0)).to(torch.int32)
    seeds = torch.arange(G, device=dev, dtype=torch.int32)
    res = {"games": G, "sad": args.sad, "repeats": args.repeats, "sampler": args.sampler}
    dst.fork_from(src, idx)   # warm-up (first launch of each kernel)
    res["fork_observe_ms"] = timed(lambda: dst.fork_from(src, idx), args.repeats)
    res["fork_observe_reseed_ms"] = timed(lambda: dst.fork_from(src, idx, seeds), args.repeats)
    # yardstick: one hsad_env_step of the same games (policy outside the timed region)
    step_ms = []
    for _ in range(args.repeats):
        src.reset()
        a, ga = src.policy_random(5)
        step_ms += timed(lambda: src.step(a, ga), 1)
    res["env_step_ms"] = step_ms
    q = src.query()
    viewer = torch.where(q[:, 0] == 0, q[:, 1], torch.full_like(q[:, 1], -1)).to(torch.int32)
    key = torch.arange(G, device=dev, dtype=torch.int64)
    det_ms, tries_mean, gave_up = [], [], 0
    for r in range(args.repeats):
        dst.fork_from(src, torch.arange(G, device=dev, dtype=torch.int32))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tries = dst.determinize(viewer, key, 100 + r)
        torch.cuda.synchronize()
        det_ms.append((time.perf_counter() - t0) * 1e3)
        done = tries[tries > 0].float()
        tries_mean.append(float(done.mean()))
        gave_up += int((tries < 0).sum())
    res["determinize_observe_ms"], res["mean_tries"], res["gave_up"] = det_ms, tries_mean, gave_up
    medians = []
    if args.sampler == "stratified":   # the chosen sampler's call on the same states, next to the rejection sampler's
        stratum = (torch.arange(G, device=dev, dtype=torch.int32) % 8).contiguous()
        exact_ms, left_alone = [], 0
        for r in range(args.repeats):
            dst.fork_from(src, torch.arange(G, device=dev, dtype=torch.int32))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rank = dst.determinize_exact(viewer, key, 100 + r, stratum=stratum, n_strata=8)
            torch.cuda.synchronize()
            exact_ms.append((time.perf_counter() - t0) * 1e3)
            left_alone += int(((rank < 0) & (viewer >= 0)).sum())
        res["determinize_exact_observe_ms"], res["exact_left_alone"] = exact_ms, left_alone
        medians.append("determinize_exact_observe_ms")
    dst.fork_from(src, torch.arange(G, device=dev, dtype=torch.int32))
    dst.hand_belief(viewer)   # warm-up
    res["hand_belief_ms"] = timed(lambda: dst.hand_belief(viewer), args.repeats)
    medians.append("hand_belief_ms")
    # playout: every game from where the fork left it to its end
    rates, play_ms = [], []
    for r in range(args.repeats):
        dst.fork_from(src, torch.arange(G, device=dev, dtype=torch.int32), seeds)
        n0 = dst.query()[:, 6].sum().item()
        ms = timed(lambda: dst.playout_random(100, 9 + r), 1)[0]
        qq = dst.query()
        assert bool((qq[:, 0] == 1).all())
        steps = qq[:, 6].sum().item() - n0
        play_ms.append(ms)
        rates.append(steps / ms * 1e3)
    dst.check_errors()
    res["playout_ms"], res["playout_env_steps_per_s"] = play_ms, rates
    if args.playout:   # the same states, the same reseeded generators, the bot in place of the random pick
        bot, rule_rates, rule_ms, rule_score = PRESETS[args.playout], [], [], []
        for r in range(args.repeats):
            dst.fork_from(src, torch.arange(G, device=dev, dtype=torch.int32), seeds)
            n0 = dst.query()[:, 6].sum().item()
            ms = timed(lambda: dst.playout_rule(100, bot, seed=9 + r), 1)[0]
            qq = dst.query()
            assert bool((qq[:, 0] == 1).all())
            rule_ms.append(ms)
            rule_rates.append((qq[:, 6].sum().item() - n0) / ms * 1e3)
            rule_score.append(float(qq[:, 5].double().mean()))
        dst.check_errors()
        res["playout_rule"], res["playout_rule_ms"], res["playout_rule_env_steps_per_s"] = args.playout, rule_ms, rule_rates
        res["playout_rule_mean_score"] = rule_score
        medians += ["playout_rule_ms", "playout_rule_env_steps_per_s"]
    for k in ("fork_observe_ms", "fork_observe_reseed_ms", "env_step_ms", "determinize_observe_ms", "playout_ms", "playout_env_steps_per_s", *medians):
        res[k + "_median"] = statistics.median(res[k])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
