"""Time per actor step with fixed partners next to the self-play step on the same games (DESIGN, "Training next to fixed partners").

    python tools/partner_probe.py --num_game 16384 --partner piers
    python tools/partner_probe.py --num_game 16384 --net_partner random

--partner takes what selfplay's --partner takes: rule-bot presets and weight files of frozen networks (FILE:skip for a skip_connect net).
--net_partner random seats, instead, one random-initialised frozen network of the learner's shape on every partner row.
Both actors are the library's loop (hsad_actor_step): the partnered one runs the network on one row per game, the self-play one on
every row.  A sample is `--steps` steps between two device synchronisations on the host clock, divided by the step count; the
figure is the median of `--repeats` samples, the two actors taking turns.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from hanabi_sad_amd.selfplay import Trainer, parse_args
    p = argparse.ArgumentParser()
    p.add_argument("--num_game", type=int, default=16384)
    p.add_argument("--partner", type=str, nargs="+", default=["piers"])
    p.add_argument("--net_partner", type=str, default=None, choices=["random"])
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--repeats", type=int, default=15)
    p.add_argument("--warmup", type=int, default=100)
    a = p.parse_args()
    common = ["--num_game", str(a.num_game), "--replay_buffer_size", "65536", "--overlap_rollout", "0"]
    tmp = None
    if a.net_partner == "random":          # a weight file of the learner's shape, written for this run and handed over like any other
        import tempfile
        from hanabi_sad_amd import BatchedHanabiEnv
        from hanabi_sad_amd.selfplay import init_weights
        base = parse_args(common)
        dims = BatchedHanabiEnv(2, players=base.num_player, hand_size=base.hand_size, sad=bool(base.sad), device="cuda:0")
        tmp = tempfile.TemporaryDirectory()
        a.partner = [os.path.join(tmp.name, "random.pthw")]
        torch.save(init_weights(dims.F, base.rnn_hid_dim, dims.A, base.hand_size, 12345, num_lstm_layer=base.num_lstm_layer), a.partner[0])
    trainers = {"partnered": Trainer(parse_args(common + ["--partner"] + a.partner), "cuda:0"), "self_play": Trainer(parse_args(common), "cuda:0")}
    for tr in trainers.values():          # past the first games' ends, so that resets and flushes are part of a step
        for _ in range(a.warmup):
            tr.actor.step()
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for _ in range(a.repeats):
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.actor.step()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    for tr in trainers.values():
        tr.env.check_errors()
        tr.replay.check_errors()
    res = {"num_game": a.num_game, "partner": a.partner, "steps_per_sample": a.steps, "repeats": a.repeats,
           "agent_rows": {k: tr.actor.N for k, tr in trainers.items()}, "n_net": len(trainers["partnered"].actor.partner_nets),
           "net_rows": sum(len(r) for r in trainers["partnered"].actor.partners.net_rows)}
    for k in trainers:
        res[k + "_step_ms_median"] = round(statistics.median(ms[k]), 4)
        res[k + "_step_ms_min"] = round(min(ms[k]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
