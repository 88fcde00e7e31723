"""Developer tool: what do game records cost?  Three timings, no threshold -- nothing asserts a time.

  1. a tournament chunk (eval._TournamentBatch.play: the rule bots piers and cautious, 4 seatings x `--deals` deals) without the
     recorder, with it and a filter that keeps nothing (the append launches alone), and with it and a filter that keeps about 1 %
     (select + gather + the host's parsing on top); per step = chunk time / steps of the longest game
  2. hsad_game_log_select + hsad_game_log_gather of 1 % of the games (every 100th by the `take` byte), device events around both
  3. hsad_env_playout_logged of those records to full length over every slot of the env (upload of the records included) against
     the same replay done move by move: hsad_env_rewind_scripted, then one hsad_env_step per move with the logged moves forced

Every variant is warmed up once and then timed `--repeat` times, alternating with the others; a host clock around work that ends in
a device synchronise unless said otherwise.  Writes JSON.

    python tools/record_probe.py --out profiles/record_probe.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0, out


def stats(xs):
    return {"runs_s": [float(x) for x in xs], "median_s": float(np.median(xs)), "spread_s": float(max(xs) - min(xs))}


def main():
    from hanabi_sad_amd import BatchedHanabiEnv
    from hanabi_sad_amd import game_record as gr
    from hanabi_sad_amd.eval import _TournamentBatch, _drain_errors
    from hanabi_sad_amd.rulebot import PRESETS
    ap = argparse.ArgumentParser()
    ap.add_argument("--deals", type=int, default=16384, help="deals per seating; 4 seatings: 65,536 games by default")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join("profiles", "record_probe.json"))
    args = ap.parse_args()
    dev, n = args.device, args.deals
    pool = [PRESETS["piers"], PRESETS["cautious"]]
    seatings = np.array([(0, 0), (0, 1), (1, 0), (1, 1)], dtype=np.int64)
    env_kw = dict(hand_size=5, bomb=0, sad=False, shuffle_color=False, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3)
    G = len(seatings) * n

    # ---- 1. the tournament chunk ----
    keep_none = gr.GameFilter(score_min=200)
    variants = {"plain": None, "append_only": keep_none, "keep_1_percent": None}
    batches = {"plain": _TournamentBatch(pool, seatings, n, env_kw, dev, 0, False, None),
               "append_only": _TournamentBatch(pool, seatings, n, env_kw, dev, 0, False, keep_none)}
    _, (scores, _) = timed(lambda: batches["plain"].play(args.seed, 200), dev)
    steps = int(batches["plain"].game_moves.max()) + 1
    # a score bound that keeps about 1 % of the games
    bound = int(np.sort(scores.reshape(-1))[max(G // 100 - 1, 0)])
    variants["keep_1_percent"] = gr.GameFilter(score_max=bound)
    batches["keep_1_percent"] = _TournamentBatch(pool, seatings, n, env_kw, dev, 0, False, variants["keep_1_percent"])
    times = {k: [] for k in batches}
    for k, b in batches.items():
        timed(lambda b=b: b.play(args.seed, 200), dev)
    for _ in range(args.repeat):
        for k, b in batches.items():
            dt, (sc, _) = timed(lambda b=b: b.play(args.seed, 200), dev)
            assert np.array_equal(sc, scores), "recording must not change the games"
            times[k].append(dt)
    chunk = {k: dict(stats(v), per_step_ms=float(np.median(v)) / steps * 1e3) for k, v in times.items()}
    chunk["kept_games"] = {k: (len(b.records) if b.records is not None else None) for k, b in batches.items()}

    # ---- 2. select + gather of 1 % ----
    b = batches["append_only"]
    rec, env = b.recorder, b.env
    take = torch.zeros(G, dtype=torch.uint8, device=dev)
    take[::100] = 1
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    idx = rec.select(None, take)
    rec.gather(idx)
    sel_ms = []
    for _ in range(10 * args.repeat):
        ev[0].record()
        idx = rec.select(None, take)        # (reads the count back: one small device-to-host copy inside the window)
        data = rec.gather(idx)
        ev[1].record()
        ev[1].synchronize()
        sel_ms.append(ev[0].elapsed_time(ev[1]))
    records = [gr.GameRecord.from_bytes(row.tobytes()) for row in data.cpu().numpy()]
    select = {"games": G, "selected": len(records), "record_bytes": rec.record_bytes, "bytes_to_host": len(records) * rec.record_bytes,
              "median_ms": float(np.median(sel_ms)), "min_ms": float(min(sel_ms)), "max_ms": float(max(sel_ms))}

    # ---- 3. replay: one launch against move by move ----
    R, P, A = len(records), 2, env.A
    src = torch.from_numpy((np.arange(G) % R).astype(np.int32)).to(dev)
    packed = np.frombuffer(b"".join(r.to_bytes() for r in records), dtype=np.uint8).reshape(R, -1)
    T = max(r.n_moves for r in records)
    mv = np.full((R, T), A - 1, np.int64)
    for j, r in enumerate(records):
        mv[j, :r.n_moves] = r.moves
    a_steps = np.full((T, G, P), A - 1, np.int64)
    srch = src.cpu().numpy()
    for t in range(T):
        a_steps[t, :, t % P] = mv[srch, t]
    a_steps = torch.from_numpy(a_steps).to(dev)
    script = np.zeros((R, 52), np.uint8)
    count = np.zeros(R, np.int32)
    for j, r in enumerate(records):
        script[j, :len(r.deck)], count[j] = r.deck, len(r.deck)
    script, count = torch.from_numpy(script[srch]).to(dev), torch.from_numpy(count[srch]).to(dev)
    renv = BatchedHanabiEnv(G, seed=args.seed, eps_list=[0.0], max_len=-1, sad=False, bomb=0, device=dev)
    renv.reset()

    def one_launch():
        return renv.playout_logged(packed, src)

    def move_by_move():
        renv.rewind_scripted(script, count)
        for t in range(T):
            renv.step(a_steps[t], a_steps[t])

    timed(one_launch, dev)
    want = renv.export_state().clone()
    timed(move_by_move, dev)
    _drain_errors(renv)
    assert torch.equal(renv.export_state(), want), "the two replays must end in the same positions"
    t_one, t_mbm = [], []
    for _ in range(args.repeat):
        t_one.append(timed(one_launch, dev)[0])
        t_mbm.append(timed(move_by_move, dev)[0])
        _drain_errors(renv)
    replay = {"games": G, "records": R, "longest_game": T, "moves_replayed": int(sum(records[j].n_moves for j in srch)),
              "playout_logged": stats(t_one), "rewind_plus_steps": stats(t_mbm),
              "ratio": float(np.median(t_mbm) / np.median(t_one))}

    res = {"device": torch.cuda.get_device_name(dev), "workload": {"bots": ["piers", "cautious"], "seatings": seatings.tolist(), "deals": n,
                                                                  "games": G, "steps_of_the_longest_game": steps},
           "tournament_chunk": chunk, "select_gather_1_percent": select, "replay": replay}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
