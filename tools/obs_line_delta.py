"""How much of the float32 observation priv_s [G, P, F] changes from one rollout iteration to the next, in the unit the delta stream
of the pipelined rollout skips (csrc/hsad_env.hip, EnvParams::delta): 32 consecutive floats = one 128-byte line of the flattened
array, or --unit N floats (16: the 64-byte half lines of the compacted form, hsad_env_set_rollout_unit).  CPU only: the games are played by the oracle (oracle/oracle.py, OracleVecEnv) under the random-legal policy of the benchmark.

  python tools/obs_line_delta.py [--games 2048] [--players 2] [--hand 5] [--sad] [--iters 130] [--window 5:25] [--unit 32] [--json OUT]

Prints the share of changed units per iteration (priv_s also in 16-float units, next to the chosen one), and its mean / min / max over the driver's window (iterations 5-24 of bench.py
--steps 20 --warmup 5) and over the steady state (iteration 50 on); the same for legal_move and own_hand, which are always streamed
in full, and the share of games that ended in each iteration."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINE = 32   # floats per 128-byte line


def changed_share(cur, prev, unit=LINE):
    """share of unit-float units of the flattened arrays that differ (a partial last unit counts as one)"""
    d = (cur.ravel() != prev.ravel())
    pad = (-d.size) % unit
    if pad:
        d = np.concatenate([d, np.zeros(pad, bool)])
    return float(d.reshape(-1, unit).any(axis=1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--players", type=int, default=2)
    ap.add_argument("--hand", type=int, default=5)
    ap.add_argument("--sad", action="store_true")
    ap.add_argument("--iters", type=int, default=130)
    ap.add_argument("--window", default="5:25", help="first:last+1 iteration of the driver's measured launch")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--policy-seed", type=int, default=12345)
    ap.add_argument("--unit", type=int, default=LINE, help="floats per unit (32: a 128-byte line, 16: a half line)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from oracle.oracle import OracleVecEnv
    eps = [0.1 ** (1 + 7 * i / 79) for i in range(80)]     # bench.py's list
    env = OracleVecEnv(args.games, args.seed, players=args.players, hand_size=args.hand, eps_list=eps, max_len=80, sad=args.sad)
    prev = None
    rows = []
    for it in range(args.iters):
        env.rollout(1, args.policy_seed)
        cur = {"priv_s": env.priv_s.copy(), "legal_move": env.legal.copy(), "own_hand": env.own_hand.copy()}
        if prev is not None:
            r = {"iteration": it, "games_ended": float(env.terminal.mean())}
            r.update({k: changed_share(cur[k], prev[k], args.unit) for k in cur})
            r["priv_s_16"] = changed_share(cur["priv_s"], prev["priv_s"], 16)
            rows.append(r)
            print("iter %3d  priv_s %.4f  (16-float units %.4f)  legal_move %.4f  own_hand %.4f  games ended %.4f"
                  % (it, r["priv_s"], r["priv_s_16"], r["legal_move"], r["own_hand"], r["games_ended"]))
        prev = cur

    def span(lo, hi):
        sel = [r for r in rows if lo <= r["iteration"] < hi]
        if not sel:
            return None
        out = {"iterations": [sel[0]["iteration"], sel[-1]["iteration"]]}
        for k in ("priv_s", "priv_s_16", "legal_move", "own_hand", "games_ended"):
            v = np.array([r[k] for r in sel])
            out[k] = {"mean": round(float(v.mean()), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}
        return out

    lo, hi = (int(x) for x in args.window.split(":"))
    rec = {"games": args.games, "players": args.players, "hand": args.hand, "sad": bool(args.sad), "feature_size": int(env.F),
           "unit_floats": args.unit, "driver_window": span(lo, hi), "steady_state": span(50, args.iters), "per_iteration": rows}
    print(json.dumps({k: v for k, v in rec.items() if k != "per_iteration"}, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
