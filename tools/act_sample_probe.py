"""The acting tail with and without sampling, timed: hsad_act_select (the unstaged form), hsad_act_select_q and hsad_act_select_q2 (a second
heads matrix as the target's) next to hsad_act_sample_q (temp NULL, all rows at temperature 1, and keyed rows at temperature 1) at
N = 32,768, A = 21 (ldh 37) on synthetic heads, and (unless --deals 0) one tournament step (eval.play_seatings: two
small nets, every seating, 1,024 deals of the standard game) with and without a temperature.  ms from a host clock around windows that
end in a device synchronise, the kinds alternating window by window; medians with the spread.  One JSON line (and --out FILE).  --lib FILE
times another build of the library (an A/B against an earlier commit's).  Needs the GPU: there is no CPU path to time."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hanabi_sad_amd import _lib                              # noqa: E402
from hanabi_sad_amd.composite import _s                      # noqa: E402
from hanabi_sad_amd.eval import env_dims, play_seatings      # noqa: E402
from hanabi_sad_amd.selfplay import init_weights             # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200, help="tail calls per window")
    ap.add_argument("--deals", type=int, default=1024, help="deals of the tournament step; 0 times the tail kinds only")
    ap.add_argument("--out", default="")
    ap.add_argument("--lib", default="", help="the library file to load instead of the package's own")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    lib = _lib.load_library()
    N, A, ldh = 32768, 21, 37
    g = torch.Generator().manual_seed(3)
    heads = (torch.randn(N, ldh, generator=g) * 2).to(dev)
    heads_t = (torch.randn(N, ldh, generator=g) * 2).to(dev)
    legal = (torch.rand(N, A, generator=g) < 0.5).float()
    legal[:, 0] = 1
    legal = legal.to(dev)
    eps = torch.where(torch.rand(N, generator=g) < 0.3, 0.1, 0.0).to(dev)
    temp = torch.ones(N, device=dev)
    key = torch.arange(N, dtype=torch.int64, device=dev) * 4096
    a, gr = torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)
    qa, tq, scratch = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.zeros(8 + (N + 255) // 256, device=dev)
    st = _s(dev)
    p = lambda t: None if t is None else t.data_ptr()

    def select():
        _lib.check(lib.hsad_act_select_q(p(heads), ldh, p(legal), p(eps), N, A, 5, 9, p(a), p(gr), p(qa), p(scratch), st))

    def select_plain():
        _lib.check(lib.hsad_act_select(p(heads), ldh, p(legal), p(eps), N, A, 5, 9, p(a), p(gr), p(scratch), st))

    def select_q2():
        _lib.check(lib.hsad_act_select_q2(p(heads), p(heads_t), ldh, p(legal), p(eps), N, A, 5, 9, p(a), p(gr), p(qa), p(tq), p(scratch), st))

    def sample(t, k):
        return lambda: _lib.check(lib.hsad_act_sample_q(p(heads), ldh, p(legal), p(eps), p(t), p(k), 11, N, A, 5, 9, p(a), p(gr), p(qa),
                                                        p(scratch), st))
    kinds = {"act_select": select_plain, "act_select_q": select, "act_select_q2": select_q2, "act_sample_q_no_temp": sample(None, None), "act_sample_q_temp1": sample(temp, None),
             "act_sample_q_temp1_keyed": sample(temp, key)}
    for fn in kinds.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in kinds}
    for _ in range(args.windows):
        for name, fn in kinds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / args.calls * 1e6)
    out = {"device": torch.cuda.get_device_name(0), "lib": args.lib or "the package's", "tail_shape": dict(N=N, A=A, ldh=ldh), "windows": args.windows, "calls_per_window": args.calls,
           "note": "us per call = adv_min_kernel (+ min_reduce_kernel: act_select) + the tail kernel, launch overhead included (back-to-back calls on one "
                   "stream)"}
    for name, v in us.items():
        out[name] = {"us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
    if args.deals > 0:      # a tournament: the whole call (env, nets, every step with its host look at one word), then per step
        F, A2 = env_dims(2, 5, True)
        pool = [init_weights(F, 512, A2, 5, 1), init_weights(F, 512, A2, 5, 2)]
        seatings = [(0, 0), (0, 1), (1, 0), (1, 1)]
        tour = {}
        for name, kw in (("greedy", {}), ("temperature1", dict(temperature=1.0, sample_seed=3))):
            play_seatings(pool, seatings, 64, 1, 0, True, device=str(dev), behaviour=True, **kw)      # warm up
            v = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = play_seatings(pool, seatings, args.deals, 1, 0, True, device=str(dev), behaviour=True, **kw)
                torch.cuda.synchronize()
                steps = int(res.behaviour.game_moves.max()) + 1
                v.append(((time.perf_counter() - t0) * 1e3, steps))
            ms, steps = sorted(v)[1]
            tour[name] = {"ms_call_median": ms, "steps": steps, "ms_per_step": ms / steps, "mean_score": float(res.mean.mean())}
        out["tournament"] = dict(tour, deals=args.deals, seatings=len(seatings), hid_dim=512)
    line = json.dumps(out, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
