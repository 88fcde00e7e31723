"""One behaviour-cloning update (CompositeLearner.clone_loss + optimizer_step: the online net alone) next to one TD update (loss +
optimizer_step: online and target net) of the SAME learner in the same process, at B = 128, T = 80, H = 512 (F = 838, A = 21):
ms per update from a host clock around windows that end in a device synchronise, the two kinds alternating window by window so that
whatever else the host does hits both alike; the spread over the windows is reported with the medians.  Also the forward halves alone
(compute_grad=False), and the clone update with the value term (clone_loss(value_weight=1): hsad_r2d2_clone_value_fwd, the same schedule
with clone_value_tail_kernel at its end).  Writes profiles/clone_probe.json (or --out).  Needs the GPU: there is no CPU path to time."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hanabi_sad_amd.composite import CompositeLearner      # noqa: E402
from hanabi_sad_amd.selfplay import init_weights            # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12, help="timed windows per kind")
    ap.add_argument("--updates", type=int, default=100, help="updates per window")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "clone_probe.json"))
    args = ap.parse_args(argv)
    dev = "cuda:0"
    F, H, A, T, B = 838, 512, 21, 80, 128
    g = torch.Generator().manual_seed(5)
    W = init_weights(F, H, A, 5, 0)
    seq_len = torch.randint(40, 81, (B,), generator=g).float()
    mask = (torch.arange(T).unsqueeze(1) < seq_len.unsqueeze(0)).float()
    legal = (torch.rand(T, B, A, generator=g) < 0.4).float()
    legal[..., 0] = 1
    a = torch.multinomial(legal.view(-1, A), 1, generator=g).view(T, B)
    batch = {"priv_s": (torch.rand(T, B, F, generator=g) < 0.15).float() * mask.unsqueeze(2), "legal_move": legal * mask.unsqueeze(2),
             "a": a * mask.long(), "reward": (torch.rand(T, B, generator=g) < 0.05).float() * mask, "bootstrap": mask.clone(), "seq_len": seq_len}
    batch["ret"] = torch.flip(torch.cumsum(torch.flip(batch["reward"], [0]), 0), [0])      # the undiscounted return-to-go of those rewards
    batch = {k: v.to(dev) for k, v in batch.items()}
    weight = torch.ones(B, device=dev)
    lr = CompositeLearner(W, W, 3, 0.999, lr=0.0, device=dev)      # lr 0: the weights, and with them the work, stay what they are

    def td():
        lr.loss(batch, weight, 0.0)
        lr.optimizer_step()

    def clone():
        lr.clone_loss(batch, weight)
        lr.optimizer_step()

    def clone_value():
        lr.clone_loss(batch, weight, value_weight=1.0)
        lr.optimizer_step()

    kinds = {"td_update": td, "clone_update": clone, "clone_value_update": clone_value,
             "td_forward": lambda: lr.loss(batch, weight, 0.0, compute_grad=False),
             "clone_forward": lambda: lr.clone_loss(batch, weight, compute_grad=False),
             "clone_value_forward": lambda: lr.clone_loss(batch, weight, compute_grad=False, value_weight=1.0)}
    plans = {}
    for name, fn in kinds.items():          # warm up every kind: code objects, counter blocks, the schedule
        for _ in range(10):
            fn()
        plans[name] = lr.plan()
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    for _ in range(args.windows):
        for name, fn in kinds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.updates):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.updates * 1e3)
    lr.check_sync()
    out = {"shape": dict(F=F, H=H, A=A, T=T, B=B), "windows": args.windows, "updates_per_window": args.updates, "device": torch.cuda.get_device_name(0)}
    for name in kinds:
        v = ms[name]
        out[name] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "fwd_nets": plans[name]["fwd_nets"],
                     "fwd_kind": plans[name]["fwd_kind"], "bwd_kind": plans[name]["bwd_kind"]}
        print("%-14s %.3f ms (min %.3f, max %.3f over %d windows of %d)" % (name, out[name]["ms_median"], min(v), max(v), args.windows, args.updates), flush=True)
    out["clone_over_td_update"] = out["clone_update"]["ms_median"] / out["td_update"]["ms_median"]
    out["clone_over_td_forward"] = out["clone_forward"]["ms_median"] / out["td_forward"]["ms_median"]
    out["clone_value_over_clone_update"] = out["clone_value_update"]["ms_median"] / out["clone_update"]["ms_median"]
    print("clone / TD: update %.3f, forward %.3f; clone with the value term / clone: update %.3f"
          % (out["clone_over_td_update"], out["clone_over_td_forward"], out["clone_value_over_clone_update"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
