"""Search distillation, measured.  Writes profiles/distill_probe.json (or --out).  Needs the GPU: there is no CPU path to time.

(a) Update time.  One clone update with the soft tail (CompositeLearner.clone_loss with batch["target"], value_weight 1:
    hsad_r2d2_clone_soft_fwd) next to one clone-value update (the same call without the key: hsad_r2d2_clone_value_fwd, whose kernel,
    entry point and schedule this change leaves as they were) of the SAME learner in the same process, at B = 128, T = 80, H = 512
    (F = 838, A = 21), the way tools/clone_probe.py times: ms per update from a host clock around windows that end in a device
    synchronise, the kinds alternating window by window; medians with the spread (min, max) over the windows.  The soft update reads
    T B A 4 = 0.86 MB more.  `soft_inside_clone_value_spread` says whether its median lies inside the clone-value update's own spread.

(b) One small loop on a cheap variant (default: 2 colours, hands of 2, 3 information tokens, 1 life; 2 players, sad = 1).  The blueprint
    is a net cloned from the rule bot `piers` (the existing path); then the blueprint's score, the score of blueprint + search over the
    same deals (search.play_with_search(records=True)), and the plain self-play score of the blueprint after it was fitted to the
    searched games with hard labels (the move made) and with soft targets at two temperatures -- each with its standard error.
    OBSERVATIONS of one run with one seed: nothing here is tuned, and no threshold hangs on them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hanabi_sad_amd import clone                            # noqa: E402
from hanabi_sad_amd.composite import CompositeLearner      # noqa: E402
from hanabi_sad_amd.selfplay import init_weights            # noqa: E402

DEV = "cuda:0"


def update_times(windows, updates):
    F, H, A, T, B = 838, 512, 21, 80, 128
    g = torch.Generator().manual_seed(5)
    W = init_weights(F, H, A, 5, 0)
    seq_len = torch.randint(40, 81, (B,), generator=g).float()
    mask = (torch.arange(T).unsqueeze(1) < seq_len.unsqueeze(0)).float()
    legal = (torch.rand(T, B, A, generator=g) < 0.4).float()
    legal[..., 0] = 1
    a = torch.multinomial(legal.view(-1, A), 1, generator=g).view(T, B)
    reward = (torch.rand(T, B, generator=g) < 0.05).float() * mask
    w = (torch.rand(T, B, A, generator=g, dtype=torch.float64) + 0.05) * legal.double()
    batch = {"priv_s": (torch.rand(T, B, F, generator=g) < 0.15).float() * mask.unsqueeze(2), "legal_move": legal * mask.unsqueeze(2),
             "a": a * mask.long(), "seq_len": seq_len, "ret": torch.flip(torch.cumsum(torch.flip(reward, [0]), 0), [0])}
    batch = {k: v.to(DEV) for k, v in batch.items()}
    soft = dict(batch, target=((w / w.sum(2, keepdim=True)).float() * mask.unsqueeze(2)).to(DEV))
    weight = torch.ones(B, device=DEV)
    lr = CompositeLearner(W, W, 3, 0.999, lr=0.0, device=DEV)      # lr 0: the weights, and with them the work, stay what they are

    def update(b):
        def fn():
            lr.clone_loss(b, weight, value_weight=1.0)
            lr.optimizer_step()
        return fn

    kinds = {"clone_value_update": update(batch), "clone_soft_update": update(soft),
             "clone_value_forward": lambda: lr.clone_loss(batch, weight, compute_grad=False, value_weight=1.0),
             "clone_soft_forward": lambda: lr.clone_loss(soft, weight, compute_grad=False, value_weight=1.0)}
    plans = {}
    for name, fn in kinds.items():          # warm up every kind: code objects, counter blocks, the schedule
        for _ in range(10):
            fn()
        plans[name] = lr.plan()
    _, stats = lr.clone_loss(soft, weight, compute_grad=False, value_weight=1.0)
    assert int(stats["bad"].sum()) == 0
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    for _ in range(windows):
        for name, fn in kinds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(updates):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / updates * 1e3)
    lr.check_sync()
    lr.close()
    out = {"shape": dict(F=F, H=H, A=A, T=T, B=B), "windows": windows, "updates_per_window": updates, "extra_bytes_read_per_update": T * B * A * 4}
    for name in kinds:
        v = ms[name]
        out[name] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "fwd_nets": plans[name]["fwd_nets"],
                     "fwd_kind": plans[name]["fwd_kind"], "bwd_kind": plans[name]["bwd_kind"]}
        print("%-20s %.4f ms (min %.4f, max %.4f over %d windows of %d)" % (name, out[name]["ms_median"], min(v), max(v), windows, updates), flush=True)
    cv, cs = out["clone_value_update"], out["clone_soft_update"]
    out["soft_over_clone_value_update"] = cs["ms_median"] / cv["ms_median"]
    out["soft_inside_clone_value_spread"] = bool(cv["ms_min"] <= cs["ms_median"] <= cv["ms_max"])
    print("soft / clone-value update: %.4f; inside the clone-value update's own spread: %s" % (out["soft_over_clone_value_update"],
                                                                                              out["soft_inside_clone_value_spread"]))
    return out


def mean_sem(scores):
    s = np.asarray(scores, dtype=np.float64)
    return {"mean": float(s.mean()), "sem": float(s.std() / np.sqrt(len(s))), "games": int(len(s))}


def fit(W0, records, targets, sad, epochs, rows, lr, seed):
    """W0 fitted to the records for `epochs` passes -> (weights, loss per decision of the last epoch, its KL per decision or None)"""
    data = clone.sequences_from_records(records, sad, device=DEV, targets=targets)
    learner = CompositeLearner(W0, W0, 1, 0.999, lr=lr, device=DEV)
    for e in range(epochs):
        loss, hits, n = clone.run_epoch(learner, data, rows, seed + e, True)
    weights = {k: v.detach().cpu().clone() for k, v in learner.online.w.items()}
    learner.close()
    return weights, loss, (loss - clone.target_entropy(data) / max(n, 1)) if targets is not None else None


def small_loop(args):
    from hanabi_sad_amd.eval import env_dims, evaluate
    from hanabi_sad_amd.rulebot import PRESETS
    from hanabi_sad_amd.search import play_with_search
    rules = dict(colors=args.colors, ranks=5, max_information_tokens=args.max_information_tokens, max_life_tokens=args.max_life_tokens)
    P, hand, sad, seed = 2, args.hand_size, True, args.seed
    F, A = env_dims(P, hand, sad, **rules)

    def score(W):
        return mean_sem(evaluate(W, args.num_eval_game, seed + 500000, 0, sad, num_player=P, hand_size=hand, device=DEV, **rules)[2])

    t0 = time.perf_counter()
    bot_games = clone.records_from_teacher([PRESETS["piers"]], args.bot_games, seed + 100000, sad, num_player=P, device=DEV, hand_size=hand, **rules)
    blueprint, _, _ = fit(init_weights(F, args.rnn_hid_dim, A, hand, seed), bot_games, None, sad, args.bot_epochs, 128, 5e-4, seed)
    out = {"rules": dict(rules, players=P, hand_size=hand, sad=int(sad)), "rnn_hid_dim": args.rnn_hid_dim, "seed": seed,
           "blueprint_from": {"teacher": "piers", "games": args.bot_games, "epochs": args.bot_epochs, "teacher_score": mean_sem([r.score for r in bot_games])},
           "search": {"worlds": args.worlds, "deals": args.num_game, "threshold": 0.05}, "fit": {"epochs": args.epochs, "rows": 128, "lr": args.lr},
           "blueprint_self_play": score(blueprint)}
    print("blueprint (cloned from piers): %s, %.0f s" % (out["blueprint_self_play"], time.perf_counter() - t0), flush=True)
    kw = dict(search_seed=seed, num_player=P, hand_size=hand, device=DEV, **rules)
    base = play_with_search(blueprint, args.num_game, seed, 0, sad, worlds=0, **kw)
    played = play_with_search(blueprint, args.num_game, seed, 0, sad, worlds=args.worlds, records=True, **kw)
    out["blueprint_on_the_search_deals"] = mean_sem(base.scores)
    out["blueprint_plus_search"] = dict(mean_sem(played.scores), deviations_per_game=float(played.deviations.double().mean()))
    print("the same deals: blueprint %s, blueprint + search %s, %.0f s" % (out["blueprint_on_the_search_deals"], out["blueprint_plus_search"],
                                                                          time.perf_counter() - t0), flush=True)
    out["distilled"] = {}
    for name, tau in [("hard_labels", None)] + [("tau_%g" % t, t) for t in args.temperatures]:
        targets = clone.search_targets(played.records, played.search_values, tau) if tau else None
        W, loss, kl = fit(blueprint, played.records, targets, sad, args.epochs, 128, args.lr, seed)
        out["distilled"][name] = dict(score(W), target_temperature=tau, last_epoch_loss_per_decision=loss, last_epoch_kl_per_decision=kl)
        print("distilled, %s: %s, %.0f s" % (name, out["distilled"][name], time.perf_counter() - t0), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12, help="(a) timed windows per kind")
    ap.add_argument("--updates", type=int, default=100, help="(a) updates per window")
    ap.add_argument("--skip_loop", type=int, default=0)
    ap.add_argument("--colors", type=int, default=2)
    ap.add_argument("--hand_size", type=int, default=2)
    ap.add_argument("--max_information_tokens", type=int, default=3)
    ap.add_argument("--max_life_tokens", type=int, default=1)
    ap.add_argument("--rnn_hid_dim", type=int, default=128)
    ap.add_argument("--bot_games", type=int, default=2000, help="(b) games of the rule bot the blueprint is cloned from")
    ap.add_argument("--bot_epochs", type=int, default=15)
    ap.add_argument("--num_game", type=int, default=512, help="(b) deals played with search and distilled")
    ap.add_argument("--worlds", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=2.5e-4)
    ap.add_argument("--temperatures", type=float, nargs=2, default=[0.1, 0.5])
    ap.add_argument("--num_eval_game", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "distill_probe.json"))
    args = ap.parse_args(argv)
    out = {"device": torch.cuda.get_device_name(0), "update_time": update_times(args.windows, args.updates)}
    if not args.skip_loop:
        out["small_loop"] = small_loop(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
