"""The learned hand belief, timed (profiles/belief_probe.json): at B = 128 sequences of T = 80 steps, H = 512, hands of 5, on the
knowledge of recorded games -- hsad_belief_tail with and without its gradient, the head's forward GEMM, the weight-gradient path (two
transposes, the split-K GEMM, the ordered column sums), and the blueprint's trunk feature pass; determinize_belief next to
determinize_exact at 4,096 games; and (unless --games 0) two small training runs on --games deals each, the held-out NLL per card of the
learned and of the exact belief after every epoch: the blueprint playing itself, and the `piers` bot's games seen through the same
trunk.  The blueprint is a random 512-unit net (its games end after a few moves and its moves follow no convention): what is measured
is the machinery, not a trained policy's conventions; the `piers` run is the one whose moves carry information.  The timed batch is
64 `piers` games (long games: most of the T x B rows are valid).  ms from a host clock around windows that end in a device synchronise,
the kinds alternating window by window; medians with the spread.  One JSON line (and --out FILE).  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hanabi_sad_amd import BatchedHanabiEnv, _lib            # noqa: E402
from hanabi_sad_amd import belief                            # noqa: E402
from hanabi_sad_amd.clone import records_from_teacher, sequences_from_records      # noqa: E402
from hanabi_sad_amd.eval import env_dims                     # noqa: E402
from hanabi_sad_amd.rulebot import PRESETS                   # noqa: E402
from hanabi_sad_amd.selfplay import init_weights             # noqa: E402


def timed(kinds, windows, calls):
    for fn in kinds.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in kinds}
    for _ in range(windows):
        for name, fn in kinds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / calls * 1e6)
    return {name: {"us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for name, v in us.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--games", type=int, default=1000, help="deals of the training run; 0 times the kernels only")
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    dev = "cuda:0"
    lib = _lib.load_library()
    T, B, H, Hs = 80, 128, 512, 5
    F, A = env_dims(2, Hs, True)
    W = init_weights(F, H, A, Hs, 1)
    records = records_from_teacher([PRESETS["piers"]], B // 2, 7, True, device=dev, names=["piers"])
    data = sequences_from_records(records, True, max_len=T, device=dev, knowledge=True)
    assert data.n_rows == B and data.T == T
    head = belief.BeliefHead(W, Hs, dev)
    g = torch.Generator().manual_seed(2)
    head.weight.copy_((torch.randn(head.NZ, H, generator=g) * 0.05).to(dev))
    head.refresh()
    o16 = head.features(data.priv_s_bf16)
    batch = dict(o16=o16, pool=data.pool, compat=data.compat, cards=data.cards, seq_len=data.seq_len)
    weight = torch.ones(B, device=dev)
    head.loss(batch, weight)
    k = head._buffers(T, B)
    M, Mp, st = T * B, k["Mp"], belief._s(head.device)
    o2 = o16.view(M, H)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def tail(grad):
        return lambda: _lib.check(lib.hsad_belief_tail(p(k["z"]), head.NZp, p(data.pool), p(data.compat), p(data.cards), p(data.seq_len), p(weight), T, B,
                                                       Hs, p(k["nll"]), p(k["nll0"]), p(k["cards"]), p(k["hits"]), p(k["hits0"]), p(k["bad"]),
                                                       p(k["dz"]) if grad else None, head.NZp, st))

    def wgrad():
        _lib.check(lib.hsad_transpose_bf16(p(k["dz"]), M, head.NZp, head.NZp, p(k["dzT"]), Mp, st))
        _lib.check(lib.hsad_transpose_bf16(p(o2), M, H, H, p(k["oT"]), Mp, st))
        _lib.check(lib.hsad_gemm_nt_bf16_splitk(p(k["dzT"]), Mp, p(k["oT"]), Mp, head.NZp, H, Mp, head.wgrad_split, p(k["ws"]), p(head.gw), H, None, st))
        _lib.check(lib.hsad_colsum_acc_ordered(p(k["dz"]), 1, M, head.NZp, head.NZp, p(head.gb), p(k["cs"]), st))

    kinds = {"belief_tail_grad": tail(True), "belief_tail_no_grad": tail(False), "head_forward_gemm": lambda: head.logits(o2, k["z"]),
             "head_wgrad_path": wgrad, "trunk_features": lambda: head.features(data.priv_s_bf16), "loss_with_grad": lambda: head.loss(batch, weight),
             "adam_step": head.step}
    out = {"device": torch.cuda.get_device_name(0), "shape": dict(T=T, B=B, H=H, hand_size=Hs, valid_rows=int(data.seq_len.sum())),
           "windows": args.windows, "calls_per_window": args.calls,
           "note": "us per call, launch overhead included (back-to-back calls on one stream); loss_with_grad = forward GEMM + tail + wgrad path + clones"}
    out.update(timed(kinds, args.windows, args.calls))
    # the two samplers at 4,096 games
    G = 4096
    env = BatchedHanabiEnv(G, seed=11, eps_list=(0.0,), sad=True, device=dev)
    env.rollout_random(14, 5)
    viewer = (torch.arange(G, device=dev) % 2).to(torch.int32)
    key = torch.arange(G, dtype=torch.int64, device=dev)
    z = (torch.randn(G, head.NZp, generator=g) * 2).to(dev)
    counter = [0]

    def det_belief():
        counter[0] += 1
        env.determinize_belief(viewer, z, key, counter[0])

    def det_exact():
        counter[0] += 1
        env.determinize_exact(viewer, key, counter[0])
    out["determinize_at_4096_games"] = dict(timed({"determinize_belief": det_belief, "determinize_exact": det_exact}, args.windows, args.calls),
                                            live_games=int((env.query()[:, 0] == 0).sum()), note="kernel + the observe pass that rewrites the rows")
    env.close()
    for name, teacher, note in (("training_run", W, "init_weights(seed 1), 512 units, playing itself greedily"),
                                ("training_run_piers", PRESETS["piers"], "the piers bot's games through the same random trunk")):
        if args.games <= 0:
            break
        t0 = time.perf_counter()
        records = records_from_teacher([teacher], args.games, 21, True, device=dev, names=[name])
        data = sequences_from_records(records, True, max_len=T, device=dev, knowledge=True)
        head = belief.BeliefHead(W, Hs, dev, lr=1e-3)
        o16 = head.features(data.priv_s_bf16)
        train, held = data.split(0.1, 3)
        games_held = set(held.game.cpu().tolist())
        is_held = torch.tensor([int(x) in games_held for x in data.game.cpu().tolist()], device=o16.device)
        o_train, o_held = o16[:, ~is_held], o16[:, is_held]
        torch.cuda.synchronize()
        setup_s = time.perf_counter() - t0
        epochs = []
        for e in range(args.epochs):
            t0 = time.perf_counter()
            tr = belief.run_epoch(head, train, o_train, B, 100 + e, True)
            ho = belief.run_epoch(head, held, o_held, B, 0, False)
            torch.cuda.synchronize()
            epochs.append(dict(epoch=e, seconds=time.perf_counter() - t0, train_nll_per_card=tr["nll"], train_nll_per_card_exact=tr["nll0"],
                               train_top1=tr["top1"], train_top1_exact=tr["top1_0"], held_nll_per_card=ho["nll"], held_nll_per_card_exact=ho["nll0"],
                               held_top1=ho["top1"], held_top1_exact=ho["top1_0"], held_cards=ho["cards"]))
        out[name] = dict(games=args.games, sequences=data.n_rows, held_out_sequences=held.n_rows, batchsize=B, lr=1e-3, truncated=data.truncated,
                         mean_score=float(sum(r.score for r in records)) / len(records), setup_seconds=setup_s, epochs=epochs, games_of=note)
    line = json.dumps(out, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
