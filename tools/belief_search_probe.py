"""The learned belief in the searches, timed (profiles/belief_search_probe.json), all in one process:
  - at 4,096 games, determinize_belief_worlds (8 worlds per group of 8 slots, logits by a row index) next to determinize_belief and
    determinize_exact -- the baseline is determinize_belief in the same run: the new kernel does the same bh_row work plus the hashes
    of the stratified uniforms;
  - one searched move of 64 root games with 8 worlds per action at capacity 4,096, sampler="learned" next to sampler="stratified"
    (PolicySearch.search, the search env kept across calls), with the sampler call's own time per 4,096-slot chunk and the time of the
    logits (hsad_search_belief_rows + the head's GEMM), so that the sampler's share of a searched move can be read off.
  - with --quality_games N, one small quality loop as a single run (quality_loop: clone `piers`, fit a head, play N deals with search,
    stratified against learned); its two training commands print their epoch lines before the JSON line.
The timed blueprint is a random 512-unit net (its games end after a few moves): what is timed is the machinery, not a trained policy.
us / ms from a host clock around windows that end in a device synchronise, the kinds alternating window by window; medians with the
spread, as tools/belief_probe.py reports them.  One JSON line (and --out FILE).  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hanabi_sad_amd import BatchedHanabiEnv                  # noqa: E402
from hanabi_sad_amd import belief                            # noqa: E402
from hanabi_sad_amd.composite import CNet, CompositeAgent    # noqa: E402
from hanabi_sad_amd.search import PolicySearch               # noqa: E402
from hanabi_sad_amd.selfplay import init_weights             # noqa: E402


def timed(kinds, windows, calls):
    for fn in kinds.values():
        for _ in range(2):
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


def quality_loop(games, worlds, dev):
    """one small quality loop, a single run: clone `piers` (2,000 games, 12 epochs), fit a head on the clone's trunk to 2,000 more `piers`
    games (8 epochs), then play the clone over the same `games` deals without search and with search, stratified and learned, at equal
    worlds -> mean +- SEM per arm and of the deal-by-deal difference.  A weak clone and a head that barely beats the exact belief: no
    claim about a trained blueprint."""
    import tempfile
    from hanabi_sad_amd import clone
    from hanabi_sad_amd.checkpoint import load_weights
    from hanabi_sad_amd.search import play_with_search
    tmp = tempfile.mkdtemp()
    clone.main(["--teacher", "piers", "--num_game", "2000", "--num_epoch", "12", "--lr", "5e-4", "--sad", "1", "--save_dir", tmp + "/clone",
                "--num_eval_game", "200", "--train_device", dev])
    belief.main(["--blueprint", tmp + "/clone/clone.pthw", "--teacher", "piers", "--num_game", "2000", "--num_epoch", "8", "--sad", "1",
                 "--save_dir", tmp + "/belief", "--seed", "20002", "--train_device", dev])
    weights = load_weights(tmp + "/clone/clone.pthw")
    res, scores = dict(games=games, worlds=worlds, deal_seed=50001, search_seed=5), {}
    for arm in ("blueprint", "stratified", "learned"):
        kw = dict(worlds=0) if arm == "blueprint" else dict(worlds=worlds, sampler=arm, search_seed=5, capacity=4096)
        if arm == "learned":
            kw["belief"] = tmp + "/belief/belief.pthw"
        r = play_with_search(weights, games, 50001, 0, True, device=dev, **kw)
        scores[arm] = np.asarray(r.scores, dtype=np.float64)
        res[arm] = dict(mean=r.mean, sem=r.sem, deviations_per_game=float(r.deviations.double().mean()))
    d = scores["learned"] - scores["stratified"]
    res["learned_minus_stratified"] = dict(mean=float(d.mean()), sem=float(d.std() / np.sqrt(len(d))))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality_games", type=int, default=0, help="> 0: also run the small quality loop over this many deals (quality_loop)")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--search_windows", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    dev = "cuda:0"
    H, Hs, W = 512, 5, 8
    gen = torch.Generator().manual_seed(2)
    sd = {"belief.weight": torch.randn(25 * Hs, H, generator=gen) * 0.05, "belief.bias": torch.randn(25 * Hs, generator=gen) * 0.5,
          "hand_size": Hs, "H": H}
    sampler = belief.BeliefSampler(sd, dev)
    out = {"device": torch.cuda.get_device_name(0), "windows": args.windows, "calls_per_window": args.calls,
           "note": "us per call, launch overhead included (back-to-back calls on one stream)"}
    # ---- the samplers at 4,096 games ----
    G = 4096
    env = BatchedHanabiEnv(G, seed=11, eps_list=(0.0,), sad=True, device=dev)
    env.rollout_random(14, 5)
    viewer = (torch.arange(G, device=dev) % 2).to(torch.int32)
    key = torch.arange(G, dtype=torch.int64, device=dev)
    z = (torch.randn(G, sampler.NZp, generator=gen) * 2).to(dev)
    row = (torch.arange(G, device=dev) // W).to(torch.int32)           # 512 logits rows, each read by the 8 slots of its group
    group = (torch.arange(G, device=dev) // W).to(torch.int64) << 32
    world = (torch.arange(G, device=dev) % W).to(torch.int32)
    counter = [0]

    def det_worlds():
        counter[0] += 1
        env.determinize_belief_worlds(viewer, z, row, group, world, W, counter[0])

    def det_belief():
        counter[0] += 1
        env.determinize_belief(viewer, z, key, counter[0])

    def det_exact():
        counter[0] += 1
        env.determinize_exact(viewer, key, counter[0])
    out["determinize_at_4096_games"] = dict(
        timed({"determinize_belief_worlds": det_worlds, "determinize_belief": det_belief, "determinize_exact": det_exact}, args.windows, args.calls),
        live_games=int((env.query()[:, 0] == 0).sum()), n_worlds=W, note="kernel + the observe pass that rewrites the rows")
    env.close()
    # ---- one searched move ----
    Gr, cap = 64, 4096
    root = BatchedHanabiEnv(Gr, players=2, seed=17, bomb=0, eps_list=[0.0], max_len=-1, sad=True, device=dev, track_deck_history=False)
    root.reset()
    net = CNet(init_weights(root.F, H, root.A, Hs, 1), dev)
    agent = CompositeAgent(net, net, 1, 0.99)
    N = Gr * root.P
    obs = lambda: {"priv_s": root.priv_s.view(N, root.F), "legal_move": root.legal_move.view(N, root.A),      # noqa: E731
                   "eps": torch.zeros(N, device=dev)}
    hid = agent.get_h0(N)
    for _ in range(3):
        reply, hid = agent.act(obs(), hid)
        root.step(reply["a"].view(Gr, root.P).contiguous(), reply["greedy_a"].view(Gr, root.P).contiguous())
    hid = {"h0": hid["h0"].contiguous(), "c0": hid["c0"].contiguous()}
    _, nxt = agent.act(obs(), hid)
    searches = {"learned": PolicySearch(root, agent, cap, sampler="learned", belief=sampler),
                "stratified": PolicySearch(root, agent, cap, sampler="stratified")}
    seed = [0]
    info = {}

    def run(name):
        def fn():
            seed[0] += 1
            ps = searches[name]
            sv = ps.search(root, hid, W, seed[0], hid_next=nxt if name == "learned" else None)
            info[name] = dict(jobs=int(sv.totals[..., 2].sum()), env_steps=ps.iterations, chunks=-(-int(sv.totals[..., 2].sum()) // cap))
        return fn
    t = timed({name: run(name) for name in searches}, args.search_windows, 1)
    player = root.query()[:, 1].to(torch.int32).contiguous()
    h_top = nxt["h0"][-1].contiguous()
    parts = timed({"belief_logits": lambda: sampler.logits(h_top, player)}, args.windows, args.calls)
    # the sampler call of one full chunk of the search env, as _sample_hands issues it
    senv = searches["learned"].env
    logits = sampler.logits(h_top, player)
    src = (torch.arange(cap, device=dev) % Gr).to(torch.int32)
    s_viewer = player[src.long()].contiguous()
    s_world = ((torch.arange(cap, device=dev) // Gr) % W).to(torch.int32)
    s_group = src.to(torch.int64) << 32
    s_key = s_group | s_world.to(torch.int64)

    def chunk_learned():
        seed[0] += 1
        senv.determinize_belief_worlds(s_viewer, logits, src, s_group, s_world, W, seed[0])

    def chunk_stratified():
        seed[0] += 1
        senv.determinize_exact(s_viewer, s_key, seed[0], stratum=s_world, n_strata=W)
    senv.fork_from(root, src, torch.from_numpy(np.arange(cap, dtype=np.int32)))
    parts.update(timed({"sampler_chunk_learned": chunk_learned, "sampler_chunk_stratified": chunk_stratified}, args.windows, args.calls))
    out["searched_move"] = dict(root_games=Gr, worlds=W, capacity=cap, hidden=H, search_windows=args.search_windows,
                                search={k: dict(v, **info[k]) for k, v in t.items()}, parts=parts,
                                note="search: us per PolicySearch.search call (host loop included); parts: us per call; the learned search "
                                     "adds belief_logits once per call and one sampler_chunk_learned per chunk")
    for ps in searches.values():
        ps.close()
    root.close()
    if args.quality_games > 0:
        out["quality_loop"] = quality_loop(args.quality_games, W, dev)
    line = json.dumps(out, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
