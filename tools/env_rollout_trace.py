"""Per-iteration trace of one persistent rollout launch at configs[1] (65,536 two-player games): where each workgroup's time goes,
and how many workgroups stream observations on each CU and on the chip over time.

  python tools/env_rollout_trace.py [--iters 20] [--warmup 5] [--schedule pipe|single] [--pace on|off] [--delta on|off] [--compact on|off] [--unit 128|64] [--chain 0|1] [--launches N] [--prio 0..3] [--json OUT]

The driver's shape is --warmup 5 --iters 20 (one 5-iteration launch, then the traced 20-iteration launch).  --schedule single runs
env_rollout_kernel (HSAD_ENV_PIPE=0), pipe the default env_rollout_pipe_kernel.  Stamps are wall_clock64 (100 MHz, 10 ns) of
hsad_env_debug_trace; slot map in csrc/hsad_env.hip (env_stamp).  Streaming intervals: single-phase = [write-back done, rows streamed]
of each iteration; pipelined = [iteration start, stream wave done] of iterations 1.. (the rows of the previous one) plus the epilogue.

Who lags: every workgroup's rate (us per iteration over the steady part of the launch, iteration 1 to the last start) is grouped by
where the workgroup runs (XCC; SE; SH; CU = the four co-resident workgroups) and by where it writes (octile of the block index =
position of its rows in the output buffers); per grouping the spread between the group means is set against the spread inside the
groups (`share_of_variance_between_groups` is the usual eta squared).  --pace off traces the unpaced launch (HSAD_ENV_PACE=0); with
pacing on, `pace` says how many iterations delayed their stream and by how much (--l0-q8 / --cap-us: the developer switches
HSAD_ENV_PACE_L0_Q8 / HSAD_ENV_PACE_CAP_US).  The pipelined kernel's trace also carries the stream wave's HW_ID: the groupings then
include the workgroup's start rank among the workgroups of its CU, the SIMD and wave slot of either wave, and the co-tenant class
of either wave (who shares its SIMD, and which of the two workgroups started first); every grouping also splits the variance of
the workgroups' end times.  --prio sets the wave-priority mode (HSAD_ENV_PRIO).  --delta off traces the full observation stream (HSAD_ENV_DELTA=0),
--compact off the direct form of the delta stream (HSAD_ENV_COMPACT=0), --unit the bytes the compacted form decides "changed" by
(HSAD_ENV_UNIT; default: the library's).  `stored` gives what the stream wave stored per workgroup-iteration: 128-byte lines with any
change (slot 13) and, where the library has hsad_env_debug_units, the units themselves and their bytes.

--launches N makes the traced call N launches of --iters iterations each (the trace holds the last one, which with --chain 1,
HSAD_ENV_CHAIN, takes its predecessor's last rows from the env's carry buffer; the launches before it also hand over, which
costs them the copy after their epilogue and does not show in the last one's trace).  `edges` says what of the traced launch is
not its steady iteration: launch start to first iteration start, iterations 0 and 1, the epilogue, and the spread of the
workgroups' end times with its share between XCCs.

`reset_iterations` splits the logic wave's time in the workgroup-iterations whose lane 0 restarted its game (the only ones that carry
the reset stamps 6 / 7): the wait for the mt19937 window, the deal, and the rest (eps, colour shuffle, policy and step)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TICK_US = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--schedule", choices=("pipe", "single"), default="pipe")
    ap.add_argument("--pace", choices=("on", "off"), default="on")
    ap.add_argument("--delta", choices=("on", "off"), default="on")
    ap.add_argument("--compact", choices=("on", "off"), default="on")
    ap.add_argument("--unit", type=int, choices=(128, 64), default=None)
    ap.add_argument("--l0-q8", type=int, default=None)
    ap.add_argument("--cap-us", type=int, default=None)
    ap.add_argument("--chain", type=int, choices=(0, 1), default=None)
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("--prio", type=int, choices=(0, 1, 2, 3), default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.chain is not None:
        os.environ["HSAD_ENV_CHAIN"] = str(args.chain)
    os.environ["HSAD_ENV_PIPE"] = "1" if args.schedule == "pipe" else "0"
    os.environ["HSAD_ENV_PACE"] = "1" if args.pace == "on" else "0"
    os.environ["HSAD_ENV_DELTA"] = "1" if args.delta == "on" else "0"
    os.environ["HSAD_ENV_COMPACT"] = "1" if args.compact == "on" else "0"
    if args.unit is not None:
        os.environ["HSAD_ENV_UNIT"] = str(args.unit)
    if args.prio is not None:
        os.environ["HSAD_ENV_PRIO"] = str(args.prio)
    if args.l0_q8 is not None:
        os.environ["HSAD_ENV_PACE_L0_Q8"] = str(args.l0_q8)
    if args.cap_us is not None:
        os.environ["HSAD_ENV_PACE_CAP_US"] = str(args.cap_us)
    import torch
    from hanabi_sad_amd import BatchedHanabiEnv, _lib
    G = 65536
    eps = [0.1 ** (1 + 7 * i / 79) for i in range(80)]
    env = BatchedHanabiEnv(G, seed=1, eps_list=eps, device="cuda:0", track_deck_history=False)
    env.set_rollout_chunk(max(50, args.iters) if args.launches == 1 else args.iters)
    assert env.threads_per_workgroup == 128
    nwg = (G + env.games_per_workgroup - 1) // env.games_per_workgroup
    env.rollout_random(args.warmup, 12345)
    buf = torch.zeros(nwg * args.iters * 16, dtype=torch.int64, device="cuda:0")
    has_units = hasattr(env.lib, "hsad_env_debug_units")
    ubuf = torch.zeros(nwg * args.iters, dtype=torch.int64, device="cuda:0") if has_units else None
    torch.cuda.synchronize()
    _lib.check(env.lib.hsad_env_debug_trace(env.h, buf.data_ptr(), args.iters))
    if has_units:
        _lib.check(env.lib.hsad_env_debug_units(env.h, ubuf.data_ptr()))
    env.rollout_random(args.iters * args.launches, 12345)          # the trace holds the last launch of the call
    torch.cuda.synchronize()
    if has_units:
        _lib.check(env.lib.hsad_env_debug_units(env.h, None))
    _lib.check(env.lib.hsad_env_debug_trace(env.h, None, 0))
    env.check_errors()
    s = buf.view(nwg, args.iters, 16).cpu().numpy().astype(np.int64)
    rec = analyse(s, args.schedule == "pipe", args)
    if args.schedule == "pipe" and args.iters > 2:
        lines = s[:, 2:, 13]                                         # records 2..: the delta streams (record 1 stores everything)
        rec["stored"] = {"lines_with_any_change_mean": round(float(lines.mean()), 1)}
        if has_units:
            unit = env.rollout_unit()
            u = ubuf.view(nwg, args.iters).cpu().numpy()[:, 2:]
            rec["stored"].update(unit_bytes=unit, units_mean=round(float(u.mean()), 1),
                                 priv_s_bytes_per_iteration=int(round(float(u.sum(axis=0).mean()) * unit)))
            rec["rollout_unit"] = unit
            # record 1: the launch's first stream (everything, counted in lines; a chained launch: what changed, in units)
            rec["stored"]["first_stream_units_mean"] = round(float(ubuf.view(nwg, args.iters).cpu().numpy()[:, 1].mean()), 1)
    rec["launches_in_the_traced_call"] = args.launches
    if hasattr(env.lib, "hsad_env_rollout_chain_active"):
        rec["chain_mode_active"] = env.rollout_chain_active()
    if hasattr(env.lib, "hsad_env_rollout_prio"):
        rec["prio_mode"] = env.rollout_prio()
    rec["delta_stream_active"] = bool(env.rollout_delta_active())
    rec["compact_stream_active"] = bool(env.rollout_compact_active())
    rec["pace"] = dict(rec.get("pace", {}), on=args.pace == "on", cap_us=env.rollout_pace_cap_us(),
                       l0_q8=args.l0_q8 if args.l0_q8 is not None else "default")
    print(json.dumps(rec, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


def analyse(s, pipe, args):
    nwg, n, _ = s.shape
    t0 = s[:, 0, 0].min()
    t = (s[:, :, :9] - t0).astype(np.float64) * TICK_US            # µs since the first workgroup started
    t = np.concatenate([t, (s[:, :, 11:12] - t0) * TICK_US], axis=2)  # slot 11 -> column 9
    hw, xcc = s[:, 0, 9], s[:, 0, 10]
    cu = ((xcc & 0xF) << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xF)   # XCC, SE, SH, CU
    rec = {"schedule": "env_rollout_pipe_kernel<2,5>" if pipe else "env_rollout_kernel<2,5>", "iters": n, "warmup": args.warmup,
           "workgroups": nwg, "cus_seen": int(len(np.unique(cu)))}
    it_len = np.diff(t[:, :, 0], axis=1)                            # start(k+1) - start(k)
    med = lambda a: float(np.median(a))
    if pipe:
        # phase A: [0,1] drain, [1,11] logic, [11,2] wait for the stream wave; phase B: [2,3] build, [3,4] refill + scalars + barrier
        ph = {"drain_us": t[:, :, 1] - t[:, :, 0], "logic_us": t[:, :, 9] - t[:, :, 1], "wait_for_stream_wave_us": t[:, :, 2] - t[:, :, 9],
              "build_us": t[:, :, 3] - t[:, :, 2], "phase_b_rest_us": t[:, :, 4] - t[:, :, 3]}
        ph["stream_wave_stream_clear_us"] = (t[:, 1:, 8] - t[:, 1:, 0])
        streams = [(t[:, k, 0], t[:, k, 8]) for k in range(1, n)] + [(t[:, n - 1, 4], t[:, n - 1, 5])]
        end = t[:, n - 1, 5]
        # slots 6 / 7 are stamped by thread 0 inside its reset branch only: non-zero where lane 0's game restarted in that iteration
        rs = s[:, 1:, 6] != 0
        tick = lambda a, b: (s[:, 1:, a] - s[:, 1:, b])[rs].astype(np.float64) * TICK_US
        if rs.any():
            rec["reset_iterations"] = {"share_of_workgroup_iterations": round(float(rs.mean()), 4),
                                       "window_loaded_minus_drained_us": round(med(tick(6, 1)), 2),
                                       "dealt_minus_window_loaded_us": round(med(tick(7, 6)), 2),
                                       "logic_done_minus_dealt_us": round(med(tick(11, 7)), 2),
                                       "logic_us": round(med(tick(11, 1)), 2),
                                       "logic_us_without_lane0_reset": round(med((s[:, 1:, 11] - s[:, 1:, 1])[~rs] * TICK_US), 2)}
    else:
        ph = {"load_planes_incl_drain_us": t[:, :, 1] - t[:, :, 0], "logic_us": t[:, :, 2] - t[:, :, 1], "build_us": t[:, :, 3] - t[:, :, 2],
              "write_back_us": t[:, :, 4] - t[:, :, 3], "stream_us": t[:, :, 5] - t[:, :, 4]}
        streams = [(t[:, k, 4], t[:, k, 5]) for k in range(n)]
        end = t[:, n - 1, 5]
    rec["median_per_workgroup_iteration"] = {k: round(med(np.median(v[:, 1:] if v.shape[1] > 1 else v, axis=1)), 2) for k, v in ph.items()}
    rec["iteration_us_median"] = round(med(it_len), 2) if n > 1 else None
    rec["launch_us"] = round(float(end.max()), 1)
    rec["start_spread_us"] = round(float(t[:, 0, 0].max() - t[:, 0, 0].min()), 2)
    rec["end_spread_us"] = round(float(end.max() - end.min()), 2)
    if n > 2:
        # the pipelined kernel packs the stream wave's HW_ID into the upper half of slot 10 (0 from a library that does not)
        hw_stream = (xcc >> 32) & 0xFFFFFFFF
        rec["who_lags"] = who_lags(t, hw, xcc, cu, hw_stream if pipe and hw_stream.any() else None, end)
    if pipe and n > 3:
        rec["edges"] = edges(t, xcc)
    if pipe:
        d = s[:, :n - 1, 12].astype(np.float64) * TICK_US          # delay decided in iteration k = of the stream in k + 1
        rec["pace"] = {"share_of_iterations_that_slept": round(float((d > 0).mean()), 4),
                       "share_of_workgroups_that_ever_slept": round(float((d > 0).any(axis=1).mean()), 4),
                       "sleep_us_mean_when_slept": round(float(d[d > 0].mean()), 2) if (d > 0).any() else 0.0,
                       "sleep_us_total_per_workgroup_mean": round(float(d.sum(axis=1).mean()), 2),
                       "sleep_us_total_per_workgroup_max": round(float(d.sum(axis=1).max()), 2)}
    # streaming workgroups over time, 0.5 µs bins, chip-wide and per CU
    T = float(end.max())
    nb = int(T / 0.5) + 1
    chip = np.zeros(nb)
    per_cu = {}
    for a, b in streams:
        for w in range(nwg):
            i0, i1 = int(a[w] / 0.5), int(b[w] / 0.5)
            chip[i0:i1 + 1] += 1
            per_cu.setdefault(int(cu[w]), np.zeros(nb))[i0:i1 + 1] += 1
    steady = slice(int(t[:, 0, 0].max() / 0.5) + 1, int(end.min() / 0.5))   # every workgroup started, none finished
    share = np.zeros(4)
    for c, v in per_cu.items():
        vv = np.minimum(v[steady], 3).astype(int)
        share += np.bincount(vv, minlength=4)[:4]
    share /= max(share.sum(), 1)
    rec["per_cu_share_of_steady_time_with_0_1_2_3plus_streaming"] = [round(float(x), 3) for x in share]
    cs = chip[steady]
    rec["chip_streaming_workgroups_steady"] = {"mean": round(float(cs.mean()), 1), "p5": float(np.percentile(cs, 5)),
                                               "p50": float(np.percentile(cs, 50)), "p95": float(np.percentile(cs, 95))}
    step = max(1, nb // 40)
    rec["chip_streaming_workgroups_series"] = {"bin_us": 0.5 * step, "values": [int(chip[i:i + step].mean()) for i in range(0, nb, step)]}
    return rec


def edges(t, xcc):
    """what of a pipelined launch is not its steady iteration: medians over workgroups, µs.  t: [workgroup, iteration, column] as in
    analyse (columns = slots 0-8, column 9 = slot 11), relative to the first workgroup's first stamp, which stands for the launch's
    start (the kernel has no stamp before its prologue)."""
    nwg, n = t.shape[0], t.shape[1]
    med = lambda a: round(float(np.median(a)), 2)
    start, end = t[:, 0, 0], t[:, n - 1, 5]
    steady = np.median(np.diff(t[:, 2:, 0], axis=1), axis=1) if n > 3 else np.diff(t[:, 1:3, 0], axis=1)[:, 0]   # iterations 2 .. n - 2
    out = {"launch_start_to_first_iteration_start_us": med(start),
           "iteration_0_us": med(t[:, 1, 0] - t[:, 0, 0]),
           "iteration_0_phase_a_us": med(t[:, 0, 2] - t[:, 0, 0]), "iteration_0_phase_b_us": med(t[:, 0, 4] - t[:, 0, 2]),
           "iteration_1_us": med(t[:, 2, 0] - t[:, 1, 0]),
           "iteration_1_stream_and_clear_us": med(t[:, 1, 8] - t[:, 1, 0]),
           "iteration_1_phase_a_us": med(t[:, 1, 2] - t[:, 1, 0]), "iteration_1_phase_b_us": med(t[:, 1, 4] - t[:, 1, 2]),
           "steady_iteration_us": med(steady),
           "epilogue_us": med(end - t[:, n - 1, 4]),
           "end_us_first_median_last": [round(float(end.min()), 1), med(end), round(float(end.max()), 1)],
           "workgroup_time_not_n_times_its_steady_iteration_us": med((end - start) - n * steady),
           "launch_us": round(float(end.max()), 1)}
    out["launch_not_n_times_the_steady_iteration_us"] = round(out["launch_us"] - n * out["steady_iteration_us"], 1)
    out["tail_last_end_minus_median_end_us"] = round(float(end.max() - np.median(end)), 1)
    x = xcc & 0xF
    ids = np.unique(x)
    within = float(sum(((end[x == i] - end[x == i].mean()) ** 2).sum() for i in ids))
    total = float(((end - end.mean()) ** 2).sum())
    out["end_us_median_by_xcc"] = {str(int(i)): round(float(np.median(end[x == i])), 1) for i in ids}
    out["end_us_last_by_xcc"] = {str(int(i)): round(float(end[x == i].max()), 1) for i in ids}
    out["end_share_of_variance_between_xccs"] = round(1.0 - within / total, 4) if total > 0 else None
    return out


def co_tenants(cu, start, simd_logic, simd_stream):
    """Per workgroup, for its logic wave and for its stream wave: who shares the wave's SIMD among the waves of the workgroups on the
    same CU, and whether this wave's workgroup started before or after the other's.  Returns two integer arrays and the class
    names they index.  `own_...`: the other wave of the same workgroup; `several`: more than one co-tenant (more than two waves on
    the SIMD: not the placement the kernel is scheduled for)."""
    names = ["alone", "several", "own_logic", "own_stream", "logic_of_a_workgroup_started_before", "logic_of_a_workgroup_started_after",
             "stream_of_a_workgroup_started_before", "stream_of_a_workgroup_started_after"]
    nwg = len(cu)
    out = np.zeros((2, nwg), dtype=np.int64)
    for c in np.unique(cu):
        idx = np.nonzero(cu == c)[0]
        waves = [(w, role, int((simd_logic, simd_stream)[role][w])) for w in idx for role in (0, 1)]   # role 0 logic, 1 stream
        for w, role, simd in waves:
            others = [(v, r) for v, r, s in waves if s == simd and (v, r) != (w, role)]
            if not others:
                k = "alone"
            elif len(others) > 1:
                k = "several"
            else:
                v, r = others[0]
                what = ("logic", "stream")[r]
                k = "own_" + what if v == w else "%s_of_a_workgroup_started_%s" % (what, "before" if (start[v], v) < (start[w], w) else "after")
            out[role, w] = names.index(k)
    return out[0], out[1], names


def who_lags(t, hw, xcc, cu, hw_stream=None, end=None):
    """per-workgroup rate, grouped by place of execution and by place in the output buffers; with the stream wave's HW_ID (the
    pipelined kernel's trace) also by dispatch order inside the CU, by the SIMDs the two waves took and by who shares them.  `end`:
    the workgroups' end times, whose variance is split by the same groupings."""
    nwg, n = t.shape[0], t.shape[1]
    rate = (t[:, n - 1, 0] - t[:, 1, 0]) / (n - 2)                    # us per iteration, iteration 1 .. start of the last
    se, sh = (hw >> 13) & 7, (hw >> 12) & 1
    keys = {"xcc": xcc & 0xF, "se": se, "xcc_se": ((xcc & 0xF) << 3) | se, "xcc_se_sh": ((xcc & 0xF) << 4) | (se << 1) | sh,
            "cu_co_resident_workgroups": cu, "block_index_octile": np.arange(nwg) * 8 // nwg}
    labels = {}
    placement = None
    if hw_stream is not None:
        start = t[:, 0, 0]
        rank = np.zeros(nwg, dtype=np.int64)                         # 0 = the first workgroup of its CU to start
        for c in np.unique(cu):
            idx = np.nonzero(cu == c)[0]
            rank[idx[np.lexsort((idx, start[idx]))]] = np.arange(len(idx))
        simd_l, simd_s = (hw >> 4) & 3, (hw_stream >> 4) & 3
        slot_l, slot_s = hw & 0xF, hw_stream & 0xF
        co_l, co_s, names = co_tenants(cu, start, simd_l, simd_s)
        keys.update({"start_rank_in_cu": rank, "logic_wave_simd": simd_l, "stream_wave_simd": simd_s,
                     "simd_pair_logic_stream": simd_l * 4 + simd_s, "logic_wave_slot": slot_l, "stream_wave_slot": slot_s,
                     "logic_wave_co_tenant": co_l, "stream_wave_co_tenant": co_s})
        labels = {"logic_wave_co_tenant": names, "stream_wave_co_tenant": names,
                  "simd_pair_logic_stream": ["%d_%d" % (a, b) for a in range(4) for b in range(4)]}
        per_cu = np.array([(cu == c).sum() for c in np.unique(cu)])
        # does alternation have something to work with: co-tenant pairs (a stream wave and its one co-tenant) whose slots differ in bit 0
        placement = {"workgroups_per_cu_min_max": [int(per_cu.min()), int(per_cu.max())],
                     "share_of_workgroups_with_both_waves_on_one_simd": round(float((simd_l == simd_s).mean()), 4),
                     "share_of_workgroups_on_simds_0_1_or_2_3": round(float(((simd_l ^ simd_s) == 1).mean()), 4),
                     "share_of_workgroups_whose_waves_have_the_same_slot": round(float((slot_l == slot_s).mean()), 4),
                     "wave_slots_seen": sorted(int(x) for x in np.unique(np.concatenate([slot_l, slot_s])))}
    out = {"rate_us_per_iteration": {"mean": round(float(rate.mean()), 2), "std": round(float(rate.std()), 2),
                                     "min": round(float(rate.min()), 2), "p5": round(float(np.percentile(rate, 5)), 2),
                                     "p50": round(float(np.median(rate)), 2), "p95": round(float(np.percentile(rate, 95)), 2),
                                     "max": round(float(rate.max()), 2)}, "groupings": {}}
    if placement is not None:
        out["placement"] = placement
    total = float(((rate - rate.mean()) ** 2).sum())
    end_total = float(((end - end.mean()) ** 2).sum()) if end is not None else 0.0
    for name, key in keys.items():
        ids = np.unique(key)
        means = np.array([rate[key == i].mean() for i in ids])
        sizes = np.array([(key == i).sum() for i in ids])
        within = float(sum(((rate[key == i] - rate[key == i].mean()) ** 2).sum() for i in ids))
        g = {"groups": int(len(ids)), "group_size_min_max": [int(sizes.min()), int(sizes.max())],
             "between_group_means_std_us": round(float(np.sqrt((sizes * (means - rate.mean()) ** 2).sum() / nwg)), 3),
             "within_groups_std_us": round(float(np.sqrt(within / nwg)), 3),
             "share_of_variance_between_groups": round(1.0 - within / total, 4) if total > 0 else None,
             "group_means_min_max_us": [round(float(means.min()), 2), round(float(means.max()), 2)]}
        label = (lambda i: labels[name][int(i)]) if name in labels else (lambda i: str(int(i)))
        if len(ids) <= 16:
            g["group_means_us"] = {label(i): round(float(m), 2) for i, m in zip(ids, means)}
            if name in labels:
                g["group_sizes"] = {label(i): int(z) for i, z in zip(ids, sizes)}
        if end is not None:
            end_within = float(sum(((end[key == i] - end[key == i].mean()) ** 2).sum() for i in ids))
            g["end_share_of_variance_between_groups"] = round(1.0 - end_within / end_total, 4) if end_total > 0 else None
            if len(ids) <= 16:
                g["end_group_means_us"] = {label(i): round(float(end[key == i].mean()), 1) for i in ids}
        out["groupings"][name] = g
    return out


if __name__ == "__main__":
    main()
