"""A numpy restatement of hanabi_sad_amd/csrc/hsad_search_horizon.h: what one slot of a depth-limited search is worth at its horizon,
in 1/256 points, and the per-job reduction of hsad_search_horizon_stats.  Written from the specification in include/hsad.h; shared by
test_search_horizon_cpu.py (the header under the sanitizers) and test_search_horizon_gpu.py (the kernel, the search)."""
import numpy as np

SCALE = 256                     # HSAD_SEARCH_VALUE_SCALE
MOVER, TEAM = 0, 1              # HSAD_SEARCH_HORIZON_*
NOT_PLAYED = 0xFFFF
f32 = np.float32


def bootstrap(q):
    """(b int64, nonfinite bool) of fp32 q: b = (int)rintf(min(max(q, -64), 64) * 256), round-half-even; 0 where q is not finite"""
    q = np.asarray(q, dtype=f32)
    ok = np.isfinite(q)
    c = np.clip(np.where(ok, q, f32(0)), f32(-64), f32(64)).astype(f32)
    return np.rint(c * f32(SCALE)).astype(np.int64), ~ok


def team_q(q_rows):
    """fp32 sum over the last axis in seat order 0 .. P - 1, one rounding per addition"""
    q_rows = np.asarray(q_rows, dtype=f32)
    with np.errstate(all="ignore"):
        s = q_rows[..., 0].copy()
        for p in range(1, q_rows.shape[-1]):
            s = (s + q_rows[..., p]).astype(f32)
    return s


def slot_values(started, finished, last_score, fireworks_sum, num_step, q_rows, mode, perfect_score):
    """per slot: started / finished bool [G] (finished = started and terminated), last_score = the latched score, fireworks_sum = the
    sum of the board's fireworks, num_step = the env's step counter, q_rows float32 [G, P]
    -> (v int64 [G], counted, cut, nonfinite bool [G])"""
    started, finished = np.asarray(started, dtype=bool), np.asarray(finished, dtype=bool)
    q_rows = np.asarray(q_rows, dtype=f32)
    G, P = q_rows.shape
    live = started & ~finished
    q = team_q(q_rows) if mode == TEAM else q_rows[np.arange(G), np.asarray(num_step, dtype=np.int64) % P]
    b, bad = bootstrap(q)
    v_live = np.clip(np.asarray(fireworks_sum, dtype=np.int64) * SCALE + b, 0, int(perfect_score) * SCALE)
    v = np.where(finished, np.asarray(last_score, dtype=np.int64) * SCALE, np.where(live, v_live, 0))
    return v, started, live, live & bad


def job_reduce(v, counted, cut, nonfinite, job, n_job, world=None, worlds=0, out=None):
    """hsad_search_horizon_stats' reduction, accumulating into out = (stats int64 [n_job, 3], cut int64 [n_job], nonfinite int64 [1],
    world_values uint16 [n_job, worlds] or None); None makes zeroed tables (world_values 0xFFFF) -> out"""
    if out is None:
        out = (np.zeros((n_job, 3), dtype=np.int64), np.zeros(n_job, dtype=np.int64), np.zeros(1, dtype=np.int64),
               np.full((n_job, worlds), NOT_PLAYED, dtype=np.uint16) if world is not None else None)
    stats, cuts, bad, table = out
    for g in range(len(v)):
        j = int(job[g])
        if not 0 <= j < n_job or not counted[g]:
            continue
        stats[j] += (int(v[g]), int(v[g]) * int(v[g]), 1)
        cuts[j] += int(cut[g])
        bad[0] += int(nonfinite[g])
        if table is not None and 0 <= int(world[g]) < worlds:
            table[j, int(world[g])] = int(v[g]) & 0xFFFF
    return out


def from_query(q, q_rows, mode, perfect_score):
    """slot_values from the rows of BatchedHanabiEnv.query() (HSAD_Q_*: terminated 0, score 2, last_score 5, num_step 6, fireworks 8..12,
    started 14) as a numpy array [G, 16]"""
    started = q[:, 14] == 1
    finished = started & (q[:, 0] == 1)
    return slot_values(started, finished, q[:, 5], q[:, 8:13].sum(axis=1), q[:, 6], q_rows, mode, perfect_score)
