"""Determinised Monte-Carlo action values on the device env (SPARTA-style single-agent search with a random-legal rollout policy):
for the player on turn, every legal action is tried in `worlds` sampled worlds -- the player's own hidden hand resampled from the
hands its card knowledge allows, the deck reshuffled -- and each world is played out to the end.  Built from the env's search
primitives (BatchedHanabiEnv.fork_from / determinize / step / playout_random); the rollouts of all (game, action, world) jobs run
batched in one search env, `capacity` games at a time."""
import numpy as np
import torch

from .env import BatchedHanabiEnv

Q_TERMINATED, Q_CUR_PLAYER, Q_SCORE, Q_STARTED = 0, 1, 2, 14   # include/hsad.h HSAD_Q_*
_M64 = (1 << 64) - 1


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def world_seed(seed, g, w):
    """generator seed (non-negative int32) of world w of root game g: a function of (seed, g, w) alone"""
    return _mix64((seed & _M64) ^ _mix64((g << 32) | w)) & 0x7FFFFFFF


def world_key(g, w):
    """hash key of world w of root game g, shared by the sampler and the rollout policy: (g, w) only, so every action of a game
    is evaluated in the same worlds with the same rollout randomness (common random numbers)"""
    return (int(g) << 32) | int(w)


def search_jobs(root):
    """(game, action) pairs to evaluate: every legal action of the player on turn of every live root game, in (game, action) order;
    also that player per game.  Reads the root's legal_move rows."""
    q = root.query().cpu().numpy()
    live = (q[:, Q_STARTED] == 1) & (q[:, Q_TERMINATED] == 0)
    cur = q[:, Q_CUR_PLAYER].astype(np.int64)
    legal = root.legal_move.cpu().numpy()
    pairs = [(g, a) for g in range(root.G) if live[g] for a in range(root.A) if legal[g, cur[g], a] != 0]
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2), cur


def mc_action_values(root, worlds, seed, capacity=4096, max_iter=None):
    """float32 [G, A] on the root's device: values[g, a] = mean final score (HSAD_Q_SCORE: honours `bomb`) over `worlds` random
    playouts of action a by the player on turn of root game g; NaN for illegal actions and for games that are not live.  The root
    env is only read.  The result does not depend on `capacity` (jobs are keyed by (game, world), never by the slot they run in).
    A world whose sampler gave up (32 rejected tries: not seen in practice) keeps the true hand."""
    G, P, A = root.G, root.P, root.A
    dev = root.device
    values = np.full((G, A), np.nan, dtype=np.float32)
    pairs, cur = search_jobs(root)
    if len(pairs) == 0 or worlds < 1:
        return torch.from_numpy(values).to(dev)
    # jobs in (game, action, world) order
    gj = np.repeat(pairs[:, 0], worlds)
    aj = np.repeat(pairs[:, 1], worlds)
    wj = np.tile(np.arange(worlds, dtype=np.int64), len(pairs))
    n = len(gj)
    if max_iter is None:
        max_iter = root.config["max_len"] if root.config["max_len"] > 0 else 128   # no game of Hanabi is that long
    senv = BatchedHanabiEnv(capacity, seed=0, eps_list=(0.0,), device=str(dev), track_deck_history=False, **root.config)
    scores = np.zeros(n, dtype=np.int64)
    slot = torch.arange(capacity, device=dev)
    try:
        for c0 in range(0, n, capacity):
            m = min(capacity, n - c0)
            j = np.minimum(np.arange(c0, c0 + capacity), n - 1)   # a short last chunk repeats its last job in the spare slots
            g_c, a_c, w_c = gj[j], aj[j], wj[j]
            seeds = np.asarray([world_seed(seed, int(g), int(w)) for g, w in zip(g_c, w_c)], dtype=np.int32)
            key = torch.from_numpy((g_c << 32) | w_c).to(dev)
            p_c = torch.from_numpy(cur[g_c]).to(dev)
            senv.fork_from(root, torch.from_numpy(g_c.astype(np.int32)), torch.from_numpy(seeds))
            senv.determinize(p_c, key, seed)
            act = torch.full((capacity, P), A - 1, dtype=torch.int64, device=dev)   # the noop for the players not on turn
            act[slot, p_c] = torch.from_numpy(a_c).to(dev)
            senv.step(act, act)
            senv.playout_random(max_iter, seed, key=key)
            scores[c0:c0 + m] = senv.query()[:m, Q_SCORE].cpu().numpy()
        senv.check_errors()
    finally:
        senv.close()
    mean = (scores.reshape(len(pairs), worlds).sum(axis=1).astype(np.float32) / np.float32(worlds)).astype(np.float32)
    values[pairs[:, 0], pairs[:, 1]] = mean
    return torch.from_numpy(values).to(dev)


def mc_greedy_action(values):
    """int64 [G]: the action with the highest value per game (lowest uid on ties), -1 where every entry is NaN"""
    v = torch.as_tensor(values)
    filled = torch.where(torch.isnan(v), torch.full_like(v, -float("inf")), v)
    best = filled.argmax(dim=1)
    return torch.where(torch.isnan(v).all(dim=1), torch.full_like(best, -1), best)
