"""Behaviour cloning: fit the R2D2 net to recorded games (game_record.GameRecord) on the device.

  records_from_teacher     play the games to clone: eval.play_seatings(records=True) with rule bots, networks or both in the seats
  sequences_from_records   records -> the observation sequences of every seat: game_record.replay(stop=0), then one env.step per move
                           with the recorded move and its recorded greedy alternative (the deals come from the record's deck script)
  CloneDataset             those sequences; split(holdout, seed) by game, batches(rows, seed) of a fixed row count
  CompositeLearner.clone_loss (composite.py) is the update: cross-entropy of the recorded move under softmax over the legal
  advantages (hsad_r2d2_clone_fwd), BPTT and Adam as in the TD learner.  The greedy policy of the fitted net is what every consumer of
  an R2D2 weight file plays: eval.evaluate, eval_model --cross_play, actor.NetPartner, search's blueprint, selfplay --load_model.
  The value head gets no gradient from cloning -- unless the value term is asked for (--value_weight W > 0): then the dataset carries
  the discounted return-to-go of every recorded game (returns_to_go, sequences_from_records(gamma=...)) and the update also regresses
  Q(o_t, a_t) on it (hsad_r2d2_clone_value_fwd), so that the cloned net's Q-values are on the scale TD training continues from.

    python -m hanabi_sad_amd.clone (--games FILE.jsonl | --teacher piers [--num_game N]) [--seat NAME] --sad 1 \\
           --num_epoch E --batchsize 128 --holdout 0.1 --save_dir D [--value_weight 1 --gamma 0.999]

  Search distillation: the label need not be the one move made.  soft_targets turns action values (search.SearchValues.values, a mean
  playout score per legal action) into a distribution per position, sequences_from_records(targets=...) carries it as
  CloneDataset.target and the update takes the cross-entropy against it (hsad_r2d2_clone_soft_fwd).  --blueprint plays the deals with
  search.play_with_search(records=True) on top of a weight file, so what the search found is fitted back into the net:

    python -m hanabi_sad_amd.clone --blueprint FILE.pthw --search_worlds 8 --target_temperature 0.5 --num_game 1000 --sad 1 --save_dir D
"""
import os

import numpy as np
import torch

from . import game_record as gr


# ---- host-side logic (no device) --------------------------------------------------------------------------------------------------
def check_rules(records):
    """the rules all records share; ValueError for none or for records of different rules"""
    records = list(records)
    if not records:
        raise ValueError("no records")
    r = records[0].rules
    if any(rec.rules != r for rec in records):
        raise ValueError("the records were played under different rules")
    return dict(r)


def select_seats(records, seats):
    """-> bool [len(records), P]: the seats whose sequences are kept.  seats: None = all; a list of seat indices; or a name held
    against each record's meta["seats"] (what play_seatings writes: the pool member on every seat), e.g. only the seats `piers` played"""
    P = check_rules(records)["players"]
    keep = np.zeros((len(records), P), dtype=bool)
    if seats is None:
        keep[:] = True
    elif isinstance(seats, str):
        for j, rec in enumerate(records):
            names = rec.meta.get("seats")
            if not names or len(names) != P:
                raise ValueError("record %d carries no seat names (meta[\"seats\"]); select seats by index" % j)
            keep[j] = [n == seats for n in names]
        if not keep.any():
            raise ValueError("no seat of these records is named %r" % seats)
    else:
        idx = [int(s) for s in seats]
        if not idx or any(not 0 <= s < P for s in idx):
            raise ValueError("seats %s: a %d-player game has seats 0..%d" % (idx, P, P - 1))
        keep[:, idx] = True
    return keep


def sequence_lengths(n_moves, max_len, capacity=None):
    """-> (int64 [n]: moves kept per game, how many games were cut).  max_len None: the rules' capacity (nothing is cut)"""
    n = np.asarray(list(n_moves), dtype=np.int64)
    T = int(capacity if max_len is None else max_len)
    return np.minimum(n, T), int((n > T).sum())


def returns_to_go(rewards, n_moves, gamma):
    """rewards [steps, G] (the reward of move t of game j), n_moves [G] -> float32 [steps, G]: G_t = r_t + gamma G_{t+1} for t < n_moves[j],
    0 at and past it (whatever rewards holds there).  Accumulated in float64, rounded to float32 once."""
    r = np.asarray(rewards, dtype=np.float64)
    n = np.asarray(n_moves, dtype=np.int64)
    steps, G = r.shape
    out = np.zeros((steps, G), dtype=np.float64)
    run = np.zeros(G, dtype=np.float64)
    for t in range(steps - 1, -1, -1):
        run = np.where(t < n, r[t] + float(gamma) * run, 0.0)
        out[t] = run
    return out.astype(np.float32)


def soft_targets(values, legal, a, tau):
    """action values -> target distributions for the cloning loss (CompositeLearner.clone_loss with batch["target"]).  values float32
    [n, A], NaN where there is no estimate (SearchValues.values: illegal actions, moves without a search); legal [n, A] (nonzero =
    legal); a int [n], the move made; tau > 0.  -> float32 [n, A] (a tensor on values' device if values is one, else numpy): a row with
    >= 2 finite values is softmax((v_j - max v) / tau) over its finite entries and 0 elsewhere; any other row is the one-hot of a.
    Softmax is shift-invariant, so mean final scores serve as well as returns-to-go.  Computed in float64 and rounded to float32 once: a
    row sums to 1 within A 2^-24.  ValueError: tau not finite or not positive, shapes that do not agree, a finite value on an illegal
    action, a move out of range."""
    tau = float(tau)
    if not np.isfinite(tau) or tau <= 0.0:
        raise ValueError("the target temperature must be finite and positive; got %r" % tau)
    as_tensor = torch.is_tensor(values)
    v = (values.detach().cpu().numpy() if as_tensor else np.asarray(values)).astype(np.float64)
    lg = np.asarray(legal.detach().cpu().numpy() if torch.is_tensor(legal) else legal) != 0
    act = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).astype(np.int64)
    if v.ndim != 2 or lg.shape != v.shape or act.shape != (v.shape[0],):
        raise ValueError("soft_targets takes values [n, A], legal [n, A], a [n]; got %s, %s, %s" % (v.shape, lg.shape, act.shape))
    n, A = v.shape
    if n and (act.min() < 0 or act.max() >= A):
        raise ValueError("a move is outside 0..%d" % (A - 1))
    finite = np.isfinite(v)
    if (finite & ~lg).any():
        raise ValueError("row %d has a value on an illegal action" % int(np.nonzero((finite & ~lg).any(1))[0][0]))
    soft = finite.sum(1) >= 2
    out = np.zeros((n, A), dtype=np.float64)
    out[np.arange(n), act] = 1.0
    if soft.any():
        vs = np.where(finite[soft], v[soft], -np.inf)
        e = np.exp((vs - vs.max(1, keepdims=True)) / tau)      # (exp(-inf) = 0: the entries without an estimate)
        out[soft] = e / e.sum(1, keepdims=True)
    out = out.astype(np.float32)
    return torch.from_numpy(out).to(values.device) if as_tensor else out


def search_targets(records, search_values, tau):
    """[soft_targets(...)] per record of a search.play_with_search(records=True) run: SearchPlay.search_values[k] (float32 [n_moves, A],
    finite on the legal actions of the searched moves) at temperature tau, the one-hot of the move made where no search ran.  The
    legal set handed to soft_targets is the finite set plus the move made; the device checks every row against the position's legal
    mask again when it is cloned (bad rows)."""
    records, search_values = list(records), list(search_values)
    if len(records) != len(search_values):
        raise ValueError("%d records but %d value arrays" % (len(records), len(search_values)))
    out = []
    for j, (rec, v) in enumerate(zip(records, search_values)):
        v = np.asarray(v, dtype=np.float32)
        A = gr.num_actions(rec.rules)
        if v.shape != (rec.n_moves, A):
            raise ValueError("values of record %d must be [n_moves, A] = [%d, %d]; got %s" % (j, rec.n_moves, A, v.shape))
        mv = np.asarray(rec.moves, dtype=np.int64)
        legal = np.isfinite(v)
        legal[np.arange(rec.n_moves), mv] = True
        out.append(soft_targets(v, legal, mv, tau))
    return out


def check_targets(records, targets, A):
    """targets as sequences_from_records takes them -> [float32 [n_moves, A]]; ValueError unless there is one array per record, of that
    shape, every row a distribution: finite, not negative, summing to 1 within 1e-3 (the device's limit)"""
    records, targets = list(records), list(targets)
    if len(targets) != len(records):
        raise ValueError("%d records but %d target arrays" % (len(records), len(targets)))
    out = []
    for j, (rec, tg) in enumerate(zip(records, targets)):
        tg = np.asarray(tg.detach().cpu().numpy() if torch.is_tensor(tg) else tg)
        if tg.shape != (rec.n_moves, A) or tg.dtype.kind != "f":
            raise ValueError("targets of record %d must be float [n_moves, A] = [%d, %d]; got %s %s" % (j, rec.n_moves, A, tg.dtype, tg.shape))
        tg = tg.astype(np.float32)
        if not (np.isfinite(tg).all() and (tg >= 0).all() and (np.abs(tg.astype(np.float64).sum(1) - 1.0) <= 1e-3).all()):
            raise ValueError("targets of record %d: every row must be a distribution (finite, not negative, summing to 1)" % j)
        out.append(tg)
    return out


def target_entropy(data):
    """-> the summed entropy -sum pi log pi of every target row of a CloneDataset (float; 0 log 0 = 0).  Padding, off-turn and
    single-action rows are zero or one-hot rows and add nothing, so this is the entropy over the decisions, and the cross-entropy loss less
    this is the KL divergence from the targets to the net's policy."""
    if data.target is None:
        return 0.0
    p = data.target.double()
    return float(-(torch.where(p > 0, p * torch.log(p.clamp(min=1e-300)), torch.zeros_like(p))).sum())


def padding_rows(n_rows, rows):
    """rows of weight 0 that fill the last batch"""
    return (-int(n_rows)) % int(rows)


class CloneDataset:
    """priv_s float32 [T, N, F] or priv_s_bf16 [T, N, in_dim_padded] (the other None); legal_move float32 [T, N, A]; a int64 [T, N]
    (the recorded move on the mover's row, the no-op on the others); seq_len float32 [N]; game, seat int64 [N] (game = the record's
    index); truncated = games cut at max_len.  Rows at and past seq_len are padding: zeros, no-op.  ret (None unless the sequences were
    made with a gamma): float32 [T, N], the discounted return-to-go of the WHOLE recorded game from step t on, the same on every seat's
    row of a game, 0 at and past seq_len.  target (None unless the sequences were made with targets): float32 [T, N, A], the distribution
    the cross-entropy is taken against -- the record's target row on the mover's row, the one-hot of the no-op on every other valid row,
    zeros at and past seq_len.  pool int64 [T, N], compat / cards int32 [T, N, hand_size] (None unless the sequences were made with
    knowledge=True): env.hand_knowledge() of the row's seat before move t -- what the seat knows about its own hand and the hand itself,
    the labels of belief.BeliefHead; zeros and -1 at and past seq_len."""

    def __init__(self, priv_s, priv_s_bf16, legal_move, a, seq_len, game, seat, truncated=0, ret=None, target=None, pool=None, compat=None,
                 cards=None):
        self.priv_s, self.priv_s_bf16, self.legal_move, self.a = priv_s, priv_s_bf16, legal_move, a
        self.seq_len, self.game, self.seat, self.truncated, self.ret, self.target = seq_len, game, seat, int(truncated), ret, target
        self.pool, self.compat, self.cards = pool, compat, cards

    @property
    def n_rows(self):
        return int(self.seq_len.shape[0])

    @property
    def T(self):
        return int(self.legal_move.shape[0])

    def _obs(self):
        return ("priv_s_bf16", self.priv_s_bf16) if self.priv_s_bf16 is not None else ("priv_s", self.priv_s)

    def take(self, rows):
        """the dataset of these rows (an index tensor), in that order"""
        rows = torch.as_tensor(rows, dtype=torch.int64, device=self.seq_len.device)
        sel = lambda x: None if x is None else x.index_select(1, rows)      # noqa: E731
        return CloneDataset(sel(self.priv_s), sel(self.priv_s_bf16), sel(self.legal_move), sel(self.a), self.seq_len[rows], self.game[rows],
                            self.seat[rows], self.truncated, sel(self.ret), sel(self.target), sel(self.pool), sel(self.compat), sel(self.cards))

    def split(self, holdout, seed):
        """-> (train, held_out), split by GAME: every kept seat of a game goes to the same side.  holdout: the fraction of games held
        out (at least one, never all)"""
        games = torch.unique(self.game.cpu()).tolist()
        n_held = max(1, int(round(float(holdout) * len(games))))
        if not 0.0 < float(holdout) < 1.0 or n_held >= len(games):
            raise ValueError("holdout %s of %d games leaves nothing on one side" % (holdout, len(games)))
        order = torch.randperm(len(games), generator=torch.Generator().manual_seed(int(seed))).tolist()
        held = torch.tensor(sorted(games[k] for k in order[:n_held]), dtype=torch.int64)
        is_held = torch.isin(self.game.cpu(), held)
        rows = torch.arange(self.n_rows)
        return self.take(rows[~is_held]), self.take(rows[is_held])

    def batches(self, rows, seed):
        """shuffled batches of exactly `rows` sequences -> (batch, weight, index) each: batch = the dict CompositeLearner.clone_loss
        takes, weight float32 [rows], index int64 [rows] = the dataset row in each column.  The last batch is filled with padding
        columns (index -1): weight 0, seq_len 0, zero observations -- a CompositeLearner is created for one (T, rows)."""
        rows, dev = int(rows), self.seq_len.device
        order = torch.randperm(self.n_rows, generator=torch.Generator().manual_seed(int(seed)))
        key, obs = self._obs()
        for start in range(0, self.n_rows, rows):
            index = torch.full((rows,), -1, dtype=torch.int64)
            part = order[start:start + rows]
            index[:len(part)] = part
            index = index.to(dev)
            real = index >= 0
            src = index.clamp(min=0)
            full = bool(len(part) == rows)
            pick = lambda x: x.index_select(1, src) if full else x.index_select(1, src) * real.view(1, -1, *([1] * (x.dim() - 2))).to(x.dtype)   # noqa: E731
            noop = self.legal_move.shape[2] - 1
            a = self.a.index_select(1, src)
            if not full:
                a = torch.where(real.view(1, -1), a, torch.full_like(a, noop))
            batch = {key: pick(obs), "legal_move": pick(self.legal_move), "a": a, "seq_len": self.seq_len[src] * real.float()}
            if self.ret is not None:
                batch["ret"] = pick(self.ret)
            if self.target is not None:      # (a padding column has seq_len 0: its zero rows are never read)
                batch["target"] = pick(self.target)
            if self.pool is not None:
                batch["pool"], batch["compat"], batch["cards"] = pick(self.pool), pick(self.compat), pick(self.cards)
            yield batch, real.float(), index


# ---- device side --------------------------------------------------------------------------------------------------------------------
def sequences_from_records(records, sad, seats=None, max_len=None, device="cuda:0", bf16=True, gamma=None, knowledge=False, targets=None):
    """the observation sequences of the recorded games -> CloneDataset with T = max_len (None: game_record.capacity(rules)).
    Game j is records[j] reopened at its first deal (game_record.replay(records, stop=0) on an env of the records' rules, sad as
    given) and stepped with its recorded moves and greedy alternatives; step t's rows are the observations BEFORE move t.  One
    sequence per kept seat (select_seats), row order game-major.  Games longer than max_len are cut and counted in .truncated.
    gamma (None: no returns, and nothing below happens): env.reward is collected after every step and CloneDataset.ret is
    returns_to_go of it.  A game cut at max_len is then stepped on with its recorded moves to its recorded end, no observations
    stored, so that its return is that of the whole recorded game and not of the kept part.
    targets (None: no target field, and nothing below happens): one float [n_moves, A] array per record whose rows ARE distributions over
    the actions of the position before move t -- soft_targets / search_targets make them from action values; nothing is normalised here.
    check_targets holds them to that (shape, finite, not negative, mass 1) before any device work; that the mass lies on legal actions is
    checked by the update itself (bad rows).  CloneDataset.target then carries, at step t, the record's row t on the mover's row (seat
    t % P) and the one-hot of the no-op on every other valid row.
    knowledge (False: no such fields, and nothing below happens): env.hand_knowledge() of the kept seats is stored at every kept step as
    CloneDataset.pool / .compat / .cards (zeros and -1 on padding rows)."""
    from .env import BatchedHanabiEnv
    from .eval import _drain_errors
    records = list(records)
    r = check_rules(records)
    for j, rec in enumerate(records):
        if not len(rec.moves) == len(rec.greedy):
            raise ValueError("record %d has %d moves and %d greedy moves" % (j, len(rec.moves), len(rec.greedy)))
    keep = select_seats(records, seats)
    G, P = len(records), r["players"]
    if targets is not None:
        targets = check_targets(records, targets, gr.num_actions(r))
    lens, truncated = sequence_lengths([rec.n_moves for rec in records], max_len, gr.capacity(r))
    T = int(gr.capacity(r) if max_len is None else max_len)
    n_all = np.asarray([rec.n_moves for rec in records], dtype=np.int64)
    kept_steps = int(lens.max()) if G else 0
    steps = kept_steps if gamma is None else int(n_all.max()) if G else 0
    step_lens = lens if gamma is None else n_all      # how far each game is stepped
    env = BatchedHanabiEnv(G, players=P, hand_size=r["hand_size"], bomb=r["bomb"], eps_list=[0.0], max_len=-1, sad=bool(sad), device=device,
                           colors=r["colors"], ranks=r["ranks"], max_information_tokens=r["max_information_tokens"],
                           max_life_tokens=r["max_life_tokens"])
    try:
        env.reset()
        gr.replay(records, stop=[0] * G, env=env)
        status = env.replay_status.cpu().numpy()[:G]
        if (status < 0).any():
            j = int(np.nonzero(status < 0)[0][0])
            raise ValueError("record %d cannot be dealt under its rules (replay status %d)" % (j, int(status[j])))
        dev, F, A = env.device, env.F, env.A
        noop = A - 1
        mv, gv = np.full((max(steps, 1), G), noop, dtype=np.int64), np.full((max(steps, 1), G), noop, dtype=np.int64)
        for j, rec in enumerate(records):
            n = int(step_lens[j])
            mv[:n, j], gv[:n, j] = rec.moves[:n], rec.greedy[:n]
        mv, gv = torch.from_numpy(mv).to(dev), torch.from_numpy(gv).to(dev)
        flat = np.nonzero(keep.reshape(-1))[0]
        rows = torch.from_numpy(flat).to(dev)
        row_game = torch.from_numpy(flat // P).to(dev)
        N = int(len(flat))
        Fp = (F + 63) // 64 * 64
        priv = torch.zeros(T, N, Fp, dtype=torch.bfloat16, device=dev) if bf16 else torch.zeros(T, N, F, dtype=torch.float32, device=dev)
        legal = torch.zeros(T, N, A, dtype=torch.float32, device=dev)
        act = torch.full((T, N), noop, dtype=torch.int64, device=dev)
        lens_d, step_lens_d = torch.from_numpy(lens).to(dev), torch.from_numpy(step_lens).to(dev)
        rewards = torch.zeros(max(steps, 1), G, dtype=torch.float32, device=dev) if gamma is not None else None
        a_step, g_step = torch.empty(G, P, dtype=torch.int64, device=dev), torch.empty(G, P, dtype=torch.int64, device=dev)
        target = tg = None
        if targets is not None:
            tg_host = np.zeros((max(kept_steps, 1), G, A), dtype=np.float32)      # the movers' rows; past a game's kept moves: never read
            for j, arr in enumerate(targets):
                tg_host[:int(lens[j]), j] = arr[:int(lens[j])]
            tg = torch.from_numpy(tg_host).to(dev)
            target = torch.zeros(T, N, A, dtype=torch.float32, device=dev)
            t_step = torch.empty(G, P, A, dtype=torch.float32, device=dev)
        k_pool = k_compat = k_cards = None
        if knowledge:
            Hs = r["hand_size"]
            k_pool = torch.zeros(T, N, dtype=torch.int64, device=dev)
            k_compat = torch.zeros(T, N, Hs, dtype=torch.int32, device=dev)
            k_cards = torch.full((T, N, Hs), -1, dtype=torch.int32, device=dev)
        for t in range(steps):
            live = t < lens_d                                   # [G]: the step is kept
            moving = t < step_lens_d                            # [G]: the game is stepped (past `live` only for the returns of cut games)
            if t < kept_steps:
                live_rows = live[row_game]
                p_rows = env.priv_s.view(G * P, F)[rows] * live_rows.view(-1, 1)
                if bf16:
                    priv[t, :, :F] = p_rows.to(torch.bfloat16)  # (0 / 1 features: exact)
                else:
                    priv[t] = p_rows
                legal[t] = env.legal_move.view(G * P, A)[rows] * live_rows.view(-1, 1)
                if knowledge:
                    hp, hc, hk = env.hand_knowledge()
                    k_pool[t] = hp.view(G * P)[rows] * live_rows
                    k_compat[t] = hc.view(G * P, Hs)[rows] * live_rows.view(-1, 1)
                    k_cards[t] = torch.where(live_rows.view(-1, 1), hk.view(G * P, Hs)[rows], torch.full_like(k_cards[t], -1))
            a_step.fill_(noop)
            g_step.fill_(noop)
            a_step[:, t % P] = torch.where(moving, mv[t], torch.full_like(mv[t], noop))
            g_step[:, t % P] = torch.where(moving, gv[t], torch.full_like(gv[t], noop))
            if t < kept_steps:
                act[t] = a_step.view(-1)[rows]                  # (t < kept_steps <= T: a game that still moves here is live here)
                if target is not None:
                    t_step.zero_()
                    t_step[:, :, noop] = 1.0
                    t_step[:, t % P] = tg[t]
                    target[t] = t_step.view(G * P, A)[rows] * live_rows.view(-1, 1)
            env.step(a_step, g_step)                            # (a game past its moves is handed the no-op and left alone)
            if rewards is not None:
                rewards[t] = env.reward[:G] * moving            # (the reward of move t; past a game's end: whatever, never read)
        _drain_errors(env)
        torch.cuda.synchronize(dev)
    finally:
        env.close()
    seq_len = torch.from_numpy(lens[flat // P]).to(dev).float()
    ret = None
    if gamma is not None:
        whole = torch.from_numpy(returns_to_go(rewards.cpu().numpy()[:steps], n_all, gamma)).to(dev)      # [steps, G]
        ret = torch.zeros(T, N, dtype=torch.float32, device=dev)
        ret[:kept_steps] = whole[:kept_steps][:, row_game] * (torch.arange(kept_steps, device=dev).view(-1, 1) < seq_len.view(1, -1))
    return CloneDataset(None if bf16 else priv, priv if bf16 else None, legal, act, seq_len, row_game.clone(), torch.from_numpy(flat % P).to(dev),
                        truncated, ret, target, k_pool, k_compat, k_cards)


def records_from_teacher(pool, num_game, seed, sad, *, seating=None, num_player=2, bomb=0, device="cuda:0", names=None, temperature=None,
                         sample_seed=0, **env_kw):
    """play the games to clone -> [GameRecord], tagged with seat names: eval.play_seatings(pool, [seating], ..., records=True).  pool:
    rulebot.RuleBot members, weight dicts / files / agents, or both; seating: the pool index on every seat (default: member
    p % len(pool) on seat p -- one teacher plays itself).  env_kw: hand_size and the rule keywords of play_seatings.
    temperature / sample_seed: play_seatings' -- a network teacher at a temperature > 0 plays its softmax policy, so the set holds more
    than one line of play per deal-and-position; the records keep the move made and the greedy move apart."""
    from .eval import play_seatings
    pool = list(pool)
    if seating is None:
        seating = [p % len(pool) for p in range(int(num_player))]
    res = play_seatings(pool, [list(seating)], int(num_game), int(seed), bomb, sad, device=device, records=True, names=names, bot_seed=int(seed),
                        temperature=temperature, sample_seed=sample_seed, **env_kw)
    return res.records


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def run_epoch(learner, data, rows, seed, train, value_weight=0.0):
    """one pass over `data` in batches of `rows` -> (loss per decision, hits, decisions); train: backward + optimizer step per batch.
    value_weight > 0 (data.ret needed): the updates carry the value term, and a fourth result is the value loss per step.
    A dataset with targets (data.target) hands them to every update: the loss is then the cross-entropy against them."""
    dev = data.seq_len.device
    total = torch.zeros(5 if value_weight else 3, dtype=torch.float64, device=dev)
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    for batch, weight, _ in data.batches(rows, seed):
        loss, stats = learner.clone_loss(batch, weight, compute_grad=train, value_weight=value_weight)
        if train:
            learner.optimizer_step()
        sums = [(loss * weight).sum().double(), stats["hits"].sum().double(), stats["decisions"].sum().double()]
        if value_weight:      # (a padding column has seq_len 0: no steps, no value loss)
            sums += [stats["value_loss"].sum().double(), stats["steps"].sum().double()]
        total += torch.stack(sums)
        bad += stats["bad"].sum()
    if int(bad):
        from ._lib import HsadError
        raise HsadError("%d recorded moves are illegal in their position or out of range%s"
                        % (int(bad), ", or their target rows are no distribution over the legal actions" if data.target is not None else ""))
    s, h, n = total.tolist()[:3]
    if value_weight:
        v, k = total.tolist()[3:]
        return s / max(n, 1.0), int(h), int(n), v / max(k, 1.0)
    return s / max(n, 1.0), int(h), int(n)


def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="fit the R2D2 net to recorded games")
    p.add_argument("--games", type=str, default="", help="a file of game records (JSON lines, game_record.save)")
    p.add_argument("--teacher", type=str, nargs="+", default=[], help="instead of --games: rule-bot presets of rulebot.py or weight files; "
                                                                      "member p %% len plays seat p, the games are recorded and cloned")
    p.add_argument("--num_game", type=int, default=1000, help="with --teacher: games to play")
    p.add_argument("--seat", type=str, default="", help="clone only the seats of this name (the records' meta[\"seats\"]), or a seat index")
    p.add_argument("--save_dir", type=str, default="")
    p.add_argument("--load_model", type=str, default="")
    p.add_argument("--seed", type=int, default=10001)
    p.add_argument("--sad", type=int, default=1)
    p.add_argument("--num_player", type=int, default=2)
    p.add_argument("--hand_size", type=int, default=5)
    p.add_argument("--colors", type=int, default=5)
    p.add_argument("--ranks", type=int, default=5)
    p.add_argument("--max_information_tokens", type=int, default=8)
    p.add_argument("--max_life_tokens", type=int, default=3)
    p.add_argument("--eval_bomb", type=int, default=0)
    p.add_argument("--lr", type=float, default=6.25e-5)
    p.add_argument("--eps", type=float, default=1.5e-5)
    p.add_argument("--grad_clip", type=float, default=5.0)
    p.add_argument("--num_lstm_layer", type=int, default=2)
    p.add_argument("--rnn_hid_dim", type=int, default=512)
    p.add_argument("--train_device", type=str, default="cuda:0")
    p.add_argument("--batchsize", type=int, default=128)
    p.add_argument("--num_epoch", type=int, default=10)
    p.add_argument("--max_len", type=int, default=80)
    p.add_argument("--holdout", type=float, default=0.1)
    p.add_argument("--num_eval_game", type=int, default=1000)
    p.add_argument("--value_weight", type=float, default=0.0, help="> 0: also fit Q(o, a_recorded) to the discounted return of the recorded game "
                                                                   "(Huber), with this weight next to the cross-entropy")
    p.add_argument("--eval_temperature", type=float, default=0.0, help="> 0: each epoch line also gives the self-play score of the net "
                                                                       "playing its softmax policy at this temperature (1 = the fitted distribution)")
    p.add_argument("--teacher_temperature", type=float, default=0.0, help="with --teacher: network teachers play their softmax policy at this "
                                                                          "temperature (rule bots ignore it)")
    p.add_argument("--gamma", type=float, default=0.999, help="with --value_weight: the discount of the returns (the one TD training will use)")
    p.add_argument("--blueprint", type=str, default="", help="instead of --games / --teacher: a weight file; --num_game deals are played with "
                                                             "blueprint-policy search on top of it (search.play_with_search), recorded and cloned")
    p.add_argument("--search_worlds", type=int, default=0, help="with --blueprint: sampled worlds per legal action")
    p.add_argument("--search_rounds", default=None, type=lambda s: tuple(int(x) for x in s.split(",")),
                   help="with --blueprint: world counts per round, e.g. 8,8,16 (summing to --search_worlds)")
    p.add_argument("--search_depth", default=None, type=int, metavar="D", help="with --blueprint --search_worlds: stop every sampled world D "
                   "moves after the candidate action and value it as its score so far + the blueprint's own Q; not with --search_rounds")
    p.add_argument("--search_horizon_value", default="mover", type=str, choices=["mover", "team"],
                   help="with --search_depth: the Q of the seat on turn at the horizon, or the sum over the game's seats")
    p.add_argument("--searcher", type=str, default="all", help="with --blueprint: all, or the one seat that searches")
    p.add_argument("--search_threshold", type=float, default=0.05, help="with --blueprint: deviate from the blueprint only for a larger value gain")
    p.add_argument("--target_temperature", type=float, default=0.0, help="with --blueprint: > 0 clones softmax(search values / this) "
                                                                         "(clone.soft_targets) instead of the move made; 0 = hard labels")
    return p.parse_args(argv)


def main(argv=None):
    from .checkpoint import load_weights, save_weights
    from .composite import CompositeLearner
    from .eval import env_dims, evaluate
    from .rulebot import PRESETS
    from .selfplay import game_rules, init_weights
    args = parse_args(argv)
    dev = args.train_device
    if bool(args.games) + bool(args.teacher) + bool(args.blueprint) != 1:
        raise SystemExit("give either --games FILE or --teacher NAME" + (" or --blueprint FILE" if args.blueprint else ""))
    for flag in ("eval_temperature", "teacher_temperature", "target_temperature"):
        if not np.isfinite(getattr(args, flag)) or getattr(args, flag) < 0:
            raise SystemExit("--%s must be finite and not negative" % flag)
    search_values = None
    if args.search_depth is not None:
        if not args.blueprint or args.search_worlds < 1:
            raise SystemExit("--search_depth needs --blueprint FILE --search_worlds N > 0")
        if args.search_rounds is not None:
            raise SystemExit("--search_depth and --search_rounds do not combine (the round kernel compares whole scores)")
        if args.search_depth < 0:
            raise SystemExit("--search_depth must not be negative")
    if args.blueprint:
        if not os.path.isfile(args.blueprint):
            raise SystemExit("--blueprint %s: no such weight file" % args.blueprint)
        if args.search_worlds < 1:
            raise SystemExit("--blueprint needs --search_worlds N > 0")
        if args.searcher != "all" and not args.searcher.isdigit():
            raise SystemExit("--searcher must be all or a seat number")
    elif args.target_temperature > 0:
        raise SystemExit("--target_temperature needs --blueprint: the targets are made from the search's action values")
    if args.blueprint:
        from .search import play_with_search
        played = play_with_search(load_weights(args.blueprint), args.num_game, args.seed, args.eval_bomb, args.sad, worlds=args.search_worlds,
                                  threshold=args.search_threshold, search_seed=args.seed, searcher="all" if args.searcher == "all" else int(args.searcher),
                                  num_player=args.num_player, hand_size=args.hand_size, device=dev, rounds=args.search_rounds, records=True,
                                  depth=args.search_depth, horizon_value=args.search_horizon_value, **game_rules(args))
        records, search_values = played.records, played.search_values
        print("blueprint + search (%d worlds): %.3f +/- %.3f over %d deals, %d moves changed by the search"
              % (args.search_worlds, played.mean, played.sem, args.num_game, int(played.deviations.sum())), flush=True)
        if args.search_depth is not None:
            print("depth %d (%s): %.4f of the worlds cut at the horizon" % (args.search_depth, args.search_horizon_value, played.cut_share),
                  flush=True)
    elif args.games:
        records = gr.load(args.games)
    else:
        pool = []
        for entry in args.teacher:
            if entry not in PRESETS and not os.path.isfile(entry):
                raise SystemExit("--teacher %s: no rule-bot preset of that name (have: %s) and no weight file" % (entry, ", ".join(sorted(PRESETS))))
            pool.append(PRESETS.get(entry, entry))
        names = [e if e in PRESETS else os.path.basename(e) for e in args.teacher]
        records = records_from_teacher(pool, args.num_game, args.seed, args.sad, num_player=args.num_player, bomb=args.eval_bomb, device=dev,
                                       names=names, hand_size=args.hand_size, temperature=args.teacher_temperature or None,
                                       sample_seed=args.seed, **game_rules(args))
    if args.save_dir:
        os.makedirs(args.save_dir, exist_ok=True)
        if args.teacher or args.blueprint:     # the games that were cloned, for --games of a later run
            gr.save(os.path.join(args.save_dir, "games.jsonl"), records)
    r = check_rules(records)
    seats = None if not args.seat else ([int(args.seat)] if args.seat.isdigit() else args.seat)
    vw = float(args.value_weight)
    if vw < 0:
        raise SystemExit("--value_weight must not be negative")
    targets = search_targets(records, search_values, args.target_temperature) if args.target_temperature > 0 else None
    data = sequences_from_records(records, args.sad, seats=seats, max_len=args.max_len, device=dev, gamma=args.gamma if vw > 0 else None,
                                  targets=targets)
    train, held = data.split(args.holdout, args.seed)
    entropy = target_entropy(train)      # once, on the host: the loss less this is the KL divergence from the targets
    print("%d games (%d cut at %d moves, mean score %.2f), %d sequences: %d to fit, %d held out"
          % (len(records), data.truncated, args.max_len, float(np.mean([rec.score for rec in records])), data.n_rows, train.n_rows, held.n_rows))
    rules = {k: r[k] for k in ("colors", "ranks", "max_information_tokens", "max_life_tokens")}
    F, A = env_dims(r["players"], r["hand_size"], args.sad, **rules)
    if args.load_model:
        W = load_weights(args.load_model)
    else:
        W = init_weights(F, args.rnn_hid_dim, A, r["hand_size"], args.seed, num_lstm_layer=args.num_lstm_layer)
    learner = CompositeLearner(W, W, 1, 0.999, lr=args.lr, eps=args.eps, grad_clip=args.grad_clip, device=dev)
    for epoch in range(args.num_epoch):
        loss, hits, n, *vtrain = run_epoch(learner, train, args.batchsize, args.seed + epoch, True, vw)
        _, hh, hn, *vheld = run_epoch(learner, held, args.batchsize, 0, False, vw)
        weights = {k: v.detach().clone() for k, v in learner.online.w.items()}
        score = evaluate(weights, args.num_eval_game, args.seed, args.eval_bomb, args.sad, num_player=r["players"], hand_size=r["hand_size"],
                         device=dev, **rules)[0]
        if args.eval_temperature > 0:      # the policy the loss fits, next to its mode
            soft = evaluate(weights, args.num_eval_game, args.seed, args.eval_bomb, args.sad, num_player=r["players"], hand_size=r["hand_size"],
                            device=dev, temperature=args.eval_temperature, sample_seed=args.seed, **rules)[0]
            score_text = "%.3f (sampled at temperature %g: %.3f)" % (score, args.eval_temperature, soft)
        else:
            score_text = "%.3f" % score
        value = ", value loss per step %.4f, held-out value loss per step %.4f" % (vtrain[0], vheld[0]) if vw > 0 else ""
        if targets is not None:
            value += ", KL per decision %.4f" % (loss - entropy / max(n, 1))
        print("epoch %d: loss per decision %.4f, agreement %.4f (%d / %d), held-out agreement %.4f (%d / %d), self-play score %s%s"
              % (epoch, loss, hits / max(n, 1), hits, n, hh / max(hn, 1), hh, hn, score_text, value), flush=True)
        if args.save_dir:
            save_weights(weights, os.path.join(args.save_dir, "clone_epoch%d.pthw" % epoch))
            save_weights(weights, os.path.join(args.save_dir, "clone.pthw"))
    learner.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
