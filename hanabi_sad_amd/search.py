"""Determinised Monte-Carlo action values on the device env (SPARTA-style single-agent search):
for the player on turn, every legal action is tried in `worlds` sampled worlds -- the player's own hidden hand resampled from the
hands its card knowledge allows, the deck reshuffled -- and each world is played out to the end.  Built from the env's search
primitives (BatchedHanabiEnv.fork_from / determinize / step / playout_random); the rollouts of all (game, action, world) jobs run
batched in one search env, `capacity` games at a time.

Rollout policies: mc_action_values plays the worlds out with random legal moves (one launch, hsad_env_playout_random) or, with
playout=<rulebot.RuleBot>, with a rule-list bot on every seat (one launch as well, hsad_env_playout_rule);
policy_action_values / PolicySearch play them out with the blueprint itself -- the R2D2 agent acting greedily for every seat --
which is what can improve on that agent (choose_action, play_with_search).  The glue kernels of the latter are csrc/hsad_search.hip.

PolicySearch(replay=True) first plays every sampled world again from its first move (GameLog, hsad_search_world_script,
hsad_env_rewind_scripted, hsad_search_replay_actions), so that each seat's LSTM state is the one that world's observations give.

search(rounds=(n0, n1, ...)) plays the worlds in rounds: the per-world scores are kept (hsad_search_world_scores), and after each
round hsad_search_round compares every action with the round's leader world by world -- the actions of a game meet the same worlds
-- and drops those that are already hopeless (round_world_order, SearchValues.paired / pruned_round, choose_action_paired).

PolicySearch(depth=D) does not play the worlds to the end: the forced action and D more blueprint moves, then one act(with_q=True)
on the position reached, and hsad_search_horizon_stats values every world still running as its score so far + the blueprint's own Q,
in 1/256 points (SearchValues.scale / cut / nonfinite / world_values).  D + 2 act calls per chunk, no host read-back."""
from fractions import Fraction

import numpy as np
import torch

from . import _lib
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


SAMPLERS = ("rejection", "stratified", "learned")


def _check_sampler(sampler):
    if sampler not in SAMPLERS:
        raise ValueError("sampler must be one of %s; got %r" % (", ".join(SAMPLERS), sampler))
    return sampler


def _check_belief(sampler, belief, agent=None, hand_size=None):
    """the refusals of sampler="learned", all before anything touches the device.  belief: None, or what carries a head's shape --
    a belief.BeliefSampler / BeliefHead (hand_size, H), a head's state dict or the path of a saved one.  -> (hand_size, H) | None"""
    _check_sampler(sampler)
    if sampler != "learned":
        if belief is not None:
            raise ValueError("belief= is what sampler=\"learned\" draws from; sampler=%r takes none" % (sampler,))
        return None
    if belief is None:
        raise ValueError("sampler=\"learned\" needs belief=: a belief.BeliefSampler, a BeliefHead, a head's state dict or its file")
    if hasattr(belief, "hand_size") and hasattr(belief, "H"):
        hs, H = int(belief.hand_size), int(belief.H)
    else:
        import os
        from .belief import check_state
        if isinstance(belief, (str, os.PathLike)):
            if not os.path.isfile(belief):
                raise ValueError("belief=%r: no such file" % (belief,))
            belief = torch.load(belief, map_location="cpu")
        if not isinstance(belief, dict):
            raise ValueError("belief= must be a belief.BeliefSampler, a BeliefHead, a head's state dict or its file; got %s" % type(belief).__name__)
        hs, H = check_state(belief)
    if hand_size is not None and hs != int(hand_size):
        raise ValueError("the belief head is for hands of %d, the env deals hands of %d" % (hs, int(hand_size)))
    if agent is not None:
        net = getattr(agent, "online", None)
        if getattr(net, "skip", False):
            raise ValueError("sampler=\"learned\" reads the top LSTM layer's h as the head's features; a skip_connect agent's trunk output "
                             "is not that")
        if getattr(net, "H", None) is not None and int(net.H) != H:
            raise ValueError("the belief head reads a trunk of width %d, the agent's is %d" % (H, int(net.H)))
    return hs, H


HORIZON_VALUES = ("mover", "team")          # include/hsad.h: HSAD_SEARCH_HORIZON_MOVER, HSAD_SEARCH_HORIZON_TEAM
VALUE_SCALE = 256                           # HSAD_SEARCH_VALUE_SCALE


def _check_depth(depth, horizon_value, max_steps, agent=None):
    """the refusals of a depth-limited search, all before anything touches the device -> depth (None, or an int)"""
    if horizon_value not in HORIZON_VALUES:
        raise ValueError("horizon_value must be one of %s; got %r" % (", ".join(HORIZON_VALUES), horizon_value))
    if depth is None:
        return None
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 0 <= int(depth) < int(max_steps):
        raise ValueError("depth must be None or an int with 0 <= depth < max_steps = %d; got %r" % (int(max_steps), depth))
    if getattr(getattr(agent, "online", None), "skip", False):
        raise ValueError("a depth-limited search values the horizon with the agent's cached Q (act(with_q=True)), which is undefined "
                         "for a skip_connect agent")
    return int(depth)


def _sample_hands(env, sampler, viewer, key, seed, world, worlds, belief=None):
    """the hidden hands of the slots' worlds: "rejection" = determinize, independent draws per world; "stratified" =
    determinize_exact with world w of a game drawing from the w-th of `worlds` equal parts of that game's exact belief; "learned"
    = determinize_belief_worlds under belief = (logits float32 [root games, >= 25 H], src int32 [slots]: the root game of each
    slot), the worlds of a game stratified per slot of the hand -> its (status, logp, logp0), else None"""
    if sampler == "rejection":
        env.determinize(viewer, key, seed)
    elif sampler == "stratified":
        env.determinize_exact(viewer, key, seed, stratum=world, n_strata=worlds)
    else:
        logits, src = belief
        return env.determinize_belief_worlds(viewer, logits, src, key - world.to(key.device, torch.int64), world, worlds, seed)
    return None


def search_jobs(root):
    """(game, action) pairs to evaluate: every legal action of the player on turn of every live root game, in (game, action) order;
    also that player per game.  Reads the root's legal_move rows."""
    q = root.query().cpu().numpy()
    live = (q[:, Q_STARTED] == 1) & (q[:, Q_TERMINATED] == 0)
    cur = q[:, Q_CUR_PLAYER].astype(np.int64)
    legal = root.legal_move.cpu().numpy()
    pairs = [(g, a) for g in range(root.G) if live[g] for a in range(root.A) if legal[g, cur[g], a] != 0]
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2), cur


def mc_action_values(root, worlds, seed, capacity=4096, max_iter=None, sampler="rejection", playout=None):
    """float32 [G, A] on the root's device: values[g, a] = mean final score (HSAD_Q_SCORE: honours `bomb`) over `worlds` random
    playouts of action a by the player on turn of root game g; NaN for illegal actions and for games that are not live.  The root
    env is only read.  The result does not depend on `capacity` (jobs are keyed by (game, world), never by the slot they run in).
    A world whose sampler gave up (32 rejected tries: not seen in practice) keeps the true hand.  sampler="stratified" draws the
    hands with determinize_exact instead: never gives up, and the worlds of a game cover its exact belief evenly (world w takes the
    w-th of `worlds` equal parts); keys, seeds and everything after the draw are the same.  playout: None plays the worlds out with
    random legal moves; a rulebot.RuleBot plays them out with that bot on every seat (playout_rule in place of playout_random:
    jobs, keys, seeds and samplers are unchanged).  sampler="learned" is refused (ValueError): there is no agent state here."""
    _check_sampler(sampler)
    if sampler == "learned":
        raise ValueError("mc_action_values has no learned sampler: random and rule-bot playouts carry no network state for the head to "
                         "read (policy_action_values / PolicySearch take sampler=\"learned\")")
    if playout is not None:
        from .rulebot import RuleBot
        if not isinstance(playout, RuleBot):
            raise ValueError("playout must be None or a rulebot.RuleBot; got %r" % (playout,))
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
            _sample_hands(senv, sampler, p_c, key, seed, torch.from_numpy(w_c.astype(np.int32)), worlds)
            act = torch.full((capacity, P), A - 1, dtype=torch.int64, device=dev)   # the noop for the players not on turn
            act[slot, p_c] = torch.from_numpy(a_c).to(dev)
            senv.step(act, act)
            if playout is None:
                senv.playout_random(max_iter, seed, key=key)
            else:
                senv.playout_rule(max_iter, playout, seed=seed, key=key)
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


# ---------------------------------------------------------------------------------------------------------
# blueprint-policy search: the sampled worlds are played out by the agent itself
# ---------------------------------------------------------------------------------------------------------
MAX_ROUND_WORLDS, MAX_Z2_DEN, MAX_Z2_NUM = 4096, 1024, 16384     # the int64 bounds of hsad_search_round (include/hsad.h)


def round_world_order(worlds):
    """the order in which a search in rounds plays a game's worlds: the indices 0 .. worlds - 1 sorted by their bit-reversed value
    over (worlds - 1).bit_length() bits -- 8 -> [0, 4, 2, 6, 1, 5, 3, 7].  Every prefix is spread over [0, worlds): with the stratified
    sampler world w is stratum w of the belief in rank order, so an early round does not sit in one corner of it.  World 0 is first."""
    bits = max(int(worlds) - 1, 0).bit_length()
    return sorted(range(int(worlds)), key=lambda w: int(format(w, "0%db" % bits)[::-1], 2) if bits else 0)


def _check_rounds(rounds, worlds, prune_z, min_n):
    """-> (rounds as a tuple of ints, z2_num, z2_den): prune_z^2 as the fraction hsad_search_round takes"""
    try:
        rounds = tuple(int(r) for r in rounds)
    except TypeError:
        raise ValueError("rounds must be a tuple of positive world counts; got %r" % (rounds,))
    if not rounds or any(r < 1 for r in rounds) or sum(rounds) != worlds:
        raise ValueError("rounds must be positive world counts that sum to worlds = %d; got %r" % (worlds, rounds))
    if worlds > MAX_ROUND_WORLDS:
        raise ValueError("a search in rounds takes at most %d worlds; got %d" % (MAX_ROUND_WORLDS, worlds))
    if not prune_z >= 0 or int(min_n) < 1:
        raise ValueError("prune_z must be >= 0 and min_n >= 1; got %r, %r" % (prune_z, min_n))
    z2 = Fraction(prune_z * prune_z).limit_denominator(MAX_Z2_DEN)
    if z2.numerator > MAX_Z2_NUM:
        raise ValueError("prune_z = %r: z^2 = %s has a numerator above %d" % (prune_z, z2, MAX_Z2_NUM))
    return rounds, z2.numerator, z2.denominator


class SearchValues:
    """what PolicySearch.search returns, all on the device of `totals`:
    totals int64 [G, A, 3] = (sum score, sum score^2, worlds counted) per (root game, action) as hsad_search_job_stats reduced them;
    values float32 [G, A] = sum / worlds in float32 from those integers, NaN where nothing was counted (illegal actions, games that
    are not live, turns of a player who does not search); sem float32 [G, A] = population std / sqrt(worlds) from the integers;
    blueprint_a int64 [G] = the agent's own greedy action at the root, -1 for games that were not searched;
    mismatch int32 [G, worlds] (replay only, else None) = per sampled world the number of past partner moves at which the blueprint,
    replayed in that world, showed another greedy action than the logged one (0 for games that were not searched).
    A search in rounds (search(rounds=...), else all None) adds: paired int64 [G, A, 3] = (sum d, sum d^2, worlds) of d = the action's
    score minus the blueprint action's in the same world, over the worlds both were played in; paired_mean / paired_sem float32
    [G, A] from those integers as values / sem are (NaN where no world is shared); pruned_round int32 [G, A] = the round after which
    the action was dropped, -1 if never; world_scores uint8 [G, A, worlds] = the score per world, 0xFF where not played.
    sampler="learned" (else both None) adds belief_logp / belief_logp0 float32 [G, worlds]: the log-probability of world w's sampled
    hand under the learned belief and under the exact belief (their difference is the log importance ratio), NaN where no world was
    sampled.
    A depth-limited search (PolicySearch(depth=D), else scale = 1, cut = None, nonfinite = 0) counts in fixed point: scale = 256
    (HSAD_SEARCH_VALUE_SCALE), and totals is then (sum v, sum v^2, worlds) in units of 1 / scale and 1 / scale^2 -- v = a world's score
    so far plus the blueprint's Q at the horizon, or scale x its final score (hsad_search_horizon_stats); values and sem are computed
    in float64 from those integers, divided by scale and cast to float32, so they stay in points.  cut int64 [G, A] = the worlds
    valued at the horizon (the others ended within the depth); nonfinite = how many of them had a Q that was NaN or infinite and
    counted as 0.  world_values uint16 [G, A, worlds] (search(keep_world_values=True), else None) = v per world in units of 1 / scale,
    0xFFFF where not played."""

    def __init__(self, totals, blueprint_a, mismatch=None, paired=None, pruned_round=None, world_scores=None, belief_logp=None,
                 belief_logp0=None, scale=1, cut=None, nonfinite=0, world_values=None):
        self.totals = totals = torch.as_tensor(totals).to(torch.int64)
        self.blueprint_a = torch.as_tensor(blueprint_a).to(torch.int64)
        self.mismatch = mismatch
        self.belief_logp, self.belief_logp0 = belief_logp, belief_logp0
        self.scale, self.nonfinite, self.world_values = int(scale), int(nonfinite), world_values
        if self.scale < 1:
            raise ValueError("scale must be >= 1; got %r" % (scale,))
        self.cut = None if cut is None else torch.as_tensor(cut).to(torch.int64)
        s, sq, n = totals[..., 0], totals[..., 1], totals[..., 2]
        nan = torch.full(s.shape, float("nan"), dtype=torch.float32, device=totals.device)
        counted = n > 0
        nf = torch.where(counted, n, torch.ones_like(n))
        var_n2 = (nf * sq - s * s).clamp(min=0).to(torch.float64)        # n^2 * population variance, exact in int64
        nd = nf.to(torch.float64)
        if self.scale == 1:
            self.values = torch.where(counted, s.to(torch.float32) / nf.to(torch.float32), nan)
            self.sem = torch.where(counted, (torch.sqrt(var_n2) / nd / torch.sqrt(nd)).to(torch.float32), nan)
        else:
            self.values = torch.where(counted, (s.to(torch.float64) / nd / self.scale).to(torch.float32), nan)
            self.sem = torch.where(counted, (torch.sqrt(var_n2) / nd / torch.sqrt(nd) / self.scale).to(torch.float32), nan)
        self.paired, self.pruned_round, self.world_scores = paired, pruned_round, world_scores
        self.paired_mean = self.paired_sem = None
        if paired is not None:
            self.paired = paired = torch.as_tensor(paired).to(torch.int64)
            d, dq, dn = paired[..., 0], paired[..., 1], paired[..., 2]
            shared = dn > 0
            nf = torch.where(shared, dn, torch.ones_like(dn))
            self.paired_mean = torch.where(shared, d.to(torch.float32) / nf.to(torch.float32), nan)
            var_n2 = (nf * dq - d * d).clamp(min=0).to(torch.float64)
            nd = nf.to(torch.float64)
            self.paired_sem = torch.where(shared, (torch.sqrt(var_n2) / nd / torch.sqrt(nd)).to(torch.float32), nan)


def _searched_games(searcher, cur, G):
    """bool [G] (numpy): the games whose player on turn searches.  searcher: None (everyone), a seat number, or an int [G] mask"""
    if searcher is None:
        return np.ones(G, dtype=bool)
    if isinstance(searcher, (int, np.integer)):
        return cur == int(searcher)
    m = searcher.cpu().numpy() if isinstance(searcher, torch.Tensor) else np.asarray(searcher)
    if m.shape != (G,):
        raise ValueError("searcher must be None, a seat number or an int [%d] mask; got shape %s" % (G, tuple(m.shape)))
    return m != 0


class GameLog:
    """The root's moves as stepped: a / greedy_a int64 [n_moves, G, P] on the device (views of a buffer that grows by doubling),
    and sad int64 [n_moves, G, P]: the SAD greedy-action section every seat was shown after the move (zeros with sad = 0).
    Once per root step: append() with the rows hsad_env_step is given, then observed(env) after the step."""

    def __init__(self, G, P, device, room=128):
        self.G, self.P, self.device, self.n_moves = int(G), int(P), torch.device(device), 0
        self._a = torch.zeros(room, self.G, self.P, dtype=torch.int64, device=self.device)
        self._g = torch.zeros_like(self._a)
        self._s = torch.zeros_like(self._a)

    def append(self, a, greedy_a=None):
        if self.n_moves == self._a.shape[0]:
            self._a = torch.cat([self._a, torch.zeros_like(self._a)])
            self._g = torch.cat([self._g, torch.zeros_like(self._g)])
            self._s = torch.cat([self._s, torch.zeros_like(self._s)])
        self._a[self.n_moves].copy_(a.view(self.G, self.P))
        self._g[self.n_moves].copy_((a if greedy_a is None else greedy_a).view(self.G, self.P))
        self.n_moves += 1

    def observed(self, env):
        """after the step of the move just appended: keeps what the root's rows now show of the greedy action"""
        if env.sad:
            env.sad_section(self._s[self.n_moves - 1])

    @property
    def sad(self):
        return self._s[:self.n_moves]

    @property
    def a(self):
        return self._a[:self.n_moves]

    @property
    def greedy_a(self):
        return self._g[:self.n_moves]


class _WorldChunk:
    """`capacity` world slots of the replay stage: their env and the agent's state after the replay"""

    def __init__(self, env):
        self.env, self.h, self.c = env, None, None


class _Drawn:
    """sampler="learned", one search call: the root games' logits and where the kernel's log-probabilities are kept per (game,
    world) -- row G takes the writes of the spare slots"""

    def __init__(self, logits, G, worlds, dev):
        self.logits, self.G = logits, G
        self.logp = torch.full((G + 1, worlds), float("nan"), dtype=torch.float32, device=dev)
        self.logp0 = torch.full((G + 1, worlds), float("nan"), dtype=torch.float32, device=dev)

    def scatter(self, g_c, w_c, valid, got):
        status, logp, logp0 = got
        dev = self.logp.device
        gi = torch.from_numpy(np.where(valid, g_c, self.G).astype(np.int64)).to(dev)
        wi = torch.from_numpy(np.asarray(w_c, dtype=np.int64)).to(dev)
        nan = torch.full_like(logp, float("nan"))
        # every slot of a (game, world) holds the same hand, so the duplicate writes carry the same bits
        self.logp[gi, wi] = torch.where(status == 1, logp, nan)
        self.logp0[gi, wi] = torch.where(status == 1, logp0, nan)


class PolicySearch:
    """The search env of `capacity` slots, the agent's state buffers for its capacity * P rows and the host loop that plays one
    chunk of jobs; search() may be called move after move (play_with_search does).  `like` is any env with the root's rules.
    replay=True: search() takes the root's GameLog and rebuilds the LSTM states of every sampled world by replay (world envs of
    `capacity` slots each, made when first needed and kept); consistent_only=True then counts only the worlds without a mismatch.
    sampler: "rejection" (determinize) or "stratified" (determinize_exact, world w of a game in stratum w of `worlds`), for the
    act chunks and the world envs of the replay stage alike; or "learned" with belief= (a belief.BeliefSampler, or what makes
    one: a BeliefHead, a head's state dict, its file): determinize_belief_worlds under the head's logits for the root act's state.
    ValueError -- before any device work -- for "learned" without a belief, a belief with another sampler, a head whose trunk
    width or hand size is not the agent's / the env's, and a skip_connect agent.
    depth=D (None: every world is played to the end of its game, as ever): a chunk plays the forced action and D more blueprint
    moves -- D + 1 act / step iterations with no host read-back -- then acts once more with with_q=True without stepping, and
    hsad_search_horizon_stats values every world still running as its score so far + that Q (horizon_value "mover": the Q of the
    seat on turn; "team": the sum over the game's seats), worlds that ended within the depth as their final score; SearchValues is
    then in fixed point (scale = 256) and carries cut / nonfinite.  ValueError -- before any device work -- for a depth that is
    no int in [0, max_steps), another horizon_value, and a skip_connect agent (its cached Q is undefined)."""

    def __init__(self, like, agent, capacity=4096, max_steps=200, replay=False, consistent_only=False, sampler="rejection", belief=None,
                 depth=None, horizon_value="mover"):
        self.agent, self.capacity, self.max_steps = agent, int(capacity), int(max_steps)
        self.depth, self.horizon_value = _check_depth(depth, horizon_value, max_steps, agent), horizon_value
        self.sampler = _check_sampler(sampler)
        _check_belief(sampler, belief, agent, like.H)
        self.belief = belief
        self.replay, self.consistent_only = bool(replay), bool(consistent_only)
        if self.consistent_only and not self.replay:
            raise ValueError("consistent_only needs replay=True: the mismatch count comes from the replay")
        self.device = dev = like.device
        if belief is not None and not hasattr(belief, "logits"):
            from .belief import BeliefSampler
            self.belief = BeliefSampler(belief, str(dev))
        self.bf16 = bool(getattr(agent, "accepts_bf16_obs", False))
        self.env = env = self._make_env(like.config)
        self.config, self.worlds_env = dict(like.config), []
        self.lib = env.lib
        env.reset()       # spare slots of a short chunk hold started games: they play on with the rest and are never counted
        N = self.capacity * env.P
        z = agent.get_h0(N)
        self.h, self.c = torch.zeros_like(z["h0"]).contiguous(), torch.zeros_like(z["c0"]).contiguous()
        self.h16 = torch.zeros(self.h.shape, dtype=torch.bfloat16, device=dev) if N >= 1024 else None
        self.eps = torch.zeros(N, dtype=torch.float32, device=dev)
        self.stats4 = torch.zeros(1, 4, dtype=torch.int64, device=dev)
        self.unfinished = torch.zeros(1, dtype=torch.int32, device=dev)
        self.host = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(2)]
        self.copied = [torch.cuda.Event() for _ in range(2)]
        self.iterations = 0        # env steps of the last search, over all its chunks
        self.open_games = []       # the "games still running" words the host read during the last search (one per step, one step late)
        self.round_jobs = []       # jobs played per round of the last search in rounds
        self.acts = 0              # agent.act calls of the last search, over all its stages
        self.q_rows = None         # depth-limited search: Q_online(s, a) of the search env's rows at the horizon of the last chunk
        if self.depth is not None:
            import inspect
            self._defer = "defer_target" in inspect.signature(agent.act).parameters     # the online net alone, where the agent can

    def _make_env(self, config):
        env = BatchedHanabiEnv(self.capacity, seed=0, eps_list=(0.0,), device=str(self.device), track_deck_history=False, **config)
        if self.bf16:     # a bf16 kernel agent reads the env's packed rows: the first GEMM's operand, written by the env itself
            env.enable_packed(bf16_row_len=self.agent.online.Fp, keep_float32=False)
        return env

    def close(self):
        self.env.close()
        for w in self.worlds_env:
            w.env.close()
        self.worlds_env = []

    def _obs(self, env=None):
        env = self.env if env is None else env
        N = env.G * env.P
        if self.bf16:
            return {"priv_s_bf16": env.priv_s_bf16.view(N, -1), "legal_move": env.legal_move.view(N, env.A), "eps": self.eps}
        return {"priv_s": env.priv_s.view(N, env.F), "legal_move": env.legal_move.view(N, env.A), "eps": self.eps}

    def _play_chunk(self, player, override, bp_rows):
        """greedy acting for every seat of every slot until all games of the search env have ended; the candidate action is forced
        on iteration 0 only.  -> the greedy actions of the rows `bp_rows` at iteration 0 (the blueprint's move at the root)"""
        env, lib, agent = self.env, self.lib, self.agent
        hid = {"h0": self.h, "c0": self.c}
        if self.h16 is not None:
            hid["h0_16"] = self.h16
        if self.depth is not None:
            return self._play_chunk_to_depth(player, override, bp_rows, hid)
        bp, done = None, False
        for t in range(self.max_steps):
            reply, hid = agent.act(self._obs(), hid)
            self.acts += 1
            a, g = reply["a"].contiguous(), reply["greedy_a"].contiguous()
            if t == 0 and bp_rows is not None:
                bp = g[bp_rows]
            _lib.check(lib.hsad_search_actions(env.h, a.data_ptr(), g.data_ptr(), player.data_ptr(), override.data_ptr() if t == 0 else None,
                                               env.a.data_ptr(), env.greedy_a.data_ptr(), env._stream()))
            env.step(env.a, env.greedy_a)
            _lib.check(lib.hsad_seating_stats(env.h, env.G, self.stats4.data_ptr(), self.unfinished.data_ptr(), env._stream()))
            # the host looks at ONE word, and one step late (eval._TournamentBatch.play): it never waits for the step it has just
            # enqueued; the extra step at the end only hands finished games their noop
            self.host[t & 1].copy_(self.unfinished, non_blocking=True)
            self.copied[t & 1].record(torch.cuda.current_stream(self.device))
            self.iterations += 1
            if t > 0:
                self.copied[(t - 1) & 1].synchronize()
                left = int(self.host[(t - 1) & 1][0])
                self.open_games.append(left)
                if left == 0:
                    done = True
                    break
        if not done and int(self.unfinished.cpu()[0]) != 0:
            raise RuntimeError("%d game(s) of the search env still running after %d steps" % (int(self.unfinished.cpu()[0]), self.max_steps))
        return bp

    def _play_chunk_to_depth(self, player, override, bp_rows, hid):
        """the forced action and `depth` more greedy moves for every seat of every slot, then one act with Q on the position reached
        and no step after it: nothing here reads the device, the host never waits.  -> as _play_chunk; the Q rows in self.q_rows"""
        env, lib, agent = self.env, self.lib, self.agent
        bp = None
        for t in range(self.depth + 1):
            reply, hid = agent.act(self._obs(), hid)
            a, g = reply["a"].contiguous(), reply["greedy_a"].contiguous()
            if t == 0 and bp_rows is not None:
                bp = g[bp_rows]
            _lib.check(lib.hsad_search_actions(env.h, a.data_ptr(), g.data_ptr(), player.data_ptr(), override.data_ptr() if t == 0 else None,
                                               env.a.data_ptr(), env.greedy_a.data_ptr(), env._stream()))
            env.step(env.a, env.greedy_a)
            self.iterations += 1
        counter = getattr(agent, "counter", None)
        if self._defer:
            reply, _ = agent.act(self._obs(), hid, with_q=True, defer_target=True)
        else:
            reply, _ = agent.act(self._obs(), hid, with_q=True)
        if counter is not None:      # the valuing act is no move of the agent's: its exploration counter stays where it was
            agent.counter = counter
        self.acts += self.depth + 2
        self.q_rows = reply["q_online_a"].contiguous()
        return bp

    def _replay(self, root, log, games, cur, worlds, seed, seed_of, drawn=None):
        """the replay stage: world slot i * worlds + w = world w of root game games[i], `capacity` slots per world env.  Per env: fork
        the root with the world seeds, determinize, hsad_search_world_script, hsad_env_rewind_scripted, zero agent state, then per
        logged move agent.act -> hsad_search_replay_actions -> step -> (sad = 1) hsad_env_observe_sad with the section the root's
        rows showed after that move.  -> mismatch int32 [len(games) * worlds] on the device"""
        from .eval import _drain_errors
        if log is None or (log.G, log.P) != (root.G, root.P):
            raise ValueError("replay=True needs log=, the GameLog of the root's %d x %d action rows" % (root.G, root.P))
        cap, dev, lib, agent, G, P = self.capacity, self.device, self.lib, self.agent, root.G, root.P
        nw = len(games) * worlds
        n_chunk = (nw + cap - 1) // cap
        while len(self.worlds_env) < n_chunk:
            self.worlds_env.append(_WorldChunk(self._make_env(self.config)))
        dh, cnt = root.deck_history()
        if int(cnt.max()) == 0:
            raise ValueError("replay=True needs a root env built with track_deck_history=True")
        dh = torch.nn.functional.pad(dh, (0, 2)).contiguous()
        n_moves = log.n_moves
        la, lg = log.a, log.greedy_a
        mismatch = torch.zeros(n_chunk * cap, dtype=torch.int32, device=dev)
        script = torch.zeros(cap, 52, dtype=torch.uint8, device=dev)
        count = torch.zeros(cap, dtype=torch.int32, device=dev)
        for ci in range(n_chunk):
            w = self.worlds_env[ci]
            env = w.env
            k = np.arange(ci * cap, (ci + 1) * cap)
            valid = k < nw
            kk = np.minimum(k, nw - 1)
            g_c, w_c = games[kk // worlds], kk % worlds
            src = torch.from_numpy(np.where(valid, g_c, -1).astype(np.int32)).to(dev)
            seeds = torch.from_numpy(seed_of[g_c, w_c]).to(dev)
            key = torch.from_numpy((g_c << 32) | w_c).to(dev)
            viewer = torch.from_numpy(np.where(valid, cur[g_c], -1).astype(np.int32)).to(dev)
            env.reseed(0)       # every slot "not started": the spare ones get the noop and never hold a world of an earlier search
            env.fork_from(root, src, seeds)
            world_d = torch.from_numpy(w_c.astype(np.int32)).to(dev)
            got = _sample_hands(env, self.sampler, viewer, key, seed, world_d, worlds, (drawn.logits, src) if drawn is not None else None)
            if drawn is not None:
                drawn.scatter(g_c, w_c, valid, got)
            _lib.check(lib.hsad_search_world_script(env.h, src.data_ptr(), viewer.data_ptr(), dh.data_ptr(), cnt.data_ptr(), G,
                                                    la.data_ptr() if n_moves else None, n_moves, script.data_ptr(), count.data_ptr(),
                                                    env._stream()))
            env.rewind_scripted(script, count)
            src = torch.where(count > 0, src, torch.full_like(src, -1))     # a slot whose script was refused replays nothing
            z = agent.get_h0(cap * P)
            hid = {"h0": torch.zeros_like(z["h0"]).contiguous(), "c0": torch.zeros_like(z["c0"]).contiguous()}
            if self.h16 is not None:
                hid["h0_16"] = torch.zeros_like(self.h16)
            mm = mismatch[ci * cap:(ci + 1) * cap]
            for t in range(n_moves):
                reply, hid = agent.act(self._obs(env), hid)
                self.acts += 1
                g = reply["greedy_a"].contiguous()
                _lib.check(lib.hsad_search_replay_actions(env.h, src.data_ptr(), viewer.data_ptr(), la[t].data_ptr(), lg[t].data_ptr(), G,
                                                          g.data_ptr(), env.a.data_ptr(), env.greedy_a.data_ptr(), mm.data_ptr(),
                                                          env._stream()))
                env.step(env.a, env.greedy_a)
                if env.sad:     # every seat saw the greedy action as the TRUE cards showed it, whatever hand this world holds
                    env.observe_sad(src, log.sad[t])
            w.h, w.c = hid["h0"].contiguous(), hid["c0"].contiguous()
            n_err, g_err, code = _drain_errors(env)   # finished and spare slots were handed the noop: code 3 notes
            if n_err and code != 3:
                raise RuntimeError("replay: %d game(s) of the world env left their history; first: slot %d, code %d" % (n_err, g_err, code))
        return mismatch[:nw]

    def _rounds(self, play, rounds, z2, min_n, scores, pairs, games, first_pair, blueprint):
        """the round loop of search(rounds=...).  Round r plays the next rounds[r] worlds of round_world_order for every pair still
        alive, jobs in (pair, world-order) order and chunked by capacity like the flat search; then hsad_search_round names each game's
        leader, fills the paired tables and prunes, and `alive` comes to the host: the one synchronisation of the round.  The job lists
        stay host-built numpy: per chunk a few thousand entries against tens of act steps.
        -> (paired against the blueprint's action int64 [n_pair, 3] on the device, pruned_round int32 [n_pair] numpy)"""
        cap, dev, lib, env = self.capacity, self.device, self.lib, self.env
        n_pair, worlds = scores.shape
        n_game = len(games)
        order = np.asarray(round_world_order(worlds), dtype=np.int64)
        first_d = torch.from_numpy(np.append(first_pair, n_pair).astype(np.int32)).to(dev)
        pair_of = torch.full((int(games[-1]) + 1, env.A), -1, dtype=torch.int32, device=dev)      # (game, action) -> pair
        pd = torch.from_numpy(pairs).to(dev)
        pair_of[pd[:, 0], pd[:, 1]] = torch.arange(n_pair, dtype=torch.int32, device=dev)
        games_d = torch.from_numpy(games).to(dev)
        alive_d = torch.ones(n_pair, dtype=torch.uint8, device=dev)
        leader = torch.zeros(n_game, dtype=torch.int32, device=dev)
        raw = torch.zeros(n_pair, 2, dtype=torch.int64, device=dev)
        paired_ref, paired_bp = torch.zeros(n_pair, 3, dtype=torch.int64, device=dev), torch.zeros(n_pair, 3, dtype=torch.int64, device=dev)
        alive = np.ones(n_pair, dtype=bool)
        pruned_round = np.full(n_pair, -1, dtype=np.int32)
        game_of_pair = np.searchsorted(first_pair, np.arange(n_pair), side="right") - 1
        bp_pair, off = None, 0
        for r, n_w in enumerate(rounds):
            ws = order[off:off + n_w]
            off += n_w
            # a game down to one alive pair -- necessarily the blueprint's -- has nothing left to compare
            left = np.bincount(game_of_pair[alive], minlength=n_game)
            ap = np.nonzero(alive & (left[game_of_pair] > 1))[0] if r else np.arange(n_pair)
            n = len(ap) * n_w
            self.round_jobs.append(n)
            if n == 0:
                break
            # round 0 holds every pair, world 0 first: the first job of each game's first pair is where the blueprint's move is read
            first_job = first_pair * n_w
            for c0 in range(0, n, cap):
                k = np.arange(c0, c0 + cap)
                kk = np.minimum(k, n - 1)
                here = (first_job >= c0) & (first_job < c0 + cap) if r == 0 else np.zeros(n_game, dtype=bool)
                play(ap[kk // n_w], ws[kk % n_w], k < n, first_job - c0, here)
            if bp_pair is None:
                bp_a = blueprint[games_d]
                bp_pair = torch.where(bp_a >= 0, pair_of[games_d, bp_a.clamp(min=0)], torch.full_like(leader, -1)).contiguous()
            _lib.check(lib.hsad_search_round(scores.data_ptr(), n_pair, worlds, first_d.data_ptr(), n_game, bp_pair.data_ptr(), z2[0], z2[1],
                                             int(min_n), alive_d.data_ptr(), leader.data_ptr(), raw.data_ptr(), paired_ref.data_ptr(),
                                             paired_bp.data_ptr(), env._stream()))
            now = alive_d.cpu().numpy() != 0
            pruned_round[alive & ~now] = r
            alive = now
        return paired_bp, pruned_round

    def search(self, root, hid, worlds, seed, searcher=None, log=None, rounds=None, prune_z=2.0, min_n=2, hid_next=None,
               keep_world_values=False):
        """-> SearchValues for the root env's games; root and hid ({"h0", "c0"}: [L, root.G * root.P, H], the agent's state entering
        the root step) are only read.  log: the root's GameLog (replay=True).  rounds: None, or world counts per round (their sum is
        `worlds`) for the search in rounds with pruning at prune_z paired standard errors.  hid_next (sampler="learned" only): the
        agent's state AFTER the root act, whose top layer's h is what the belief head reads; None: the search runs that one act on
        the root's float32 rows itself.  keep_world_values: SearchValues.world_values, every world's value by itself (one more
        kernel per chunk without a depth; none with one).  See policy_action_values."""
        from .eval import _drain_errors
        z2 = None
        depth = self.depth
        if rounds is not None and depth is not None:
            raise ValueError("search(rounds=...) with a depth is out of scope: hsad_search_round compares whole uint8 scores, a "
                             "depth-limited search counts in 1/256 points")
        if rounds is not None:
            rounds, *z2 = _check_rounds(rounds, worlds, prune_z, min_n)
        G, P, A, cap = root.G, root.P, root.A, self.capacity
        dev, env, lib = self.device, self.env, self.lib
        if (P, A) != (env.P, env.A):
            raise ValueError("the root env has %d players / %d actions, the search env %d / %d" % (P, A, env.P, env.A))
        h_src, c_src = hid["h0"], hid["c0"]
        if tuple(h_src.shape) != (self.h.shape[0], G * P, self.h.shape[2]) or h_src.shape != c_src.shape:
            raise ValueError("hid must hold h0 / c0 of shape [%d, %d, %d]; got %s" % (self.h.shape[0], G * P, self.h.shape[2], tuple(h_src.shape)))
        h_src, c_src = h_src.contiguous(), c_src.contiguous()
        self.iterations, self.open_games, self.round_jobs, self.acts = 0, [], [], 0
        scale = 1 if depth is None else VALUE_SCALE
        totals = torch.zeros(G, A, 3, dtype=torch.int64, device=dev)
        blueprint = torch.full((G,), -1, dtype=torch.int64, device=dev)
        pairs, cur = search_jobs(root)
        if len(pairs):
            pairs = pairs[_searched_games(searcher, cur, G)[pairs[:, 0]]]
        if len(pairs) == 0 or worlds < 1:
            extra = {}
            if rounds is not None:
                extra = dict(paired=torch.zeros(G, A, 3, dtype=torch.int64, device=dev),
                             pruned_round=torch.full((G, A), -1, dtype=torch.int32, device=dev),
                             world_scores=torch.full((G, A, worlds), 0xFF, dtype=torch.uint8, device=dev))
            if depth is not None:
                extra.update(scale=scale, cut=torch.zeros(G, A, dtype=torch.int64, device=dev))
            if keep_world_values:
                extra.update(world_values=torch.full((G, A, max(worlds, 0)), -1, dtype=torch.int16, device=dev).view(torch.uint16))
            return SearchValues(totals, blueprint, torch.zeros(G, max(worlds, 0), dtype=torch.int32, device=dev) if self.replay else None,
                                **extra)
        drawn = None
        if self.sampler == "learned":
            if hid_next is None:
                N, counter = G * P, getattr(self.agent, "counter", None)
                obs = {"priv_s": root.priv_s.view(N, root.F), "legal_move": root.legal_move.view(N, A),
                       "eps": torch.zeros(N, dtype=torch.float32, device=dev)}
                hid_next = self.agent.act(obs, {"h0": h_src, "c0": c_src})[1]
                self.acts += 1
                if counter is not None:      # the extra act is no move of the agent's: its exploration counter stays where it was
                    self.agent.counter = counter
            h_top = hid_next["h0"]
            if tuple(h_top.shape) != tuple(h_src.shape):
                raise ValueError("hid_next must hold h0 of shape %s; got %s" % (tuple(h_src.shape), tuple(h_top.shape)))
            player = torch.from_numpy(cur.astype(np.int32)).to(dev)
            drawn = _Drawn(self.belief.logits(h_top[h_top.shape[0] - 1].contiguous(), player), G, worlds, dev)
        n_job = len(pairs)
        n = n_job * worlds                                   # jobs in (game, action, world) order; job k works for pair k // worlds
        games, first_pair = np.unique(pairs[:, 0], return_index=True)
        seed_of = np.zeros((G, worlds), dtype=np.int32)      # common random numbers: a world's seed and key know (game, world) only
        for g in games:
            seed_of[g] = [world_seed(seed, int(g), w) for w in range(worlds)]
        first_job = first_pair * worlds                      # world 0 of each game's first job: where the blueprint's own move is read
        stats = torch.zeros(n_job, 3, dtype=torch.int64, device=dev)
        L, H = self.h.shape[0], self.h.shape[2]
        keep = mismatch = None
        if self.replay:
            mism = self._replay(root, log, games, cur, worlds, seed, seed_of, drawn).view(len(games), worlds)
            mismatch = torch.zeros(G, worlds, dtype=torch.int32, device=dev)
            mismatch[torch.from_numpy(games).to(dev)] = mism
            if self.consistent_only:      # a game with no consistent world falls back to all of its worlds
                keep = mism == 0
                keep = torch.where(keep.any(dim=1, keepdim=True), keep, torch.ones_like(keep))
            game_pos = np.zeros(G, dtype=np.int64)
            game_pos[games] = np.arange(len(games))
        scores = None
        if rounds is not None or (keep_world_values and depth is None):
            scores = torch.full((n_job, worlds), 0xFF, dtype=torch.uint8, device=dev)
        cut = nonfinite = wv = None
        if depth is not None:
            cut, nonfinite = torch.zeros(n_job, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
            mode = HORIZON_VALUES.index(self.horizon_value)
            if keep_world_values:      # 0xFFFF = not played; index_put and fill know int16, the caller sees the same words as uint16
                wv = torch.full((n_job, worlds), -1, dtype=torch.int16, device=dev)

        def play(pj, w_c, valid, bp_slot, here):
            """one chunk: slot i plays world w_c[i] of pair pj[i] where valid[i]; bp_slot[here] are the slots whose first act is the
            blueprint's own move of the games games[here]"""
            g_c, a_c = pairs[pj, 0], pairs[pj, 1]
            src = torch.from_numpy(np.where(valid, g_c, -1).astype(np.int32)).to(dev)      # spare slots: no fork, no job
            seeds = torch.from_numpy(seed_of[g_c, w_c]).to(dev)
            key = torch.from_numpy((g_c << 32) | w_c).to(dev)
            player = torch.from_numpy(np.where(valid, cur[g_c], -1).astype(np.int32)).to(dev)
            override = torch.from_numpy(np.where(valid, a_c, -1).astype(np.int64)).to(dev)
            job = torch.from_numpy(np.where(valid, pj, -1).astype(np.int32)).to(dev)
            if not self.replay:
                env.fork_from(root, src, seeds)
                world_d = torch.from_numpy(w_c.astype(np.int32)).to(dev)
                got = _sample_hands(env, self.sampler, player, key, seed, world_d, worlds, (drawn.logits, src) if drawn is not None else None)
                if drawn is not None:
                    drawn.scatter(g_c, w_c, valid, got)
                _lib.check(lib.hsad_search_fork_state(src.data_ptr(), cap, G, P, L, H, h_src.data_ptr(), c_src.data_ptr(), self.h.data_ptr(),
                                                      self.c.data_ptr(), self.h16.data_ptr() if self.h16 is not None else None, env._stream()))
            else:
                # the worlds stand in the world envs, determinised and replayed: fork them and their rebuilt h / c, with the world
                # seeds again (the generator a fork of the root would have)
                ws = game_pos[g_c] * worlds + w_c
                for wc in np.unique(ws[valid] // cap):
                    w = self.worlds_env[int(wc)]
                    src_w = torch.from_numpy(np.where(valid & (ws // cap == wc), ws % cap, -1).astype(np.int32)).to(dev)
                    env.fork_from(w.env, src_w, seeds)
                    _lib.check(lib.hsad_search_fork_state(src_w.data_ptr(), cap, cap, P, L, H, w.h.data_ptr(), w.c.data_ptr(), self.h.data_ptr(),
                                                          self.c.data_ptr(), self.h16.data_ptr() if self.h16 is not None else None,
                                                          env._stream()))
                if keep is not None:
                    kept = keep[torch.from_numpy(game_pos[g_c]).to(dev), torch.from_numpy(w_c).to(dev)]
                    job = torch.where(kept, job, torch.full_like(job, -1))
            bp_rows = None
            if here.any():
                bp_rows = torch.from_numpy(bp_slot[here] * P + cur[games[here]]).to(dev)
            bp = self._play_chunk(player, override, bp_rows)
            if bp is not None:
                blueprint[torch.from_numpy(games[here]).to(dev)] = bp
            if depth is not None:
                world_d = torch.from_numpy(w_c.astype(np.int32)).to(dev) if wv is not None else None
                _lib.check(lib.hsad_search_horizon_stats(env.h, job.data_ptr(), n_job, self.q_rows.data_ptr(), mode, stats.data_ptr(),
                                                         cut.data_ptr(), nonfinite.data_ptr(), world_d.data_ptr() if wv is not None else None,
                                                         worlds, wv.data_ptr() if wv is not None else None, env._stream()))
                return
            _lib.check(lib.hsad_search_job_stats(env.h, job.data_ptr(), n_job, stats.data_ptr(), env._stream()))
            if scores is not None:
                world_d = torch.from_numpy(w_c.astype(np.int32)).to(dev)
                _lib.check(lib.hsad_search_world_scores(env.h, job.data_ptr(), world_d.data_ptr(), n_job, worlds, scores.data_ptr(),
                                                        env._stream()))

        if rounds is None:
            for c0 in range(0, n, cap):
                k = np.arange(c0, c0 + cap)
                kk = np.minimum(k, n - 1)
                play(kk // worlds, kk % worlds, k < n, first_job - c0, (first_job >= c0) & (first_job < c0 + cap))
        else:
            extra = self._rounds(play, rounds, z2, min_n, scores, pairs, games, first_pair, blueprint)
        _drain_errors(env)        # finished games were handed the noop: the "step on a finished game" notes
        pd = torch.from_numpy(pairs).to(dev)
        totals[pd[:, 0], pd[:, 1]] = stats
        lp = dict(belief_logp=drawn.logp[:G], belief_logp0=drawn.logp0[:G]) if drawn is not None else {}
        if depth is not None:
            cut_ga = torch.zeros(G, A, dtype=torch.int64, device=dev)
            cut_ga[pd[:, 0], pd[:, 1]] = cut
            lp.update(scale=scale, cut=cut_ga, nonfinite=int(nonfinite.cpu()[0]))
        if keep_world_values:
            table = torch.full((G, A, worlds), -1, dtype=torch.int16, device=dev)
            # without a depth the table is hsad_search_world_scores' bytes widened: whole points (scale = 1), 0xFF -> 0xFFFF
            table[pd[:, 0], pd[:, 1]] = wv if wv is not None else torch.where(scores == 0xFF, -1, scores.to(torch.int16)).to(torch.int16)
            lp.update(world_values=table.view(torch.uint16))
        if rounds is None:
            return SearchValues(totals, blueprint, mismatch, **lp)
        paired = torch.zeros(G, A, 3, dtype=torch.int64, device=dev)
        pruned = torch.full((G, A), -1, dtype=torch.int32, device=dev)
        table = torch.full((G, A, worlds), 0xFF, dtype=torch.uint8, device=dev)
        paired[pd[:, 0], pd[:, 1]] = extra[0]
        pruned[pd[:, 0], pd[:, 1]] = torch.from_numpy(extra[1]).to(dev)
        table[pd[:, 0], pd[:, 1]] = scores
        return SearchValues(totals, blueprint, mismatch, paired=paired, pruned_round=pruned, world_scores=table, **lp)


def policy_action_values(root, agent, hid, worlds, seed, capacity=4096, max_steps=200, searcher=None, replay=False, log=None,
                         consistent_only=False, sampler="rejection", rounds=None, prune_z=2.0, min_n=2, belief=None, hid_next=None,
                         depth=None, horizon_value="mover", keep_world_values=False):
    """SearchValues: values[g, a] = mean final score (HSAD_Q_SCORE) over `worlds` sampled worlds when the player on turn of root game
    g plays a and EVERY player, the searcher included, then follows the blueprint `agent` greedily to the end of the game.

    agent: what eval._acting_agent produces.  An agent with accepts_bf16_obs reads the search env's packed bf16 rows, any other the
    float32 rows.  hid: the agent's state entering the root step, {"h0", "c0"} as [L, root.G * root.P, H]; read, never written, and
    neither is the root env.  searcher: None, a seat number or an int [G] mask -- games whose player on turn does not search get no
    jobs, all-NaN rows and blueprint_a = -1.

    Jobs are (root game, legal action of the player on turn, world), keyed and seeded as in mc_action_values (world_seed / world_key:
    every action of a game meets the same worlds).  Per chunk of `capacity` jobs: fork_from with the seeds, determinize for the player
    on turn, hsad_search_fork_state (the root game's LSTM state into every seat of its forks), then the loop -- agent.act on all
    capacity * P rows, hsad_search_actions (the candidate action forced on iteration 0, the noop for finished games), env.step,
    hsad_seating_stats for the one word the host reads a step late -- and hsad_search_job_stats.  The first act of a chunk is also
    the blueprint's own move at the root (the searcher does not observe its own hand, so its row is the root's): blueprint_a.
    RuntimeError if games are still running after max_steps.

    The result does not depend on `capacity` (a job knows (game, action, world), never its slot; a row's result depends on no other
    row) AS LONG AS every act call stays in one acting regime: at 1,024 rows the act kernels switch to the fused GEMM + cell path
    (net_step in csrc/hsad_agent.hip, CompositeAgent.act, R2D2Agent._fused), whose bf16 rounding differs.  capacity * P below 1,024
    and capacity * P from 1,024 up are two regimes.

    replay=False: every seat of a fork starts from the LSTM state its root game carries -- the partners' states are those of the TRUE
    world, although in a sampled world their observations differed in the searcher's hand.  replay=True (needs log, the root's
    GameLog, and a root that tracks its deck history) rebuilds them: before the act chunks, every world (root game, w) is forked,
    determinised, rewound to its first deal with the sampled hand in the deal script (hsad_search_world_script,
    hsad_env_rewind_scripted) and played again move by move from zero state with the logged actions forced
    (hsad_search_replay_actions) and, with sad = 1, the greedy-action section of the rows forced to what the root's rows showed
    (GameLog.sad, hsad_env_observe_sad: that section was computed from the true cards and seen by every seat, so a sampled world
    must show it too -- which also keeps the searcher's own replayed state equal to the one it carries); the act chunks then fork the worlds and their h / c from the world envs.  A world's cards and
    generator are the same either way.  SearchValues.mismatch counts, per world, the partner moves whose greedy action differs in
    that world; consistent_only=True leaves worlds with a mismatch out of the totals (all worlds where none is consistent).  The
    replay costs one act + step per logged move on all searched games x worlds slots.

    sampler="stratified": the hands come from determinize_exact(stratum = world, n_strata = worlds) wherever determinize is named
    above, the world envs of the replay included (see mc_action_values).

    sampler="learned" with belief= (belief.BeliefSampler, or a BeliefHead / state dict / file to make one from): the hands come from
    the learned belief instead.  Once per call the head's logits are computed for the player on turn of every root game from
    hid_next["h0"][L - 1] -- the agent's state AFTER the root act (play_with_search has it; None: one agent.act on the root's
    rows here) -- by hsad_search_belief_rows and the head's GEMM; every sampler call is then determinize_belief_worlds with row =
    the slot's root game, group = world_key(g, 0), world = w, n_worlds = worlds and the search seed.  A (game, world) hand depends
    on (seed, game, world) and the root's logits only -- not on the action, chunk, slot or capacity -- and is the same in the
    replay stage's world envs; the worlds of a game are stratified per slot of the hand (include/hsad.h,
    hsad_env_determinize_belief_worlds).  SearchValues.belief_logp / belief_logp0 carry each world's log-probability under the
    learned and the exact belief.  A game whose logits row is not finite keeps its true hand in every world.  ValueError for
    "learned" without belief, belief with another sampler, a head not matching the agent's width or the env's hand size, a
    skip_connect agent.

    rounds=(n0, n1, ...) (positive, summing to `worlds` <= 4,096; None = the flat search above, untouched): the worlds are played in
    rounds and actions that are already hopeless are dropped in between.  A game's worlds are taken in round_world_order; round r
    plays its next rounds[r] worlds for every action still alive (jobs in (action, world-order) order, chunked as above -- a (game,
    action, world) job is the very job of the flat search: same stratum, seed and key, whenever it runs).  Each chunk also stores its
    scores per world (hsad_search_world_scores), and after each round hsad_search_round picks the game's leader (largest raw mean
    among the alive actions, exact, lowest action on ties), sums d = score - leader's score world by world and drops an action iff it
    was played in >= min_n shared worlds and its paired mean lies more than prune_z paired standard errors below zero (prune_z^2 as
    Fraction(z * z).limit_denominator(1024), numerator <= 16,384; equality keeps the action).  The leader and the blueprint's own
    action are never dropped; a game down to one action plays no more.  The host reads `alive` once per round.  The replay stage is
    not split: it replays all worlds up front.  SearchValues then carries paired / paired_mean / paired_sem (against the blueprint's
    action), pruned_round and world_scores; totals / values count the worlds each action was played in.

    depth=D (None = all of the above, untouched: the same calls, the same bits): the worlds are not played to the end.  A chunk runs
    D + 1 iterations of act -> hsad_search_actions -> env.step (the candidate action, then D blueprint moves) with no
    hsad_seating_stats and no host read-back, then ONE more act with with_q=True on the position reached (defer_target=True where
    the agent takes it: the online net alone; the env is not stepped after it and the agent's counter is put back), and
    hsad_search_horizon_stats in place of hsad_search_job_stats: a world that ended within the depth counts 256 x its final score,
    a world still running counts 256 x its score so far + the blueprint's Q rounded to 1/256 -- horizon_value="mover": Q_online(s, a)
    of the seat on turn; "team": the fp32 sum over the game's seats in seat order (VDN's joint value) -- clamped to [0, 256 x the
    perfect score]; a Q that is not finite counts as 0 and is reported (SearchValues.nonfinite).  A searched move then costs D + 2
    act calls per chunk whatever the game's length.  SearchValues.scale = 256, totals in 1/256 points, values / sem in points, cut =
    the worlds valued at the horizon.  How good the value is depends on how well the agent's Q is calibrated (clone --value_weight
    fits it to recorded returns); a random net's Q says nothing.  Samplers, replay, searcher and consistent_only work as above.
    ValueError before any device work: depth no int in [0, max_steps), horizon_value not "mover" / "team", a skip_connect agent;
    and for rounds= together with a depth (hsad_search_round compares whole uint8 scores: out of scope).
    keep_world_values=True: SearchValues.world_values uint16 [G, A, worlds], every world's own value in units of 1 / scale (0xFFFF =
    not played) -- with a depth written by hsad_search_horizon_stats, without one hsad_search_world_scores' table widened."""
    ps = PolicySearch(root, agent, capacity, max_steps, replay=replay, consistent_only=consistent_only, sampler=sampler, belief=belief,
                      depth=depth, horizon_value=horizon_value)
    try:
        return ps.search(root, hid, worlds, seed, searcher, log=log, rounds=rounds, prune_z=prune_z, min_n=min_n, hid_next=hid_next,
                         keep_world_values=keep_world_values)
    finally:
        ps.close()


def choose_action(values, blueprint_a, threshold=0.05):
    """int64 [G]: the best action (lowest uid on ties) where values[best] - values[blueprint_a] > threshold, else blueprint_a;
    -1 where blueprint_a is -1.  NaN entries never win.  Pure tensor code (CPU tensors work)."""
    v = torch.as_tensor(values)
    bp = torch.as_tensor(blueprint_a).to(torch.int64)
    filled = torch.where(torch.isnan(v), torch.full_like(v, -float("inf")), v)
    best = filled.argmax(dim=1)
    v_best = filled.gather(1, best.unsqueeze(1)).squeeze(1)
    v_bp = filled.gather(1, bp.clamp(min=0).unsqueeze(1)).squeeze(1)
    deviate = (v_best - v_bp) > threshold            # NaN (nothing to compare) is False
    return torch.where(bp < 0, torch.full_like(bp, -1), torch.where(deviate, best, bp))


def choose_action_paired(sv, threshold=0.05, z=0.0):
    """int64 [G] from the SearchValues of a search in rounds: among the actions never pruned -- all played in the same worlds -- the
    one with the largest paired_mean (the mean gain over the blueprint's action, world by world; lowest uid on ties), where that mean
    is > threshold and > z * its paired_sem; else blueprint_a.  -1 where blueprint_a is -1.  Pure tensor code (CPU tensors work)."""
    if sv.paired is None:
        raise ValueError("choose_action_paired needs the SearchValues of a search in rounds (search(rounds=...))")
    pm, ps = sv.paired_mean, sv.paired_sem
    bp = torch.as_tensor(sv.blueprint_a).to(torch.int64)
    out = torch.isnan(pm) | (torch.as_tensor(sv.pruned_round) >= 0)
    filled = torch.where(out, torch.full_like(pm, -float("inf")), pm)
    best = filled.argmax(dim=1)
    m_best = filled.gather(1, best.unsqueeze(1)).squeeze(1)
    s_best = torch.nan_to_num(ps.gather(1, best.unsqueeze(1)).squeeze(1), nan=0.0)
    deviate = (m_best > threshold) & (m_best > z * s_best)     # -inf (no candidate) is False
    return torch.where(bp < 0, torch.full_like(bp, -1), torch.where(deviate, best, bp))


def move_seed(search_seed, move):
    """the search seed of move number `move` of a play_with_search run: a function of (search_seed, move) alone"""
    return _mix64((int(search_seed) & _M64) ^ _mix64(int(move) + 1)) & 0x7FFFFFFFFFFFFFFF


class SearchPlay:
    """what play_with_search returns: scores (list, one per deal), mean, perfect (fraction of perfect games), num_perfect,
    deviations int64 [num_game] (moves where search overrode the blueprint) and trace: per move a pair of int64 [num_game] CPU
    tensors (chosen, blueprint), -1 where the game's player on turn did not search.  From play_with_search(records=...), else None:
    records = the game_record.GameRecord list of the games played (moves = the moves made, search's choices included; greedy = the
    blueprint's), meta = {game, deal_seed, worlds, search_seed}; search_values = one float32 [n_moves, A] numpy array per record, in the
    same order: SearchValues.values of every move, NaN rows where the game's player on turn did not search.
    A depth-limited run (play_with_search(depth=D), else all None) adds: worlds_played / worlds_cut = the worlds counted over all
    moves and how many of them were valued at the horizon, cut_share = their ratio, nonfinite = the Q-values that were not finite;
    its records' meta also carry depth and horizon_value"""

    def __init__(self, scores, perfect_score, deviations, trace, records=None, search_values=None, worlds_played=None, worlds_cut=None,
                 nonfinite=None):
        self.worlds_played, self.worlds_cut, self.nonfinite = worlds_played, worlds_cut, nonfinite
        self.cut_share = None if worlds_cut is None else (worlds_cut / worlds_played if worlds_played else 0.0)
        self.scores = [int(s) for s in scores]
        self.mean = float(np.mean(scores))
        self.num_perfect = int((np.asarray(scores) == perfect_score).sum())
        self.perfect = self.num_perfect / len(self.scores)
        self.sem = float(np.std(scores) / np.sqrt(len(self.scores)))
        self.deviations, self.trace = deviations, trace
        self.records, self.search_values = records, search_values


def play_with_search(agent, num_game, seed, bomb, sad, *, worlds, threshold=0.05, search_seed=0, searcher="all", capacity=4096,
                     num_player=2, hand_size=5, device="cuda:0", max_steps=200, precision="bf16", shuffle_color=False, colors=5, ranks=5,
                     max_information_tokens=8, max_life_tokens=3, replay_history=False, consistent_only=False, sampler="rejection",
                     rounds=None, prune_z=2.0, deviate_z=0.0, records=False, belief=None, depth=None, horizon_value="mover"):
    """eval.evaluate's lock-step loop over the deals seed .. seed + num_game - 1 with search on top of the blueprint -> SearchPlay.
    Before each step: PolicySearch values for the games whose player on turn searches (searcher: "all" or a seat number),
    choose_action, then the root steps with a = the chosen action and greedy_a = the blueprint's greedy action; the carried state
    is advanced by the blueprint's act as usual.  The search seed of a move is move_seed(search_seed, move), so a run repeats
    exactly.  worlds = 0 takes no search path at all and returns evaluate's scores.  The search env has min(capacity, num_game x
    (A - 1) x worlds) slots -- the most jobs a move can have -- and capacity x P decides the acting regime (policy_action_values).
    replay_history=True: the root tracks its deck history, a GameLog keeps the rows it was stepped with and the search rebuilds
    every world's LSTM states by replay (PolicySearch(replay=True)); consistent_only and sampler as there.
    rounds=(n0, n1, ...): every search runs in rounds with pruning at prune_z (policy_action_values) and the move is
    choose_action_paired(sv, threshold, deviate_z) instead of choose_action.
    records=True, or a game_record.GameFilter (as in eval.play_seatings): the games are also written down.  The root tracks its deck
    history, a game_record.GameRecorder appends (a, greedy_a) as the root is stepped with them -- a is the move made, search's choice
    included, greedy_a the blueprint's move -- and every move's SearchValues.values is kept on the device ([max_steps, G, A] float32,
    NaN where no search ran).  SearchPlay.records / .search_values hold the kept games; only those cross to the host.  What search
    found can then be cloned back into the net: clone.search_targets, clone.sequences_from_records(targets=...).  records=False
    changes nothing: no call more per move, the same scores, deviations and trace.
    sampler="learned", belief=...: every search draws its worlds from the learned belief (policy_action_values), with the root act's
    new state -- which this loop has anyway -- as the head's features.  worlds = 0 never looks at the belief beyond the argument
    checks.
    depth=D, horizon_value=...: every search stops D moves after the candidate action and values the worlds still running with the
    blueprint's Q (policy_action_values); SearchPlay then carries worlds_played / worlds_cut / cut_share / nonfinite and the records'
    meta depth and horizon_value.  ValueError as there, rounds= with a depth included.  depth=None changes nothing."""
    if records is False:
        records = None
    _check_depth(depth, horizon_value, max_steps, agent)
    if depth is not None and rounds is not None:
        raise ValueError("rounds= with a depth is out of scope: hsad_search_round compares whole uint8 scores, a depth-limited search "
                         "counts in 1/256 points")
    _check_belief(sampler, belief, None, hand_size)
    if rounds is not None and worlds > 0:
        _check_rounds(rounds, worlds, prune_z, 2)
    from .eval import _acting_agent, _drain_errors
    agent = _acting_agent(agent, precision, device)
    env = BatchedHanabiEnv(num_game, players=num_player, hand_size=hand_size, seed=seed, bomb=bomb, eps_list=[0.0], max_len=-1, sad=bool(sad),
                           shuffle_color=bool(shuffle_color), device=device, track_deck_history=bool(replay_history) or records is not None, colors=colors, ranks=ranks,
                           max_information_tokens=max_information_tokens, max_life_tokens=max_life_tokens)
    seat = None if searcher == "all" else int(searcher)
    if seat is not None and not 0 <= seat < num_player:
        raise ValueError("searcher must be \"all\" or a seat in 0..%d" % (num_player - 1))
    # no move has more jobs than games x playable actions x worlds: a smaller batch needs no more slots than that
    ps = PolicySearch(env, agent, min(int(capacity), num_game * (env.A - 1) * worlds), max_steps, replay=bool(replay_history),
                      consistent_only=bool(consistent_only), sampler=sampler, belief=belief, depth=depth,
                      horizon_value=horizon_value) if worlds > 0 else None
    counted = torch.zeros(2, dtype=torch.int64, device=env.device) if depth is not None else None     # worlds played, worlds cut
    nonfinite = 0
    log = GameLog(num_game, num_player, env.device) if ps is not None and replay_history else None
    N = num_game * num_player
    deviations = torch.zeros(num_game, dtype=torch.int64, device=env.device)
    trace = []
    recorder = kept = kept_values = all_values = None
    try:
        if records is not None:
            from .game_record import GameRecorder
            recorder = GameRecorder(env)
            all_values = torch.full((max_steps, num_game, env.A), float("nan"), dtype=torch.float32, device=env.device)
        hid = agent.get_h0(N)
        env.reset()
        if recorder is not None:
            recorder.clear()
        noop = env.A - 1
        for t in range(max_steps):
            q = env.query()
            done = q[:, Q_TERMINATED] == 1
            if bool(done.all()):
                break
            obs = {"priv_s": env.priv_s.view(N, env.F), "legal_move": env.legal_move.view(N, env.A), "eps": env.eps.view(N)}
            reply, new_hid = agent.act(obs, hid)
            a, g = reply["a"].contiguous(), reply["greedy_a"].contiguous()
            if ps is None:
                live = (~done).unsqueeze(1)
                a = torch.where(live, a.view(num_game, num_player), torch.full_like(a.view(num_game, num_player), noop)).contiguous()
                if recorder is not None:
                    recorder.append(a, a)
                env.step(a, a)
            else:
                sv = ps.search(env, hid, worlds, move_seed(search_seed, t), seat, log=log, rounds=rounds, prune_z=prune_z,
                               hid_next=new_hid if belief is not None else None)
                if counted is not None:
                    counted += torch.stack([sv.totals[..., 2].sum(), sv.cut.sum()])
                    nonfinite += sv.nonfinite
                player = q[:, Q_CUR_PLAYER].contiguous()
                # the blueprint's move is the root act's own greedy action (the search's first act gives the same one while both
                # run in one acting regime; this one holds in any)
                own = g.view(num_game, num_player).gather(1, player.to(torch.int64).clamp(0, num_player - 1).unsqueeze(1)).squeeze(1)
                blueprint = torch.where(sv.blueprint_a >= 0, own, sv.blueprint_a)
                if rounds is None:
                    chosen = choose_action(sv.values, blueprint, threshold)
                else:       # the paired statistics are against the search's blueprint_a: "no deviation" is the root act's own move
                    chosen = choose_action_paired(sv, threshold, deviate_z)
                    chosen = torch.where(chosen == sv.blueprint_a, blueprint, chosen)
                chosen = chosen.contiguous()
                _lib.check(env.lib.hsad_search_actions(env.h, a.data_ptr(), g.data_ptr(), player.data_ptr(), chosen.data_ptr(),
                                                       env.a.data_ptr(), env.greedy_a.data_ptr(), env._stream()))
                if log is not None:
                    log.append(env.a, env.greedy_a)
                if recorder is not None:      # the move about to be made, on the position before it (as the tournament loop logs)
                    recorder.append(env.a, env.greedy_a)
                    all_values[t].copy_(sv.values)
                env.step(env.a, env.greedy_a)
                if log is not None:
                    log.observed(env)
                deviations += ((chosen >= 0) & (chosen != blueprint)).to(torch.int64)
                trace.append((chosen.cpu(), blueprint.cpu()))
            hid = new_hid
        _drain_errors(env)
        scores = env.query()[:, 5].cpu().numpy().astype(np.int64)
        if recorder is not None:      # filtered on the device; only the kept games' records and values cross to the host
            lost = recorder.overflow_count()
            if lost:
                raise _lib.HsadError("the game log overflowed %d time(s): a game ran past the capacity the rules allow" % lost)
            kept = recorder.collect(None if records is True else records)
            index = torch.tensor([rec.meta["game"] for rec in kept], dtype=torch.int64, device=env.device)
            values = all_values.index_select(1, index).cpu().numpy()      # [max_steps, kept, A]
            kept_values = []
            for k, rec in enumerate(kept):
                rec.meta.update(deal_seed=int(seed + rec.meta["game"]), worlds=int(worlds), search_seed=int(search_seed))
                if depth is not None:
                    rec.meta.update(depth=int(depth), horizon_value=horizon_value)
                kept_values.append(np.ascontiguousarray(values[:rec.n_moves, k]))
    finally:
        if recorder is not None:
            recorder.close()
        if ps is not None:
            ps.close()
        env.close()
    if counted is None:
        return SearchPlay(scores, colors * ranks, deviations.cpu(), trace, kept, kept_values)
    played, cut = (int(x) for x in counted.cpu())
    return SearchPlay(scores, colors * ranks, deviations.cpu(), trace, kept, kept_values, worlds_played=played, worlds_cut=cut,
                      nonfinite=nonfinite)
