"""Batched evaluation and checkpoints.

`evaluate` = pyhanabi/eval.py:19-66: `num_game` fresh games (seed+game_idx, max_len = -1, eps = 0), every player
acts greedily, score = last_score(); the reference spins one thread per game, here all games advance in
lock-step on the GPU and finished games simply stop acting.
`save_weights` / `load_weights` keep the reference's `.pthw` format: torch.save(online_net.state_dict())
with the key names net.0.*, lstm.*_l{0,1}, fc_v.*, fc_a.*, pred.* (common_utils/saver.py:17-61; utils.py:278-299)."""
import numpy as np
import torch

from . import _lib
from .env import BatchedHanabiEnv
from .r2d2 import R2D2Agent, R2D2NetKernels
from .rulebot import RuleBot


SAMPLE_KEY_STEPS = 4096      # move numbers per (deal, seat) in a sample key: max_steps may not exceed it when a seat samples


def sample_key_base(deal_seed, seat):
    """the sample key of (deal seed, seat, move t) is sample_key_base + t: injective over the deals of one call (seat < 8,
    t < SAMPLE_KEY_STEPS; int64 arithmetic, wrapping).  deal_seed, seat: int64 tensors"""
    return (deal_seed * 8 + seat) * SAMPLE_KEY_STEPS


def pool_temperatures(temperature, K):
    """the `temperature` argument of play_seatings / cross_play -> None (nobody samples: the greedy code path) or float32 [K].
    None, a number for every member, or one number per member; negative and non-finite values are refused"""
    if temperature is None:
        return None
    t = np.asarray(temperature, dtype=np.float64)
    if t.ndim == 0:
        t = np.full(K, float(t))
    if t.ndim != 1 or len(t) != K:
        raise ValueError("temperature must be None, one number, or one per pool member (%d); got shape %s" % (K, tuple(t.shape)))
    if not np.all(np.isfinite(t)) or np.any(t < 0):
        raise ValueError("temperatures must be finite and >= 0; got %s" % t.tolist())
    return t.astype(np.float32) if np.any(t > 0) else None


def _is_bf16_kernel_agent(x):
    """the Python-orchestrated bf16 agent: r2d2.R2D2Agent over an R2D2NetKernels (what checkpoint.agent_from_file builds for the
    default architecture at bf16).  It has no sampling tail itself, but its fp32 master weights make the composite agent that has"""
    return isinstance(x, R2D2Agent) and type(x.online) is R2D2NetKernels


def _samples_on_device(x, precision):
    """can this pool member (as _check_pool returns it) play at a temperature?  The sampling tail belongs to the library's bf16 agent
    (composite.CompositeAgent): weight dicts become one at precision "bf16", and a bf16 R2D2Agent is re-seated as one over its own
    weights (_soft_agent).  The fp32 agents (R2D2Agent over R2D2NetF32, weights at precision "fp32"), obl.OBLAgent and
    rela.ContractAgent are not"""
    from .composite import CompositeAgent
    if isinstance(x, dict):
        return precision == "bf16"
    return isinstance(x, CompositeAgent) or _is_bf16_kernel_agent(x)


def _soft_agent(x, precision, device):
    """the acting agent of a member that plays at a temperature > 0 (check_pool_temperatures has passed it): a CompositeAgent.  A bf16
    R2D2Agent is re-seated as CNet + CompositeAgent over its online net's fp32 master weights -- the same kernels behind one library
    call, as NetPartner.seating_member does for a borrowed net; a member at temperature 0 keeps the agent it always had"""
    if _is_bf16_kernel_agent(x):
        from .composite import CNet, CompositeAgent
        net = CNet(x.online.w, device)
        return CompositeAgent(net, net, 1, 0.99)
    return _acting_agent(x, precision, device)


def check_pool_temperatures(models, temps, names, precision):
    """refuses, before any device work, a temperature > 0 on a member without the sampling tail (rule bots ignore theirs)"""
    if temps is None:
        return
    for k, (x, t) in enumerate(zip(models, temps)):
        if t > 0 and not isinstance(x, RuleBot) and not _samples_on_device(x, precision):
            raise ValueError("pool member %d (%s) cannot play at temperature %g: only bf16 kernel agents (weights at precision \"bf16\", "
                             "composite.CompositeAgent, a bf16 r2d2.R2D2Agent) sample their softmax policy; fp32 nets, obl.OBLAgent, "
                             "rela.ContractAgent and bare nets act greedily" % (k, names[k], t))


def evaluate(weights, num_game, seed, bomb, sad, *, num_player=2, hand_size=5, device="cuda:0", max_steps=200, precision="bf16",
             shuffle_color=False, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3, temperature=0.0, sample_seed=0):
    """-> (mean score, fraction of perfect games, scores list, num perfect) like eval.evaluate.  `weights`: a weight dict, or
    an R2D2Agent / net already on the device (its online net acts for every player).  temperature > 0 (bf16 kernel agents only): every
    player samples its move from the softmax over the legal advantages at that temperature, keyed by (sample_seed; deal seed, seat,
    move number) like play_seatings, whose one-member tournament over the same deals plays the same games"""
    temperature = float(temperature)
    if not np.isfinite(temperature) or temperature < 0:
        raise ValueError("temperature must be finite and >= 0; got %r" % temperature)
    if temperature > 0:
        check_pool_temperatures([weights], [temperature], ["weights"], precision)
        if max_steps > SAMPLE_KEY_STEPS:
            raise ValueError("max_steps %d exceeds the %d moves a sample key numbers" % (max_steps, SAMPLE_KEY_STEPS))
    env = BatchedHanabiEnv(num_game, players=num_player, hand_size=hand_size, seed=seed, bomb=bomb, eps_list=[0.0],
                           max_len=-1, sad=bool(sad), shuffle_color=bool(shuffle_color), device=device, track_deck_history=False,
                           colors=colors, ranks=ranks, max_information_tokens=max_information_tokens, max_life_tokens=max_life_tokens)
    if temperature > 0:
        agent = _soft_agent(weights, precision, device)
    elif isinstance(weights, R2D2Agent):
        agent = R2D2Agent(weights.online, weights.online, 1, 0.99)
    elif hasattr(weights, "act") and hasattr(weights, "get_h0"):
        agent = weights                      # any acting agent (obl.OBLAgent, rela.ContractAgent): used as it is
    elif hasattr(weights, "trunk"):
        agent = R2D2Agent(weights, weights, 1, 0.99)
    elif precision == "bf16":
        from .composite import CNet, CompositeAgent
        net = CNet(weights, device)
        agent = CompositeAgent(net, net, 1, 0.99)
    else:
        net = R2D2NetKernels.make(weights, device, precision)
        agent = R2D2Agent(net, net, 1, 0.99)
    N = num_game * num_player
    hid = agent.get_h0(N)
    env.reset()
    done = torch.zeros(num_game, dtype=torch.bool, device=device)
    noop = env.A - 1
    if temperature > 0:
        row = torch.arange(N, dtype=torch.int64, device=device)
        key0 = sample_key_base(row // num_player + int(seed), row % num_player)
        temp = torch.full((N,), temperature, dtype=torch.float32, device=device)
    for t in range(max_steps):
        obs = {"priv_s": env.priv_s.view(N, env.F), "legal_move": env.legal_move.view(N, env.A), "eps": env.eps.view(N)}
        if temperature > 0:
            obs["temp"], obs["sample_key"] = temp, key0 + t
            reply, hid = agent.act(obs, hid, sample_seed=sample_seed)
        else:
            reply, hid = agent.act(obs, hid)
        a = reply["a"].view(num_game, num_player)
        # finished games may not be stepped again (HanabiEnv::step asserts !terminated()): park them on a copy that
        # the kernel ignores by keeping their state untouched -> step only the live ones through a masked action
        q = env.query()
        done = q[:, 0] == 1
        if bool(done.all()):
            break
        live = ~done
        if bool(live.all()):
            env.step(a.contiguous(), reply["greedy_a"].view(num_game, num_player).contiguous())
        else:
            # lock-step with stragglers: finished games receive an (ignored) illegal noop and are skipped by the
            # error log below; their last_score is already latched
            aa = torch.where(live.unsqueeze(1), a, torch.full_like(a, noop)).contiguous()
            env.step(aa, aa)
            n, g, c = _drain_errors(env)
    scores = env.query()[:, 5].cpu().numpy().astype(np.int64)
    perfect = int((scores == colors * ranks).sum())   # every firework complete: 25 in the full game
    return float(scores.mean()), perfect / num_game, scores.tolist(), perfect


# ---------------------------------------------------------------------------------------------------------
# cross-play: every seating of a model pool over the same deals, as one batched run
# (pyhanabi/tools/eval_model.py produces one cell of models/op_raw_data.txt per invocation)
# ---------------------------------------------------------------------------------------------------------
def env_dims(num_player=2, hand_size=5, sad=False, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3):
    """(feature_size, num_action) of BatchedHanabiEnv for these rules, computed on the host (the canonical encoder's sections:
    hands | board | discards | last action | card knowledge (| SAD's last action))"""
    P, H, Cn, Rn = int(num_player), int(hand_size), int(colors), int(ranks)
    deck = Cn * (3 if Rn == 1 else 2 * Rn)
    last_action = P + 4 + P + Cn + Rn + H + H + Cn * Rn + 2
    board = deck - P * H + Cn * Rn + int(max_information_tokens) + int(max_life_tokens)
    F = P * H * Cn * Rn + P + board + deck + last_action + P * H * (Cn * Rn + Cn + Rn)
    return F + (last_action if sad else 0), 2 * H + (P - 1) * (Cn + Rn) + 1


def seating_rows(seatings, num_game, num_model=None):
    """the rows each model owns in a tournament batch: game g = s * num_game + d is deal d of seating s, its seat p is the flat row
    g * P + p and belongs to model seatings[s][p].  -> one ascending int32 array per model (empty for a model no seating names)"""
    seatings = np.asarray(seatings, dtype=np.int64)
    owner = np.repeat(seatings, int(num_game), axis=0).reshape(-1)
    K = int(num_model) if num_model is not None else (int(seatings.max()) + 1 if seatings.size else 0)
    return [np.nonzero(owner == k)[0].astype(np.int32) for k in range(K)]


def _model_dims(x):
    """(in_dim, out_dim, exact) of a pool member without touching a device; exact=False: the model reads the first in_dim features
    of a longer observation (obl.OBLAgent on the SAD observation); None when the object does not tell"""
    if isinstance(x, dict):
        return int(x["net.0.weight"].shape[1]), int(x["fc_a.weight"].shape[0]), True
    net = getattr(x, "online", None)
    if net is not None and hasattr(net, "in_dim") and hasattr(net, "A"):          # obl.OBLNetKernels
        return int(net.in_dim), int(net.A), False
    if net is not None and hasattr(net, "F") and hasattr(net, "A"):
        return int(net.F), int(net.A), True
    if hasattr(x, "F") and hasattr(x, "A"):                                         # a bare net
        return int(x.F), int(x.A), True
    return None


def _check_pool(agents, seatings, num_player, F, A):
    """the refusals of play_seatings, all before any device work; -> (models as given, paths read into weight dicts; seatings [S, P])"""
    seatings = np.asarray(seatings)
    if seatings.ndim != 2 or seatings.shape[1] != num_player:
        raise ValueError("seatings must be [S, %d] (one model index per seat of a %d-player game); got shape %s"
                         % (num_player, num_player, tuple(seatings.shape)))
    if seatings.shape[0] < 1:
        raise ValueError("seatings is empty")
    if not np.issubdtype(seatings.dtype, np.integer):
        raise ValueError("seatings must hold integer model indices; got dtype %s" % seatings.dtype)
    K = len(agents)
    bad = np.argwhere((seatings < 0) | (seatings >= K))
    if len(bad):
        s, p = bad[0]
        raise ValueError("seating %d seat %d names model %d; the pool has models 0..%d" % (s, p, seatings[s, p], K - 1))
    models = []
    for k, x in enumerate(agents):
        if isinstance(x, RuleBot):           # no net: nothing to hold against the env's dimensions
            models.append(x)
            continue
        if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__"):
            x = load_weights(x)
        dims = _model_dims(x)
        if dims is not None:
            in_dim, out_dim, exact = dims
            if (in_dim != F if exact else in_dim > F) or out_dim != A:
                raise ValueError("model %d has %d inputs and %d actions; the env of this game has %d features and %d actions "
                                 "(sad and the game's rules decide both)" % (k, in_dim, out_dim, F, A))
        models.append(x)
    return models, seatings.astype(np.int64)


def _acting_agent(x, precision, device):
    """what evaluate() turns its `weights` argument into"""
    if isinstance(x, R2D2Agent):
        return R2D2Agent(x.online, x.online, 1, 0.99)
    if hasattr(x, "act") and hasattr(x, "get_h0"):
        return x
    if hasattr(x, "trunk"):
        return R2D2Agent(x, x, 1, 0.99)
    if precision == "bf16":
        from .composite import CNet, CompositeAgent
        net = CNet(x, device)
        return CompositeAgent(net, net, 1, 0.99)
    net = R2D2NetKernels.make(x, device, precision)
    return R2D2Agent(net, net, 1, 0.99)


BEHAVIOUR_NAMES = ("MOVES", "PLAY_OK", "PLAY_FAIL", "PLAY_CERTAIN", "DISCARD", "DISCARD_CERTAIN_DEAD", "HINT_COLOUR", "HINT_RANK",
                   "HINT_CARDS", "HINT_PLAYABLE", "LAST_COPY_LOST", "INFO_SUM", "LAST_LIFE")     # include/hsad.h: HSAD_BH_*
BEHAVIOUR_RATES = ("hint_share", "play_share", "discard_share", "colour_hint_share", "certain_play_share", "misplay_rate",
                   "safe_discard_share", "playable_hint_share", "cards_per_hint", "mean_info")


class BehaviourStats:
    """the behaviour counters of a tournament: counts int64 [..., P, 13] as hsad_seating_behaviour summed them on the device (the
    counters of include/hsad.h, HSAD_BH_*; names = their names in that order; play_seatings gives [S, P, 13], cross_play
    [K, K, P, 13]) and the rates derived from them, float64 [..., P], nan where the denominator is 0:
      hint_share, play_share, discard_share   of the seat's moves
      colour_hint_share, playable_hint_share  of its hints;  cards_per_hint = cards touched per hint
      certain_play_share, misplay_rate        of its plays (PLAY_CERTAIN, PLAY_FAIL)
      safe_discard_share                      of its discards (DISCARD_CERTAIN_DEAD)
      mean_info                               information tokens available per move
    game_moves (play_seatings / cross_play only, else None): int64 [S, num_game], the moves each game took by the env's own step
    counter; a seating's MOVES counters add up to its sum"""
    names = BEHAVIOUR_NAMES

    def __init__(self, counts, game_moves=None):
        self.game_moves = game_moves
        self.counts = c = np.ascontiguousarray(counts, dtype=np.int64)
        assert c.ndim >= 2 and c.shape[-1] == len(self.names)
        k = {n: c[..., i].astype(np.float64) for i, n in enumerate(self.names)}
        moves, plays, hints, discards = k["MOVES"], k["PLAY_OK"] + k["PLAY_FAIL"], k["HINT_COLOUR"] + k["HINT_RANK"], k["DISCARD"]

        def over(x, d):
            return np.divide(x, d, out=np.full(d.shape, np.nan), where=d != 0)
        self.hint_share, self.play_share, self.discard_share = over(hints, moves), over(plays, moves), over(discards, moves)
        self.colour_hint_share, self.playable_hint_share = over(k["HINT_COLOUR"], hints), over(k["HINT_PLAYABLE"], hints)
        self.cards_per_hint = over(k["HINT_CARDS"], hints)
        self.certain_play_share, self.misplay_rate = over(k["PLAY_CERTAIN"], plays), over(k["PLAY_FAIL"], plays)
        self.safe_discard_share = over(k["DISCARD_CERTAIN_DEAD"], discards)
        self.mean_info = over(k["INFO_SUM"], moves)

    def row(self, *index):
        """row(s, p) (cross_play: row(i, j, p)) -> {counter name: int, ..., rate name: float, ...} of that seat"""
        out = {n: int(v) for n, v in zip(self.names, self.counts[index])}
        out.update({r: float(getattr(self, r)[index]) for r in BEHAVIOUR_RATES})
        return out

    def summed(self, cells):
        """the counters of several (s, p) cells added up, as a BehaviourStats of shape [1, 13]"""
        return BehaviourStats(sum(self.counts[c] for c in cells).reshape(1, -1))


class SeatingScores:
    """what play_seatings returns: scores int64 [S, num_game]; totals int64 [S, 4] = (sum score, sum score^2, perfect, finished) as
    hsad_seating_stats reduced them on the device; mean / sem / perfect float64 [S] from those integers (sem = population std /
    sqrt(n), tools/eval_model.py:41-42); behaviour = a BehaviourStats [S, P, 13] when play_seatings(behaviour=True) counted, else
    None; records = the game_record.GameRecord list of play_seatings(records=...), each tagged meta = {seating, deal_seed, seats (the
    seat names), game (its deal's index in `scores`)}, else None"""

    def __init__(self, scores, totals, seatings, behaviour=None, records=None):
        import math
        self.scores, self.totals, self.seatings, self.behaviour, self.records = scores, totals, seatings, behaviour, records
        n = scores.shape[1]
        self.num_game = n
        t = [[int(v) for v in row] for row in totals]
        self.mean = np.array([r[0] / n for r in t], dtype=np.float64)
        self.sem = np.array([math.sqrt(n * r[1] - r[0] * r[0]) / n / math.sqrt(n) for r in t], dtype=np.float64)
        self.perfect = np.array([r[2] / n for r in t], dtype=np.float64)


class _SeatedModel:
    """one pool member inside a tournament batch: its rows, its act operands and its carried state"""

    def __init__(self, agent, rows, env, device, temperature=0.0, deals=None):
        self.agent, self.n = agent, int(len(rows))
        # a member that samples: its temperature on every row, and what the sample key of a row is made of (game s * deals + d
        # plays deal d; the seat is the row's player) -- key0 is set per chunk by _TournamentBatch.play
        self.temp = self.key0 = None
        if temperature > 0:
            self.temp = torch.full((self.n,), float(temperature), dtype=torch.float32, device=device)
            self.deal = torch.from_numpy((rows.astype(np.int64) // env.P) % int(deals)).to(device)
            self.seat = torch.from_numpy(rows.astype(np.int64) % env.P).to(device)
        self.rows = torch.from_numpy(rows).to(device)
        self.bf16 = bool(getattr(agent, "accepts_bf16_obs", False))
        self.Kp = agent.online.Fp if self.bf16 else env.F
        self.obs = torch.empty(self.n, self.Kp, dtype=torch.bfloat16 if self.bf16 else torch.float32, device=device)
        self.legal = torch.empty(self.n, env.A, dtype=torch.float32, device=device)
        self.eps = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.hid = None


class _TournamentBatch:
    """one env object of S x n games (seating-major) and the pool seated on it; play(seed) runs one chunk of n deals"""

    def __init__(self, agents, seatings, n, env_kw, device, bot_seed=0, behaviour=False, records=None, temps=None, sample_seed=0):
        S, P = seatings.shape
        self.n, self.S = n, S
        self.sample_seed = int(sample_seed)
        self.behaviour = torch.zeros(S, P, len(BEHAVIOUR_NAMES), dtype=torch.int64, device=device) if behaviour else None
        # a record needs the deal: only a recording tournament's env tracks its deck history
        self.env = env = BatchedHanabiEnv(S * n, players=P, seed=0, eps_list=[0.0], max_len=-1, device=device,
                                          track_deck_history=records is not None, **env_kw)
        self.recorder = self.where = self.records = None
        if records is not None:
            from .game_record import GameRecorder
            self.recorder, self.where = GameRecorder(env), (None if records is True else records)
        self.lib, self.device = env.lib, env.device
        owned = seating_rows(seatings, n, len(agents))
        self.models = [_SeatedModel(ag, rows, env, self.device, 0.0 if temps is None else float(temps[k]), n)
                       for k, (ag, rows) in enumerate(zip(agents, owned)) if len(rows) and not isinstance(ag, RuleBot)]
        # the rule bots of the pool own no _SeatedModel: one policy_rule call per step serves all their rows
        seated_bots = [k for k, ag in enumerate(agents) if isinstance(ag, RuleBot) and len(owned[k])]
        self.bots, self.bot_seed = [agents[k] for k in seated_bots], int(bot_seed)
        if self.bots:
            sb = np.full(S * n * P, -1, dtype=np.int32)
            for b, k in enumerate(seated_bots):
                sb[owned[k]] = b
            self.seat_bot = torch.from_numpy(sb).view(S * n, P).to(self.device)
            self.deal = (torch.arange(S * n, dtype=torch.int64) % n).to(self.device)   # game s * n + d plays deal d
        widths = {m.Kp for m in self.models if m.bf16}
        if len(widths) > 1:
            raise _lib.HsadError("the pool's bf16 nets pad the observation to different row lengths: %s" % sorted(widths))
        if widths:     # the env writes the first GEMM's operand itself; the 3.3 KB float32 row only if a pool member reads it
            env.enable_packed(bf16_row_len=widths.pop(), keep_float32=any(not m.bf16 for m in self.models))
        self.stats = torch.zeros(S, 4, dtype=torch.int64, device=self.device)
        self.unfinished = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.host = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(2)]
        self.copied = [torch.cuda.Event() for _ in range(2)]

    def _act(self, m, t=0):
        env, lib, st = self.env, self.lib, self.env._stream()
        src = env.priv_s_bf16 if m.bf16 else env.priv_s
        _lib.check(lib.hsad_seat_gather(m.rows.data_ptr(), m.n, env.G * env.P, 0 if m.bf16 else 2, src.data_ptr(), env.F, m.Kp,
                                   env.legal_move.data_ptr(), env.A, m.obs.data_ptr(), m.legal.data_ptr(), st))
        obs = {"priv_s_bf16" if m.bf16 else "priv_s": m.obs, "legal_move": m.legal, "eps": m.eps}
        if m.temp is not None:      # the key names (deal, seat, move): a deal plays the same in every chunking
            obs["temp"], obs["sample_key"] = m.temp, m.key0 + t
            reply, m.hid = m.agent.act(obs, m.hid, sample_seed=self.sample_seed)
        else:
            reply, m.hid = m.agent.act(obs, m.hid)
        a, g = reply["a"].contiguous(), reply["greedy_a"].contiguous()
        _lib.check(lib.hsad_seat_scatter(env.h, m.rows.data_ptr(), m.n, a.data_ptr(), g.data_ptr(), env.a.data_ptr(),
                                    env.greedy_a.data_ptr(), st))

    def play(self, seed, max_steps):
        """deals seed .. seed + n - 1 for every seating -> (scores int64 [S, n], totals int64 [S, 4]); with behaviour counting,
        self.behaviour holds this chunk's counters afterwards"""
        env = self.env
        env.reseed(seed, self.n)
        env.reset()
        if self.behaviour is not None:
            self.behaviour.zero_()
        if self.recorder is not None:
            self.recorder.clear()
        for m in self.models:
            m.hid = m.agent.get_h0(m.n)
            if m.temp is not None:
                m.key0 = sample_key_base(m.deal + int(seed), m.seat)
        done = False
        for t in range(max_steps):
            for m in self.models:
                self._act(m, t)
            if self.bots:     # the hash of a *_RANDOM rule is keyed by the deal's seed: a deal plays the same in every chunking
                env.policy_rule(self.bots, self.seat_bot, seed=self.bot_seed, key=self.deal + int(seed))
            if self.behaviour is not None:     # every seat's action is merged and the env not yet stepped: the moves about to be made
                _lib.check(self.lib.hsad_seating_behaviour(env.h, self.n, env.a.data_ptr(), self.behaviour.data_ptr(), env._stream()))
            if self.recorder is not None:      # the same moment: the log classifies the move on the position before it
                self.recorder.append(env.a, env.greedy_a)
            env.step(env.a, env.greedy_a)
            _lib.check(self.lib.hsad_seating_stats(env.h, self.n, self.stats.data_ptr(), self.unfinished.data_ptr(), env._stream()))
            # the host looks at ONE word, and one step late: it never waits for the step it has just enqueued (the extra step
            # at the end only hands finished games their noop)
            self.host[t & 1].copy_(self.unfinished, non_blocking=True)
            self.copied[t & 1].record(torch.cuda.current_stream(self.device))
            if t > 0:
                self.copied[(t - 1) & 1].synchronize()
                if int(self.host[(t - 1) & 1][0]) == 0:
                    done = True
                    break
        _drain_errors(env)        # finished games were handed the noop: the "step on a finished game" notes
        totals = self.stats.cpu().numpy()
        if not done and int(self.unfinished.cpu()[0]) != 0:
            raise RuntimeError("%d game(s) still running after %d steps" % (int(self.unfinished.cpu()[0]), max_steps))
        q = env.query().cpu().numpy().astype(np.int64)
        scores = q[:, 5].reshape(self.S, self.n)
        self.game_moves = q[:, 6].reshape(self.S, self.n)      # HSAD_Q_NUM_STEP: what the MOVES counters of a seating add up to
        if self.recorder is not None:     # filtered on the device; only the kept games' bytes cross to the host
            lost = self.recorder.overflow_count()
            if lost:
                raise _lib.HsadError("the game log overflowed %d time(s): a game ran past the capacity the rules allow" % lost)
            self.records = self.recorder.collect(self.where)
        return scores, totals


def play_seatings(agents, seatings, num_game, seed, bomb, sad, *, games_per_launch=1 << 18, precision="bf16", device="cuda:0",
                  hand_size=5, shuffle_color=False, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3, max_steps=200,
                  bot_seed=0, behaviour=False, records=None, names=None, temperature=None, sample_seed=0):
    """Every seating of a model pool over the SAME deals, in one batched run -> SeatingScores.

    agents: the pool -- whatever `evaluate` accepts (weight dicts, kernel agents / nets, any object with act / get_h0 such as
    obl.OBLAgent or rela.ContractAgent), `.pthw` paths, or rulebot.RuleBot members (at most 8: hand-coded partners, served by one
    BatchedHanabiEnv.policy_rule call per step; bot_seed seeds their *_RANDOM rules, keyed by the deal).  seatings: int [S, P], the model index on each seat.  Seating s plays the
    deals seed .. seed + num_game - 1, the ones evaluate(..., seed) plays; every player acts greedily (max_len -1, eps 0).

    One env object holds S x n games, seating-major, reseeded with period n (BatchedHanabiEnv.reseed); per step each model acts ONCE
    on the rows it owns (seating_rows; fixed ascending order, so its hidden state never moves): hsad_seat_gather -> act ->
    hsad_seat_scatter, and hsad_seating_stats reduces the per-seating statistics on the device.  bf16 kernel nets read the env's
    packed bf16 rows; every other agent gets the float32 rows by the same index list.  games_per_launch caps S x n per env object;
    larger jobs run in chunks of deals on the same object.

    behaviour=True also counts what kind of moves every seat of every seating makes (SeatingScores.behaviour, a BehaviourStats):
    one hsad_seating_behaviour launch per step, between the last action merge and the env step.  The games are the same either way.

    records=True, or a game_record.GameFilter, also writes every game down on the device (one hsad_game_log_append launch per step
    at that same point; the env then tracks its deck history) and returns the finished games the filter keeps as
    SeatingScores.records, tagged with seating, deal seed and seat names (names: one per pool member; default a RuleBot's own name,
    "model<k>" otherwise).  The games are the same either way.

    temperature: None, one number, or one per pool member.  A member with temperature > 0 plays its softmax policy: each of its moves is
    sampled from the softmax over the legal advantages at that temperature (hsad_r2d2_act_soft; at 1 the distribution behaviour cloning
    fits) instead of their argmax.  The draw is keyed by sample_seed and (deal seed, seat, move number), so a deal plays the same in
    every games_per_launch chunking and the same call gives the same games.  Rule bots ignore their entry; a member with a
    temperature > 0 that is not a bf16 kernel agent is refused.  Records keep `a` and `greedy_a` apart, as for eps-greedy play.
    None or all zeros runs the greedy calls: the same launches and the same bits as without the argument."""
    try:
        shape = tuple(np.asarray(seatings).shape)
    except ValueError:                    # seatings of different widths
        shape = None
    if shape is None or len(shape) != 2 or not 2 <= shape[1] <= 5:
        raise ValueError("seatings must be [S, players] with 2..5 players, every seating as wide as the game has seats; got %s"
                         % ("shape %s" % (shape,) if shape is not None else "rows of different widths"))
    P = shape[1]
    rules = dict(colors=colors, ranks=ranks, max_information_tokens=max_information_tokens, max_life_tokens=max_life_tokens)
    F, A = env_dims(P, hand_size, sad, **rules)
    if num_game < 1:
        raise ValueError("num_game must be >= 1")
    models, seatings = _check_pool(agents, seatings, P, F, A)
    S = seatings.shape[0]
    if names is None:
        names = [getattr(x, "name", None) if isinstance(x, RuleBot) else None for x in models]
        names = [n if n is not None else "model%d" % k for k, n in enumerate(names)]
    temps = pool_temperatures(temperature, len(models))
    check_pool_temperatures(models, temps, names, precision)
    if temps is not None and max_steps > SAMPLE_KEY_STEPS:
        raise ValueError("max_steps %d exceeds the %d moves a sample key numbers" % (max_steps, SAMPLE_KEY_STEPS))
    acting = [x if isinstance(x, RuleBot) else
              (_soft_agent if temps is not None and temps[k] > 0 else _acting_agent)(x, precision, device) for k, x in enumerate(models)]
    env_kw = dict(hand_size=hand_size, bomb=bomb, sad=bool(sad), shuffle_color=bool(shuffle_color), **rules)
    per = max(1, min(int(num_game), int(games_per_launch) // S))
    scores = np.zeros((S, num_game), dtype=np.int64)
    totals = np.zeros((S, 4), dtype=np.int64)
    counts = np.zeros((S, P, len(BEHAVIOUR_NAMES)), dtype=np.int64) if behaviour else None
    game_moves = np.zeros((S, num_game), dtype=np.int64) if behaviour else None
    if records is False:
        records = None
    kept = [] if records is not None else None
    batches = {}
    for start in range(0, num_game, per):
        n = min(per, num_game - start)
        if n not in batches:
            batches[n] = _TournamentBatch(acting, seatings, n, env_kw, device, bot_seed, bool(behaviour), records, temps, sample_seed)
            if (batches[n].env.F, batches[n].env.A) != (F, A):
                raise _lib.HsadError("env_dims gives (%d, %d), the library (%d, %d)" % (F, A, batches[n].env.F, batches[n].env.A))
        sc, tt = batches[n].play(seed + start, max_steps)
        scores[:, start:start + n] = sc
        totals += tt
        if behaviour:
            counts += batches[n].behaviour.cpu().numpy()
            game_moves[:, start:start + n] = batches[n].game_moves
        if kept is not None:
            for rec in batches[n].records:
                s, d = divmod(rec.meta.pop("game"), n)
                rec.meta.update(seating=int(s), deal_seed=int(seed + start + d), game=int(start + d),
                                seats=[str(names[k]) for k in seatings[s]])
                kept.append(rec)
    for b in batches.values():
        if b.recorder is not None:
            b.recorder.close()
        b.env.close()
    return SeatingScores(scores, totals, seatings, BehaviourStats(counts, game_moves) if behaviour else None, kept)


class CrossPlayScores:
    """cross_play's K x K view of SeatingScores: entry [i][j] = model i on seat 0 with model j on seat 1; row_mean[i] = the mean
    of row i with the diagonal included (the last column of models/op_raw_data.txt); behaviour = the BehaviourStats of
    cross_play(behaviour=True) with counts [K, K, P, 13], else None; records = the GameRecord list of cross_play(records=...)
    (meta["seating"] = i * K + j), else None"""

    def __init__(self, res, K):
        self.seatings, self.num_game, self.records = res, res.num_game, res.records
        self.behaviour = None if res.behaviour is None else BehaviourStats(res.behaviour.counts.reshape((K, K) + res.behaviour.counts.shape[1:]),
                                                                         res.behaviour.game_moves.reshape(K, K, -1))
        self.scores = res.scores.reshape(K, K, -1)
        self.mean, self.sem, self.perfect = res.mean.reshape(K, K), res.sem.reshape(K, K), res.perfect.reshape(K, K)
        self.row_mean = self.mean.mean(axis=1)


def cross_play(agents, num_game, seed, bomb, sad, **kw):
    """the two-player tournament: all K^2 ordered seatings of the pool over the same deals -> CrossPlayScores"""
    K = len(agents)
    seatings = [(i, j) for i in range(K) for j in range(K)]
    return CrossPlayScores(play_seatings(agents, seatings, num_game, seed, bomb, sad, **kw), K)


def format_cross_play_table(title, names, mean, row_mean=None):
    """the layout of models/op_raw_data.txt: title, rule, header `name M0 ... mean`, dashes, one row per model, two decimals"""
    mean = np.asarray(mean, dtype=np.float64)
    row_mean = mean.mean(axis=1) if row_mean is None else row_mean
    head = "%-6s" % "name" + "".join("  %5s" % n for n in names) + "  %6s" % "mean"
    lines = [title, "-" * len(head), head, "------" + "  -----" * len(names) + "  ------"]
    for n, row, m in zip(names, mean, row_mean):
        lines.append("%-6s" % n + "".join("  %5.2f" % v for v in row) + "  %6.2f" % m)
    return "\n".join(lines)


def parse_cross_play_table(text):
    """-> (title, names, mean [K, K], row_mean [K]) of a table format_cross_play_table wrote"""
    lines = [l for l in text.splitlines() if l.strip()]
    names = lines[2].split()[1:-1]
    body = [l.split() for l in lines[4:4 + len(names)]]
    vals = np.array([[float(v) for v in r[1:]] for r in body], dtype=np.float64)
    return lines[0], names, vals[:, :-1], vals[:, -1]


def format_behaviour_rates(stats, index):
    """the derived rates of one seat as `name value` pairs on one line (nan where a denominator is 0)"""
    return " ".join("%s %.4f" % (r, float(getattr(stats, r)[index])) for r in BEHAVIOUR_RATES)


def format_behaviour_table(names, stats):
    """the behaviour of a cross_play: a title, a rule, the header, then one line per (pairing, seat) -- `seat0-seat1 seat who`, the 13
    counters, `|`, the derived rates.  stats: a BehaviourStats with counts [K, K, P, 13] (or [K * K, P, 13])"""
    K = len(names)
    counts = stats.counts.reshape((K, K) + stats.counts.shape[-2:])
    assert counts.shape[2] == 2, "cross_play is the two-player tournament"
    st = BehaviourStats(counts)
    head = "%-15s %4s %-8s" % ("pairing", "seat", "who") + "".join(" %s" % n for n in BEHAVIOUR_NAMES) + " |" + "".join(" %s" % r for r in BEHAVIOUR_RATES)
    lines = ["behaviour per pairing and seat", "-" * 30, head]
    for i in range(K):
        for j in range(K):
            for p in range(counts.shape[2]):
                lines.append("%-15s %4d %-8s" % ("%s-%s" % (names[i], names[j]), p, names[(i, j)[p]])
                             + "".join(" %d" % v for v in counts[i, j, p]) + " |"
                             + "".join(" %.4f" % float(getattr(st, r)[i, j, p]) for r in BEHAVIOUR_RATES))
    return "\n".join(lines)


def parse_behaviour_table(text):
    """-> (names, counts int64 [K, K, P, 13]) of a table format_behaviour_table wrote (the counters are printed exactly)"""
    lines = [l for l in text.splitlines() if l.strip()]
    start = lines.index("behaviour per pairing and seat")
    rows = []
    for l in lines[start + 3:]:
        left = l.split("|")[0].split()
        if "|" not in l or len(left) != 3 + len(BEHAVIOUR_NAMES):
            break
        rows.append((left[0], int(left[1]), left[2], [int(v) for v in left[3:]]))
    P = max(r[1] for r in rows) + 1
    K = int(round((len(rows) // P) ** 0.5))
    assert K * K * P == len(rows), "not a K x K x P table: %d lines" % len(rows)
    names = [rows[i * K * P][2] for i in range(K)]          # seat 0 of the pairings (i, 0)
    counts = np.array([r[3] for r in rows], dtype=np.int64).reshape(K, K, P, len(BEHAVIOUR_NAMES))
    return names, counts


def _drain_errors(env):
    import ctypes as C
    n, g, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    env.lib.hsad_env_error_count(env.h, C.byref(n), C.byref(g), C.byref(c))
    return n.value, g.value, c.value


from .checkpoint import load_weights, save_weights  # noqa: E402,F401  (kept importable from here)
