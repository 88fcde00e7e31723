"""Device-resident actor: the reference's R2D2Actor + HanabiThreadLoop (rela/r2d2_actor.h:23-172,
cpp/thread_loop.h:42-88) for ALL games in lock-step on one GPU — no threads, no batcher, no host copies.

IQL layout (reference create.py:115-131: one actor per player): every (game, player) pair is one "env row"
of the agent / sequence writer; reward and terminal are shared by the players of a game.
VDN layout (create.py:98-113: one actor sees [E, P, ·]): the agent still acts on (game, player) rows, but a transition
is one GAME (fields of width P·w, one reward / terminal / priority per game) and priorities sum Q over the players."""
from collections import deque

import torch

from .env import BatchedHanabiEnv
from .r2d2 import R2D2Agent, zero_hidden_rows
from .replay import Bits, DeviceReplay, SequenceWriter


def transition_fields(env, vdn=False):
    """per-step fields of an RNNTransition: obs {priv_s, legal_move, eps, own_hand} + action {a, greedy_a}
    (cpp/hanabi_env.cc:197-204; pyhanabi/r2d2.py:296-303).  IQL: one transition per (game, player); VDN: one per
    game with the players' rows concatenated ([P, w] flattened)."""
    m = env.P if vdn else 1
    # every plane of the observation, the legal-move mask and the own-hand target are 0/1: stored as bits (32x less HBM per
    # stored step and per sampled batch).  The V0-belief encoding (knowledge_mode 1) holds count ratios and stays float32.
    binary = Bits(m)
    obs_dt = binary if getattr(env, "knowledge_mode", 0) == 0 else torch.float32
    return [("priv_s", m * env.F, obs_dt), ("legal_move", m * env.A, binary), ("eps", m, torch.float32),
            ("own_hand", m * 3 * env.H, binary), ("a", m, torch.int64), ("greedy_a", m, torch.int64)]


class PartnerSeatsError(ValueError):
    """a seat layout hsad_actor_create_partnered refuses; .verdict = (code, index, value)"""

    def __init__(self, text, verdict):
        super().__init__(text)
        self.verdict = verdict


class NetPartner:
    """A frozen network as a partner of a partnered actor (include/hsad.h, hsad_actor_net_partners): it acts greedily on the rows it
    owns, carries its own LSTM state and never reaches the replay.  `source`: a weight dict (R2D2Net.state_dict() names), the path
    of a weight file, or a composite.CNet, which is borrowed as it is -- the actor reads its weights on every step, so weights
    written and refreshed between two steps act from the next step on (it must not be the learner's online or target net).
    skip_connect is a constructor flag of the reference's net, not a weight, and therefore given here.
    temperature > 0: the partner plays its softmax policy instead -- every move sampled from the softmax over its legal advantages at that
    temperature (hsad_actor_set_partner_temperature; at 1 the distribution behaviour cloning fits), the common way to a population of
    partners out of one frozen net.  0 (the default) is the greedy partner, with the launches it always had."""
    MAX_NETS = 8

    def __init__(self, source, name=None, skip_connect=False, temperature=0.0):
        import math
        import os
        self.source, self.skip_connect = source, bool(skip_connect)
        self.temperature = float(temperature)
        if not math.isfinite(self.temperature) or self.temperature < 0:
            raise ValueError("NetPartner: temperature must be finite and >= 0; got %r" % (temperature,))
        self.path = os.fspath(source) if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__") else None
        self.name = name if name is not None else (os.path.basename(self.path) if self.path is not None else "net")
        self._weights = source if isinstance(source, dict) else None

    @property
    def is_cnet(self):
        return self.path is None and not isinstance(self.source, dict)

    def weights(self):
        """the weight dict (a file is read once, on the host)"""
        if self._weights is None and self.path is not None:
            from .checkpoint import load_weights
            self._weights = load_weights(self.path)
        return self._weights

    def dims(self):
        """(in_dim, num_action), without a device"""
        if self.is_cnet:
            return int(self.source.F), int(self.source.A)
        w = self.weights()
        return int(w["net.0.weight"].shape[1]), int(w["fc_a.weight"].shape[0])

    def make_net(self, device):
        """the inference net on `device`: the borrowed CNet, or a new one from the weights"""
        from .composite import CNet
        if self.is_cnet:
            return self.source
        return CNet(self.weights(), device, skip_connect=self.skip_connect)

    def seating_member(self, device):
        """what eval.play_seatings seats for this partner; its entry of play_seatings' `temperature` list is self.temperature (every
        member this returns is, or becomes at precision "bf16", a kernel agent with the sampling tail)"""
        if self.path is not None and self.skip_connect:
            from .checkpoint import agent_from_file
            return agent_from_file(self.path, str(device), skip_connect=True)
        if self.path is not None:
            return self.path
        if self.is_cnet or self.skip_connect:
            from .composite import CompositeAgent
            net = self.make_net(device)
            return CompositeAgent(net, net, 1, 0.99)
        return self.source


class PartnerSeats:
    """Who sits where when the learner trains next to fixed partners (include/hsad.h, hsad_actor_partners and hsad_actor_net_partners):
    `rows` int32 [M], the learner's rows g * P + p, strictly ascending; `seat_bot` int32 [G * P], -1 on exactly those rows and an index
    into `bots` (rulebot.RuleBot, at most 8) on every other row.  With frozen networks among the partners (NetPartner, at most 8) a
    partner row is either a bot's (seat_bot[r] = its index in `bots`, seat_net[r] = -1) or a net's (seat_net[r] = its index in `nets`,
    seat_bot[r] = -1); `seat_net` is None for a layout without nets.  The partner list may mix both kinds: `bots` and `nets` hold its
    members of each kind in the order given.  `verdict` / `check` restate the library's check (csrc/hsad_partner.h), refusal
    for refusal and in its order, so that a layout can be judged without a device."""
    OK, VDN, PLAYERS, NUM_ROWS, ROW_RANGE, ROW_ORDER, N_BOT, N_RULES, RULE_CODE, RULE_K, LEARNER_BOT, PARTNER_BOT = range(12)
    N_NET, NET_IN_DIM, NET_NUM_ACTION, LEARNER_NET, NET_RANGE, BOT_NET, NO_OWNER, NET_NO_ROW = range(12, 20)

    def __init__(self, bots, rows, seat_bot, bot_seed=0, seat_net=None):
        import numpy as np
        self.partners = self._as_list(bots)
        self.bots = [x for x in self.partners if not isinstance(x, NetPartner)]
        self.nets = [x for x in self.partners if isinstance(x, NetPartner)]
        self.rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1).astype(np.int32))
        self.seat_bot = np.ascontiguousarray(np.asarray(seat_bot, dtype=np.int64).reshape(-1).astype(np.int32))
        if seat_net is None and self.nets:
            seat_net = np.full(self.seat_bot.shape, -1)
        self.seat_net = None if seat_net is None else np.ascontiguousarray(np.asarray(seat_net, dtype=np.int64).reshape(-1).astype(np.int32))
        self.bot_seed = int(bot_seed)

    @staticmethod
    def _as_list(partners):
        from . import rulebot
        return [partners] if isinstance(partners, (rulebot.RuleBot, NetPartner)) else list(partners)

    @property
    def M(self):
        return int(self.rows.shape[0])

    @property
    def net_rows(self):
        """per net k: its rows, ascending (the order of its compact rows)"""
        import numpy as np
        return [np.nonzero(self.seat_net == k)[0].astype(np.int32) for k in range(len(self.nets))]

    @classmethod
    def alternate(cls, G, P, bots, bot_seed=0):
        """the learner sits on seat g % P of game g and every other seat of that game gets partner (g // P) % len(bots): seats and
        partners are balanced over the batch"""
        import numpy as np
        bots = cls._as_list(bots)
        g = np.arange(G)
        return cls._one_learner_seat(G, P, g % P, (g // P) % max(len(bots), 1), bots, bot_seed)

    @classmethod
    def fixed_seat(cls, G, P, seat, bots, bot_seed=0):
        """the learner sits on `seat` in every game; the other seats of game g get partner g % len(bots)"""
        import numpy as np
        bots = cls._as_list(bots)
        if not 0 <= int(seat) < P:
            raise PartnerSeatsError("fixed_seat: seat = %d, must be 0..%d" % (seat, P - 1), (cls.ROW_RANGE, 0, int(seat)))
        g = np.arange(G)
        return cls._one_learner_seat(G, P, np.full(G, int(seat)), g % max(len(bots), 1), bots, bot_seed)

    @classmethod
    def _one_learner_seat(cls, G, P, seat_of_game, bot_of_game, bots, bot_seed):
        """partner j of the (mixed) list gets the games with bot_of_game == j, whatever its kind"""
        import numpy as np
        is_net = np.array([isinstance(x, NetPartner) for x in bots] + [False], dtype=bool)      # (+ one entry: an empty list indexes too)
        kind_index = np.array([sum(1 for y in bots[:j] if isinstance(y, NetPartner) == isinstance(x, NetPartner))
                               for j, x in enumerate(bots)] + [0], dtype=np.int32)
        own = np.repeat(bot_of_game.astype(np.int64), P).reshape(G, P)
        seat_bot = np.where(is_net[own], -1, kind_index[own]).astype(np.int32)
        seat_bot[np.arange(G), seat_of_game] = -1
        seat_net = None
        if is_net.any():
            seat_net = np.where(is_net[own], kind_index[own], -1).astype(np.int32)
            seat_net[np.arange(G), seat_of_game] = -1
        return cls(bots, np.arange(G) * P + seat_of_game, seat_bot, bot_seed, seat_net)

    def verdict(self, G, P, hand_size=5, vdn=False, F=None, A=None):
        """(code, index, value) of partner_layout_verdict_nets (csrc/hsad_partner.h; without nets: of partner_layout_verdict):
        (0, 0, 0) for a layout the library runs.  F, A: the env's feature size and action count, which the nets are held to (None:
        not known yet, that refusal is left to the call that knows them)"""
        from . import rulebot
        N, M, n_bot = G * P, self.M, len(self.bots)
        rows, sb = self.rows.tolist(), self.seat_bot.tolist()
        with_nets = bool(self.nets) or self.seat_net is not None
        if vdn:
            return (self.VDN, 0, int(vdn))
        if P > 5 or hand_size > 5:
            return (self.PLAYERS, 0, P)
        if M < 1 or M > N:
            return (self.NUM_ROWS, 0, M)
        for i, r in enumerate(rows):
            if r < 0 or r >= N:
                return (self.ROW_RANGE, i, r)
            if i > 0 and r <= rows[i - 1]:
                return (self.ROW_ORDER, i, r)
        if n_bot > rulebot.MAX_BOTS or (n_bot == 0 and M != N and not with_nets):
            return (self.N_BOT, 0, n_bot)
        for b, bot in enumerate(self.bots):
            if not 1 <= len(bot.rules) <= rulebot.MAX_RULES:
                return (self.N_RULES, b, len(bot.rules))
            for code, k in bot.rules:      # rb_rules_invalid: per rule, the code first, then k
                if not rulebot.PLAY_CERTAIN <= code <= rulebot.LEGAL_RANDOM:
                    return (self.RULE_CODE, b, 0)
                if (not 0 <= k <= 100) if code in rulebot._WITH_K else (k != 0):
                    return (self.RULE_K, b, 0)
        if len(sb) != N:
            raise PartnerSeatsError("seat_bot has %d entries, the env has %d rows" % (len(sb), N), (self.PARTNER_BOT, len(sb), 0))
        learner = set(rows)
        if with_nets:
            return self._verdict_nets(N, learner, sb, n_bot, F, A)
        for r in range(N):
            if r in learner:
                if sb[r] != -1:
                    return (self.LEARNER_BOT, r, sb[r])
            elif sb[r] < 0 or sb[r] >= n_bot:
                return (self.PARTNER_BOT, r, sb[r])
        return (self.OK, 0, 0)

    def _verdict_nets(self, N, learner, sb, n_bot, F, A):
        """the part of partner_layout_verdict_nets behind the bots' rule lists: the nets, then one scan over the rows"""
        n_net = len(self.nets)
        if not 1 <= n_net <= NetPartner.MAX_NETS:
            return (self.N_NET, 0, n_net)
        for k, net in enumerate(self.nets):
            in_dim, num_action = net.dims()
            if F is not None and in_dim != F:
                return (self.NET_IN_DIM, k, in_dim)
            if A is not None and num_action != A:
                return (self.NET_NUM_ACTION, k, num_action)
        sn = self.seat_net.tolist()
        if len(sn) != N:
            raise PartnerSeatsError("seat_net has %d entries, the env has %d rows" % (len(sn), N), (self.NET_RANGE, len(sn), 0))
        owns = [False] * n_net
        for r in range(N):
            b, k = sb[r], sn[r]
            if r in learner:
                if b != -1:
                    return (self.LEARNER_BOT, r, b)
                if k != -1:
                    return (self.LEARNER_NET, r, k)
                continue
            if b < -1 or b >= n_bot:
                return (self.PARTNER_BOT, r, b)
            if k < -1 or k >= n_net:
                return (self.NET_RANGE, r, k)
            if b >= 0 and k >= 0:
                return (self.BOT_NET, r, k)
            if b < 0 and k < 0:
                return (self.NO_OWNER, r, 0)
            if k >= 0:
                owns[k] = True
        for k in range(n_net):
            if not owns[k]:
                return (self.NET_NO_ROW, k, 0)
        return (self.OK, 0, 0)

    def explain(self, verdict, G, P, F=None, A=None):
        """the text of a refusal (partner_verdict_text / partner_verdict_text_nets); it names the offending entry"""
        from . import rulebot
        code, i, v = verdict
        n_bot, n_net = len(self.bots), len(self.nets)
        if n_net or code >= self.N_NET:      # (the codes 0 .. 11 with n_net == 0: partner_verdict_text)
            nets_text = {self.N_BOT: "n_bot = %d, must be 0..%d" % (v, rulebot.MAX_BOTS),
                         self.PARTNER_BOT: "seat_bot[%d] = %d on a partner row, must be -1..%d" % (i, v, n_bot - 1),
                         self.N_NET: "n_net = %d, must be 1..%d" % (v, NetPartner.MAX_NETS),
                         self.NET_IN_DIM: "net %d has in_dim %d, the env's observation has %d features" % (i, v, -1 if F is None else F),
                         self.NET_NUM_ACTION: "net %d has num_action %d, the env has %d actions" % (i, v, -1 if A is None else A),
                         self.LEARNER_NET: "seat_net[%d] = %d on a learner row, must be -1" % (i, v),
                         self.NET_RANGE: "seat_net[%d] = %d, must be -1..%d" % (i, v, n_net - 1),
                         self.BOT_NET: "seat_net[%d] = %d on a row seat_bot gives to a bot: a row has one owner" % (i, v),
                         self.NO_OWNER: "row %d is neither the learner's nor a bot's nor a net's (seat_bot[%d] = seat_net[%d] = -1)" % (i, i, i),
                         self.NET_NO_ROW: "net %d owns no row: every net of the table must be seated" % i}
            if code in nets_text:
                return nets_text[code]
        return {self.OK: "ok",
                self.VDN: "cfg->vdn = %d: a partnered actor is an IQL actor (one transition per learner row)" % v,
                self.PLAYERS: "more than 5 players or 5 cards a hand (players = %d)" % v,
                self.NUM_ROWS: "M = %d learner rows, must be 1..%d" % (v, G * P),
                self.ROW_RANGE: "rows[%d] = %d, must be 0..%d" % (i, v, G * P - 1),
                self.ROW_ORDER: "rows[%d] = %d is not above rows[%d]: rows must be strictly ascending" % (i, v, i - 1),
                self.N_BOT: "n_bot = %d, must be 1..%d (0 only when every row is the learner's)" % (v, rulebot.MAX_BOTS),
                self.N_RULES: "bot %d has %d rules, must be 1..%d" % (i, v, rulebot.MAX_RULES),
                self.RULE_CODE: "bot %d names an unknown rule code" % i,
                self.RULE_K: "bot %d: k must be 0..100 for the PROBABLE rules and 0 for every other" % i,
                self.LEARNER_BOT: "seat_bot[%d] = %d on a learner row, must be -1" % (i, v),
                self.PARTNER_BOT: "seat_bot[%d] = %d on a partner row, must be 0..%d" % (i, v, n_bot - 1)}[code]

    def check(self, G, P, hand_size=5, vdn=False, F=None, A=None):
        v = self.verdict(G, P, hand_size, vdn, F, A)
        if v[0] != self.OK:
            raise PartnerSeatsError("PartnerSeats: " + self.explain(v, G, P, F, A), v)
        return self


class DeviceActor:
    def __init__(self, env: BatchedHanabiEnv, agent: R2D2Agent, replay: DeviceReplay, multi_step, gamma, eta, seq_len,
                 vdn=False, packed_obs=None, native=None, partners=None):
        self.env, self.agent, self.replay = env, agent, replay
        self.G, self.P = env.G, env.P
        self.partners = partners
        self.partner_nets = []
        if partners is not None:
            if native is not None and not native:
                self._refuse_python_partners()
            partners.check(self.G, self.P, env.H, vdn, env.F, env.A)
        # agent rows (hidden state [L, N, H]) in both layouts; with partners (PartnerSeats): the learner's rows only
        self.N = self.G * self.P if partners is None else partners.M
        self.vdn = bool(vdn)
        self.E = self.G if self.vdn else self.N   # transitions per step
        self.eta = float(eta)
        self.multi_step = int(multi_step)
        self.writer = SequenceWriter(self.E, multi_step, gamma, seq_len, transition_fields(env, self.vdn), env.device)
        self.cached_q = getattr(agent, "cached_q", True)      # False: a contract model (rela.ContractAgent): reference flow
        # packed observation path: the env kernel writes the observation as the replay's bit words and as the net's bf16 operand
        # from its on-chip bit rows; the float32 observation (the reference's API-boundary format) is not written at all, and
        # neither the bf16 cast nor the row-pack pass runs.  Needs an agent that takes bf16 input (composite.CompositeAgent).
        if packed_obs is None:
            packed_obs = bool(getattr(agent, "accepts_bf16_obs", False)) and self.cached_q and getattr(env, "knowledge_mode", 0) == 0
        self.packed_obs = bool(packed_obs)
        if self.packed_obs:
            env.enable_packed(agent.online.Fp, keep_float32=False)
            self.writer.set_prepacked(("priv_s", "legal_move", "own_hand"))
        if hasattr(agent, "configure"):
            agent.configure(self.P, self.vdn)
        self.hid = agent.get_h0(self.N)
        self.history_hid = deque()
        self.q_hist = deque()                 # (Q_online(s_t, a_t), online weight version) per step still in the n-step window
        self._verify_cached_priority = False   # tests: also run compute_priority on the unpacked transition and compare
        self.n_checked = self.n_checked_stale = 0
        self.num_act = 0          # R2D2Actor::numAct summed over the P per-player actors
        self.n_finished = torch.zeros(1, dtype=torch.int32, device=env.device)
        self._side = torch.cuda.Stream(env.device) if self.cached_q else None      # reset of ended games, see _reset_terminated
        self._side_flush = torch.cuda.Stream(env.device) if self.cached_q else None   # flush of finished sequences, see _flush
        self._reset_pending = False
        # The loop body itself lives in the library (include/hsad.h hsad_actor_*, csrc/hsad_actor.hip): with the library's composite
        # agent and the packed observation path, step() is ONE C call and this class only holds the objects it drives.  The Python
        # body below remains for models behind the reference's contract (rela.ContractAgent), for the Python-orchestrated agent
        # and for the priority cross-check of the tests (verify_cached_priority).
        self.c_actor = None
        if native is None:
            native = self.packed_obs and hasattr(agent, "online") and hasattr(agent.online, "h") and hasattr(agent, "lib") and not getattr(agent.online, "skip", False)
        if partners is not None and not native:
            self._refuse_python_partners()
        if native:
            self._make_native(multi_step, gamma, seq_len)

    @staticmethod
    def _refuse_python_partners():
        from . import _lib
        raise _lib.HsadError("PartnerSeats need the library's loop body (hsad_actor_create_partnered): the Python actor path runs the "
                             "agent on every row; use the composite bf16 agent with the packed observation path and native != False")

    @property
    def verify_cached_priority(self):
        return self._verify_cached_priority

    @verify_cached_priority.setter
    def verify_cached_priority(self, on):
        """the cross-check runs in the Python loop body, which pushes into this object's own sequence writer -- a native actor has
        handed that role (and closed that writer) to the library's loop: refuse instead of stepping on a freed handle"""
        if on and self.c_actor is not None:
            from . import _lib
            raise _lib.HsadError("verify_cached_priority needs the Python loop body: construct the DeviceActor with native=False "
                                 "(selfplay: --native_actor 0); this actor runs hsad_actor_step and owns no Python-side sequence writer")
        self._verify_cached_priority = bool(on)

    def _make_native(self, multi_step, gamma, seq_len):
        import ctypes as C
        from . import _lib
        env, agent = self.env, self.agent
        self.writer.close()                       # the library's actor owns its own sequence writer
        cfg = _lib.ActorConfig(int(self.vdn), int(multi_step), int(seq_len), int(env.H), int(agent.online.H), float(gamma), float(self.eta),
                               int(agent.seed))
        io = _lib.ActorIO(env.legal_move.data_ptr(), env.own_hand.data_ptr(), env.eps.data_ptr(), env.reward.data_ptr(), env.terminal.data_ptr(),
                          env.priv_bits.data_ptr(), env.legal_bits.data_ptr(), env.own_bits.data_ptr(), env.priv_s_bf16.data_ptr())
        h = C.c_void_p()
        if self.partners is not None:
            from . import rulebot
            pt = self.partners
            rules, n_rules, n_bot = rulebot.pack(pt.bots)
            part = _lib.ActorPartners(pt.rows.ctypes.data, pt.M, C.addressof(rules), C.addressof(n_rules), n_bot, pt.seat_bot.ctypes.data,
                                      pt.bot_seed)
            if pt.nets:
                # one inference net per NetPartner on the env's device, built here or borrowed, alive as long as the actor
                self.partner_nets = [n.make_net(env.device) for n in pt.nets]
                handles = (C.c_void_p * len(self.partner_nets))(*[n.h for n in self.partner_nets])
                net_part = _lib.ActorNetPartners(C.addressof(handles), len(self.partner_nets), pt.seat_net.ctypes.data)
                _lib.check(agent.lib.hsad_actor_create_partnered_nets(env.h, agent.online.h, agent.target.h, self.replay.h, C.byref(cfg),
                                                                      C.byref(io), C.byref(part), C.byref(net_part), C.byref(h)))
            else:
                _lib.check(agent.lib.hsad_actor_create_partnered(env.h, agent.online.h, agent.target.h, self.replay.h, C.byref(cfg), C.byref(io),
                                                                 C.byref(part), C.byref(h)))
        else:
            _lib.check(agent.lib.hsad_actor_create(env.h, agent.online.h, agent.target.h, self.replay.h, C.byref(cfg), C.byref(io), C.byref(h)))
        for k, n in enumerate(self.partners.nets if self.partners is not None else []):
            if n.temperature > 0:       # a greedy partner makes no call: the actor is the one built without the keyword
                _lib.check(agent.lib.hsad_actor_set_partner_temperature(h, k, n.temperature))
        self.c_actor, self._lib = h, agent.lib
        nf = agent.lib.hsad_actor_n_finished_dev(h)
        from .composite import _view
        self.n_finished = _view(nf, 1, env.device, self, dtype=torch.int32)

    def close(self):
        if getattr(self, "c_actor", None):
            self._lib.hsad_actor_destroy(self.c_actor)
            self.c_actor = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def last_reply(self):
        """{a, greedy_a} int64 [G * P] of the last step (native loop: views of the library's buffers)"""
        import ctypes as C
        from .composite import _view
        g = C.c_void_p()
        a = self._lib.hsad_actor_last_actions(self.c_actor, C.byref(g))
        n = self.G * self.P
        return {"a": _view(a, n, self.env.device, self, dtype=torch.int64), "greedy_a": _view(g.value, n, self.env.device, self, dtype=torch.int64)}

    @property
    def state(self):
        """(h, c) fp32 [L, N, H]: the carried state entering the next step (native loop: views of the library's buffers)"""
        import ctypes as C
        from . import _lib
        from .composite import _view
        h, c = C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.hsad_actor_state(self.c_actor, C.byref(h), C.byref(c)))
        n = self.agent.online.L * self.N * self.agent.online.H
        return _view(h.value, n, self.env.device, self), _view(c.value, n, self.env.device, self)

    def partner_state(self, k):
        """(h, c) fp32 [L_k, n_k, H_k] of network partner k: its carried state entering the next step (views of the library's buffers)"""
        import ctypes as C
        from . import _lib
        from .composite import _view
        h, c, n = C.c_void_p(), C.c_void_p(), C.c_int32()
        _lib.check(self._lib.hsad_actor_partner_state(self.c_actor, int(k), C.byref(h), C.byref(c), C.byref(n)))
        net = self.partner_nets[k]
        shape = (net.L, n.value, net.H)
        size = net.L * n.value * net.H
        return _view(h.value, size, self.env.device, self).view(shape), _view(c.value, size, self.env.device, self).view(shape)

    @property
    def last_priority(self):
        """float32 [E] n-step priorities pushed by the last step, None while the n-step window was still filling (native loop)"""
        import ctypes as C
        from .composite import _view
        n = C.c_int32()
        p = self._lib.hsad_actor_last_priority(self.c_actor, C.byref(n))
        return _view(p, n.value, self.env.device, self) if p else None

    @property
    def num_redo(self):
        return int(self._lib.hsad_actor_num_redo(self.c_actor)) if self.c_actor is not None else self.n_checked_stale

    def _rows(self):
        e, N = self.env, self.N
        if self.packed_obs:
            return {"priv_s_bf16": e.priv_s_bf16.view(N, -1), "legal_move": e.legal_move.view(N, e.A), "eps": e.eps.view(N),
                    "own_hand": e.own_hand.view(N, 3 * e.H)}
        return {"priv_s": e.priv_s.view(N, e.F), "legal_move": e.legal_move.view(N, e.A), "eps": e.eps.view(N),
                "own_hand": e.own_hand.view(N, 3 * e.H)}

    def _reset_terminated(self):
        """`if (terminated) reset` at the top of the thread-loop body (cpp/thread_loop.h:46-52).  The reset kernel is latency-bound --
        a handful of lanes each shuffle a deck with mt19937 while the rest of the chip idles (~35 us) -- and nothing between one
        env.step and the next act() touches the env, so the reset of the games that just ended is issued on a side stream right
        after env.step (_prefetch_reset) and overlaps the n-step / sequence / replay bookkeeping of the same iteration; the end of
        step() joins it, so nothing outside step() ever runs next to it."""
        if self._reset_pending:
            self._reset_pending = False       # already issued behind the previous env.step and joined at the end of that step()
        else:
            self.env.reset()

    def _prefetch_reset(self):
        if self._side is None:
            return
        main = torch.cuda.current_stream(self.env.device)
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            self.env.reset()
        self._reset_pending = True

    def _join_reset(self):
        if self._reset_pending:
            torch.cuda.current_stream(self.env.device).wait_stream(self._side)

    def set_run_ahead(self, steps):
        """bound how far the host may run ahead of the device (hsad_actor_set_run_ahead; 0 = unbounded): an actor rank of a multi-GPU
        job must be able to serve the learner's round within a few steps, not behind hundreds of queued ones"""
        self._run_ahead, self._step_events = int(steps), []
        if self.c_actor is not None:
            from . import _lib
            _lib.check(self._lib.hsad_actor_set_run_ahead(self.c_actor, int(steps)))

    def _bound_run_ahead(self):
        """the Python body's twin of the library's bound (polling, never a blocking wait)"""
        import time
        e = torch.cuda.Event()
        e.record()
        self._step_events.append(e)
        if len(self._step_events) > self._run_ahead:
            old = self._step_events.pop(0)
            while not old.query():
                time.sleep(0)

    def step(self):
        """one iteration of the thread-loop body: reset-terminated -> act -> step -> postAct"""
        if self.c_actor is not None:
            from . import _lib
            from .composite import _s
            _lib.check(self._lib.hsad_actor_step(self.c_actor, _s(self.env.device)))
            self.num_act = int(self._lib.hsad_actor_num_act(self.c_actor))
            return
        if getattr(self, "_run_ahead", 0) > 0:
            self._bound_run_ahead()
        env, agent, P = self.env, self.agent, self.P
        self._reset_terminated()
        obs = self._rows()
        # historyHidden_.push_back(hidden_): by reference -- R2D2Agent.act returns fresh state tensors and never writes the
        # ones it is given, and zero_hidden_rows below only touches the new ones, which enter the history next step
        self.history_hid.append(dict(self.hid))
        # with_q: Q_online(s_t, a_t) comes out of the pass that picks the action and Q_target(s_t, greedy_t) costs one target
        # pass on the live observation -- exactly the two numbers compute_priority needs from time t (as `obs` n steps from
        # now, as `next_obs` right now).  Two network passes per step instead of the reference's four, no observation ever
        # read back from the n-step ring.
        if not self.cached_q:
            return self._step_contract(obs)
        reply, self.hid = agent.act(obs, self.hid, with_q=True)
        self.q_hist.append((reply["q_online_a"], reply["versions"][0]))
        if self.packed_obs:
            fields = {"priv_s": env.priv_bits, "legal_move": env.legal_bits, "own_hand": env.own_bits, "eps": obs["eps"]}
        else:
            fields = dict(obs)
        fields["a"], fields["greedy_a"] = reply["a"], reply["greedy_a"]
        self.writer.push_obs_action(fields)
        env.step(reply["a"].view(self.G, P), reply["greedy_a"].view(self.G, P))
        self._prefetch_reset()
        self.num_act += self.N               # Tachometer counts P acts per game step in both layouts (utils.py:229-236)
        # postAct: reward / terminal of the game go to each of its players' rows (IQL) or to the game's row (VDN)
        self.writer.push_reward_terminal(env.reward, env.terminal, repeat=1 if self.vdn else P)
        zero_hidden_rows(self.hid, env.terminal, P)                                    # r2d2_actor.h:109-126
        if not self.writer.can_pop():
            self._join_reset()
            return
        hid_s = self.history_hid.popleft()
        qa_s, version_s = self.q_hist.popleft()
        stale = version_s != agent.online.version   # the online weights were synced since step t-n: the reference would
        np_ = P if self.vdn else 1                  # evaluate Q_online(s_{t-n}, a) with the NEW weights, so redo that pass
        N, F, A = self.N, env.F, env.A              # VDN rows [G, P*w] are the same memory as [G*P, w]
        check = self.verify_cached_priority
        cur, nxt, rew, term, boot = self.writer.pop_transition(want_fields=stale or check, want_next=check)
        if stale or check:
            cur_obs = {"priv_s": cur["priv_s"].view(N, F), "legal_move": cur["legal_move"].view(N, A)}
        if stale:
            qa_s = agent.q_of(agent.online, cur_obs, cur["a"].view(-1), hid_s)
        prio = agent.priority_from_q(qa_s, reply["q_target_greedy"], rew, boot, num_player=np_)
        if check:   # tests: the reference's call on the unpacked transition must give the same bits
            nxt_obs = {"priv_s": nxt["priv_s"].view(N, F), "legal_move": nxt["legal_move"].view(N, A)}
            full = agent.compute_priority(cur_obs, cur["a"].view(-1), nxt_obs, hid_s, self.history_hid[-1], rew, boot,
                                          num_player=np_)
            assert torch.equal(prio, full), "cached-Q priorities differ from compute_priority"
            self.n_checked += 1
            self.n_checked_stale += int(stale)
        self.writer.push_sequence(prio)
        self._flush()
        self._join_reset()

    def _flush(self):
        """finished sequences -> replay.  The chain is five small launches, three of them single-workgroup scans (~80 us with the
        chip idle around them); issued on a side stream it overlaps the next step's network passes.  No join here: the library
        orders whoever touches the writer's cursors or the replay next -- on any stream -- behind it (StreamFence in
        csrc/hsad_replay.hip)."""
        if self._side_flush is None:
            self.n_finished = self.writer.flush_to_replay(self.replay, self.eta, out=self.n_finished)
            return
        self._side_flush.wait_stream(torch.cuda.current_stream(self.env.device))
        with torch.cuda.stream(self._side_flush):
            self.n_finished = self.writer.flush_to_replay(self.replay, self.eta, out=self.n_finished)

    def _step_contract(self, obs):
        """the rest of step() for a model that only offers the reference's contract (act / compute_priority): the n-step
        priority is ITS compute_priority on the popped transition with the hidden states of t-n and t (r2d2_actor.h:128-156)"""
        env, agent, P = self.env, self.agent, self.P
        reply, self.hid = agent.act(obs, self.hid)
        fields = dict(obs)
        fields["a"], fields["greedy_a"] = reply["a"], reply["greedy_a"]
        self.writer.push_obs_action(fields)
        env.step(reply["a"].view(self.G, P), reply["greedy_a"].view(self.G, P))
        self.num_act += self.N
        r = env.reward if self.vdn else env.reward.repeat_interleave(P)
        t = env.terminal if self.vdn else env.terminal.repeat_interleave(P)
        self.writer.push_reward_terminal(r, t)
        zero_hidden_rows(self.hid, env.terminal, P)
        if not self.writer.can_pop():
            return
        hid_s = self.history_hid.popleft()
        cur, nxt, rew, term, boot = self.writer.pop_transition(want_fields=True, want_next=True)
        prio = agent.compute_priority_dict(cur, nxt, hid_s, self.history_hid[-1], rew, term, boot)
        self.writer.push_sequence(prio)
        self.n_finished = self.writer.flush_to_replay(self.replay, self.eta)
