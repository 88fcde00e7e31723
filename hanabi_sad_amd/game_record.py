"""Game records: one game written down -- rules, deal, every move with its greedy alternative and a flag byte from the move
classifier, and how it ended (include/hsad.h: HSAD_GR_*, csrc/hsad_game_record.h holds the byte layout).

  GameRecorder(env)   logs a tournament's moves on the device (append) and reads the finished games a filter keeps (collect)
  GameRecord          the record on the host: bytes / JSON both ways, validate(), describe(), position(k)
  save / load         JSON lines
  replay              records -> a BatchedHanabiEnv whose game j is record j at move stop[j] (hsad_env_playout_logged)

`GameRecord.position` and `validate` replay the rules in plain Python, with no device and no oracle: they are written from the rules
(HanabiState::ApplyMove as include/hsad.h's position record describes its result), and the tests hold them to the CPU oracle move by
move.  Only GameRecorder and replay need torch and a device.

    python -m hanabi_sad_amd.game_record FILE [--game I] [--at K]
"""
import dataclasses
import json

from . import position as pos

VERSION = 1
OFF_DECK, OFF_MOVES = 16, 68
FLAG_NAMES = ("counted", "play_fail", "play_uncertain", "last_copy_lost", "last_life", "hint_not_playable", "discard_uncertain", "no_info")
FLAGS = {n: 1 << i for i, n in enumerate(FLAG_NAMES)}
END_NAMES = ("unfinished", "lives", "deck", "perfect", "max_len")
ENDS = {n: i for i, n in enumerate(END_NAMES)}
RULE_KEYS = ("players", "hand_size", "colors", "ranks", "max_information_tokens", "max_life_tokens", "bomb")
_COLOURS = "RYGWB"


def deck_size(rules):
    return sum(pos.full_deck(rules))


def capacity(rules):
    """L: no game of these rules has more moves (csrc/hsad_game_record.h gives the derivation)"""
    return (2 * (deck_size(rules) - rules["players"] * rules["hand_size"]) + rules["max_information_tokens"] + rules["colors"]
            + rules["players"])


def record_bytes(rules):
    return OFF_MOVES + 3 * capacity(rules)


def num_actions(rules):
    return 2 * rules["hand_size"] + (rules["players"] - 1) * (rules["colors"] + rules["ranks"]) + 1


def decode_move(rules, uid):
    """uid -> ("discard" | "play", slot) or ("hint_colour" | "hint_rank", target offset, value); None for anything else"""
    P, H, nC, nR = rules["players"], rules["hand_size"], rules["colors"], rules["ranks"]
    uid = int(uid)
    if 0 <= uid < H:
        return ("discard", uid)
    if H <= uid < 2 * H:
        return ("play", uid - H)
    k = uid - 2 * H
    if 0 <= k < (P - 1) * nC:
        return ("hint_colour", k // nC + 1, k % nC)
    k -= (P - 1) * nC
    if 0 <= k < (P - 1) * nR:
        return ("hint_rank", k // nR + 1, k % nR)
    return None


def flag_names(byte):
    return [n for n in FLAG_NAMES if int(byte) & FLAGS[n]]


@dataclasses.dataclass
class GameFilter:
    """hsad_game_filter: which finished games to keep.  end_mask: bits 1 << ENDS[name], 0 = any; flag_mask: FLAGS bits, 0 = no
    condition on the moves; seat_mask: bit p = seat p, 0 = every seat.  A game passes the pair when some move by a seat of
    seat_mask carries a flag of flag_mask."""
    score_min: int = 0
    score_max: int = 255
    max_lives: int = 255
    moves_min: int = 0
    moves_max: int = 255
    end_mask: int = 0
    seat_mask: int = 0
    flag_mask: int = 0

    @classmethod
    def parse(cls, text):
        """"score<=10,flag=last_life,seat=1": comma-separated terms score / lives / moves with <=, >= or =, end=NAME, flag=NAME,
        seat=P (end, flag and seat may repeat: any of them)"""
        f = cls()
        for term in [t.strip() for t in (text or "").split(",") if t.strip()]:
            for op in ("<=", ">=", "="):
                if op in term:
                    key, val = [s.strip() for s in term.split(op, 1)]
                    break
            else:
                raise ValueError("filter term %r has no <=, >= or =" % term)
            if key == "flag":
                if val not in FLAGS or op != "=":
                    raise ValueError("flag=%s: the flags are %s" % (val, ", ".join(FLAG_NAMES)))
                f.flag_mask |= FLAGS[val]
            elif key == "end":
                if val not in ENDS or op != "=":
                    raise ValueError("end=%s: a game ends by %s" % (val, ", ".join(END_NAMES[1:])))
                f.end_mask |= 1 << ENDS[val]
            elif key == "seat" and op == "=":
                f.seat_mask |= 1 << int(val)
            elif key in ("score", "moves"):
                v = int(val)
                if op in ("<=", "="):
                    setattr(f, key + "_max", v)
                if op in (">=", "="):
                    setattr(f, key + "_min", v)
            elif key == "lives" and op == "<=":
                f.max_lives = int(val)
            else:
                raise ValueError("filter term %r: unknown key or operator" % term)
        return f

    def matches(self, rec):
        """the host's statement of the device filter"""
        if rec.end == ENDS["unfinished"]:
            return False
        P = rec.rules["players"]
        seats = self.seat_mask or ~0
        hit = any((seats >> (k % P)) & 1 and f & self.flag_mask for k, f in enumerate(rec.flags))
        return (self.score_min <= rec.score <= self.score_max and rec.lives <= self.max_lives
                and self.moves_min <= len(rec.moves) <= self.moves_max and (not self.end_mask or (self.end_mask >> rec.end) & 1)
                and (not self.flag_mask or hit))


class _Game:
    """the rules of Hanabi on plain lists: what GameRecord.position and validate replay a record with"""

    def __init__(self, rules, deck):
        self.rules = r = rules
        self.P, self.H, self.nC, self.nR = r["players"], r["hand_size"], r["colors"], r["ranks"]
        self.max_info, self.bomb = r["max_information_tokens"], int(r.get("bomb", 0))
        self.script, self.dealt = [int(t) for t in deck], 0
        self.deck = pos.full_deck(r)
        self.discards, self.fireworks = [0] * 25, [0] * 5
        self.info, self.life = self.max_info, r["max_life_tokens"]
        self.hands = [[] for _ in range(self.P)]
        self.mover, self.next, self.turns, self.num_step = 0, 1 % self.P, self.P, 0
        self.last_move, self.last_score, self.terminal = None, -1, False
        self.drawn = []                      # the card each move's deal brought: (seat, card type) or None
        if len(self.script) < self.P * self.H:
            raise ValueError("the deck holds %d cards, the first deal needs %d" % (len(self.script), self.P * self.H))
        for p in range(self.P):
            for _ in range(self.H):
                self._deal(p)

    def _deal(self, p):
        if self.dealt >= len(self.script):
            raise ValueError("the deck's %d cards are dealt and move %d needs another" % (len(self.script), self.num_step))
        t = self.script[self.dealt]
        if not 0 <= t < 25 or self.deck[t] < 1:
            raise ValueError("deck card %d is type %d, which the deck does not hold" % (self.dealt, t))
        self.dealt += 1
        self.deck[t] -= 1
        self.hands[p].append([t, (1 << self.nC) - 1, (1 << self.nR) - 1, -1, -1])
        return t

    def score(self):
        return 0 if (self.life <= 0 and self.bomb) else sum(self.fireworks)

    def illegal(self, uid):
        """why the seat on turn may not play uid, or None"""
        m = decode_move(self.rules, uid)
        if self.terminal:
            return "the game is over"
        if m is None:
            return "uid %d is no move" % uid
        if m[0] in ("discard", "play"):
            if m[1] >= len(self.hands[self.mover]):
                return "slot %d is empty" % m[1]
            if m[0] == "discard" and self.info >= self.max_info:
                return "a discard with every information token in stock"
            return None
        if self.info <= 0:
            return "a hint without an information token"
        target = self.hands[(self.mover + m[1]) % self.P]
        if not any((c[0] // 5 if m[0] == "hint_colour" else c[0] % 5) == m[2] for c in target):
            return "a hint that touches no card"
        return None

    def apply(self, uid):
        why = self.illegal(uid)
        if why:
            raise ValueError("move %d (uid %d) is illegal: %s" % (self.num_step, uid, why))
        m, p = decode_move(self.rules, uid), self.mover
        if sum(self.deck) == 0:
            self.turns -= 1
        if m[0] in ("discard", "play"):
            t = self.hands[p].pop(m[1])[0]
            c, rk = divmod(t, 5)
            scored = token = 0
            if m[0] == "discard":
                token = 1                       # legal only below the maximum
                self.discards[t] += 1
            elif rk == self.fireworks[c]:
                scored = 1
                self.fireworks[c] += 1
                token = int(rk + 1 == self.nR and self.info < self.max_info)
            else:
                self.life -= 1
                self.discards[t] += 1
            self.info += token
            self.last_move = dict(type=m[0], player=p, card_index=m[1], colour=c, rank=rk, scored=scored, info_token=token)
        else:
            self.info -= 1
            by_colour, reveal = m[0] == "hint_colour", 0
            for i, card in enumerate(self.hands[(p + m[1]) % self.P]):
                k = 1 if by_colour else 2
                if (card[0] // 5 if by_colour else card[0] % 5) == m[2]:
                    reveal |= 1 << i
                    card[k], card[k + 2] = 1 << m[2], m[2]
                else:
                    card[k] &= ~(1 << m[2])
            self.last_move = dict(type=m[0], player=p, target_offset=m[1], value=m[2], reveal_mask=reveal)
        self.num_step += 1
        self._advance()
        self.terminal = self.life < 1 or sum(self.fireworks) >= self.nC * self.nR or self.turns <= 0
        draw = None
        if self.terminal:
            self.last_score = self.score()
        else:
            while self.mover < 0:
                to = min(q for q in range(self.P) if len(self.hands[q]) < self.H)
                draw = (to, self._deal(to))
                self._advance()
        self.drawn.append(draw)

    def _advance(self):
        if sum(self.deck) > 0 and any(len(h) < self.H for h in self.hands):
            self.mover = -1                    # a deal comes first
        else:
            self.mover, self.next = self.next, (self.next + 1) % self.P

    def end(self):
        if not self.terminal:
            return ENDS["unfinished"]
        if self.life < 1:
            return ENDS["lives"]
        if sum(self.fireworks) >= self.nC * self.nR:
            return ENDS["perfect"]
        return ENDS["deck"]

    def position(self, perms=None):
        r = {k: self.rules[k] for k in RULE_KEYS[:6]}
        hands = [[pos.Card(c[0] // 5, c[0] % 5, c[1], c[2], c[3], c[4]) for c in h] for h in self.hands]
        return pos.Position(r, hands, fireworks=self.fireworks, discards=list(self.discards), deck=list(self.deck), info=self.info,
                            life=self.life, mover=self.mover, turns_to_play=self.turns, num_step=self.num_step,
                            last_move=self.last_move, last_score=self.last_score, perms=perms)


def _card(t):
    return "%s%d" % (_COLOURS[t // 5], t % 5 + 1)


class GameRecord:
    """rules: dict of RULE_KEYS; deck: the card types (colour * 5 + rank) in deal order, n_dealt of them; moves / greedy / flags:
    one entry per move (uids with a colour hint's colour as the cards' true colour; FLAGS bits); score, lives, info, end: the
    result (end: ENDS); meta: free, JSON-able (deal seed, seat names, seating, ...)"""

    def __init__(self, rules, deck, moves, greedy=None, flags=None, score=0, lives=0, info=0, end=0, meta=None):
        self.rules = {k: int(rules.get(k, 0)) for k in RULE_KEYS}
        self.deck = [int(t) for t in deck]
        self.moves = [int(m) for m in moves]
        self.greedy = [int(m) for m in (greedy if greedy is not None else moves)]
        self.flags = [int(f) for f in (flags if flags is not None else [0] * len(self.moves))]
        self.score, self.lives, self.info, self.end = int(score), int(lives), int(info), int(end)
        self.meta = dict(meta or {})

    @property
    def n_moves(self):
        return len(self.moves)

    def _key(self):
        return (self.rules, self.deck, self.moves, self.greedy, self.flags, self.score, self.lives, self.info, self.end, self.meta)

    def __eq__(self, other):
        return isinstance(other, GameRecord) and self._key() == other._key()

    def __repr__(self):
        return "GameRecord(%d moves, score %d, ended by %s, meta=%r)" % (self.n_moves, self.score, END_NAMES[self.end], self.meta)

    @classmethod
    def from_game(cls, rules, deck, moves, greedy=None, flags=None, meta=None):
        """a record from a deal and its moves alone: the result fields are what the rules give"""
        rec = cls(rules, deck, moves, greedy, flags, meta=meta)
        g = rec._replay(len(rec.moves))
        rec.deck = rec.deck[:g.dealt]
        rec.score, rec.lives, rec.info, rec.end = g.score(), g.life, g.info, g.end()
        return rec

    # -- bytes (the device's layout) --
    def to_bytes(self):
        L = capacity(self.rules)
        if not (len(self.moves) == len(self.greedy) == len(self.flags)) or len(self.moves) > L or len(self.deck) > 52 or L > 255:
            raise ValueError("the record does not fit its layout: %d / %d / %d moves (capacity %d), %d deck cards"
                             % (len(self.moves), len(self.greedy), len(self.flags), L, len(self.deck)))
        r = self.rules
        out = bytearray(record_bytes(r))
        out[0:16] = bytes([VERSION] + [r[k] for k in RULE_KEYS] + [len(self.moves), len(self.deck), self.score, self.lives, self.info,
                                                                  self.end, L, 0])
        out[OFF_DECK:OFF_DECK + len(self.deck)] = bytes(self.deck)
        for q, plane in enumerate((self.moves, self.greedy, self.flags)):
            out[OFF_MOVES + q * L:OFF_MOVES + q * L + len(plane)] = bytes(plane)
        return bytes(out)

    @classmethod
    def from_bytes(cls, data, meta=None):
        data = bytes(data)
        if len(data) < OFF_MOVES:
            raise ValueError("%d bytes are no record (the header alone has %d)" % (len(data), OFF_MOVES))
        if data[0] != VERSION:
            raise ValueError("record version %d, this code reads version %d" % (data[0], VERSION))
        rules = dict(zip(RULE_KEYS, data[1:8]))
        n_moves, n_dealt, score, lives, info, end, L = data[8:15]
        if L != capacity(rules) or len(data) != record_bytes(rules):
            raise ValueError("a record of these rules has capacity %d and %d bytes, this one says %d and has %d"
                             % (capacity(rules), record_bytes(rules), L, len(data)))
        if n_moves > L or n_dealt > 52 or end >= len(END_NAMES):
            raise ValueError("n_moves %d, n_dealt %d or end %d out of range" % (n_moves, n_dealt, end))
        planes = [list(data[OFF_MOVES + q * L:OFF_MOVES + q * L + n_moves]) for q in range(3)]
        return cls(rules, list(data[OFF_DECK:OFF_DECK + n_dealt]), planes[0], planes[1], planes[2], score, lives, info, end, meta)

    # -- JSON --
    def to_json(self):
        return json.dumps(dict(version=VERSION, rules=self.rules, deck=self.deck, moves=self.moves, greedy=self.greedy, flags=self.flags,
                               result=dict(score=self.score, lives=self.lives, info=self.info, end=END_NAMES[self.end]), meta=self.meta),
                          sort_keys=True, separators=(",", ":"))

    @classmethod
    def from_json(cls, text):
        d = json.loads(text)
        if d.get("version") != VERSION:
            raise ValueError("record version %r, this code reads version %d" % (d.get("version"), VERSION))
        res = d["result"]
        return cls(d["rules"], d["deck"], d["moves"], d["greedy"], d["flags"], res["score"], res["lives"], res["info"], ENDS[res["end"]],
                   d.get("meta"))

    # -- the rules --
    def _replay(self, k):
        if not 0 <= k <= len(self.moves):
            raise ValueError("move %d of a game of %d moves" % (k, len(self.moves)))
        g = _Game(self.rules, self.deck)
        for uid in self.moves[:k]:
            g.apply(uid)
        return g

    def position(self, k, perms=None):
        """the position before move k (k = n_moves: the last one) as a position.Position; perms: the seats' colour permutations
        if the position is meant for an env that shuffles colours (the record itself names true colours)"""
        return self._replay(k).position(perms)

    def validate(self):
        """raises ValueError with the reason unless the record is a game of its rules: a deck the rules can deal, dealt exactly as
        far as the moves need, every move legal, nothing after the end, and result fields that are what the moves lead to"""
        r = self.rules
        if not (2 <= r["players"] <= 5 and 1 <= r["hand_size"] <= 5 and 1 <= r["colors"] <= 5 and 1 <= r["ranks"] <= 5):
            raise ValueError("rules out of range: %s" % r)
        if capacity(r) > 255:
            raise ValueError("a game of these rules can have %d moves, a record holds at most 255" % capacity(r))
        if not len(self.moves) == len(self.greedy) == len(self.flags):
            raise ValueError("%d moves, %d greedy moves, %d flag bytes" % (len(self.moves), len(self.greedy), len(self.flags)))
        if len(self.moves) > capacity(r):
            raise ValueError("%d moves, the rules allow %d" % (len(self.moves), capacity(r)))
        if any(decode_move(r, u) is None for u in self.greedy):
            raise ValueError("a greedy uid is no move")
        g = self._replay(len(self.moves))
        if g.dealt != len(self.deck):
            raise ValueError("the moves deal %d cards, the deck lists %d" % (g.dealt, len(self.deck)))
        if not 0 <= self.end < len(END_NAMES):
            raise ValueError("end %d names no reason" % self.end)
        if self.end == ENDS["unfinished"]:
            if g.terminal:
                raise ValueError("the record says unfinished and the game ends with move %d" % (len(self.moves) - 1))
        elif not g.terminal and self.end != ENDS["max_len"]:
            raise ValueError("n_moves is wrong: the record says the game ended by %s, and after its %d moves it is still running"
                             % (END_NAMES[self.end], len(self.moves)))
        elif g.terminal and self.end != g.end():
            raise ValueError("the game ends by %s, the record says %s" % (END_NAMES[g.end()], END_NAMES[self.end]))
        if (self.lives, self.info) != (g.life, g.info) or (self.end != ENDS["max_len"] and self.score != g.score()):
            raise ValueError("result (score %d, lives %d, info %d), the moves lead to (%d, %d, %d)"
                             % (self.score, self.lives, self.info, g.score(), g.life, g.info))
        return self

    def describe(self):
        """turn by turn: mover, move in words, card dealt, flags by name, running score / lives / tokens"""
        r, names = self.rules, self.meta.get("seats")
        who = lambda p: "seat %d%s" % (p, " (%s)" % names[p] if names and p < len(names) else "")   # noqa: E731
        g = _Game(r, self.deck)
        lines = ["%d players, hands of %d, %d colours x %d ranks, %d information and %d life tokens%s"
                 % (r["players"], r["hand_size"], r["colors"], r["ranks"], r["max_information_tokens"], r["max_life_tokens"],
                    ", bomb" if r["bomb"] else "")]
        if self.meta:
            lines.append("meta: " + json.dumps(self.meta, sort_keys=True))
        for p, h in enumerate(g.hands):
            lines.append("%s is dealt %s" % (who(p), " ".join(_card(c[0]) for c in h)))
        for k, uid in enumerate(self.moves):
            p, m = g.mover, decode_move(r, uid)
            if m and m[0] in ("play", "discard") and m[1] < len(g.hands[p]):
                what = "%ss slot %d (%s)" % (m[0], m[1], _card(g.hands[p][m[1]][0]))
            elif m:
                what = "tells %s its %s cards" % (who((p + m[1]) % r["players"]),
                                                  _COLOURS[m[2]] if m[0] == "hint_colour" else "rank-%d" % (m[2] + 1))
            else:
                what = "uid %d" % uid
            g.apply(uid)
            if m and m[0] == "play":
                what += ": " + ("scores" if g.last_move["scored"] else "MISFIRE")
            if self.greedy[k] != uid:
                what += " [greedy: uid %d]" % self.greedy[k]
            d = g.drawn[-1]
            draw = ", %s draws %s" % (who(d[0]), _card(d[1])) if d else ""
            fl = flag_names(self.flags[k] & ~FLAGS["counted"])
            lines.append("%3d  %s %s%s%s  | score %d lives %d tokens %d deck %d"
                         % (k, who(p), what, draw, "  {%s}" % ", ".join(fl) if fl else "", sum(g.fireworks), g.life, g.info, sum(g.deck)))
        lines.append("result: score %d, %d lives, %d tokens, ended by %s" % (self.score, self.lives, self.info, END_NAMES[self.end]))
        return "\n".join(lines)


def save(path, records):
    """JSON lines: one record per line"""
    with open(path, "w") as f:
        for rec in records:
            f.write(rec.to_json() + "\n")


def load(path):
    with open(path) as f:
        return [GameRecord.from_json(line) for line in f if line.strip()]


# ---- the device side ---------------------------------------------------------------------------------------------------------------
class GameRecorder:
    """the device log of `env`'s games (hsad_game_log): append(a, greedy_a) where the tournament counts behaviour -- every seat's
    action merged, env not yet stepped -- and collect() once games have finished.  The env must track its deck history."""

    def __init__(self, env):
        import ctypes as C
        from . import _lib
        self.env, self.lib, self._lib = env, env.lib, _lib
        self.h = C.c_void_p()
        _lib.check(self.lib.hsad_game_log_create(env.h, C.byref(self.h)))
        self.capacity = int(self.lib.hsad_game_log_capacity(self.h))
        self.record_bytes = int(self.lib.hsad_game_record_bytes(env.h))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.hsad_game_log_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        self._lib.check(self.lib.hsad_game_log_clear(self.h, self.env._stream()))

    def append(self, a, greedy_a=None):
        self._lib.check(self.lib.hsad_game_log_append(self.h, self.env.h, a.data_ptr(), greedy_a.data_ptr() if greedy_a is not None else None,
                                                      self.env._stream()))

    def overflow_count(self):
        import ctypes as C
        n = C.c_int32(0)
        self._lib.check(self.lib.hsad_game_log_overflow_count(self.h, C.byref(n)))
        return int(n.value)

    def select(self, where=None, take=None):
        """-> int32 tensor (on the device) of the finished games `where` (a GameFilter) and `take` (uint8 / bool [G]) keep, ascending"""
        import ctypes as C
        import torch
        env = self.env
        f = None
        if where is not None:
            f = self._lib.GameFilter(*[int(getattr(where, k)) for k, _ in self._lib.GameFilter._fields_])
        tk = None
        if take is not None:
            tk = torch.as_tensor(take, device=env.device).to(torch.uint8).contiguous()
            assert tk.shape == (env.G,)
        index = torch.zeros(env.G, dtype=torch.int32, device=env.device)
        n = torch.zeros(1, dtype=torch.int32, device=env.device)
        self._lib.check(self.lib.hsad_game_log_select(self.h, env.h, C.byref(f) if f is not None else None,
                                                      tk.data_ptr() if tk is not None else None, index.data_ptr(), n.data_ptr(),
                                                      env._stream()))
        return index[:int(n.cpu()[0])]

    def gather(self, index):
        """-> uint8 tensor [n, record_bytes] on the device: the records of the games in `index` (int32 on the device)"""
        import torch
        index = torch.as_tensor(index, device=self.env.device).to(torch.int32).contiguous()
        out = torch.zeros(int(index.numel()), self.record_bytes, dtype=torch.uint8, device=self.env.device)
        self._lib.check(self.lib.hsad_game_log_gather(self.h, self.env.h, index.data_ptr(), int(index.numel()), out.data_ptr(),
                                                      self.env._stream()))
        return out

    def collect(self, where=None, take=None):
        """the records of the finished games the filter keeps, each with meta["game"] = its index in the env; only those games'
        bytes cross to the host"""
        index = self.select(where, take)
        data = self.gather(index).cpu().numpy()
        games = index.cpu().numpy()
        return [GameRecord.from_bytes(data[j].tobytes(), meta={"game": int(games[j])}) for j in range(len(games))]


def replay(records, stop=None, env=None):
    """-> a BatchedHanabiEnv whose game j is records[j] played from its first deal up to move min(stop[j], n_moves) (stop None: to
    the end), in one launch (hsad_env_playout_logged).  env None: a fresh env of len(records) games under the records' rules (eps 0,
    no max_len); a given env must be started (reset) and have the records' rules and at least len(records) games -- the games past
    them are left alone.  env.replay_status (int32 [G]) holds the moves played per game (negative: HSAD_GR_STATUS_*)."""
    import numpy as np
    import torch
    from .env import BatchedHanabiEnv
    records = list(records)
    assert records, "no records"
    r = records[0].rules
    if any(rec.rules != r for rec in records):
        raise ValueError("the records were played under different rules")
    if env is None:
        env = BatchedHanabiEnv(len(records), players=r["players"], hand_size=r["hand_size"], bomb=r["bomb"], eps_list=[0.0], max_len=-1,
                               colors=r["colors"], ranks=r["ranks"], max_information_tokens=r["max_information_tokens"],
                               max_life_tokens=r["max_life_tokens"])
        env.reset()
    if len(records) > env.G:
        raise ValueError("%d records for an env of %d games" % (len(records), env.G))
    src = np.full(env.G, -1, dtype=np.int32)
    src[:len(records)] = np.arange(len(records))
    st = None
    if stop is not None:
        st = np.zeros(env.G, dtype=np.int32)
        st[:len(records)] = np.asarray(stop, dtype=np.int32)
    data = np.frombuffer(b"".join(rec.to_bytes() for rec in records), dtype=np.uint8).reshape(len(records), -1)
    env.replay_status = env.playout_logged(data, torch.from_numpy(src), None if st is None else torch.from_numpy(st))
    return env


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="print the games of a record file (JSON lines) turn by turn, or one position")
    ap.add_argument("file")
    ap.add_argument("--game", type=int, default=None, help="only this record of the file")
    ap.add_argument("--at", type=int, default=None, help="print the position before this move instead of the game")
    args = ap.parse_args(argv)
    records = load(args.file)
    chosen = range(len(records)) if args.game is None else [args.game]
    for i in chosen:
        if not 0 <= i < len(records):
            raise SystemExit("%s holds records 0..%d" % (args.file, len(records) - 1))
        print("== game %d ==" % i)
        print(records[i].describe() if args.at is None else repr(records[i].position(args.at)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
