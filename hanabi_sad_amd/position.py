"""Hanabi positions as data: a small readable description (`Position`) that converts to and from the canonical int32 record
`BatchedHanabiEnv.export_state` writes and `import_state` reads, and `validate`, the plain-Python statement of which records are
positions (include/hsad.h, HSAD_POS_*).  `validate` is written from that specification, not from the kernel: it tells a user why
a position was refused, and it is the reference the device's status words are held to.  No torch, no device.

Record layout (all int32; card type t = colour * 5 + rank):
  [0..25) deck counts   [25..50) discard counts   [50..55) fireworks   55 info   56 life   57 cur_player   58 next_non_chance_player
  59 turns_to_play   60 num_step   61 deck size   62 last move type (0 none, 1 play, 2 discard, 3 colour hint, 4 rank hint)
  63 player   64 target offset   65 colour   66 rank   67 card index   68 reveal mask   69 card colour   70 card rank   71 scored
  72 info token   73 generator draws (ignored by import)   74 last score   [80 ..) per seat and slot 6 words: card (-1 empty),
  plausible colours, plausible ranks, hinted colour (-1 none), hinted rank, 0   then per seat 5 words colour permutation and, after
  all of those, per seat 5 words its inverse.
"""
import numpy as np

CONSERVATION, BOARD, HANDS, KNOWLEDGE, LASTMOVE, STEP, PERM, TERMINAL = 1, 2, 4, 8, 16, 32, 64, 128
FIELD, NO_GENERATOR, LOOKAHEAD, HISTORY, SCRIPT, RECORD = 256, 512, 1024, 2048, 4096, 8192

_EXPLAIN = [
    (CONSERVATION, "conservation: some card type's deck + discards + hands + firework differs from the full deck, the deck-size "
                   "word is not the sum of the deck counts, or something sits in a colour or rank the rules do not have"),
    (BOARD, "board: a firework above the ranks, too many information or life tokens, the mover outside the seats, "
            "next_non_chance_player not the seat after the mover, or turns_to_play not what the deck allows"),
    (HANDS, "hands: a hole in a hand, a hand that is neither full nor one short on an empty deck, or more short hands than "
            "moves were made on the empty deck"),
    (KNOWLEDGE, "knowledge: a plausibility mask that is empty, leaves the rules or excludes the card itself, or a hinted colour / "
                "rank that is not the card's or not the mask's only bit"),
    (LASTMOVE, "last move: type, player, target offset, colour, rank, card index or reveal mask out of range"),
    (STEP, "step counter: num_step above 255 or above max_len"),
    (PERM, "colour permutation: not a permutation of the colours, inverse not its inverse, or not the identity with shuffle_color off"),
    (TERMINAL, "terminal: the position is finished (no life, all fireworks complete, no turn left, or max_len reached)"),
    (FIELD, "field: a record word does not fit the bit field that holds it"),
    (NO_GENERATOR, "no generator: seeds=None for a game that was never started"),
    (LOOKAHEAD, "look-ahead: more than two buffered generator outputs"),
    (HISTORY, "history: a deck-history or script card >= 25, or a script count out of range"),
    (SCRIPT, "script: the remaining scripted deals name a card the deck does not hold"),
    (RECORD, "record: the terminated bit disagrees with the position"),
]


def explain(flags):
    """the reasons in a status word, one string per flag set; [] for 0"""
    flags = int(flags)
    out = [text for bit, text in _EXPLAIN if flags & bit]
    rest = flags & ~sum(bit for bit, _ in _EXPLAIN)
    if flags < 0:
        return ["not taken (status %d)" % flags]
    if rest:
        out.append("unknown flag bits 0x%x" % rest)
    return out


def _rules(rules):
    return (int(rules.get("players", 2)), int(rules.get("hand_size", 5)), int(rules.get("colors", 5)), int(rules.get("ranks", 5)),
            int(rules.get("max_information_tokens", 8)), int(rules.get("max_life_tokens", 3)))


def state_words(rules):
    P, H = _rules(rules)[:2]
    return 80 + P * H * 6 + P * 10


def full_deck(rules):
    """copies of each card type in the rules' deck: 3 of the lowest rank, 1 of the highest, 2 between; 0 outside the rules"""
    _, _, nC, nR, _, _ = _rules(rules)
    return [0 if (t // 5 >= nC or t % 5 >= nR) else (3 if t % 5 == 0 else (1 if t % 5 == nR - 1 else 2)) for t in range(25)]


def _slot(o, P, H, p, i):
    b = 80 + (p * H + i) * 6
    return o[b:b + 5]


def validate(record, rules, env_flags=None):
    """record (state_words(rules) ints) -> HSAD_POS_* flags; 0 = a live position import_state accepts.  env_flags: max_len
    (default 80) and shuffle_color (default False) of the env the position is for."""
    env_flags = env_flags or {}
    max_len, shuffle = int(env_flags.get("max_len", 80)), bool(env_flags.get("shuffle_color", False))
    P, H, nC, nR, max_info, max_life = _rules(rules)
    o = [int(x) for x in np.asarray(record).reshape(-1)]
    assert len(o) == state_words(rules), "record has %d words, these rules need %d" % (len(o), state_words(rules))
    deck, disc, fw = o[0:25], o[25:50], o[50:55]
    info, life, cur, nxt, turns, num_step, deck_size = o[55:62]
    mtype = o[62]

    # -- what does not fit the bit field that will hold it (reported alone) --
    def fits(v, lo, hi):
        return lo <= v <= hi
    ok = all(fits(v, 0, 3) for v in deck + disc) and all(fits(v, 0, 7) for v in fw)
    ok = ok and fits(info, 0, 15) and fits(life, 0, 3) and fits(cur, -1, 6) and fits(nxt, 0, 7) and fits(turns, 0, 7)
    ok = ok and fits(deck_size, 0, 63) and fits(o[74], -1, 62) and fits(mtype, 0, 7)
    if mtype:
        ok = ok and fits(o[63], 0, 7)
    if mtype >= 3:
        ok = ok and fits(o[64], 0, 7) and fits(o[68], 0, 31)
        ok = ok and (mtype != 3 or fits(o[65], 0, 7)) and (mtype != 4 or fits(o[66], 0, 7))
    elif mtype:
        ok = ok and fits(o[67], 0, 7) and fits(o[69], 0, 7) and fits(o[70], 0, 7) and fits(o[71], 0, 1) and fits(o[72], 0, 1)
    hole = False
    hands = []
    for p in range(P):
        cards, gap = [], False
        for i in range(H):
            s = _slot(o, P, H, p, i)
            if s[0] == -1:
                gap = True
                continue
            if gap:
                hole = True
                continue
            ok = ok and fits(s[0], 0, 31) and fits(s[1], 0, 31) and fits(s[2], 0, 31) and fits(s[3], -1, 6) and fits(s[4], -1, 6)
            cards.append(s)
        hands.append(cards)
    pbase = 80 + P * H * 6
    perms = [o[pbase + p * 5:pbase + p * 5 + 5] for p in range(P)]
    invs = [o[pbase + P * 5 + p * 5:pbase + P * 5 + p * 5 + 5] for p in range(P)]
    ok = ok and all(fits(v, 0, 7) for row in perms + invs for v in row)
    if not ok:
        return FIELD
    if hole:
        return HANDS   # nothing more can be said about hands that are not lists

    flags = 0
    # -- step counter, and whether the game is over --
    if not fits(num_step, 0, 255) or (max_len > 0 and num_step > max_len):
        flags |= STEP
    fsum = sum(fw[:nC])
    term = life < 1 or fsum >= nC * nR or turns < 1 or (max_len > 0 and num_step == max_len)

    # -- conservation --
    full = full_deck(rules)
    held = [0] * 32
    for cards in hands:
        for s in cards:
            held[s[0]] += 1
            if s[0] >= 25 or s[0] // 5 >= nC or s[0] % 5 >= nR:
                flags |= CONSERVATION
    for t in range(25):
        c, r = divmod(t, 5)
        on_table = 1 if (c < nC and fw[c] > r) else 0
        if deck[t] + disc[t] + held[t] + on_table != full[t]:
            flags |= CONSERVATION
    if any(fw[c] for c in range(nC, 5)):
        flags |= CONSERVATION
    deck_n = sum(deck)
    if deck_size != deck_n:
        flags |= CONSERVATION

    # -- board --
    if any(fw[c] > nR for c in range(nC)) or info > max_info or life > max_life or turns > P or cur >= P or nxt >= P:
        flags |= BOARD
    short = [p for p in range(P) if len(hands[p]) < H]
    if any(len(h) < H - 1 for h in hands):
        flags |= HANDS
    if deck_n > 0:
        # a live game is dealt back to full hands after every move; a final move is followed by no deal
        if turns != P:
            flags |= BOARD
        if len(short) > (1 if term else 0):
            flags |= HANDS
        if term and len(short) == 1:
            if cur != -1 or nxt != (short[0] + 1) % P:
                flags |= BOARD
        elif cur < 0:
            flags |= BOARD
    else:
        if len(short) > P - turns:
            flags |= HANDS
        if cur < 0:
            flags |= BOARD
    if 0 <= cur < P and nxt != (cur + 1) % P:
        flags |= BOARD

    # -- knowledge --
    cmask, rmask = (1 << nC) - 1, (1 << nR) - 1
    for cards in hands:
        for card, cm, rm, hc, hr in cards:
            if card >= 25 or card // 5 >= nC or card % 5 >= nR:
                continue
            c, r = divmod(card, 5)
            if cm == 0 or rm == 0 or cm & ~cmask or rm & ~rmask or not (cm >> c) & 1 or not (rm >> r) & 1:
                flags |= KNOWLEDGE
            if hc >= 0 and (hc != c or cm != 1 << c):
                flags |= KNOWLEDGE
            if hr >= 0 and (hr != r or rm != 1 << r):
                flags |= KNOWLEDGE

    # -- last move --
    if mtype > 4:
        flags |= LASTMOVE
    elif mtype >= 1:
        bad = o[63] >= P
        if mtype >= 3:
            bad = bad or not 1 <= o[64] <= P - 1 or (mtype == 3 and o[65] >= nC) or (mtype == 4 and o[66] >= nR) or o[68] >= 1 << H
        else:
            bad = bad or o[67] >= H or o[69] >= nC or o[70] >= nR
        if bad:
            flags |= LASTMOVE

    # -- colour permutations --
    for pm, inv in zip(perms, invs):
        good = sorted(pm) == [0, 1, 2, 3, 4] and all(v < 5 and inv[v] == c for c, v in enumerate(pm) if v < 5)
        good = good and all(pm[c] == c for c in range(nC, 5)) and (shuffle or pm == [0, 1, 2, 3, 4])
        if not good:
            flags |= PERM
    return flags | (TERMINAL if term else 0)


class Card:
    """one card in a hand with what its holder has been told: colours / ranks = plausible masks (None: every colour / rank of the
    rules), hinted_colour / hinted_rank = the value a hint named, -1 if none"""

    def __init__(self, colour, rank, colours=None, ranks=None, hinted_colour=-1, hinted_rank=-1):
        self.colour, self.rank, self.colours, self.ranks = int(colour), int(rank), colours, ranks
        self.hinted_colour, self.hinted_rank = int(hinted_colour), int(hinted_rank)

    def _key(self):
        return (self.colour, self.rank, self.colours, self.ranks, self.hinted_colour, self.hinted_rank)

    def __eq__(self, other):
        return isinstance(other, Card) and self._key() == other._key()

    def __repr__(self):
        return "Card(%d, %d, colours=%s, ranks=%s, hinted_colour=%d, hinted_rank=%d)" % self._key()


_MOVE_TYPES = {"play": 1, "discard": 2, "hint_colour": 3, "hint_rank": 4}
_MOVE_NAMES = {v: k for k, v in _MOVE_TYPES.items()}


class Position:
    """A Hanabi position somebody can write down.
      rules      dict with players, hand_size, colors, ranks, max_information_tokens, max_life_tokens (tests/search_fixtures.CONFIGS)
      hands      per seat a list of Card or (colour, rank), slot 0 first
      fireworks  per colour the number of cards played (default none)
      discards   list of (colour, rank), or 25 counts
      deck       "rest" (every card not in a hand, on a firework or discarded), 25 counts, or {(colour, rank): n}
      info, life tokens left (default: the rules' maximum);  mover: the seat on turn
      turns_to_play  default P (it counts down only once the deck is empty);  num_step, last_score
      last_move  None or dict(type="play"|"discard", player, card_index, colour, rank, scored, info_token)
                 or dict(type="hint_colour"|"hint_rank", player, target_offset, value, reveal_mask)
      perms      per seat its colour permutation (default the identity; the inverse is derived)
    Everything is normalised at construction, so two positions are equal iff they describe the same record."""

    def __init__(self, rules, hands, fireworks=None, discards=(), deck="rest", info=None, life=None, mover=0, turns_to_play=None,
                 num_step=0, last_move=None, last_score=-1, perms=None):
        P, H, nC, nR, max_info, max_life = _rules(rules)
        self.rules = dict(players=P, hand_size=H, colors=nC, ranks=nR, max_information_tokens=max_info, max_life_tokens=max_life)
        assert len(hands) == P, "one hand per seat"
        cmask, rmask = (1 << nC) - 1, (1 << nR) - 1
        self.hands = []
        for hand in hands:
            assert len(hand) <= H
            cards = []
            for c in hand:
                c = c if isinstance(c, Card) else Card(*c)
                cards.append(Card(c.colour, c.rank, cmask if c.colours is None else int(c.colours),
                                  rmask if c.ranks is None else int(c.ranks), c.hinted_colour, c.hinted_rank))
            self.hands.append(cards)
        self.fireworks = [int(v) for v in (fireworks if fireworks is not None else [0] * 5)]
        self.fireworks += [0] * (5 - len(self.fireworks))
        if len(discards) == 25 and not isinstance(discards[0], (tuple, list)):
            self.discards = [int(v) for v in discards]
        else:
            self.discards = [0] * 25
            for c, r in discards:
                self.discards[c * 5 + r] += 1
        if isinstance(deck, str):
            assert deck == "rest"
            left = full_deck(rules)
            for cards in self.hands:
                for c in cards:
                    left[c.colour * 5 + c.rank] -= 1
            for t in range(25):
                left[t] -= self.discards[t] + (1 if self.fireworks[t // 5] > t % 5 else 0)
            assert min(left) >= 0, "more copies of a card than the deck has: %s" % left
            self.deck = left
        elif isinstance(deck, dict):
            self.deck = [0] * 25
            for (c, r), n in deck.items():
                self.deck[c * 5 + r] = int(n)
        else:
            self.deck = [int(v) for v in deck]
            assert len(self.deck) == 25
        self.info = max_info if info is None else int(info)
        self.life = max_life if life is None else int(life)
        self.mover = int(mover)
        self.turns_to_play = P if turns_to_play is None else int(turns_to_play)
        self.num_step, self.last_score = int(num_step), int(last_score)
        self.last_move = dict(last_move) if last_move else None
        if self.last_move and self.last_move["type"] in ("play", "discard"):
            self.last_move.setdefault("scored", 0)
            self.last_move.setdefault("info_token", 0)
        self.perms = [[int(v) for v in row] for row in perms] if perms is not None else [[0, 1, 2, 3, 4] for _ in range(P)]

    def _fields(self):
        return (self.rules, self.hands, self.fireworks, self.discards, self.deck, self.info, self.life, self.mover, self.turns_to_play,
                self.num_step, self.last_move, self.last_score, self.perms)

    def __eq__(self, other):
        return isinstance(other, Position) and self._fields() == other._fields()

    def __repr__(self):
        return "Position(%s)" % ", ".join("%s=%r" % kv for kv in zip(
            ("rules", "hands", "fireworks", "discards", "deck", "info", "life", "mover", "turns_to_play", "num_step", "last_move",
             "last_score", "perms"), self._fields()))

    def to_record(self):
        """the canonical record, int32 [state_words(rules)]"""
        P, H = self.rules["players"], self.rules["hand_size"]
        o = np.zeros(state_words(self.rules), np.int32)
        o[0:25], o[25:50], o[50:55] = self.deck, self.discards, self.fireworks
        o[55:62] = [self.info, self.life, self.mover, (self.mover + 1) % P, self.turns_to_play, self.num_step, sum(self.deck)]
        o[63:68] = -1
        o[69:71] = -1
        m = self.last_move
        if m:
            t = _MOVE_TYPES[m["type"]]
            o[62], o[63] = t, m["player"]
            if t >= 3:
                o[64], o[65 if t == 3 else 66], o[68] = m["target_offset"], m["value"], m["reveal_mask"]
            else:
                o[67], o[69], o[70], o[71], o[72] = m["card_index"], m["colour"], m["rank"], m.get("scored", 0), m.get("info_token", 0)
        o[74] = self.last_score
        for p in range(P):
            for i in range(H):
                b = 80 + (p * H + i) * 6
                if i < len(self.hands[p]):
                    c = self.hands[p][i]
                    o[b:b + 5] = [c.colour * 5 + c.rank, c.colours, c.ranks, c.hinted_colour, c.hinted_rank]
                else:
                    o[b:b + 5] = [-1, 0, 0, -1, -1]
        base = 80 + P * H * 6
        for p in range(P):
            for c in range(5):
                o[base + p * 5 + c] = self.perms[p][c]
                if 0 <= self.perms[p][c] < 5:
                    o[base + P * 5 + p * 5 + self.perms[p][c]] = c
        return o


def from_record(record, rules):
    """the Position a record describes (the record should validate: holes in hands and fields the last move's type does not use
    are not represented)"""
    P, H = _rules(rules)[:2]
    o = [int(x) for x in np.asarray(record).reshape(-1)]
    assert len(o) == state_words(rules)
    hands = []
    for p in range(P):
        cards = []
        for i in range(H):
            s = _slot(o, P, H, p, i)
            if s[0] >= 0:
                cards.append(Card(s[0] // 5, s[0] % 5, s[1], s[2], s[3], s[4]))
        hands.append(cards)
    t = o[62]
    m = None
    if t >= 3:
        m = dict(type=_MOVE_NAMES.get(t, t), player=o[63], target_offset=o[64], value=o[65] if t == 3 else o[66], reveal_mask=o[68])
    elif t:
        m = dict(type=_MOVE_NAMES[t], player=o[63], card_index=o[67], colour=o[69], rank=o[70], scored=o[71], info_token=o[72])
    base = 80 + P * H * 6
    return Position(rules, hands, fireworks=o[50:55], discards=o[25:50], deck=o[0:25], info=o[55], life=o[56], mover=o[57],
                    turns_to_play=o[59], num_step=o[60], last_move=m, last_score=o[74],
                    perms=[o[base + p * 5:base + p * 5 + 5] for p in range(P)])
