"""Plain-Python rule-list bot over `position.Position` (position.from_record of an export_state record), written from the rule table
of the specification: ordered rules, the first that fires gives the uid, else the lowest legal uid.  Independent of
csrc/hsad_rulebot.h; the tests hold the header and the kernels to it, action for action."""
from hanabi_sad_amd import position as pos
from tests.determinize_ref import policy_hash

(PLAY_CERTAIN, PLAY_PROBABLE, PLAY_PROBABLE_ENDGAME, HINT_PLAYABLE, HINT_USEFUL, HINT_DEAD, HINT_RANDOM, DISCARD_CERTAIN_DEAD,
 DISCARD_PROBABLE_DEAD, DISCARD_UNHINTED_OLDEST, DISCARD_OLDEST, DISCARD_RANDOM, LEGAL_RANDOM) = range(1, 14)

PRESETS = {
    "cautious": [(1, 0), (4, 0), (8, 0), (10, 0), (11, 0), (7, 0)],
    "piers": [(3, 0), (1, 0), (2, 60), (4, 0), (6, 0), (8, 0), (10, 0), (7, 0)],
    "flawed": [(1, 0), (2, 25), (7, 0), (10, 0), (12, 0)],
    "random": [(13, 0)],
}


def num_actions(rules):
    return 2 * rules["hand_size"] + (rules["players"] - 1) * (rules["colors"] + rules["ranks"]) + 1


def legal_uids(P_, p):
    """sorted uids seat p may play in position P_ (the legal_move row of that seat)"""
    r = P_.rules
    P, H, nC, nR = r["players"], r["hand_size"], r["colors"], r["ranks"]
    if P_.mover != p:
        return [num_actions(r) - 1]
    out = set()
    n = len(P_.hands[p])
    if P_.info < r["max_information_tokens"]:
        out |= set(range(n))
    out |= set(H + i for i in range(n))
    if P_.info > 0:
        for o in range(1, P):
            for card in P_.hands[(p + o) % P]:
                out.add(2 * H + (o - 1) * nC + P_.perms[p][card.colour])
                out.add(2 * H + (P - 1) * nC + (o - 1) * nR + card.rank)
    return sorted(out) or [num_actions(r) - 1]


def _pick(h, uids):
    return uids[h % len(uids)]


def act(P_, p, bot, seed=0, key=0, counter=0):
    """(uid, index of the deciding rule or -1) for seat p of position P_ under the rule list `bot` = [(code, k)]"""
    r = P_.rules
    P, H, nC, nR, max_info = r["players"], r["hand_size"], r["colors"], r["ranks"], r["max_information_tokens"]
    if P_.mover != p:
        return num_actions(r) - 1, -1
    full = pos.full_deck(r)
    fw, disc = P_.fireworks, P_.discards
    legal = legal_uids(P_, p)
    own = P_.hands[p]
    pool = list(P_.deck)
    for c in own:
        pool[c.colour * 5 + c.rank] += 1

    def playable(t):
        return t % 5 == fw[t // 5]

    def dead(t):
        c, rk = divmod(t, 5)
        return rk < fw[c] or any(disc[c * 5 + q] == full[c * 5 + q] for q in range(fw[c], rk))

    def compat(card):
        return [t for t in range(25) if (card.colours >> (t // 5)) & 1 and (card.ranks >> (t % 5)) & 1]

    n = [sum(pool[t] for t in compat(c)) for c in own]
    play = [sum(pool[t] for t in compat(c) if playable(t)) for c in own]
    dd = [sum(pool[t] for t in compat(c) if dead(t)) for c in own]

    def best(x):
        b = 0
        for i in range(1, len(own)):
            if x[i] * n[b] > x[b] * n[i]:
                b = i
        return b

    def publicly(card, what):
        return all(what(t) for t in compat(card) if full[t] > 0)

    def hint_for(o, card):
        if bin(card.ranks).count("1") > 1:
            return 2 * H + (P - 1) * nC + (o - 1) * nR + card.rank
        if bin(card.colours).count("1") > 1:
            return 2 * H + (o - 1) * nC + P_.perms[p][card.colour]
        return None

    def scan(hit):
        for o in range(1, P):
            for card in P_.hands[(p + o) % P]:
                if hit(card) and hint_for(o, card) is not None:
                    return hint_for(o, card)
        return None

    can_hint, can_discard = P_.info > 0, P_.info < max_info
    deck_size = sum(P_.deck)
    for j, (code, k) in enumerate(bot):
        uid = None
        h = policy_hash(seed, key, counter, 128 + 16 * p + j)
        if code == PLAY_CERTAIN:
            uid = next((H + i for i in range(len(own)) if play[i] == n[i]), None)
        elif code in (PLAY_PROBABLE, PLAY_PROBABLE_ENDGAME):
            if P_.life > 1 and own and (code == PLAY_PROBABLE or deck_size == 0):
                b = best(play)
                if play[b] * 100 >= k * n[b]:
                    uid = H + b
        elif code == HINT_PLAYABLE:
            if can_hint:
                uid = scan(lambda c: playable(c.colour * 5 + c.rank) and not publicly(c, playable))
        elif code == HINT_USEFUL:
            if can_hint:
                uid = scan(lambda c: not dead(c.colour * 5 + c.rank))
        elif code == HINT_DEAD:
            if can_hint:
                uid = scan(lambda c: dead(c.colour * 5 + c.rank) and not publicly(c, dead))
        elif code == HINT_RANDOM:
            hints = [u for u in legal if 2 * H <= u < num_actions(r) - 1]
            if can_hint and hints:
                uid = _pick(h, hints)
        elif code == DISCARD_CERTAIN_DEAD:
            if can_discard:
                uid = next((i for i in range(len(own)) if dd[i] == n[i]), None)
        elif code == DISCARD_PROBABLE_DEAD:
            if can_discard and own:
                b = best(dd)
                if dd[b] * 100 >= k * n[b]:
                    uid = b
        elif code == DISCARD_UNHINTED_OLDEST:
            if can_discard:
                uid = next((i for i, c in enumerate(own) if c.hinted_colour < 0 and c.hinted_rank < 0), None)
        elif code == DISCARD_OLDEST:
            if can_discard and own:
                uid = 0
        elif code == DISCARD_RANDOM:
            discards = [u for u in legal if u < H]
            if can_discard and discards:
                uid = _pick(h, discards)
        elif code == LEGAL_RANDOM:
            uid = _pick(h, legal)
        else:
            raise ValueError("unknown rule code %d" % code)
        if uid is not None:
            return uid, j
    return legal[0], -1


def act_record(record, rules, bot, seed=0, key=0, counter=0):
    """act for the seat on turn of an export_state record -> (seat, uid, deciding rule index)"""
    P_ = pos.from_record(record, rules)
    uid, j = act(P_, P_.mover, bot, seed, key, counter)
    return P_.mover, uid, j
