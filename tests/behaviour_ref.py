"""Plain-Python move classifier over `position.Position` plus a uid, written from the HSAD_BH_* table of include/hsad.h: the thirteen
increments of the behaviour counters for the move the seat on turn is about to make.  Independent of csrc/hsad_behaviour.h; the
tests hold the header and the kernel to it, counter for counter."""
from hanabi_sad_amd import position as pos
from tests import rulebot_ref as ref

NAMES = ("MOVES", "PLAY_OK", "PLAY_FAIL", "PLAY_CERTAIN", "DISCARD", "DISCARD_CERTAIN_DEAD", "HINT_COLOUR", "HINT_RANK", "HINT_CARDS",
         "HINT_PLAYABLE", "LAST_COPY_LOST", "INFO_SUM", "LAST_LIFE")
(MOVES, PLAY_OK, PLAY_FAIL, PLAY_CERTAIN, DISCARD, DISCARD_CERTAIN_DEAD, HINT_COLOUR, HINT_RANK, HINT_CARDS, HINT_PLAYABLE,
 LAST_COPY_LOST, INFO_SUM, LAST_LIFE) = range(13)
NSTAT = 13


def classify(P_, uid):
    """the 13 increments of the move `uid` by the seat on turn of position P_ (a list of ints; all zero when nothing is counted)"""
    r = P_.rules
    P, H, nC, nR = r["players"], r["hand_size"], r["colors"], r["ranks"]
    p = P_.mover
    out = [0] * NSTAT
    uid = int(uid)
    if uid < 0 or uid >= ref.num_actions(r) - 1:
        return out
    full = pos.full_deck(r)
    fw, disc = P_.fireworks, P_.discards

    def playable(t):
        return t % 5 == fw[t // 5]

    def dead(t):
        c, rk = divmod(t, 5)
        return rk < fw[c] or any(disc[c * 5 + q] == full[c * 5 + q] for q in range(fw[c], rk))

    def counted():
        out[MOVES] = 1
        out[INFO_SUM] = P_.info

    if uid < 2 * H:
        own = P_.hands[p]
        i = uid % H
        if i >= len(own):
            return out
        card = own[i]
        t = card.colour * 5 + card.rank
        pool = list(P_.deck)
        for c in own:
            pool[c.colour * 5 + c.rank] += 1
        compat = [x for x in range(25) if (card.colours >> (x // 5)) & 1 and (card.ranks >> (x % 5)) & 1]
        n = sum(pool[x] for x in compat)
        last_copy = not dead(t) and disc[t] == full[t] - 1
        counted()
        if uid >= H:
            out[PLAY_OK if playable(t) else PLAY_FAIL] = 1
            out[PLAY_CERTAIN] = int(sum(pool[x] for x in compat if playable(x)) == n)
            if not playable(t):
                out[LAST_COPY_LOST] = int(last_copy)
                out[LAST_LIFE] = int(P_.life == 1)
        else:
            out[DISCARD] = 1
            out[DISCARD_CERTAIN_DEAD] = int(sum(pool[x] for x in compat if dead(x)) == n)
            out[LAST_COPY_LOST] = int(last_copy)
        return out

    k = uid - 2 * H
    if k < (P - 1) * nC:
        o, named = k // nC + 1, k % nC
        colour = P_.perms[p].index(named)         # the uid names perms[p][colour]
        hit = [c for c in P_.hands[(p + o) % P] if c.colour == colour]
        kind = HINT_COLOUR
    else:
        k -= (P - 1) * nC
        o, rank = k // nR + 1, k % nR
        hit = [c for c in P_.hands[(p + o) % P] if c.rank == rank]
        kind = HINT_RANK
    if not hit:
        return out
    counted()
    out[kind] = 1
    out[HINT_CARDS] = len(hit)
    out[HINT_PLAYABLE] = int(any(playable(c.colour * 5 + c.rank) for c in hit))
    return out


def classify_record(record, rules, uid):
    """classify for the seat on turn of an export_state record -> (seat, the 13 increments)"""
    P_ = pos.from_record(record, rules)
    return P_.mover, classify(P_, uid)
