"""Shared by test_position_cpu.py and test_env_position_gpu.py: the rule sets, hand-written positions, records of games the CPU
oracle played, and the table of single-field corruptions with the one flag each must raise."""
import numpy as np

from hanabi_sad_amd import position as pos
from tests.search_fixtures import CONFIGS

RULESETS = dict(CONFIGS, p5h4=dict(players=5, hand_size=4, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3))
MAX_LEN = 80


def all_cards(rules):
    """every physical card of the rules' deck as (colour, rank), colour-major"""
    full = pos.full_deck(rules)
    return [(t // 5, t % 5) for t in range(25) for _ in range(full[t])]


def opening(rules, **kw):
    """a fresh-looking deal: the hands take the first P * H cards of the sorted deck, the rest is the deck"""
    P, H = rules["players"], rules["hand_size"]
    cards = all_cards(rules)
    return pos.Position(rules, [cards[p * H:(p + 1) * H] for p in range(P)], **kw)


def endgame(rules, turns_to_play=None, mover=0, short=(), **kw):
    """an empty deck: the hands hold the LAST cards of the sorted deck (seats in `short` one card fewer), everything else is
    discarded, no firework played"""
    P, H = rules["players"], rules["hand_size"]
    cards = all_cards(rules)[::-1]
    hands, k = [], 0
    for p in range(P):
        n = H - (1 if p in short else 0)
        hands.append(cards[k:k + n])
        k += n
    return pos.Position(rules, hands, discards=cards[k:], deck="rest", mover=mover,
                        turns_to_play=rules["players"] if turns_to_play is None else turns_to_play, **kw)


def oracle_game(name, seed, policy_seed, shuffle_color=False, sad=False, max_len=MAX_LEN, bomb=0):
    """one game of the CPU oracle under seeded random legal moves, played to its end: [(record, finished)] after the reset and after
    every move"""
    from oracle import oracle as _oracle
    from tests.variant_oracle import variant_oracle
    env = variant_oracle.VariantEnv(seed=seed, bomb=bomb, eps_list=(0.0,), max_len=max_len, sad=sad, shuffle_color=shuffle_color,
                                    **RULESETS[name])
    env.reset()
    out = [(env.export_state().copy(), False)]
    counter = 0
    while not env.terminated():
        a, g = _oracle.policy_random(env.legal, policy_seed, seed, counter)
        env.step(a, g)
        counter += 1
        out.append((env.export_state().copy(), env.terminated()))
    return out


def _slot(rules, p, i):
    return 80 + (p * rules["hand_size"] + i) * 6


def corruptions(rules, shuffle_color=False, max_len=MAX_LEN):
    """[(name, record, the one flag validate must return)]: one field changed in a valid record.  The bases are hand-written: an
    opening (deck non-empty, full hands) and an endgame (deck empty)."""
    P, H, nC, nR = rules["players"], rules["hand_size"], rules["colors"], rules["ranks"]
    a = opening(rules).to_record()
    e = endgame(rules).to_record()
    out = []

    def case(name, base, flag, edit):
        r = base.copy()
        edit(r)
        out.append((name, r, flag))

    t_low = next(t for t in range(25) if a[t] in (1, 2))          # a type the deck holds, with room in its 2-bit count
    def extra_copy(r):
        r[t_low] += 1
        r[61] += 1
    case("one copy too many", a, pos.CONSERVATION, extra_copy)
    case("deck size off by one", a, pos.CONSERVATION, lambda r: r.__setitem__(61, r[61] + 1))
    case("info above the maximum", a, pos.BOARD, lambda r: r.__setitem__(55, rules["max_information_tokens"] + 1))
    case("life 0", a, pos.TERMINAL, lambda r: r.__setitem__(56, 0))
    case("mover P", a, pos.BOARD, lambda r: r.__setitem__(57, P))
    case("next is the mover", a, pos.BOARD, lambda r: r.__setitem__(58, r[57]))
    case("turns_to_play 0", e, pos.TERMINAL, lambda r: r.__setitem__(59, 0))
    case("turns_to_play below P over a deck", a, pos.BOARD, lambda r: r.__setitem__(59, P - 1))
    case("a hole in a hand", a, pos.HANDS, lambda r: r.__setitem__(_slot(rules, 0, 0), -1))

    def short_over_deck(r):
        b = _slot(rules, 0, H - 1)
        r[r[b]] += 1          # the card goes back to the deck: every count still adds up
        r[61] += 1
        r[b:b + 5] = [-1, 0, 0, -1, -1]
    case("a short hand with cards in the deck", a, pos.HANDS, short_over_deck)

    def short_too_early(r):   # deck empty, all P turns left: no move has been made that could have shortened a hand
        b = _slot(rules, 1, H - 1)
        r[25 + r[b]] += 1
        r[b:b + 5] = [-1, 0, 0, -1, -1]
    case("a short hand before any move on the empty deck", e, pos.HANDS, short_too_early)

    def own_colour_out(r):
        b = _slot(rules, 0, 0)
        r[b + 1] &= ~(1 << (r[b] // 5))
    case("the card's colour implausible", a, pos.KNOWLEDGE, own_colour_out)

    def wrong_hint(r):
        b = _slot(rules, 0, 1 % H)
        r[b + 4] = (r[b] % 5 + 1) % nR
    case("a hinted rank that is not the card's", a, pos.KNOWLEDGE, wrong_hint)

    def discard_of(idx):
        def f(r):
            r[62:73] = [2, 0, -1, -1, -1, idx, 0, 0, 0, 0, 0]
        return f
    case("last move card index H", a, pos.LASTMOVE, discard_of(H))
    case("last move hint offset 0", a, pos.LASTMOVE, lambda r: r.__setitem__(slice(62, 73), [3, 0, 0, 0, -1, -1, 1, -1, -1, 0, 0]))
    case("last move type 5", a, pos.LASTMOVE, lambda r: r.__setitem__(slice(62, 73), [5, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]))
    case("num_step = max_len", a, pos.TERMINAL, lambda r: r.__setitem__(60, max_len))
    case("num_step above max_len", a, pos.STEP, lambda r: r.__setitem__(60, max_len + 1))
    pbase = 80 + P * H * 6
    case("a permutation with a repeated colour", a, pos.PERM, lambda r: r.__setitem__(pbase + 1, 0))

    def swapped(r):   # a real permutation with its inverse: wrong only where the env does not shuffle, or where it moves an unused colour
        r[pbase + 3], r[pbase + 4] = 4, 3
        r[pbase + P * 5 + 3], r[pbase + P * 5 + 4] = 4, 3
    if not shuffle_color or nC < 5:
        case("a permutation the env cannot have drawn", a, pos.PERM, swapped)
    if nC < 5:
        case("a discarded card of a colour the rules lack", a, pos.CONSERVATION, lambda r: r.__setitem__(25 + nC * 5, 1))

        def mask_outside(r):
            r[_slot(rules, 0, 0) + 1] |= 1 << nC
        case("a plausible colour the rules lack", a, pos.KNOWLEDGE, mask_outside)
    # values that fit no bit field
    case("deck count 4", a, pos.FIELD, lambda r: r.__setitem__(t_low, 4))
    case("info 16", a, pos.FIELD, lambda r: r.__setitem__(55, 16))
    case("card 32", a, pos.FIELD, lambda r: r.__setitem__(_slot(rules, 0, 0), 32))
    case("hinted colour -2", a, pos.FIELD, lambda r: r.__setitem__(_slot(rules, 0, 0) + 3, -2))
    case("last score 63", a, pos.FIELD, lambda r: r.__setitem__(74, 63))
    return out


def type_counts(record, rules):
    """per card type: deck + discards + hands + fireworks, from one record"""
    P, H = rules["players"], rules["hand_size"]
    r = np.asarray(record)
    n = r[0:25].astype(np.int64) + r[25:50]
    for p in range(P):
        for i in range(H):
            c = int(r[_slot(rules, p, i)])
            if c >= 0:
                n[c] += 1
    for c in range(5):
        for k in range(int(r[50 + c])):
            n[c * 5 + k] += 1
    return n
