"""Plain-Python restatement of the game-record specification (include/hsad.h, HSAD_GR_*): capacity, byte layout, the colour of a
logged colour hint, the flag byte read off the behaviour increments, the filter.  Written from the header's text, independent of
csrc/hsad_game_record.h and of hanabi_sad_amd/game_record.py; the tests hold both to it.  Also the games the record tests play on
the CPU oracle: seeded, by the random-legal policy or by the reference rule bots (tests/rulebot_ref.py)."""
import functools

import numpy as np

from tests import behaviour_ref as bref
from tests import rulebot_ref as ref

RULESETS = {
    "full": dict(players=2, hand_size=5, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3),
    "p4h4": dict(players=4, hand_size=4, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3),
    "c3r4h3": dict(players=2, hand_size=3, colors=3, ranks=4, max_information_tokens=5, max_life_tokens=2),
}
# every rule set the env's tests use: the capacity formula is checked on all of them
ALL_RULESETS = dict(RULESETS,
                    small=dict(players=2, hand_size=2, colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1),
                    c3r4=dict(players=3, hand_size=4, colors=3, ranks=4, max_information_tokens=6, max_life_tokens=2),
                    p5h4=dict(players=5, hand_size=4, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3),
                    p3h5=dict(players=3, hand_size=5, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3))

(COUNTED, PLAY_FAIL, PLAY_UNCERTAIN, LAST_COPY_LOST, LAST_LIFE, HINT_NOT_PLAYABLE, DISCARD_UNCERTAIN, NO_INFO) = (1 << i for i in range(8))
END_UNFINISHED, END_LIVES, END_DECK, END_PERFECT, END_MAX_LEN = range(5)


def deck_size(rules):
    per_colour = 3 if rules["ranks"] == 1 else 3 + 2 * (rules["ranks"] - 2) + 1
    return rules["colors"] * per_colour


def capacity(rules):
    """plays + discards while the deck holds a card: D.  Hints: one token each, tokens from the stock, from at most D discards and
    from at most `colors` completed stacks.  Then P turns."""
    D = deck_size(rules) - rules["players"] * rules["hand_size"]
    hints = rules["max_information_tokens"] + D + rules["colors"]
    return D + hints + rules["players"]


def record_bytes(rules):
    return 16 + 52 + 3 * capacity(rules)


def pack(rules, bomb, deck, moves, greedy, flags, score, lives, info, end):
    L = capacity(rules)
    head = [1, rules["players"], rules["hand_size"], rules["colors"], rules["ranks"], rules["max_information_tokens"],
            rules["max_life_tokens"], bomb, len(moves), len(deck), score, lives, info, end, L, 0]
    pad = lambda x, n: list(x) + [0] * (n - len(x))   # noqa: E731
    return bytes(head + pad(deck, 52) + pad(moves, L) + pad(greedy, L) + pad(flags, L))


def is_colour_hint(rules, uid):
    H = rules["hand_size"]
    return 2 * H <= uid < 2 * H + (rules["players"] - 1) * rules["colors"]


def uid_to_true(rules, uid, perm):
    """perm[c] = what the actor calls colour c"""
    if not is_colour_hint(rules, uid):
        return uid
    k = uid - 2 * rules["hand_size"]
    o, named = divmod(k, rules["colors"])
    return 2 * rules["hand_size"] + o * rules["colors"] + list(perm).index(named)


def uid_from_true(rules, uid, perm):
    if not is_colour_hint(rules, uid):
        return uid
    k = uid - 2 * rules["hand_size"]
    o, truth = divmod(k, rules["colors"])
    return 2 * rules["hand_size"] + o * rules["colors"] + perm[truth]


def flags_of(inc):
    """the flag byte of the 13 behaviour increments of a move (tests/behaviour_ref.classify)"""
    if not inc[bref.MOVES]:
        return 0
    play = inc[bref.PLAY_OK] or inc[bref.PLAY_FAIL]
    hint = inc[bref.HINT_COLOUR] or inc[bref.HINT_RANK]
    f = COUNTED
    f |= PLAY_FAIL if inc[bref.PLAY_FAIL] else 0
    f |= PLAY_UNCERTAIN if play and not inc[bref.PLAY_CERTAIN] else 0
    f |= LAST_COPY_LOST if inc[bref.LAST_COPY_LOST] else 0
    f |= LAST_LIFE if inc[bref.LAST_LIFE] else 0
    f |= HINT_NOT_PLAYABLE if hint and not inc[bref.HINT_PLAYABLE] else 0
    f |= DISCARD_UNCERTAIN if inc[bref.DISCARD] and not inc[bref.DISCARD_CERTAIN_DEAD] else 0
    f |= NO_INFO if inc[bref.INFO_SUM] == 0 else 0
    return f


def filter_pass(flt, players, score, lives, end, flags):
    """flt: dict of the eight hsad_game_filter fields; flags: the game's flag bytes, one per move"""
    if end == END_UNFINISHED:
        return False
    seats = flt["seat_mask"] or (1 << players) - 1
    hit = any((seats >> (k % players)) & 1 and f & flt["flag_mask"] for k, f in enumerate(flags))
    return bool(flt["score_min"] <= score <= flt["score_max"] and lives <= flt["max_lives"]
                and flt["moves_min"] <= len(flags) <= flt["moves_max"] and (not flt["end_mask"] or (flt["end_mask"] >> end) & 1)
                and (not flt["flag_mask"] or hit))


def end_reason(rules, record, finished):
    """from an export_state record of the final position"""
    if not finished:
        return END_UNFINISHED
    if record[56] < 1:
        return END_LIVES
    if sum(record[50:55]) >= rules["colors"] * rules["ranks"]:
        return END_PERFECT
    return END_DECK if record[59] <= 0 else END_MAX_LEN


# ---- games of the CPU oracle --------------------------------------------------------------------------------------------------------
POLICY_SEED = 977


@functools.lru_cache(maxsize=None)
def oracle_game(name, seed, policy, shuffle_color=False, policy_seed=POLICY_SEED):
    """one game of the CPU oracle (no max_len) under `policy`: "random" (oracle.policy_random) or a rule-bot preset of
    tests/rulebot_ref.py on every seat.  -> dict(rules, states = the export_state record before every move and after the last,
    moves / greedy = the uids as played (through the actor's permutation), seats, deck = deck_history() at the end)"""
    from oracle import oracle as _oracle
    from tests.variant_oracle import variant_oracle
    rules = RULESETS[name]
    env = variant_oracle.VariantEnv(seed=seed, bomb=0, eps_list=(0.0,), max_len=-1, sad=False, shuffle_color=shuffle_color, **rules)
    env.reset()
    A = ref.num_actions(rules)
    states, moves, greedy, seats, counter = [env.export_state().copy()], [], [], [], 0
    while not env.terminated():
        rec = states[-1]
        p = int(rec[57])
        if policy == "random":
            a, g = _oracle.policy_random(env.legal, policy_seed, seed, counter)
            uid, guid = int(a[p]), int(g[p])
        else:
            _, uid, _ = ref.act_record(rec, rules, ref.PRESETS[policy], policy_seed, seed, counter)
            guid = uid
        step = np.full((rules["players"],), A - 1, np.int64)
        step[p] = uid
        env.step(step, step)
        counter += 1
        moves.append(uid)
        greedy.append(guid)
        seats.append(p)
        env.terminated()   # the oracle latches the last score when it is asked, the device when the game ends
        states.append(env.export_state().copy())
    return dict(rules=rules, states=states, moves=moves, greedy=greedy, seats=seats, deck=list(env.deck_history()))
