"""Rule-list Hanabi bots for the device env: an ordered list of at most 8 rules, the first that fires gives the move (include/hsad.h,
HSAD_RULE_* and hsad_env_policy_rule, is the specification).  `RuleBot` is the list as data; `BatchedHanabiEnv.policy_rule` /
`playout_rule` run it, `search.mc_action_values(playout=bot)` plays sampled worlds out with it and `eval.play_seatings` seats it next
to networks; `actor.PartnerSeats` seats it next to the learner in the training actor (`selfplay --partner NAME`).  The presets are this project's own restatements, named after the published rule-based agents they resemble (Walton-Rivers
et al. 2017); no fidelity to any published bot is claimed.  No torch, no device."""
import ctypes as C

PLAY_CERTAIN, PLAY_PROBABLE, PLAY_PROBABLE_ENDGAME = 1, 2, 3
HINT_PLAYABLE, HINT_USEFUL, HINT_DEAD, HINT_RANDOM = 4, 5, 6, 7
DISCARD_CERTAIN_DEAD, DISCARD_PROBABLE_DEAD, DISCARD_UNHINTED_OLDEST, DISCARD_OLDEST, DISCARD_RANDOM = 8, 9, 10, 11, 12
LEGAL_RANDOM = 13
MAX_RULES, MAX_BOTS = 8, 8
RULE_NAMES = {1: "PLAY_CERTAIN", 2: "PLAY_PROBABLE", 3: "PLAY_PROBABLE_ENDGAME", 4: "HINT_PLAYABLE", 5: "HINT_USEFUL", 6: "HINT_DEAD",
              7: "HINT_RANDOM", 8: "DISCARD_CERTAIN_DEAD", 9: "DISCARD_PROBABLE_DEAD", 10: "DISCARD_UNHINTED_OLDEST", 11: "DISCARD_OLDEST",
              12: "DISCARD_RANDOM", 13: "LEGAL_RANDOM"}
_WITH_K = (PLAY_PROBABLE, PLAY_PROBABLE_ENDGAME, DISCARD_PROBABLE_DEAD)


class Rule(C.Structure):
    """hsad_rule"""
    _fields_ = [("code", C.c_int32), ("k", C.c_int32)]


class RuleBot:
    """rules: a list of codes or (code, k) pairs, k in percent for the PROBABLE rules.  The list is kept as given: what the library
    refuses (an unknown code, k out of range, no rule or more than 8) is refused there, with its message."""

    def __init__(self, rules, name="rulebot"):
        self.rules = [(int(r), 0) if not isinstance(r, (tuple, list)) else (int(r[0]), int(r[1])) for r in rules]
        self.name = str(name)

    def __repr__(self):
        return "RuleBot(%s: %s)" % (self.name, ", ".join(
            RULE_NAMES.get(c, "?%d" % c) + ("(%d)" % k if c in _WITH_K else "") for c, k in self.rules))


PRESETS = {
    "cautious": RuleBot([PLAY_CERTAIN, HINT_PLAYABLE, DISCARD_CERTAIN_DEAD, DISCARD_UNHINTED_OLDEST, DISCARD_OLDEST, HINT_RANDOM], "cautious"),
    # exactly 8 rules, so no DISCARD_OLDEST at the end: when nothing fires the lowest legal bit is taken
    "piers": RuleBot([(PLAY_PROBABLE_ENDGAME, 0), PLAY_CERTAIN, (PLAY_PROBABLE, 60), HINT_PLAYABLE, HINT_DEAD, DISCARD_CERTAIN_DEAD,
                      DISCARD_UNHINTED_OLDEST, HINT_RANDOM], "piers"),
    "flawed": RuleBot([PLAY_CERTAIN, (PLAY_PROBABLE, 25), HINT_RANDOM, DISCARD_UNHINTED_OLDEST, DISCARD_RANDOM], "flawed"),
    "random": RuleBot([LEGAL_RANDOM], "random"),
}


def pack(bots):
    """[RuleBot] -> (hsad_rule array [len(bots) * 8], int32 array [len(bots)], n_bot): the host arguments of hsad_env_policy_rule.
    A list longer than 8 is cut in the array and keeps its length in n_rules, so the library refuses it."""
    bots = list(bots)
    rules = (Rule * (max(len(bots), 1) * MAX_RULES))()
    n = (C.c_int32 * max(len(bots), 1))()
    for b, bot in enumerate(bots):
        n[b] = len(bot.rules)
        for j, (code, k) in enumerate(bot.rules[:MAX_RULES]):
            rules[b * MAX_RULES + j].code, rules[b * MAX_RULES + j].k = code, k
    return rules, n, len(bots)
