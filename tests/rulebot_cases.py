"""Shared by the rule-bot tests: games of the CPU oracle in which the reference bot itself moves (with an occasional random move, so
that odd positions occur), as records with the reference's answer next to them."""
import functools

import numpy as np

from tests import rulebot_ref as ref
from tests.determinize_ref import policy_hash
from tests.search_fixtures import CONFIGS

EXPLORE_ONE_IN = 10   # a uniformly random legal move with probability 0.1
POLICY_SEED = 90210
# (config, shuffle_color, env seeds): chosen on the CPU so that every rule of every preset decides at least 5 times
GAMES = [("full", False, range(7000, 7006)), ("full", True, range(7100, 7103)), ("small", False, range(7200, 7212)),
         ("small", True, range(7300, 7306)), ("c3r4", False, range(7400, 7416)), ("c3r4", True, range(7500, 7508))]


def bot_game(config, seed, bot, shuffle_color=False, policy_seed=POLICY_SEED):
    """one oracle game under `bot` -> [(record, key, counter, seat, uid, deciding rule)]: the position before each move and what
    the reference bot answers there (the move made is that answer, or one time in ten a random legal one)"""
    from tests.variant_oracle import variant_oracle
    rules = CONFIGS[config]
    env = variant_oracle.VariantEnv(seed=seed, bomb=0, eps_list=(0.0,), max_len=80, sad=False, shuffle_color=shuffle_color, **rules)
    env.reset()
    A = ref.num_actions(rules)
    out, counter = [], 0
    while not env.terminated():
        rec = env.export_state().copy()
        p, uid, j = ref.act_record(rec, rules, bot, policy_seed, seed, counter)
        legal = [int(u) for u in np.nonzero(env.legal[p])[0]]
        from hanabi_sad_amd import position as pos
        assert legal == ref.legal_uids(pos.from_record(rec, rules), p), "the reference's legal moves are not the oracle's"
        assert uid in legal
        out.append((rec, seed, counter, p, uid, j))
        move = uid
        if policy_hash(policy_seed, seed, counter, 200) % EXPLORE_ONE_IN == 0:
            move = legal[policy_hash(policy_seed, seed, counter, 201) % len(legal)]
        a = np.full((rules["players"],), A - 1, np.int64)
        a[p] = move
        env.step(a, a)
        counter += 1
    return out


@functools.lru_cache(maxsize=None)
def games_of(preset):
    """{(config, shuffle_color): [entries of bot_game over that case's seeds]} for a preset of rulebot_ref.PRESETS"""
    bot = ref.PRESETS[preset]
    return {(config, sc): [e for seed in seeds for e in bot_game(config, seed, bot, sc)] for config, sc, seeds in GAMES}
