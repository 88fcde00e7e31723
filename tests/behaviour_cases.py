"""Shared by the behaviour tests: games of the CPU oracle in which the reference bots of tests/rulebot_ref.py (piers, flawed, random)
play against each other, as (record before the move, uid played) with the reference classifier's increments next to them."""
import functools

import numpy as np

from tests import behaviour_ref as bref
from tests import rulebot_ref as ref
from tests.search_fixtures import CONFIGS

BOTS = ("piers", "flawed", "random")
POLICY_SEED = 4711
# (config, shuffle_color, env seeds): chosen on the CPU so that every counter occurs in the reference's own sums, and both hint
# kinds under shuffle_color (test_behaviour_cpu.test_games_reach_every_counter asserts it)
GAMES = [("full", False, range(7600, 7606)), ("full", True, range(7610, 7616)), ("c3r4", False, range(7620, 7626)),
         ("c3r4", True, range(7630, 7636)), ("small", False, range(7640, 7652)), ("small", True, range(7660, 7672))]


def seat_bots(seed, players):
    """the preset on each seat of game `seed`: the three bots rotate from game to game, so that every one meets every other"""
    return [BOTS[(seed + p) % len(BOTS)] for p in range(players)]


def mixed_game(config, seed, shuffle_color=False, policy_seed=POLICY_SEED):
    """one oracle game with seat_bots(seed) on the seats -> [(record, uid, seat, increments)]: the position before each move, the
    move the bot on turn makes there, and what the reference classifier counts for it"""
    from tests.variant_oracle import variant_oracle
    rules = CONFIGS[config]
    env = variant_oracle.VariantEnv(seed=seed, bomb=0, eps_list=(0.0,), max_len=80, sad=False, shuffle_color=shuffle_color, **rules)
    env.reset()
    A = ref.num_actions(rules)
    bots = seat_bots(seed, rules["players"])
    out, counter = [], 0
    while not env.terminated():
        rec = env.export_state().copy()
        p = int(rec[57])
        _, uid, _ = ref.act_record(rec, rules, ref.PRESETS[bots[p]], policy_seed, seed, counter)
        assert env.legal[p][uid]
        out.append((rec, uid, p, bref.classify_record(rec, rules, uid)[1]))
        a = np.full((rules["players"],), A - 1, np.int64)
        a[p] = uid
        env.step(a, a)
        counter += 1
    return out


@functools.lru_cache(maxsize=None)
def games():
    """{(config, shuffle_color): [entries of mixed_game over that case's seeds]}"""
    return {(config, sc): [e for seed in seeds for e in mixed_game(config, seed, sc)] for config, sc, seeds in GAMES}
