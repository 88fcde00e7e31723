"""Shared by the search tests: the game configurations, and the states the determinise tests run on, as recipes (config, seeds,
number of random-policy iterations).  The GPU tests make them with BatchedHanabiEnv.rollout_random, test_determinize_cpu.py makes the
same states with the CPU restatement of the env (tests/variant_oracle: bit-identical by the parity tests) and checks on them what
must hold before the GPU tests mean anything: that the sampler's restatement never gives up on these states with these seeds."""
import numpy as np

EPS = (0.1, 0.05)
CONFIGS = {
    "full": dict(players=2, hand_size=5, colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3),
    "small": dict(players=2, hand_size=2, colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1),
    "c3r4": dict(players=3, hand_size=4, colors=3, ranks=4, max_information_tokens=6, max_life_tokens=2),
}
FULL_DECK = {name: [(0 if (t // 5 >= c["colors"] or t % 5 >= c["ranks"]) else
                     (3 if t % 5 == 0 else (1 if t % 5 == c["ranks"] - 1 else 2))) for t in range(25)]
             for name, c in CONFIGS.items()}

# (id, config, sad, shuffle_color, knowledge_mode, G, games_per_workgroup, env seed, policy seed, iterations, sampler seed)
DET_CASES = [
    ("full-sad-sc-k0", "full", True, True, 0, 65, 64, 9100, 17, 14, 2024),
    ("full-k1", "full", False, False, 1, 33, 32, 9200, 19, 31, 77),
    ("small-sad-k1", "small", True, False, 1, 65, 64, 9300, 23, 9, 5),
    ("small-sc-k0", "small", False, True, 0, 33, 32, 9400, 29, 5, 11),
    ("c3r4-sad-sc-k0", "c3r4", True, True, 0, 33, 32, 9500, 31, 22, 4242),
    ("c3r4-k1", "c3r4", False, False, 1, 65, 64, 9600, 37, 12, 99),
]

# test_equal_keys_give_equal_worlds_in_different_slots: the first live game of DET_CASES[0], forked into 33 slots
PAIR_KEYS = np.arange(33, dtype=np.int64) // 2 - 3
PAIR_SEED = 31337

# the root of the search test: `small`, 3 games, after SEARCH_ROOT["iters"] random iterations
SEARCH_ROOT = dict(config="small", G=3, seed=9700, pseed=41, iters=3, worlds=8, search_seed=12345)


def env_kwargs(config, sad, shuffle_color, knowledge_mode):
    return dict(CONFIGS[config], sad=sad, shuffle_color=shuffle_color, knowledge_mode=knowledge_mode, bomb=0, max_len=80)


def viewer_of(g, P):
    """the player whose hand game g resamples; every ninth game is skipped"""
    return -1 if g % 9 == 4 else g % P


def key_of(g):
    return 1000003 * g + 5


def viewers_and_keys(G, P):
    return (np.asarray([viewer_of(g, P) for g in range(G)], np.int32), np.asarray([key_of(g) for g in range(G)], np.int64))
