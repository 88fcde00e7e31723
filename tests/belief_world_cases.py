"""Shared by tests/test_belief_world_cpu.py and tests/test_env_belief_worlds_gpu.py: the inputs of hsad_env_determinize_belief_worlds
the GPU tests use, as recipes.  The states are those of tests/test_env_belief_sample_gpu.py (CASES: 70 games, 2 and 3 players, hands
of 5, 4 and 2, every ninth viewer -1, some games finished); the CPU test builds the same states with tests/variant_oracle and checks on
them what must hold before the GPU comparison means anything: that the float64 reference alone calls at most 1 % of the live rows
`near` (a draw within the fp32 bound of a boundary, where the device may pick the neighbour)."""
import numpy as np
import torch

from tests import search_fixtures as SF

G = 70
# (id, config, sad, shuffle_color, env seed, policy seed, iterations, sampler seed): test_env_belief_sample_gpu.CASES
CASES = [("full", "full", True, False, 9150, 17, 16, 2025), ("small", "small", True, False, 9350, 23, 7, 6),
         ("c3r4", "c3r4", False, True, 9550, 31, 20, 4243)]
IDS = [c[0] for c in CASES]
WORLDS = (1, 8)
MODES = ("direct", "rows7")      # logits row g for game g; 7 logits rows with row = g % 7
PAD = 3                          # ldz = 25 H + 3: the rows are not packed


def inputs(case, H, mode, W):
    """-> dict(logits float32 [n_rows, 25 H + PAD] (CPU), row int32 [G] | None, group int64 [G], world int32 [G], seed)"""
    seed = case[7]
    n_rows = G if mode == "direct" else 7
    gen = torch.Generator().manual_seed(seed * 10 + W + (100 if mode == "rows7" else 0))
    logits = (torch.randn(n_rows, 25 * H + PAD, generator=gen) * 3.0).contiguous()
    g = np.arange(G)
    _, key = SF.viewers_and_keys(G, 2)
    return dict(logits=logits, row=None if mode == "direct" else (g % 7).astype(np.int32), group=key.astype(np.int64),
                world=((g * 3 + 1) % W).astype(np.int32), seed=seed)


def row_of(inp, g):
    return g if inp["row"] is None else int(inp["row"][g])
