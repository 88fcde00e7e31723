"""TEST INFRASTRUCTURE ONLY: ctypes wrapper around tests/variant_oracle/libvariant_oracle.so, the CPU restatement of the
game with its rules (colors, ranks, max_information_tokens, max_life_tokens) passed at creation.  Same C exports and
state dump as oracle/liboracle_hanabi.so, so the oracle's Python classes drive it with another library and create call."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle as _oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.path.join(_HERE, "libvariant_oracle.so")
_LIB = None


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-parameter", "-shared",
                           "-o", _PATH, os.path.join(_HERE, "variant_oracle.cc")])
    return _PATH


def lib():
    """the loaded restatement, (re)built first when the library is missing or older than variant_oracle.cc"""
    global _LIB
    if _LIB is not None:
        return _LIB
    src = os.path.join(_HERE, "variant_oracle.cc")
    if not os.path.exists(_PATH) or os.path.getmtime(src) > os.path.getmtime(_PATH):   # missing or older than its source
        build()
    L = C.CDLL(_PATH)
    ip, fp, ip64 = C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)
    L.orc_env_create_rules.restype = C.c_void_p
    L.orc_env_create_rules.argtypes = [ip, ip, ip, ip, fp, ip, ip, ip, ip, ip, ip, ip, ip, ip, ip]
    L.orc_env_destroy.argtypes = [C.c_void_p]
    for f in ("feature_size", "num_action", "hand_feature_size", "max_deck_size", "terminated", "cur_player",
              "last_score", "score", "life", "info", "num_step"):
        fn = getattr(L, "orc_env_" + f)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p]
    L.orc_env_fireworks.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.orc_env_move_is_legal.restype = C.c_int
    L.orc_env_move_is_legal.argtypes = [C.c_void_p, C.c_int]
    L.orc_env_rng_draws.restype = C.c_uint64
    L.orc_env_rng_draws.argtypes = [C.c_void_p]
    L.orc_env_deck_history.restype = C.c_int
    L.orc_env_deck_history.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int]
    L.orc_env_reset.argtypes = [C.c_void_p, fp, fp, fp, fp]
    L.orc_env_step.restype = C.c_int
    L.orc_env_step.argtypes = [C.c_void_p, ip64, ip64, fp, fp, fp, fp, fp, C.POINTER(C.c_uint8)]
    L.orc_env_state_words.restype = C.c_int
    L.orc_env_state_words.argtypes = [C.c_int, C.c_int]
    L.orc_env_export_state.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.orc_vec_rollout.restype = C.c_int64
    L.orc_vec_rollout.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_uint64, ip64, ip64, fp, fp, fp, fp,
                                  fp, C.POINTER(C.c_uint8), ip64, ip64, ip64, ip64]
    _LIB = L
    return L


class VariantEnv(_oracle.OracleEnv):
    """One game of the given rules; the oracle's OracleEnv interface."""

    def __init__(self, players=2, hand_size=5, seed=1, bomb=0, eps_list=(0.0,), max_len=80, sad=False,
                 shuffle_obs=False, shuffle_color=False, knowledge_mode=0, colors=5, ranks=5, max_information_tokens=8,
                 max_life_tokens=3):
        self.L = lib()
        eps = np.asarray(eps_list, dtype=np.float32)
        self.h = self.L.orc_env_create_rules(players, hand_size, seed, bomb, _oracle._fp(eps), len(eps), max_len,
                                             int(sad), int(shuffle_obs), int(shuffle_color), knowledge_mode, colors,
                                             ranks, max_information_tokens, max_life_tokens)
        if not self.h:
            raise ValueError("orc_env_create_rules rejected the configuration")
        self.P, self.H = players, hand_size
        self.C, self.R, self.max_info, self.max_life = colors, ranks, max_information_tokens, max_life_tokens
        self.F = self.L.orc_env_feature_size(self.h)
        self.A = self.L.orc_env_num_action(self.h)
        self.deck = self.L.orc_env_max_deck_size(self.h)
        self.priv_s = np.zeros((players, self.F), np.float32)
        self.legal = np.zeros((players, self.A), np.float32)
        self.own_hand = np.zeros((players, hand_size * 3), np.float32)
        self.eps = np.zeros((players,), np.float32)


class VariantVecEnv(_oracle.OracleVecEnv):
    """E games of the given rules stepped by the C loop with the random-legal policy (the oracle's OracleVecEnv)."""

    def __init__(self, n_env, seed, game_id0=0, **kw):
        self.envs = [VariantEnv(seed=seed + game_id0 + i, **kw) for i in range(n_env)]
        self.L = lib()
        e0 = self.envs[0]
        self.E, self.P, self.F, self.A, self.H = n_env, e0.P, e0.F, e0.A, e0.H
        self.handles = (C.c_void_p * n_env)(*[e.h for e in self.envs])
        self.game_ids = np.arange(game_id0, game_id0 + n_env, dtype=np.int64)
        self.counters = np.zeros((n_env,), np.int64)
        self.priv_s = np.zeros((n_env, self.P, self.F), np.float32)
        self.legal = np.zeros((n_env, self.P, self.A), np.float32)
        self.own_hand = np.zeros((n_env, self.P, self.H * 3), np.float32)
        self.eps = np.zeros((n_env, self.P), np.float32)
        self.reward = np.zeros((n_env,), np.float32)
        self.terminal = np.zeros((n_env,), np.uint8)
        self.a = np.zeros((n_env, self.P), np.int64)
        self.g = np.zeros((n_env, self.P), np.int64)
        self.score_sum = np.zeros((1,), np.int64)
        self.episodes = np.zeros((1,), np.int64)
