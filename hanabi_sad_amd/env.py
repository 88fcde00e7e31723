"""Batched device Hanabi environment: host-side owner of the tensors that libhsad's env kernels
write.  One object = G games = what the reference builds as G `hanalearn.HanabiEnv` objects inside
`HanabiVecEnv`s (pyhanabi/create.py:24-54; rela/env.h:29-108)."""
import ctypes as C

import torch

from . import _lib


class HandBelief:
    """what BatchedHanabiEnv.hand_belief returns, on the env's device: total int64 [G] = N, the number of assignments of physical
    unseen cards to the hand's slots that the card knowledge allows (0 for a skipped game); counts int64 [G, H, 25] = of those, the
    ones with card type colour * 5 + rank in the slot; trinary int64 [G, H, 3] = counts summed into [playable, rank below the
    firework, rank above it]."""

    def __init__(self, total, counts, trinary):
        self.total, self.counts, self.trinary = total, counts, trinary

    def _over_total(self, x):
        n = self.total.view(-1, 1, 1)
        p = x.to(torch.float64) / torch.where(n > 0, n, torch.ones_like(n)).to(torch.float64)
        return torch.where(n > 0, p, torch.zeros_like(p))

    def probs(self):
        """float64 [G, H, 25]: P(slot holds the type); zeros where total == 0"""
        return self._over_total(self.counts)

    def trinary_probs(self):
        """float64 [G, H, 3]; zeros where total == 0"""
        return self._over_total(self.trinary)


class BatchedHanabiEnv:
    def __init__(self, num_games, players=2, hand_size=5, seed=1, bomb=0, eps_list=(0.0,), max_len=80, sad=False,
                 shuffle_obs=False, shuffle_color=False, knowledge_mode=0, device="cuda:0", track_deck_history=True,
                 deal_mode=0, games_per_workgroup=0, threads_per_workgroup=0, colors=5, ranks=5, max_information_tokens=8,
                 max_life_tokens=3):
        """colors / ranks / max_information_tokens / max_life_tokens: the game's rules (HLE's keys; the full game is
        5 / 5 / 8 / 3, each may be lowered to 1).  Every size (F, A, hand_feature_size) follows the rules."""
        self.lib = _lib.load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HsadError("BatchedHanabiEnv needs a ROCm device (got %s); there is no CPU path" % device)
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        eps = (C.c_float * len(eps_list))(*[float(e) for e in eps_list])
        cfg = _lib.EnvConfig(num_games, players, hand_size, int(bomb), int(seed), int(max_len), int(bool(sad)),
                             int(bool(shuffle_obs)), int(bool(shuffle_color)), int(knowledge_mode), len(eps_list),
                             dev_index, int(bool(track_deck_history)), int(deal_mode), int(games_per_workgroup), eps)
        rules = _lib.EnvRules(int(colors), int(ranks), int(max_information_tokens), int(max_life_tokens))
        self.h = C.c_void_p()
        _lib.check(self.lib.hsad_env_create_rules(C.byref(cfg), C.byref(rules), C.byref(self.h)))
        L = self.lib
        # what a second env needs to be a fork target of this one (fork_from; search.py builds its search env from it)
        self.config = dict(players=players, hand_size=hand_size, bomb=int(bomb), max_len=int(max_len), sad=bool(sad),
                           shuffle_color=bool(shuffle_color), knowledge_mode=int(knowledge_mode), colors=int(colors), ranks=int(ranks),
                           max_information_tokens=int(max_information_tokens), max_life_tokens=int(max_life_tokens))
        # everything load() needs to build this env again (save / load)
        self._full_config = dict(self.config, num_games=int(num_games), seed=int(seed), eps_list=[float(e) for e in eps_list],
                                 track_deck_history=bool(track_deck_history), deal_mode=int(deal_mode),
                                 games_per_workgroup=int(games_per_workgroup))
        self.G, self.P, self.H = num_games, players, hand_size
        self.colors, self.ranks = int(colors), int(ranks)
        self.max_information_tokens, self.max_life_tokens = int(max_information_tokens), int(max_life_tokens)
        self.F = L.hsad_env_feature_size(self.h)
        self.A = L.hsad_env_num_action(self.h)
        self.sad = bool(sad)
        self.knowledge_mode = int(knowledge_mode)
        self.games_per_workgroup = L.hsad_env_games_per_workgroup(self.h)   # kernel shape in use (32 | 64)
        if threads_per_workgroup:
            _lib.check(L.hsad_env_set_threads_per_workgroup(self.h, int(threads_per_workgroup)))
        self.threads_per_workgroup = L.hsad_env_threads_per_workgroup(self.h)   # 128 | 256
        d = self.device
        self.priv_s = torch.zeros(self.G, self.P, self.F, dtype=torch.float32, device=d)
        self.legal_move = torch.zeros(self.G, self.P, self.A, dtype=torch.float32, device=d)
        self.own_hand = torch.zeros(self.G, self.P, 3 * self.H, dtype=torch.float32, device=d)
        self.eps = torch.zeros(self.G, self.P, dtype=torch.float32, device=d)
        self.reward = torch.zeros(self.G, dtype=torch.float32, device=d)
        self.terminal = torch.zeros(self.G, dtype=torch.uint8, device=d)
        self.a = torch.zeros(self.G, self.P, dtype=torch.int64, device=d)
        self.greedy_a = torch.zeros(self.G, self.P, dtype=torch.int64, device=d)
        _lib.check(L.hsad_env_bind_outputs(self.h, self.priv_s.data_ptr(), self.legal_move.data_ptr(),
                                           self.own_hand.data_ptr(), self.eps.data_ptr(), self.reward.data_ptr(),
                                           self.terminal.data_ptr()))

    def enable_packed(self, bf16_row_len=0, keep_float32=True):
        """outputs for device consumers (hsad_env_bind_packed): priv_bits int64 [G,P,ceil(F/64)], legal_bits / own_bits int64 [G,P]
        (bit j = column j of the float32 tensor) and, with bf16_row_len, priv_s_bf16 [G,P,row_len] zero-padded.
        keep_float32=False: the float32 priv_s tensor is no longer written (self.priv_s becomes None)"""
        d, G, P = self.device, self.G, self.P
        self.priv_bits = torch.zeros(G, P, (self.F + 63) // 64, dtype=torch.int64, device=d)
        self.legal_bits = torch.zeros(G, P, dtype=torch.int64, device=d)
        self.own_bits = torch.zeros(G, P, dtype=torch.int64, device=d)
        self.priv_s_bf16 = torch.zeros(G, P, bf16_row_len, dtype=torch.bfloat16, device=d) if bf16_row_len else None
        _lib.check(self.lib.hsad_env_bind_packed(self.h, self.priv_bits.data_ptr(), self.legal_bits.data_ptr(), self.own_bits.data_ptr(),
                                                 self.priv_s_bf16.data_ptr() if bf16_row_len else None, int(bf16_row_len),
                                                 int(bool(keep_float32))))
        if not keep_float32:
            self.priv_s = None

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.hsad_env_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- reference-shaped accessors (cpp/hanabi_env.h:53-72) --
    def feature_size(self):
        return self.F

    def num_action(self):
        return self.A

    def hand_feature_size(self):
        return self.lib.hsad_env_hand_feature_size(self.h)

    def rules(self):
        """the game's rules as the library holds them: {colors, ranks, max_information_tokens, max_life_tokens}"""
        r = _lib.EnvRules()
        _lib.check(self.lib.hsad_env_get_rules(self.h, C.byref(r)))
        return {k: int(getattr(r, k)) for k, _ in _lib.EnvRules._fields_}

    def max_deck_size(self):
        return self.lib.hsad_env_max_deck_size(self.h)

    def state_bytes(self):
        return int(self.lib.hsad_env_state_bytes(self.h))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def obs(self):
        """TensorDict view produced by VectorEnv::reset/step (rela/env.h:48-87)."""
        if self.priv_s is None:   # enable_packed(keep_float32=False): the observation only exists as bit words / bf16 rows
            return {"priv_s_bf16": self.priv_s_bf16, "priv_bits": self.priv_bits, "legal_move": self.legal_move, "eps": self.eps,
                    "own_hand": self.own_hand}
        return {"priv_s": self.priv_s, "legal_move": self.legal_move, "eps": self.eps, "own_hand": self.own_hand}

    def reset(self):
        _lib.check(self.lib.hsad_env_reset(self.h, self._stream()))
        return self.obs()

    def reseed(self, seed, period=0):
        """every game back to "not started", game g seeded seed + (g % period) (period <= 0: seed + g, as at construction);
        the next reset() starts all games.  Groups of `period` games then play the same deals."""
        _lib.check(self.lib.hsad_env_reseed(self.h, int(seed), int(period), self._stream()))

    def step(self, a, greedy_a=None):
        assert a.dtype == torch.int64 and a.is_contiguous() and a.device == self.legal_move.device
        g = greedy_a if greedy_a is not None else (a if self.sad else None)
        _lib.check(self.lib.hsad_env_step(self.h, a.data_ptr(), g.data_ptr() if g is not None else None,
                                          self._stream()))
        return self.obs(), self.reward, self.terminal

    def policy_random(self, policy_seed):
        _lib.check(self.lib.hsad_env_policy_random(self.h, policy_seed, self.a.data_ptr(), self.greedy_a.data_ptr(),
                                                   self._stream()))
        return self.a, self.greedy_a

    def rollout_random(self, n_iter, policy_seed):
        _lib.check(self.lib.hsad_env_rollout_random(self.h, n_iter, policy_seed, self.a.data_ptr(),
                                                    self.greedy_a.data_ptr(), self._stream()))

    def set_partitions(self, n_part):
        """Number of independent game ranges rollout_random overlaps on private HIP streams."""
        _lib.check(self.lib.hsad_env_set_partitions(self.h, int(n_part)))

    def set_rollout_stagger(self, microseconds):
        """phase lock between the partition chains (see include/hsad.h); timing only"""
        _lib.check(self.lib.hsad_env_set_rollout_stagger(self.h, int(microseconds)))

    def set_rollout_chunk(self, iterations_per_launch):
        """persistent rollout: one launch runs this many iterations of every game (0 = one launch per iteration)"""
        _lib.check(self.lib.hsad_env_set_rollout_chunk(self.h, int(iterations_per_launch)))

    def set_rollout_pace(self, on):
        """persistent rollout: workgroups ahead of the launch's mean progress delay their observation stream (default: on,
        except where the compacted delta stream runs; timing only, see include/hsad.h)"""
        _lib.check(self.lib.hsad_env_set_rollout_pace(self.h, int(bool(on))))

    def rollout_pace_cap_us(self):
        return int(self.lib.hsad_env_rollout_pace_cap_us(self.h))

    def set_rollout_delta(self, on):
        """persistent rollout: the streams of a launch after its first store only the observation lines that changed (default on;
        results are identical, see include/hsad.h)"""
        _lib.check(self.lib.hsad_env_set_rollout_delta(self.h, int(bool(on))))

    def rollout_delta_active(self):
        """whether persistent launches use the delta stream as the env stands"""
        return bool(self.lib.hsad_env_rollout_delta_active(self.h))

    def set_rollout_chain(self, mode):
        """persistent rollout: launches 2, 3, ... of one rollout_random call take the rows their predecessor streamed last from a
        buffer of the env, so their first stream stores only what changed (1, the default; 0: every launch on its own; results are
        identical, see include/hsad.h)"""
        _lib.check(self.lib.hsad_env_set_rollout_chain(self.h, int(mode)))

    def rollout_chain_active(self):
        """the chain mode persistent launches use as the env stands: 0 wherever the delta stream is not active"""
        return int(self.lib.hsad_env_rollout_chain_active(self.h))

    def set_rollout_compact(self, on):
        """delta stream: list the changed lines first and store from the list (default on; results are identical, see
        include/hsad.h)"""
        _lib.check(self.lib.hsad_env_set_rollout_compact(self.h, int(bool(on))))

    def rollout_compact_active(self):
        """whether persistent launches use the compacted form of the delta stream as the env stands"""
        return bool(self.lib.hsad_env_rollout_compact_active(self.h))

    def set_rollout_unit(self, nbytes):
        """compacted delta stream: decide "changed" by whole lines (128) or by half lines (64, the default); results are
        identical, see include/hsad.h"""
        _lib.check(self.lib.hsad_env_set_rollout_unit(self.h, int(nbytes)))

    def rollout_unit(self):
        """the unit (bytes) persistent launches decide "changed" by as the env stands: 128 wherever the compacted form is not
        active"""
        return int(self.lib.hsad_env_rollout_unit(self.h))

    def set_rollout_prio(self, mode):
        """pipelined persistent rollout: wave priority per iteration (bit 0: co-tenants of a SIMD alternate, bit 1: the stream
        wave above the logic wave; timing only, results are identical, see include/hsad.h)"""
        _lib.check(self.lib.hsad_env_set_rollout_prio(self.h, int(mode)))

    def rollout_prio(self):
        """the priority mode persistent launches use as the env stands: 0 wherever the pipelined kernel does not run"""
        return int(self.lib.hsad_env_rollout_prio(self.h))

    def debug_pace_bias(self, bias):
        """test seam: offset of the counter base the paced kernels are told"""
        _lib.check(self.lib.hsad_env_debug_pace_bias(self.h, int(bias)))

    def debug_pace_word(self):
        """(progress word on the device, value the host expects); synchronises"""
        w, b = C.c_int64(0), C.c_int64(0)
        _lib.check(self.lib.hsad_env_debug_pace_word(self.h, C.byref(w), C.byref(b)))
        return int(w.value), int(b.value)

    def last_rollout_ms(self):
        """average launch duration (ms) on each partition stream of the last partitioned rollout_random"""
        import ctypes as C
        ms, n = (C.c_float * 16)(), C.c_int(0)
        _lib.check(self.lib.hsad_env_last_rollout_ms(self.h, ms, C.byref(n)))
        return [float(ms[k]) for k in range(n.value)]

    # -- the env as a simulator for search (include/hsad.h: hsad_env_fork / _determinize / _playout_random) --
    def _i32(self, t, n):
        t = torch.as_tensor(t, device=self.device).to(torch.int32).contiguous()
        assert t.shape == (n,), "expected %d values, got %s" % (n, tuple(t.shape))
        return t

    def fork_from(self, src, src_index, seeds=None):
        """game j of this env becomes a copy of src's game src_index[j] (int32 [G]; -1 = leave game j alone) and its rows are
        rewritten from the copied state.  seeds=None copies the generator too; seeds (int32 [G]) reseeds game j with seeds[j]."""
        idx = self._i32(src_index, self.G)
        sd = self._i32(seeds, self.G) if seeds is not None else None
        _lib.check(self.lib.hsad_env_fork(self.h, src.h, idx.data_ptr(), sd.data_ptr() if sd is not None else None, self._stream()))

    def determinize(self, viewer, key, seed):
        """resamples the hand of player viewer[g] (int32 [G]; -1 = skip) from the hands its card knowledge allows; key (int64 [G])
        and seed select the world.  Returns tries (int32 [G]: tries used, 0 skipped, -1 gave up and kept the hand)."""
        v = self._i32(viewer, self.G)
        k = torch.as_tensor(key, device=self.device).to(torch.int64).contiguous()
        assert k.shape == (self.G,)
        tries = torch.zeros(self.G, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.hsad_env_determinize(self.h, v.data_ptr(), k.data_ptr(), int(seed) & (2 ** 64 - 1), tries.data_ptr(),
                                                 self._stream()))
        return tries

    def hand_belief(self, viewer):
        """the exact belief over the hidden hand of player viewer[g] (int32 [G]; -1 = skip): how many assignments of unseen
        physical cards its card knowledge allows, and their per-slot marginals -> HandBelief.  Reads the state only.
        See hsad_env_hand_belief."""
        v = self._i32(viewer, self.G)
        total = torch.zeros(self.G, dtype=torch.int64, device=self.device)
        counts = torch.zeros(self.G, self.H, 25, dtype=torch.int64, device=self.device)
        tri = torch.zeros(self.G, self.H, 3, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.hsad_env_hand_belief(self.h, v.data_ptr(), total.data_ptr(), counts.data_ptr(), tri.data_ptr(), self._stream()))
        return HandBelief(total, counts, tri)

    def determinize_exact(self, viewer, key, seed, stratum=None, n_strata=1, rank=None):
        """determinize without rejection: the hand of player viewer[g] becomes hand number r of the N its card knowledge allows
        (counted with the weight of the physical cards).  rank (int64 [G]) gives r itself; otherwise r is drawn from stratum
        stratum[g] (int32 [G], None = 0) of n_strata equal parts of [0, N) with the hash of (seed, key[g]): the worlds
        stratum = 0 .. n_strata - 1 of a game cover its belief evenly, n_strata = 1 is a plain exact draw.  Returns rank_out
        (int64 [G]: the rank used, -1 for a game left alone -- skipped, rank or stratum out of range).  See hsad_env_determinize_exact."""
        v = self._i32(viewer, self.G)
        k = torch.as_tensor(key, device=self.device).to(torch.int64).contiguous()
        assert k.shape == (self.G,)
        st = self._i32(stratum, self.G) if stratum is not None else None
        rk = None
        if rank is not None:
            rk = torch.as_tensor(rank, device=self.device).to(torch.int64).contiguous()
            assert rk.shape == (self.G,)
        out = torch.zeros(self.G, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.hsad_env_determinize_exact(self.h, v.data_ptr(), k.data_ptr(), int(seed) & (2 ** 64 - 1),
                                                       st.data_ptr() if st is not None else None, int(n_strata),
                                                       rk.data_ptr() if rk is not None else None, out.data_ptr(), self._stream()))
        return out

    def hand_knowledge(self):
        """what every seat knows about its own hand, as the learned belief (belief.py) is trained on it -> (pool int64 [G, P],
        compat int32 [G, P, H], cards int32 [G, P, H]): the pool and per-slot masks hand_belief counts with for that viewer, and the
        seat's true cards (-1 = empty slot); zeros and -1 for a game that is not live.  Reads the state only.
        See hsad_env_hand_knowledge."""
        pool = torch.zeros(self.G, self.P, dtype=torch.int64, device=self.device)
        compat = torch.zeros(self.G, self.P, self.H, dtype=torch.int32, device=self.device)
        cards = torch.zeros(self.G, self.P, self.H, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.hsad_env_hand_knowledge(self.h, pool.data_ptr(), compat.data_ptr(), cards.data_ptr(), self._stream()))
        return pool, compat, cards

    def determinize_belief(self, viewer, logits, key, seed):
        """determinize_exact's counterpart for the learned belief: the hand of player viewer[g] (int32 [G]; -1 = skip) is sampled
        slot by slot from the belief that logits (float32 [G, >= 25 H], row g: 25 logits per slot) tilt the exact belief into; key
        (int64 [G]) and seed select the world.  All-zero logits sample the exact belief.  Returns (status int32 [G]: 1 sampled,
        0 left alone; logp float32 [G]: the sampled hand's log-probability).  See hsad_env_determinize_belief."""
        v = self._i32(viewer, self.G)
        k = torch.as_tensor(key, device=self.device).to(torch.int64).contiguous()
        assert k.shape == (self.G,)
        if not (torch.is_tensor(logits) and logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[0] == self.G
                and logits.shape[1] >= 25 * self.H and logits.stride(1) == 1 and logits.is_cuda):
            raise ValueError("logits must be float32 [%d, >= %d] on %s with unit column stride" % (self.G, 25 * self.H, self.device))
        status = torch.zeros(self.G, dtype=torch.int32, device=self.device)
        logp = torch.zeros(self.G, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hsad_env_determinize_belief(self.h, v.data_ptr(), logits.data_ptr(), int(logits.stride(0)), k.data_ptr(),
                                                        int(seed) & (2 ** 64 - 1), logp.data_ptr(), status.data_ptr(), self._stream()))
        return status, logp

    def determinize_belief_worlds(self, viewer, logits, row, group, world, n_worlds, seed):
        """determinize_belief for a search env whose slots are forks of a few root games: game g reads logits row row[g] (int32
        [G], None = row g; logits float32 [n_rows, >= 25 H]) and is world world[g] (int32 [G]) of n_worlds of the root game with
        key group[g] (int64 [G]): the worlds of a group fall into every one of the n_worlds equal parts of each slot's conditional
        exactly once.  A hand depends on (seed, group, world), the logits row and the game's state, never on the slot.  A game is
        left alone when it is skipped, when row[g] or world[g] is out of range or when its row holds a non-finite logit.  Returns
        (status int32 [G]: 1 sampled, 0 left alone; logp, logp0 float32 [G]: the sampled hand's log-probability under the belief
        and under the exact belief).  See hsad_env_determinize_belief_worlds."""
        v = self._i32(viewer, self.G)
        r = self._i32(row, self.G) if row is not None else None
        w = self._i32(world, self.G)
        k = torch.as_tensor(group, device=self.device).to(torch.int64).contiguous()
        assert k.shape == (self.G,)
        if not (torch.is_tensor(logits) and logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[0] >= 1
                and (row is not None or logits.shape[0] >= self.G) and logits.shape[1] >= 25 * self.H and logits.stride(1) == 1
                and logits.is_cuda):
            raise ValueError("logits must be float32 [%s, >= %d] on %s with unit column stride"
                             % ("n_rows >= 1" if row is not None else ">= %d" % self.G, 25 * self.H, self.device))
        if not 1 <= int(n_worlds) <= 1 << 20:
            raise ValueError("n_worlds must be in [1, 2^20]; got %r" % (n_worlds,))
        status = torch.zeros(self.G, dtype=torch.int32, device=self.device)
        logp = torch.zeros(self.G, dtype=torch.float32, device=self.device)
        logp0 = torch.zeros(self.G, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hsad_env_determinize_belief_worlds(self.h, v.data_ptr(), logits.data_ptr(), int(logits.stride(0)),
                                                               int(logits.shape[0]), r.data_ptr() if r is not None else None, k.data_ptr(),
                                                               w.data_ptr(), int(n_worlds), int(seed) & (2 ** 64 - 1), logp.data_ptr(),
                                                               logp0.data_ptr(), status.data_ptr(), self._stream()))
        return status, logp, logp0

    def playout_random(self, max_iter, policy_seed, key=None):
        """random-legal policy -> step until every live game has ended (at most max_iter iterations), finished games left alone.
        The observation rows are NOT rewritten (stale until the next fork_from / reset / step); terminal and query() are current.
        key (int64 [G]) replaces the game index in the policy's hash."""
        k = None
        if key is not None:
            k = torch.as_tensor(key, device=self.device).to(torch.int64).contiguous()
            assert k.shape == (self.G,)
        _lib.check(self.lib.hsad_env_playout_random_keyed(self.h, int(max_iter), int(policy_seed) & (2 ** 64 - 1),
                                                          k.data_ptr() if k is not None else None, self.a.data_ptr(),
                                                          self.greedy_a.data_ptr(), self._stream()))
        return self.a, self.greedy_a

    # -- rule-list bots (include/hsad.h: HSAD_RULE_*, hsad_env_policy_rule / _playout_rule; hanabi_sad_amd/rulebot.py) --
    def _key64(self, key):
        if key is None:
            return None
        k = torch.as_tensor(key, device=self.device).to(torch.int64).contiguous()
        assert k.shape == (self.G,)
        return k

    def policy_rule(self, bots, seat_bot=None, seed=0, key=None):
        """one policy call of rule bots on the current state: row (g, p) of a / greedy_a gets the move of bots[seat_bot[g, p]] (the
        noop when seat p is not on turn).  bots: a RuleBot or a list of at most 8; seat_bot: int32 [G, P], or [P] for the same
        seating in every game, None = bot 0 everywhere; -1 leaves the row untouched, and a game with no bot at all keeps its policy
        counter.  key (int64 [G]) replaces the game index in the hash of the *_RANDOM rules.  Returns (a, greedy_a)."""
        from . import rulebot
        bots = [bots] if isinstance(bots, rulebot.RuleBot) else list(bots)
        rules, n_rules, n_bot = rulebot.pack(bots)
        if seat_bot is None:
            sb = torch.zeros(self.G, self.P, dtype=torch.int32, device=self.device)
        else:
            sb = torch.as_tensor(seat_bot, device=self.device).to(torch.int32)
            if sb.dim() == 1:
                sb = sb.view(1, self.P).expand(self.G, self.P)
            sb = sb.contiguous()
            assert sb.shape == (self.G, self.P), "seat_bot must be [G, P] or [P], got %s" % (tuple(sb.shape),)
        k = self._key64(key)
        _lib.check(self.lib.hsad_env_policy_rule(self.h, rules, n_rules, n_bot, sb.data_ptr(), int(seed) & (2 ** 64 - 1),
                                                 k.data_ptr() if k is not None else None, self.a.data_ptr(), self.greedy_a.data_ptr(),
                                                 self._stream()))
        return self.a, self.greedy_a

    def playout_rule(self, max_iter, bots, seats=None, seed=0, key=None):
        """playout_random with rule bots in place of the random pick: bot -> step until every live game has ended (at most max_iter
        iterations) in one launch, finished games left alone, observation rows NOT rewritten.  bots: a RuleBot or a list of at most
        8; seats: per seat the index of its bot (None = bot 0 on every seat).  A live game's trajectory is that of policy_rule +
        step.  Returns (a, greedy_a)."""
        from . import rulebot
        bots = [bots] if isinstance(bots, rulebot.RuleBot) else list(bots)
        rules, n_rules, n_bot = rulebot.pack(bots)
        seats = [0] * self.P if seats is None else [int(s) for s in seats]
        assert len(seats) == self.P, "one bot index per seat"
        k = self._key64(key)
        _lib.check(self.lib.hsad_env_playout_rule(self.h, int(max_iter), rules, n_rules, n_bot, (C.c_int32 * self.P)(*seats),
                                                  int(seed) & (2 ** 64 - 1), k.data_ptr() if k is not None else None,
                                                  self.a.data_ptr(), self.greedy_a.data_ptr(), self._stream()))
        return self.a, self.greedy_a

    def rewind_scripted(self, script, count):
        """games with count[g] > 0 (int32 [G]) start again from a fresh deal whose cards are script[g] (uint8 [G, 52], or [G, 50]
        as deck_history() returns it): the hands from its first P * H entries, every later deal of step() from the script until
        count[g] cards are dealt, then from the generator.  eps, colour permutation and generator are kept; reset() / reseed()
        clear the script.  See hsad_env_rewind_scripted."""
        s = torch.as_tensor(script, device=self.device).to(torch.uint8)
        if s.dim() == 2 and s.shape[1] == 50:
            s = torch.nn.functional.pad(s, (0, 2))
        s = s.contiguous()
        assert s.shape == (self.G, 52), "expected a [%d, 52] script, got %s" % (self.G, tuple(s.shape))
        c = self._i32(count, self.G)
        _lib.check(self.lib.hsad_env_rewind_scripted(self.h, s.data_ptr(), c.data_ptr(), self._stream()))

    def playout_logged(self, records, src_index, stop=None):
        """game j becomes game record src_index[j] (int32 [G]; -1 = leave game j alone) played from its first deal up to move
        min(stop[j], n_moves) (int32 [G]; None: to the end) in one launch, and its rows are rewritten (SAD section all-zero, reward
        0).  records: uint8 [n, record_bytes] on the host (numpy or a CPU tensor; game_record.GameRecord.to_bytes rows).  The game
        is rewound as rewind_scripted rewinds it, the record's deck its script.  Returns status int32 [G]: the moves played, or
        HSAD_GR_STATUS_* (-1 left alone, -2 refused: bad deck or a game never started, -3 index out of range); a logged move that
        is illegal stops its game there (check_errors() reports code 8).  See hsad_env_playout_logged."""
        import numpy as np
        rec = np.ascontiguousarray(records.numpy() if isinstance(records, torch.Tensor) else records, dtype=np.uint8)
        rb = int(self.lib.hsad_game_record_bytes(self.h))
        assert rec.ndim == 2 and rec.shape[1] == rb, "expected uint8 [n, %d] records, got %s" % (rb, tuple(rec.shape))
        idx = self._i32(src_index, self.G)
        st = self._i32(stop, self.G) if stop is not None else None
        status = torch.zeros(self.G, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.hsad_env_playout_logged(self.h, rec.ctypes.data, int(rec.shape[0]), idx.data_ptr(),
                                                    st.data_ptr() if st is not None else None, status.data_ptr(), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()   # `rec` is host memory the copy reads: keep it alive until it is done
        return status

    def sad_section(self, out=None):
        """int64 [G, P]: the SAD greedy-action section of the current rows, one word per row (zeros with sad = 0); what a GameLog
        keeps of an observation.  See hsad_env_sad_section."""
        if out is None:
            out = torch.zeros(self.G, self.P, dtype=torch.int64, device=self.device)
        assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == self.G * self.P
        _lib.check(self.lib.hsad_env_sad_section(self.h, out.data_ptr(), self._stream()))
        return out

    def observe_sad(self, src_index, sad):
        """rewrites the rows of every game g with src_index[g] >= 0 from its state, the SAD section of seat p = sad[src_index[g], p]
        (int64 [G_src, P]): a replayed world is shown what was seen, not what its own cards would have shown.  No-op with sad = 0."""
        idx = self._i32(src_index, self.G)
        s = torch.as_tensor(sad, device=self.device).to(torch.int64).contiguous()
        assert s.dim() == 2 and s.shape[1] == self.P
        _lib.check(self.lib.hsad_env_observe_sad(self.h, idx.data_ptr(), int(s.shape[0]), s.data_ptr(), self._stream()))

    # -- positions in and out (include/hsad.h: hsad_env_import_state / _snapshot / _restore; hanabi_sad_amd/position.py) --
    def import_state(self, states, games=None, seeds=None, eps=None):
        """the games listed in `games` (list or tensor of indices; None: all G in order) become the positions `states` (int32, one
        canonical record per entry: export_state's layout, position.Position.to_record).  seeds (one int32 per entry) reseeds
        each game's generator, None keeps it; eps (float [entries, P]) sets its eps row, None keeps it.  Returns status int32
        [G]: -1 not listed, 0 imported, else the HSAD_POS_* flags of a refused record (position.explain; the game is untouched
        and check_errors() reports it).
        The cards of an imported position have no deal order: the game's deck-history row is cleared, but deck_history() still
        counts deck size minus cards left for it, so it returns that many cards of type 0 until the next reset deals afresh.
        Do not feed such a history to rewind_scripted (the deck does not hold those cards: error code 5)."""
        W = self.lib.hsad_env_state_words(self.h)
        st = torch.as_tensor(states, device=self.device).to(torch.int32)
        if st.dim() == 1:
            st = st.view(1, -1)
        idx = torch.arange(self.G, device=self.device) if games is None else torch.as_tensor(games, device=self.device).to(torch.int64).view(-1)
        n = idx.numel()
        assert st.shape == (n, W), "expected %d records of %d words, got %s" % (n, W, tuple(st.shape))
        if n and (int(idx.min()) < 0 or int(idx.max()) >= self.G or idx.unique().numel() != n):
            raise ValueError("import_state: games must be distinct indices in [0, %d)" % self.G)
        full = torch.zeros(self.G, W, dtype=torch.int32, device=self.device)
        full[idx] = st
        take = torch.zeros(self.G, dtype=torch.uint8, device=self.device)
        take[idx] = 1
        sd = ep = None
        if seeds is not None:
            sd = torch.zeros(self.G, dtype=torch.int32, device=self.device)
            sd[idx] = torch.as_tensor(seeds, device=self.device).to(torch.int32).view(n)
        if eps is not None:
            ep = torch.zeros(self.G, self.P, dtype=torch.float32, device=self.device)
            ep[idx] = torch.as_tensor(eps, device=self.device).to(torch.float32).view(n, self.P)
        status = torch.zeros(self.G, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.hsad_env_import_state(self.h, full.data_ptr(), take.data_ptr(), sd.data_ptr() if sd is not None else None,
                                                  ep.data_ptr() if ep is not None else None, status.data_ptr(), self._stream()))
        return status

    def snapshot_record_bytes(self):
        return int(self.lib.hsad_env_snapshot_record_bytes(self.h))

    def snapshot(self):
        """uint8 [G, record_bytes]: every game complete -- state, generator, policy counter, deck history, deal script, the SAD
        section of its rows.  Opaque and exact; restore() of it continues bit for bit."""
        out = torch.zeros(self.G, self.snapshot_record_bytes(), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.hsad_env_snapshot(self.h, out.data_ptr(), self._stream()))
        return out

    def restore(self, snap, src_index=None):
        """game j becomes record src_index[j] of snap (int32 [G]; None: record j, and snap must hold G records; -1 leaves game j
        alone) and its rows are rewritten as they were.  Returns status int32 [G]: 0 restored, -1 left alone, else the
        HSAD_POS_* flags of a refused record (game untouched; check_errors() reports it)."""
        assert snap.dtype == torch.uint8 and snap.dim() == 2, "expected a uint8 [G_src, record_bytes] snapshot"
        snap = snap.to(self.device).contiguous()
        idx = self._i32(src_index, self.G) if src_index is not None else None
        status = torch.zeros(self.G, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.hsad_env_restore(self.h, snap.data_ptr(), int(snap.shape[1]), int(snap.shape[0]),
                                             idx.data_ptr() if idx is not None else None, status.data_ptr(), self._stream()))
        return status

    SAVE_VERSION = 1

    @staticmethod
    def _record_bytes(players, track_deck_history, script):
        """hsad_env_snapshot_record_bytes, from the configuration alone (include/hsad.h gives the layout)"""
        return 4 * (10 + 6 * players + 1 + 624 + (13 if track_deck_history else 0) + (14 if script else 0) + 2 * players)

    def save(self, path):
        """one torch.save dict: format version, the env's full configuration, record_bytes, the snapshot"""
        snap = self.snapshot()
        cfg = dict(self._full_config)
        script = int(snap.shape[1]) != self._record_bytes(cfg["players"], cfg["track_deck_history"], False)
        # `layout`: what the records were made for, apart from the configuration they are saved with
        torch.save(dict(version=self.SAVE_VERSION, config=cfg, record_bytes=int(snap.shape[1]),
                        layout=dict(players=cfg["players"], hand_size=cfg["hand_size"], track_deck_history=cfg["track_deck_history"],
                                    script=bool(script)), snapshot=snap.cpu()), path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        """the env save() wrote, on `device`, its games where they were.  ValueError, before anything is launched on the games, for
        another format version, a record size that is not this configuration's or a snapshot of another length; HsadError if the
        device refuses a record.  The record size does not depend on the hand size, so the hand-size check rests on the file
        saying it twice (`config` and `layout`): a file in which both were changed together gets as far as the device, whose
        position check then refuses the records (HsadError)."""
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or d.get("version") != cls.SAVE_VERSION:
            raise ValueError("%s: not a saved env of format version %d" % (path, cls.SAVE_VERSION))
        cfg, snap, rb, lay = dict(d["config"]), d["snapshot"], int(d["record_bytes"]), dict(d["layout"])
        for k in ("players", "hand_size", "track_deck_history"):
            if lay[k] != cfg[k]:
                raise ValueError("%s: the records were made for %s = %s, the configuration says %s" % (path, k, lay[k], cfg[k]))
        want = cls._record_bytes(cfg["players"], cfg["track_deck_history"], lay["script"])
        if rb != want:
            raise ValueError("%s: records of %d bytes, this configuration's are %d" % (path, rb, want))
        if snap.dtype != torch.uint8 or snap.dim() != 2 or tuple(snap.shape) != (int(cfg["num_games"]), rb):
            raise ValueError("%s: the snapshot is not %d records of %d bytes" % (path, int(cfg["num_games"]), rb))
        env = cls(device=device, **cfg)
        status = env.restore(snap)
        if bool((status != 0).any()):
            bad = int((status != 0).nonzero()[0])
            env.close()
            raise _lib.HsadError("%s: record %d was refused (flags %d)" % (path, bad, int(status[bad])))
        return env

    def query(self):
        out = torch.zeros(self.G, 16, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.hsad_env_query(self.h, out.data_ptr(), self._stream()))
        return out

    def move_is_legal(self, uid):
        uid = uid.to(self.device, torch.int32).contiguous()
        out = torch.zeros(self.G, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.hsad_env_move_is_legal(self.h, uid.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def deck_history(self):
        out = torch.zeros(self.G, 50, dtype=torch.uint8, device=self.device)
        cnt = torch.zeros(self.G, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.hsad_env_deck_history(self.h, out.data_ptr(), cnt.data_ptr(), self._stream()))
        return out, cnt

    def export_state(self):
        w = self.lib.hsad_env_state_words(self.h)
        out = torch.zeros(self.G, w, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.hsad_env_export_state(self.h, out.data_ptr(), self._stream()))
        return out

    def check_errors(self):
        """Raises if any game hit what the reference treats as assert(false) (hanabi_env.cc:50,63-80)."""
        n, g, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(self.lib.hsad_env_error_count(self.h, C.byref(n), C.byref(g), C.byref(c)))
        if n.value:
            what = {1: "illegal move", 2: "illegal greedy move", 3: "step on a finished game",
                    4: "fork source index out of range", 5: "deal script names a card the deck does not hold",
                    6: "position refused (import_state / restore; see the call's status)",
                    7: "policy_rule: a seat_bot entry names no bot",
                    8: "replay of a game record met an illegal logged move"}.get(c.value, "?")
            raise _lib.HsadError("%d game(s) violated the env contract; first: game %d, %s" % (n.value, g.value, what))
