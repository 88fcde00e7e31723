"""GPU: frozen networks as partners of the partnered actor (hsad_actor_create_partnered_nets, actor.NetPartner).  Every comparison is
exact: the actor is held to the loop of primitives of tests/test_actor_partner_gpu.py, extended by one hsad_seat_gather -> act (greedy)
-> hsad_seat_scatter -> zero_hidden_rows per network partner, on a twin env with the same seeds."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_actor_partner_gpu import (AGENT_SEED, BOT_SEED, DEV, ETA, FULL, GAMMA, N_STEP, SMALL, Side, Twin, make_actor,
                                          replays_equal, same_state)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
STEPS = 12


def frozen_net(side, seed, hid_dim=64, num_fc_layer=1, num_lstm_layer=2, skip_connect=False):
    """a CNet of the env's dimensions with weights of another seed than the learner's (5)"""
    from hanabi_sad_amd.composite import CNet
    from hanabi_sad_amd.selfplay import init_weights
    W = init_weights(side.env.F, hid_dim, side.env.A, side.env.H, seed, num_lstm_layer=num_lstm_layer, num_fc_layer=num_fc_layer)
    return CNet(W, DEV, skip_connect=skip_connect)


class NetTwin(Twin):
    """Twin with network partners: per net k, hsad_seat_gather of its rows -> CompositeAgent.act without eps (greedy, no target pass,
    h0_16 iff n_k >= 1024) -> hsad_seat_scatter -> zero_hidden_rows on the terminal of each row's game.  `cnets`: the nets of
    seats.nets, the very handles the actor borrows (both sides run on one stream, one after the other)."""

    def __init__(self, side, seats, with_writer, cnets):
        from hanabi_sad_amd.composite import CompositeAgent
        super().__init__(side, seats, with_writer)
        self.net_agents = [CompositeAgent(n, n, N_STEP, GAMMA, seed=AGENT_SEED) for n in cnets]
        self.net_rows = [torch.tensor(r, dtype=torch.int32, device=DEV) for r in seats.net_rows]
        self.net_hid = []
        for ag, rows in zip(self.net_agents, self.net_rows):
            hid = ag.get_h0(len(rows))
            if len(rows) >= 1024:
                hid["h0_16"] = torch.zeros_like(hid["h0"], dtype=torch.bfloat16)
            self.net_hid.append(hid)
        # the learner's net asked on the partners' inputs (from a zero state): does it ever disagree with the partner?
        self.probe = CompositeAgent(side.nets[0], side.nets[0], N_STEP, GAMMA, seed=AGENT_SEED)
        self.net_greedy, self.probe_greedy = [], []

    def _gather(self, rows):
        from hanabi_sad_amd import _lib
        from hanabi_sad_amd.composite import _s
        env, Fp = self.s.env, self.s.agent.online.Fp
        n = len(rows)
        obs16 = torch.empty(n, Fp, dtype=torch.bfloat16, device=DEV)
        legal = torch.empty(n, env.A, dtype=torch.float32, device=DEV)
        _lib.check(env.lib.hsad_seat_gather(rows.data_ptr(), n, env.G * env.P, 0, env.priv_s_bf16.data_ptr(), env.F, Fp, env.legal_move.data_ptr(),
                                            env.A, obs16.data_ptr(), legal.data_ptr(), _s(env.device)))
        return obs16, legal

    def _scatter(self, rows, reply):
        from hanabi_sad_amd import _lib
        from hanabi_sad_amd.composite import _s
        env = self.s.env
        _lib.check(env.lib.hsad_seat_scatter(env.h, rows.data_ptr(), len(rows), reply["a"].data_ptr(), reply["greedy_a"].data_ptr(),
                                             env.a.data_ptr(), env.greedy_a.data_ptr(), _s(env.device)))

    def step(self):
        from hanabi_sad_amd.r2d2 import zero_hidden_rows
        s, env, agent, M = self.s, self.s.env, self.s.agent, self.M
        N = env.G * env.P
        obs16, legal = self._gather(self.rows)
        eps = env.eps.view(N)[self.rows_l].contiguous()
        if self.writer is not None:
            self.hist_hid.append(dict(self.hid))
        reply, self.hid = agent.act({"priv_s_bf16": obs16, "legal_move": legal, "eps": eps}, self.hid, with_q=True)
        if self.writer is not None:
            self.hist_q.append((reply["q_online_a"], reply["versions"][0]))
        net_replies, self.net_greedy, self.probe_greedy = [], [], []
        for k, (ag, rows) in enumerate(zip(self.net_agents, self.net_rows)):
            o16, lg = self._gather(rows)
            r, self.net_hid[k] = ag.act({"priv_s_bf16": o16, "legal_move": lg}, self.net_hid[k])
            assert torch.equal(r["a"], r["greedy_a"])
            net_replies.append(r)
            pr, _ = self.probe.act({"priv_s_bf16": o16, "legal_move": lg}, self.probe.get_h0(len(rows)))
            self.net_greedy.append(r["greedy_a"])
            self.probe_greedy.append(pr["greedy_a"])
        if self.seats.bots:
            env.policy_rule(self.seats.bots, self.seat_bot, seed=self.seats.bot_seed)
        self._scatter(self.rows, reply)
        for rows, r in zip(self.net_rows, net_replies):
            self._scatter(rows, r)
        if self.writer is not None:
            self.writer.push_obs_action({"priv_s": env.priv_bits.view(N, -1)[self.rows_l].contiguous(),
                                         "legal_move": env.legal_bits.view(N)[self.rows_l].contiguous(),
                                         "own_hand": env.own_bits.view(N)[self.rows_l].contiguous(), "eps": eps,
                                         "a": reply["a"], "greedy_a": reply["greedy_a"]})
        self.a, self.greedy_a = env.a.clone(), env.greedy_a.clone()
        env.step(env.a, env.greedy_a)
        game = self.rows_l // env.P
        rew, term = env.reward[game].contiguous(), env.terminal[game].to(torch.uint8).contiguous()
        self.net_term = [env.terminal[rows.long() // env.P].to(torch.uint8).contiguous() for rows in self.net_rows]
        env.reset()
        self.prio = None
        if self.writer is not None:
            self.writer.push_reward_terminal(rew, term)
        zero_hidden_rows(self.hid, term, 1)
        for hid, t in zip(self.net_hid, self.net_term):
            zero_hidden_rows(hid, t, 1)
        if self.writer is None or not self.writer.can_pop():
            return
        hid_s = self.hist_hid.pop(0)
        qa, version = self.hist_q.pop(0)
        stale = version != agent.online.version
        cur, _, r, t, boot = self.writer.pop_transition(want_fields=stale, want_next=False)
        if stale:
            qa = agent.q_of(agent.online, {"priv_s": cur["priv_s"].view(M, env.F), "legal_move": cur["legal_move"].view(M, env.A)},
                            cur["a"].view(-1), hid_s)
            self.n_stale = getattr(self, "n_stale", 0) + 1
        self.prio = agent.priority_from_q(qa, reply["q_target_greedy"], r, boot)
        self.writer.push_sequence(self.prio)
        self.writer.flush_to_replay(s.replay, ETA)


def same_partner_states(ac, twin):
    for k, hid in enumerate(twin.net_hid):
        h, c = ac.partner_state(k)
        if h.shape != hid["h0"].shape or not (torch.equal(h, hid["h0"]) and torch.equal(c, hid["c0"])):
            return False
    return True


def run_against_twin(a_side, b_side, seats, cnets, steps=STEPS, want_terminal=True):
    """the actor next to the twin, step by step; returns (partner moves on turn, of those: the learner's net would have moved otherwise,
    state rows zeroed)"""
    G, P, A = a_side.env.G, a_side.env.P, a_side.env.A
    ac = make_actor(a_side, seats)
    assert len(ac.partner_nets) == len(cnets) and all(x is y for x, y in zip(ac.partner_nets, cnets))
    twin = NetTwin(b_side, seats, False, cnets)
    sn = seats.seat_net.reshape(G, P)
    on_turn = differs = zeroed = 0
    for t in range(steps):
        rec = a_side.env.export_state().cpu().numpy()
        ac.step()
        twin.step()
        last = ac.last_reply
        assert torch.equal(last["a"].view(G, P), twin.a) and torch.equal(last["greedy_a"].view(G, P), twin.greedy_a), t
        assert torch.equal(a_side.env.snapshot(), b_side.env.snapshot()), t
        assert same_state(ac, twin), t
        assert same_partner_states(ac, twin), t
        a = last["a"].view(G, P).cpu().numpy()
        turn = rec[:, 57].astype(np.int64)                       # the seat on turn (record word 57)
        moved = (sn[np.arange(G), turn] >= 0) & (a[np.arange(G), turn] != A - 1)      # a net's seat on turn in a live game
        on_turn += int(moved.sum())
        for k, rows in enumerate(seats.net_rows):
            mine = moved[rows // P] & (turn[rows // P] == rows % P)
            differs += int((twin.net_greedy[k].cpu().numpy() != twin.probe_greedy[k].cpu().numpy())[mine].sum())
            zeroed += int(twin.net_term[k].sum())
            assert (a.reshape(-1)[rows][~(turn[rows // P] == rows % P)] == A - 1).all()      # off turn: the noop
    assert ac.num_act == steps * seats.M                           # the learner's rows only
    torch.cuda.synchronize()
    a_side.env.check_errors()
    b_side.env.check_errors()
    ac.close()
    return on_turn, differs, zeroed


def hand_made_p3(G, net):
    """P = 3, the learner on seat 1 of every game.  Even games: piers on seat 0 and the net on seat 2 (bot, learner and net in one
    game); odd games: the net on seats 0 and 2.  Row stride 3, two kinds of games, a net with two rows in one game."""
    from hanabi_sad_amd import rulebot
    from hanabi_sad_amd.actor import NetPartner, PartnerSeats
    sb, sn = np.full((G, 3), -1), np.full((G, 3), -1)
    sb[0::2, 0] = 0
    sn[0::2, 2] = 0
    sn[1::2, 0] = sn[1::2, 2] = 0
    return PartnerSeats([rulebot.PRESETS["piers"], NetPartner(net, name="frozen")], np.arange(G) * 3 + 1, sb, BOT_SEED, sn)


# (id, G, P, sad, rules, hand, max_len, layout).  max_len 8 cuts every game of the full-rule cases inside the 12 steps: each ends, and
# every state row is zeroed once; the SMALL case ends its games one by one (bombs and empty decks), so single rows are zeroed.
CASES = [("g33-p2-one-net", 33, 2, 1, FULL, 5, 8, "one"), ("g40-p3-bot-learner-net", 40, 3, 1, FULL, 5, 80, "p3"),
         ("g33-p2-two-shapes", 33, 2, 1, FULL, 5, 8, "two"), ("g1024-p2-bf16-state", 1024, 2, 1, FULL, 5, 8, "one"),
         ("g33-p2-nosad", 33, 2, 0, FULL, 5, 8, "one"), ("g33-p2-small-rules", 33, 2, 1, SMALL, 2, 10, "one")]


@pytest.mark.parametrize("name,G,P,sad,rules,hand,max_len,layout", CASES, ids=[c[0] for c in CASES])
def test_net_partners_are_the_loop_of_existing_primitives(name, G, P, sad, rules, hand, max_len, layout):
    from hanabi_sad_amd.actor import NetPartner, PartnerSeats
    a_side = Side(G, P, hand, sad, rules, max_len)
    b_side = Side(G, P, hand, sad, rules, max_len, nets=a_side.nets)
    if layout == "two":      # per-net L_k, H_k and offsets: (2 fc, 1 layer, skip, hid 128) and (1 fc, 3 layers, hid 64) next to the learner's (1, 2, 64)
        cnets = [frozen_net(a_side, 21, hid_dim=128, num_fc_layer=2, num_lstm_layer=1, skip_connect=True),
                 frozen_net(a_side, 22, hid_dim=64, num_fc_layer=1, num_lstm_layer=3)]
    else:
        cnets = [frozen_net(a_side, 21)]
    if layout == "p3":
        seats = hand_made_p3(G, cnets[0])
    else:
        seats = PartnerSeats.alternate(G, P, [NetPartner(n, name="frozen%d" % k) for k, n in enumerate(cnets)], bot_seed=BOT_SEED)
    assert seats.M == G and sum(len(r) for r in seats.net_rows) == (G if layout != "p3" else G + G // 2)
    on_turn, differs, zeroed = run_against_twin(a_side, b_side, seats, cnets)
    print("%s: partners on turn %d of %d game-steps, the learner's net differs on %d, state rows zeroed %d" % (name, on_turn, STEPS * G, differs, zeroed))
    assert on_turn >= 4 * G
    assert differs >= 1
    if max_len < 80:
        assert zeroed >= 1


# ---- what reaches the replay ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync", [False, True], ids=["one-launch-tail", "stale-q-redo"])
def test_replay_holds_the_learner_rows_only(sync):
    from hanabi_sad_amd.actor import NetPartner, PartnerSeats
    G, P, H, max_len = 33, 2, 2, 10
    a_side = Side(G, P, H, 1, SMALL, max_len)
    b_side = Side(G, P, H, 1, SMALL, max_len, nets=a_side.nets)
    cnets = [frozen_net(a_side, 21)]
    seats = PartnerSeats.alternate(G, P, [NetPartner(cnets[0], name="frozen")], bot_seed=BOT_SEED)
    ac = make_actor(a_side, seats)
    twin = NetTwin(b_side, seats, True, cnets)
    pushed = 0
    for t in range(30):
        if sync and t in (8, 9, 17):       # the learner's weights are rewritten inside the n-step window; no partner action changes
            for net in a_side.nets:
                net.w["fc_a.weight"].mul_(1.02)
                net.w["lstm.weight_hh_l0"].mul_(0.99)
                net.refresh()
        ac.step()
        twin.step()
        assert torch.equal(ac.last_reply["a"].view(G, P), twin.a) and torch.equal(ac.last_reply["greedy_a"].view(G, P), twin.greedy_a), t
        assert same_state(ac, twin) and same_partner_states(ac, twin), t
        pa = ac.last_priority
        assert (pa is None) == (twin.prio is None), t
        if pa is not None:
            assert pa.shape == (seats.M,) and torch.equal(pa, twin.prio), t
            pushed += 1
    torch.cuda.synchronize()
    assert pushed >= 30 - N_STEP - 1
    if sync:
        assert ac.num_redo == twin.n_stale and ac.num_redo >= 6
    else:
        assert ac.num_redo == 0
    replays_equal(a_side.replay, b_side.replay, seats.M)      # (num_add of both sides: the hand-driven writer has M envs)
    a_side.env.check_errors()
    ac.close()


# ---- the library's own refusals ------------------------------------------------------------------------------------------------------
def test_the_abi_refuses_bad_net_partners_by_name():
    from hanabi_sad_amd import _lib, rulebot
    G, P = 4, 2
    side = Side(G, P, 5, 1, FULL, 80)
    side.env.enable_packed(side.agent.online.Fp, keep_float32=False)
    env, agent = side.env, side.agent
    cfg = _lib.ActorConfig(0, N_STEP, 80, 5, agent.online.H, GAMMA, ETA, 1)
    io = _lib.ActorIO(env.legal_move.data_ptr(), env.own_hand.data_ptr(), env.eps.data_ptr(), env.reward.data_ptr(), env.terminal.data_ptr(),
                      env.priv_bits.data_ptr(), env.legal_bits.data_ptr(), env.own_bits.data_ptr(), env.priv_s_bf16.data_ptr())
    rules, n_rules, n_bot = rulebot.pack([rulebot.PRESETS["piers"]])
    net_a, net_b = frozen_net(side, 21), frozen_net(side, 22, hid_dim=128)
    from hanabi_sad_amd.composite import CNet
    from hanabi_sad_amd.selfplay import init_weights
    wide = CNet(init_weights(env.F + 3, 64, env.A, 5, 23), DEV)
    rows = np.asarray([0, 3, 4, 7], dtype=np.int32)
    good_sb, good_sn = [-1, 0, 0, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, 0, 1, -1]

    def create(nets, seat_net, seat_bot=good_sb):
        sb, sn = np.asarray(seat_bot, dtype=np.int32), np.asarray(seat_net, dtype=np.int32)
        part = _lib.ActorPartners(rows.ctypes.data, len(rows), C.addressof(rules), C.addressof(n_rules), n_bot, sb.ctypes.data, 1)
        handles = (C.c_void_p * len(nets))(*[n.h for n in nets])
        net_part = _lib.ActorNetPartners(C.addressof(handles), len(nets), sn.ctypes.data)
        h = C.c_void_p()
        rc = env.lib.hsad_actor_create_partnered_nets(env.h, agent.online.h, agent.target.h, side.replay.h, C.byref(cfg), C.byref(io),
                                                      C.byref(part), C.byref(net_part), C.byref(h))
        if rc == 0:
            env.lib.hsad_actor_destroy(h)
        return rc, env.lib.hsad_last_error().decode()
    assert create([net_a, net_b], good_sn)[0] == 0
    for nets, sn, text in (([net_a, wide], good_sn, "net 1 has in_dim %d, the env's observation has %d features" % (env.F + 3, env.F)),
                           ([net_a, net_a], good_sn, "nets[1] is the same handle as nets[0]"),
                           ([net_a, agent.online], good_sn, "nets[1] is the online net of this actor"),
                           ([net_a, net_b], [0, -1, -1, -1, -1, 0, 1, -1], "seat_net[0] = 0 on a learner row"),
                           ([net_a, net_b], [-1, -1, -1, -1, -1, 0, 0, -1], "net 1 owns no row")):
        rc, msg = create(nets, sn)
        assert rc != 0 and "actor_create_partnered" in msg and text in msg, (rc, msg)


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def test_driver_trains_next_to_a_bot_and_a_weight_file(capsys, tmp_path):
    import re
    from hanabi_sad_amd import BatchedHanabiEnv, selfplay
    probe = BatchedHanabiEnv(2, players=2, hand_size=2, seed=1, sad=True, device=DEV, colors=2, ranks=5, max_information_tokens=8,      # (the driver's --sad 1)
                             max_life_tokens=1)
    f = str(tmp_path / "frozen.pthw")
    torch.save(selfplay.init_weights(probe.F, 64, probe.A, 2, 31), f)
    selfplay.main(["--num_game", "128", "--partner", "piers", f, "--num_update", "3", "--burn_in_frames", "64",
                   "--replay_buffer_size", "512", "--batchsize", "32", "--colors", "2", "--hand_size", "2", "--max_life_tokens", "1"])
    out = capsys.readouterr().out
    loss = re.findall(r"update 0 loss (\S+) grad_norm (\S+)", out)
    assert loss and np.isfinite(float(loss[0][0])) and np.isfinite(float(loss[0][1])), out[-2000:]
    assert "Speed: train:" in out
    lines = re.findall(r"^partner (\S+): score (\S+) \(", out, flags=re.M)
    assert [n for n, _ in lines] == ["piers", "frozen.pthw"], out[-2000:]
    for _, sc in lines:
        assert 0.0 <= float(sc) <= 2 * 5          # 2 colours of 5 ranks
