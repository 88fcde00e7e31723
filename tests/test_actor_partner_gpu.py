"""GPU: the partnered actor (hsad_actor_create_partnered, actor.DeviceActor(partners=...)).  Every comparison is exact: the actor is
held to a loop of the primitives that existed before it (hsad_seat_gather -> hsad_r2d2_act -> hsad_env_policy_rule -> hsad_seat_scatter
-> step -> reset, and the sequence writer's separate entry points) on a twin env with the same seeds, to hsad_actor_create when every
row is the learner's, and -- for the partner rows -- to the plain-Python bot of tests/rulebot_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import rulebot_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
FULL = dict(colors=5, ranks=5, max_information_tokens=8, max_life_tokens=3)
SMALL = dict(colors=2, ranks=5, max_information_tokens=8, max_life_tokens=1)      # with hand_size 2: every game ends within a few steps
N_STEP, GAMMA, ETA, BOT_SEED, AGENT_SEED = 3, 0.999, 0.9, 4242, 77
EPS = [0.4, 0.1, 0.0]


class Side:
    """env + replay of one side of a comparison; the nets are shared by both sides (the same weights, the same version)"""

    def __init__(self, G, P, H, sad, rules, max_len, nets=None, hid_dim=64, capacity=4096):
        from hanabi_sad_amd import BatchedHanabiEnv
        from hanabi_sad_amd.actor import transition_fields
        from hanabi_sad_amd.composite import CNet, CompositeAgent
        from hanabi_sad_amd.replay import DeviceReplay
        from hanabi_sad_amd.selfplay import init_weights
        self.env = BatchedHanabiEnv(G, players=P, hand_size=H, seed=9001, eps_list=EPS, max_len=max_len, sad=bool(sad), device=DEV,
                                    track_deck_history=False, **rules)
        if nets is None:
            W = init_weights(self.env.F, hid_dim, self.env.A, H, 5)
            nets = (CNet(W, DEV), CNet(W, DEV))
        self.nets = nets
        self.agent = CompositeAgent(nets[0], nets[1], N_STEP, GAMMA, seed=AGENT_SEED)
        self.fields = transition_fields(self.env)
        self.replay = DeviceReplay(capacity, 3, 0.9, 0.6, 3, max_len, self.fields, DEV)
        self.max_len = max_len
        self.rules = dict(rules, players=P, hand_size=H)


class Twin:
    """the loop of existing primitives on M learner rows, one call per step"""

    def __init__(self, side, seats, with_writer):
        from hanabi_sad_amd.replay import SequenceWriter
        self.s, self.seats = side, seats
        env = side.env
        env.enable_packed(side.agent.online.Fp, keep_float32=False)
        self.M = seats.M
        self.rows = torch.tensor(seats.rows, dtype=torch.int32, device=DEV)
        self.rows_l = self.rows.long()
        self.seat_bot = torch.tensor(seats.seat_bot, dtype=torch.int32, device=DEV).view(env.G, env.P)
        self.hid = side.agent.get_h0(self.M)
        if self.M >= 1024:
            self.hid["h0_16"] = torch.zeros_like(self.hid["h0"], dtype=torch.bfloat16)
        self.writer = None
        if with_writer:
            self.writer = SequenceWriter(self.M, N_STEP, GAMMA, side.max_len, side.fields, DEV)
            self.writer.set_prepacked(("priv_s", "legal_move", "own_hand"))
        self.hist_hid, self.hist_q = [], []
        self.prio = None
        env.reset()

    def step(self):
        from hanabi_sad_amd import _lib
        from hanabi_sad_amd.composite import _s
        from hanabi_sad_amd.r2d2 import zero_hidden_rows
        s, env, agent, M = self.s, self.s.env, self.s.agent, self.M
        N, Fp = env.G * env.P, agent.online.Fp
        obs16 = torch.empty(M, Fp, dtype=torch.bfloat16, device=DEV)
        legal = torch.empty(M, env.A, dtype=torch.float32, device=DEV)
        _lib.check(env.lib.hsad_seat_gather(self.rows.data_ptr(), M, N, 0, env.priv_s_bf16.data_ptr(), env.F, Fp, env.legal_move.data_ptr(),
                                            env.A, obs16.data_ptr(), legal.data_ptr(), _s(env.device)))
        eps = env.eps.view(N)[self.rows_l].contiguous()
        if self.writer is not None:      # the state that enters this step is needed again if its Q_online pass is redone
            self.hist_hid.append(dict(self.hid))
        reply, self.hid = agent.act({"priv_s_bf16": obs16, "legal_move": legal, "eps": eps}, self.hid, with_q=True)
        if self.writer is not None:
            self.hist_q.append((reply["q_online_a"], reply["versions"][0]))
        if self.seats.bots:
            env.policy_rule(self.seats.bots, self.seat_bot, seed=self.seats.bot_seed)
        _lib.check(env.lib.hsad_seat_scatter(env.h, self.rows.data_ptr(), M, reply["a"].data_ptr(), reply["greedy_a"].data_ptr(),
                                             env.a.data_ptr(), env.greedy_a.data_ptr(), _s(env.device)))
        if self.writer is not None:
            self.writer.push_obs_action({"priv_s": env.priv_bits.view(N, -1)[self.rows_l].contiguous(),
                                         "legal_move": env.legal_bits.view(N)[self.rows_l].contiguous(),
                                         "own_hand": env.own_bits.view(N)[self.rows_l].contiguous(), "eps": eps,
                                         "a": reply["a"], "greedy_a": reply["greedy_a"]})
        self.a, self.greedy_a = env.a.clone(), env.greedy_a.clone()
        env.step(env.a, env.greedy_a)
        game = self.rows_l // env.P
        rew, term = env.reward[game].contiguous(), env.terminal[game].to(torch.uint8).contiguous()
        env.reset()
        self.prio = None
        if self.writer is not None:
            self.writer.push_reward_terminal(rew, term)
        zero_hidden_rows(self.hid, term, 1)
        if self.writer is None:
            return
        if not self.writer.can_pop():
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


def make_actor(side, seats):
    from hanabi_sad_amd.actor import DeviceActor
    ac = DeviceActor(side.env, side.agent, side.replay, N_STEP, GAMMA, ETA, side.max_len, partners=seats)
    assert ac.c_actor is not None
    side.env.reset()
    return ac


def seats_of(kind, G, P, names=("cautious", "piers")):
    from hanabi_sad_amd import rulebot
    from hanabi_sad_amd.actor import PartnerSeats
    bots = [rulebot.PRESETS[n] for n in names]
    if kind == "alternate":
        return PartnerSeats.alternate(G, P, bots, bot_seed=BOT_SEED)
    return PartnerSeats.fixed_seat(G, P, int(kind), bots, bot_seed=BOT_SEED)


def same_state(ac, twin):
    h, c = ac.state
    return torch.equal(h, twin.hid["h0"].reshape(-1)) and torch.equal(c, twin.hid["c0"].reshape(-1))


def replays_equal(ra, rb, M):
    na, nb = ra.size(), rb.size()
    assert ra.num_add() >= M, "the run added %d sequences, fewer than the %d learner rows" % (ra.num_add(), M)
    assert (na, ra.num_add()) == (nb, rb.num_add())
    for i in range(na):
        fa, fb = ra.get(i), rb.get(i)
        for k in fa[0]:
            assert torch.equal(fa[0][k], fb[0][k]), (i, k)
        for x, y, what in zip(fa[1:], fb[1:], ("reward", "terminal", "bootstrap", "seq_len")):
            assert torch.equal(x, y), (i, what)
    ra.check_errors()
    rb.check_errors()
    # the stored priorities: the weight sum, and the weight of the sequence under each point of an even grid
    # (finer than the slots of the small cases; every pushed priority is also compared step by step by the callers)
    (sa, _), (sb, _) = ra.priority_sum(), rb.priority_sum()
    assert sa == sb and sa > 0
    n_pts = min(4 * na, 256)      # (one sample_at call takes a batch of a few hundred at the most)
    grid = (np.arange(n_pts, dtype=np.float64) + 0.5) * (sa / n_pts)
    (_, _, _, _, la), wa = ra.sample_at(grid.astype(np.float32))
    (_, _, _, _, lb), wb = rb.sample_at(grid.astype(np.float32))
    assert torch.equal(wa, wb) and torch.equal(la, lb)


# (id, G, P, sad, seat layout): a partial wave with an odd row count; row stride 3 with another F and bit-row width; M = 1,024 crosses the
# actor's fused_state threshold (the bf16 state copy is live); and sad off
CASES = [("g33-p2", 33, 2, 1, "alternate"), ("g40-p3", 40, 3, 1, "1"), ("g1024-p2", 1024, 2, 1, "alternate"), ("g33-p2-nosad", 33, 2, 0, "alternate")]


# ---- 1 and 4: the actor is the loop of primitives, and the partner rows are the bots' ------------------------------------------------
@pytest.mark.parametrize("name,G,P,sad,layout", CASES, ids=[c[0] for c in CASES])
def test_partnered_actor_is_the_loop_of_existing_primitives(name, G, P, sad, layout):
    a_side = Side(G, P, 5, sad, FULL, 80)
    b_side = Side(G, P, 5, sad, FULL, 80, nets=a_side.nets)
    seats = seats_of(layout, G, P)
    M = seats.M
    assert M == G
    ac = make_actor(a_side, seats)
    twin = Twin(b_side, seats, with_writer=False)
    sb = seats.seat_bot.reshape(G, P)
    n_bot_moves = 0
    for t in range(12):
        rec = a_side.env.export_state().cpu().numpy()
        ac.step()
        twin.step()
        last = ac.last_reply
        assert torch.equal(last["a"].view(G, P), twin.a) and torch.equal(last["greedy_a"].view(G, P), twin.greedy_a), t
        assert torch.equal(a_side.env.snapshot(), b_side.env.snapshot()), t      # planes, generator, policy counter
        assert same_state(ac, twin), t
        # no partner row learns, no learner row is scripted: the partner on turn plays the reference bot's move (key = the game
        # index, counter = one policy call per step since the env was made)
        a = last["a"].view(G, P).cpu().numpy()
        ga = last["greedy_a"].view(G, P).cpu().numpy()
        for g in range(G):
            p = int(rec[g][57])           # the seat on turn (record word 57)
            if sb[g, p] < 0:
                continue
            bot = seats.bots[sb[g, p]]
            p_ref, uid, _ = ref.act_record(rec[g], a_side.rules, ref.PRESETS[bot.name], BOT_SEED, g, t)
            assert p_ref == p and a[g, p] == uid and ga[g, p] == uid, (t, g, p, bot.name)
            n_bot_moves += 1
        off_turn = (sb >= 0) & (np.arange(P)[None, :] != rec[:, 57][:, None])
        assert (a[off_turn] == a_side.env.A - 1).all()
    assert n_bot_moves >= 4 * G                   # about half the turns are the partners'
    assert ac.num_act == 12 * M
    torch.cuda.synchronize()
    a_side.env.check_errors()
    b_side.env.check_errors()
    ac.close()


# ---- 2: what reaches the replay ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync", [False, True], ids=["one-launch-tail", "stale-q-redo"])
def test_replay_content_equals_the_hand_driven_sequence_writer(sync):
    G, P, H, max_len = 33, 2, 2, 10
    a_side = Side(G, P, H, 1, SMALL, max_len)
    b_side = Side(G, P, H, 1, SMALL, max_len, nets=a_side.nets)
    seats = seats_of("alternate", G, P)
    ac = make_actor(a_side, seats)
    twin = Twin(b_side, seats, with_writer=True)
    pushed = 0
    for t in range(30):
        if sync and t in (8, 9, 17):       # a weight sync inside the n-step window: the cached Q_online of the steps in it is stale
            for net in a_side.nets:
                net.w["fc_a.weight"].mul_(1.02)
                net.w["lstm.weight_hh_l0"].mul_(0.99)
                net.refresh()
        ac.step()
        twin.step()
        assert torch.equal(ac.last_reply["a"].view(G, P), twin.a), t
        assert same_state(ac, twin), t
        pa = ac.last_priority
        assert (pa is None) == (twin.prio is None), t
        if pa is not None:
            assert pa.shape == (seats.M,) and torch.equal(pa, twin.prio), t
            pushed += 1
    torch.cuda.synchronize()
    assert pushed >= 30 - N_STEP - 1
    if sync:
        assert ac.num_redo == twin.n_stale and ac.num_redo >= 6      # the four-call path with the redo ran on M rows
    else:
        assert ac.num_redo == 0
    replays_equal(a_side.replay, b_side.replay, seats.M)
    a_side.env.check_errors()
    ac.close()


# ---- 3: every row the learner's and no bot = hsad_actor_create ---------------------------------------------------------------------
@pytest.mark.parametrize("G", [33, 512])
def test_all_rows_and_no_bot_is_the_self_play_actor(G):
    from hanabi_sad_amd.actor import DeviceActor, PartnerSeats
    P, max_len = 2, 6      # a game is cut at 6 steps and its sequence leaves the n-step window 3 steps later: inside the 12 steps
    a_side = Side(G, P, 5, 1, FULL, max_len, capacity=8192)
    b_side = Side(G, P, 5, 1, FULL, max_len, nets=a_side.nets, capacity=8192)
    seats = PartnerSeats([], np.arange(G * P), np.full(G * P, -1))
    ac = make_actor(a_side, seats)
    plain = DeviceActor(b_side.env, b_side.agent, b_side.replay, N_STEP, GAMMA, ETA, max_len)
    assert plain.c_actor is not None
    b_side.env.reset()
    for t in range(12):
        ac.step()
        plain.step()
        la, lb = ac.last_reply, plain.last_reply
        assert torch.equal(la["a"], lb["a"]) and torch.equal(la["greedy_a"], lb["greedy_a"]), t
        (ha, ca), (hb, cb) = ac.state, plain.state
        assert torch.equal(ha, hb) and torch.equal(ca, cb), t
        pa, pb = ac.last_priority, plain.last_priority
        assert (pa is None) == (pb is None) and (pa is None or torch.equal(pa, pb)), t
        assert torch.equal(a_side.env.snapshot(), b_side.env.snapshot()), t
    torch.cuda.synchronize()
    assert ac.num_act == plain.num_act == 12 * G * P
    replays_equal(a_side.replay, b_side.replay, G * P)
    ac.close()
    plain.close()


# ---- the library's own refusals (the header's check runs before anything is allocated) --------------------------------------------
def test_the_abi_refuses_a_bad_layout_by_name():
    from hanabi_sad_amd import _lib, rulebot
    G, P = 4, 2
    side = Side(G, P, 5, 1, FULL, 80)
    side.env.enable_packed(side.agent.online.Fp, keep_float32=False)
    env, agent = side.env, side.agent
    cfg = _lib.ActorConfig(0, N_STEP, 80, 5, agent.online.H, GAMMA, ETA, 1)
    io = _lib.ActorIO(env.legal_move.data_ptr(), env.own_hand.data_ptr(), env.eps.data_ptr(), env.reward.data_ptr(), env.terminal.data_ptr(),
                      env.priv_bits.data_ptr(), env.legal_bits.data_ptr(), env.own_bits.data_ptr(), env.priv_s_bf16.data_ptr())
    rules, n_rules, n_bot = rulebot.pack([rulebot.PRESETS["piers"]])

    def create(rows, seat_bot, vdn=0, n_bot_=n_bot):
        rows, seat_bot = np.asarray(rows, dtype=np.int32), np.asarray(seat_bot, dtype=np.int32)
        cfg.vdn = vdn
        part = _lib.ActorPartners(rows.ctypes.data, len(rows), C.addressof(rules), C.addressof(n_rules), n_bot_, seat_bot.ctypes.data, 1)
        h = C.c_void_p()
        rc = env.lib.hsad_actor_create_partnered(env.h, agent.online.h, agent.target.h, side.replay.h, C.byref(cfg), C.byref(io), C.byref(part),
                                                 C.byref(h))
        if rc == 0:
            env.lib.hsad_actor_destroy(h)
        return rc, env.lib.hsad_last_error().decode()
    good_rows, good_sb = [0, 3, 4, 7], [-1, 0, 0, -1, -1, 0, 0, -1]
    assert create(good_rows, good_sb)[0] == 0
    for rows, sb, kw, text in (([0, 3, 3, 7], good_sb, {}, "rows[2] = 3 is not above rows[1]"),
                               ([0, 3, 4, 8], good_sb, {}, "rows[3] = 8, must be 0..7"),
                               (good_rows, [-1, 0, 0, 0, -1, 0, 0, -1], {}, "seat_bot[3] = 0 on a learner row"),
                               (good_rows, [-1, -1, 0, -1, -1, 0, 0, -1], {}, "seat_bot[1] = -1 on a partner row"),
                               (good_rows, good_sb, {"vdn": 1}, "cfg->vdn = 1"),
                               (good_rows, good_sb, {"n_bot_": 0}, "n_bot = 0"),
                               (good_rows, good_sb, {"n_bot_": 9}, "n_bot = 9")):
        rc, msg = create(rows, sb, **kw)
        assert rc != 0 and "actor_create_partnered" in msg and text in msg, (rc, msg)
    bad = rulebot.pack([rulebot.RuleBot([14])])
    part_rows, part_sb = np.asarray(good_rows, dtype=np.int32), np.asarray(good_sb, dtype=np.int32)
    cfg.vdn = 0
    part = _lib.ActorPartners(part_rows.ctypes.data, 4, C.addressof(bad[0]), C.addressof(bad[1]), 1, part_sb.ctypes.data, 1)
    h = C.c_void_p()
    assert env.lib.hsad_actor_create_partnered(env.h, agent.online.h, agent.target.h, side.replay.h, C.byref(cfg), C.byref(io), C.byref(part),
                                               C.byref(h)) != 0
    assert "bot 0 names an unknown rule code" in env.lib.hsad_last_error().decode()


# ---- 5: the driver ----------------------------------------------------------------------------------------------------------------------
def test_driver_trains_next_to_partners_and_prints_their_lines(capsys):
    import re
    from hanabi_sad_amd import selfplay
    selfplay.main(["--num_game", "128", "--partner", "cautious", "piers", "--num_update", "3", "--burn_in_frames", "64",
                   "--replay_buffer_size", "512", "--batchsize", "32", "--colors", "2", "--hand_size", "2", "--max_life_tokens", "1"])
    out = capsys.readouterr().out
    loss = re.findall(r"update 0 loss (\S+) grad_norm (\S+)", out)
    assert loss and np.isfinite(float(loss[0][0])) and np.isfinite(float(loss[0][1])), out[-2000:]
    assert "Speed: train:" in out
    lines = re.findall(r"^partner (\w+): score (\S+) \(", out, flags=re.M)
    assert [n for n, _ in lines] == ["cautious", "piers"], out[-2000:]
    for _, sc in lines:
        assert 0.0 <= float(sc) <= 2 * 5          # 2 colours of 5 ranks
