"""CPU: seat layouts that mix rule bots and frozen networks (actor.PartnerSeats with actor.NetPartner), every new host refusal with
its message, partner_layout_verdict_nets of csrc/hsad_partner.h under the sanitizers against the Python restatement, and the
driver's --partner with weight files."""
import os
import subprocess

import numpy as np
import pytest
import torch

from hanabi_sad_amd import rulebot as rbt
from hanabi_sad_amd.actor import NetPartner, PartnerSeats, PartnerSeatsError
from tests.test_actor_partner_cpu import _refusals as _old_refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_ENV, A_ENV = 100, 21
BOTS = [rbt.PRESETS["cautious"], rbt.PRESETS["piers"], rbt.PRESETS["flawed"]]


def fake_net(name, in_dim=F_ENV, num_action=A_ENV):
    """a NetPartner the layout code can judge: only the shapes of two tensors are read without a device"""
    return NetPartner({"net.0.weight": torch.zeros(4, in_dim), "fc_a.weight": torch.zeros(num_action, 4)}, name=name)


NETS = [fake_net("n0"), fake_net("n1"), fake_net("n2")]
MIXES = [[NETS[0]], [BOTS[0], NETS[0]], [NETS[0], BOTS[1], NETS[1]], [BOTS[0], BOTS[1], NETS[2], NETS[0]]]


def _check_mixed(s, G, P, partners, seat_of_game, partner_of_game):
    """one owner per row; net k's rows ascending; partner j sits where bot j of an all-bot list of the same length would"""
    N = G * P
    assert s.bots == [x for x in partners if not isinstance(x, NetPartner)]
    assert s.nets == [x for x in partners if isinstance(x, NetPartner)]
    assert s.seat_bot.dtype == np.int32 and s.seat_net.dtype == np.int32 and s.seat_bot.shape == s.seat_net.shape == (N,)
    learner = np.zeros(N, dtype=bool)
    learner[s.rows] = True
    owners = learner.astype(int) + (s.seat_bot >= 0) + (s.seat_net >= 0)
    assert (owners == 1).all()
    assert (s.rows == np.arange(G) * P + seat_of_game).all()
    for k, rows in enumerate(s.net_rows):
        assert (np.diff(rows) > 0).all() and (s.seat_net[rows] == k).all()
    all_bots = PartnerSeats(BOTS[:1] * len(partners), s.rows, np.where(learner, -1, np.repeat(partner_of_game, P)))
    assert all_bots.verdict(G, P) == (0, 0, 0)
    for j, x in enumerate(partners):
        games_j = np.nonzero(partner_of_game == j)[0]
        mine = np.nonzero((s.seat_net == s.nets.index(x)) if isinstance(x, NetPartner) else (s.seat_bot == s.bots.index(x)))[0]
        assert (mine == np.nonzero(all_bots.seat_bot == j)[0]).all()
        assert set((mine // P).tolist()) == (set(games_j.tolist()) if P > 1 else set())


@pytest.mark.parametrize("G,P", [(12, 2), (13, 3), (25, 5)])
@pytest.mark.parametrize("mix", range(len(MIXES)))
def test_mixed_layouts(G, P, mix):
    partners = MIXES[mix]
    g = np.arange(G)
    s = PartnerSeats.alternate(G, P, partners, bot_seed=3)
    _check_mixed(s, G, P, partners, g % P, (g // P) % len(partners))
    assert s.verdict(G, P, 5, False, F_ENV, A_ENV) == (0, 0, 0)
    for seat in range(P):
        s = PartnerSeats.fixed_seat(G, P, seat, partners)
        _check_mixed(s, G, P, partners, np.full(G, seat), g % len(partners))
        assert s.check(G, P, 5, False, F_ENV, A_ENV) is s


def test_bot_only_layouts_keep_their_fields():
    s = PartnerSeats.alternate(6, 2, BOTS[:2])
    assert s.nets == [] and s.seat_net is None and s.bots == BOTS[:2] and s.verdict(6, 2) == (0, 0, 0)
    assert (s.seat_bot.reshape(6, 2)[np.arange(6), 1 - np.arange(6) % 2] == (np.arange(6) // 2) % 2).all()


def _net_refusals(G=4, P=2):
    """(what, PartnerSeats, G, P, hand_size, vdn, F, A, verdict, text the message must hold): one learner seat per game (rows 0 3 4 7),
    piers on the partner rows of games 0 and 1, net 0 on game 2's (row 5), net 1 on game 3's (row 6)"""
    rows = np.array([0, 3, 4, 7])
    sb = np.array([-1, 0, 0, -1, -1, -1, -1, -1])
    sn = np.array([-1, -1, -1, -1, -1, 0, 1, -1])
    mk = lambda partners=(BOTS[1], NETS[0], NETS[1]), r=rows, b=sb, n=sn: PartnerSeats(list(partners), r, b, 0, n)
    put = lambda arr, i, v: np.concatenate([arr[:i], [v], arr[i + 1:]])
    ok = mk()
    assert ok.verdict(G, P, 5, 0, F_ENV, A_ENV) == (0, 0, 0)
    return [("no net but a seat_net", mk(partners=[BOTS[1]]), (12, 0, 0), "n_net = 0, must be 1..8"),
            ("nine nets", mk(partners=[BOTS[1]] + [NETS[0]] * 9), (12, 0, 9), "n_net = 9, must be 1..8"),
            ("in_dim", mk(partners=[BOTS[1], NETS[0], fake_net("x", in_dim=77)]), (13, 1, 77), "net 1 has in_dim 77, the env's observation has 100 features"),
            ("num_action", mk(partners=[BOTS[1], fake_net("x", num_action=31), NETS[1]]), (14, 0, 31), "net 0 has num_action 31, the env has 21 actions"),
            ("net on a learner row", mk(n=put(sn, 3, 1)), (15, 3, 1), "seat_net[3] = 1 on a learner row, must be -1"),
            ("net index too large", mk(n=put(sn, 5, 2)), (16, 5, 2), "seat_net[5] = 2, must be -1..1"),
            ("net index below -1", mk(n=put(sn, 6, -2)), (16, 6, -2), "seat_net[6] = -2, must be -1..1"),
            ("net on a bot row", mk(n=put(sn, 2, 0)), (17, 2, 0), "seat_net[2] = 0 on a row seat_bot gives to a bot"),
            ("nobody's row", mk(b=put(sb, 1, -1)), (18, 1, 0), "row 1 is neither the learner's nor a bot's nor a net's"),
            ("a net without a row", mk(n=put(sn, 6, 0)), (19, 1, 0), "net 1 owns no row"),
            ("bot index on a net layout", mk(b=put(sb, 2, 1)), (11, 2, 1), "seat_bot[2] = 1 on a partner row, must be -1..0"),
            ("nine bots next to a net", mk(partners=[BOTS[1]] * 9 + [NETS[0], NETS[1]]), (6, 0, 9), "n_bot = 9, must be 0..8"),
            ("bot on a learner row", mk(b=put(sb, 4, 0)), (10, 4, 0), "seat_bot[4] = 0 on a learner row, must be -1"),
            ("vdn", ok, (1, 0, 1), "cfg->vdn = 1")], G, P


@pytest.mark.parametrize("case", _net_refusals()[0], ids=lambda c: c[0].replace(" ", "_"))
def test_every_new_refusal_names_the_entry(case):
    what, s, verdict, text = case
    G, P, vdn = 4, 2, int(what == "vdn")
    assert s.verdict(G, P, 5, vdn, F_ENV, A_ENV) == verdict, what
    with pytest.raises(PartnerSeatsError) as e:
        s.check(G, P, 5, vdn, F_ENV, A_ENV)
    assert text in str(e.value) and e.value.verdict == verdict


def test_nets_only_layout_needs_no_bot():
    s = PartnerSeats.alternate(6, 3, [NETS[0], NETS[1]])
    assert s.bots == [] and (s.seat_bot == -1).all() and s.verdict(6, 3, 5, False, F_ENV, A_ENV) == (0, 0, 0)


def _layout_text(s, G, P, H, vdn):
    has_net = s.seat_net is not None
    t = ["%d %d %d %d %d %d %d %d %d %d" % (G, P, H, int(vdn), s.M, len(s.bots), int(has_net), len(s.nets), F_ENV, A_ENV),
         " ".join(str(int(r)) for r in s.rows)]
    for bot in s.bots:
        t.append(" ".join([str(len(bot.rules))] + ["%d %d" % ck for ck in bot.rules[:rbt.MAX_RULES]]))
    t.append(" ".join(str(int(b)) for b in s.seat_bot))
    if has_net:
        t.append(" ".join("%d %d" % n.dims() for n in s.nets))
        t.append(" ".join(str(int(b)) for b in s.seat_net))
    return "\n".join(t)


def _seeded_layouts(seed, n):
    """mixed layouts of random shapes (G 1-8, P 2-5, 0-3 bots, 0-3 nets), and each again with one random entry spoiled"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        G, P, nb, nn = int(rng.randint(1, 9)), int(rng.randint(2, 6)), int(rng.randint(0, 4)), int(rng.randint(0, 4))
        partners = [BOTS[j] for j in range(nb)] + [NETS[j] for j in range(nn)]
        partners = [partners[j] for j in rng.permutation(len(partners))]
        N = G * P
        if not partners:
            s = PartnerSeats([], np.arange(N), np.full(N, -1))
        elif k % 3 == 0:
            s = PartnerSeats.alternate(G, P, partners)
        elif k % 3 == 1:
            s = PartnerSeats.fixed_seat(G, P, int(rng.randint(P)), partners)
        else:      # any owner on any row, the learner on row 0
            owner = rng.randint(-1, len(partners), N)
            owner[0] = -1
            bots, nets = [x for x in partners if not isinstance(x, NetPartner)], [x for x in partners if isinstance(x, NetPartner)]
            sb = np.array([bots.index(partners[o]) if o >= 0 and partners[o] in bots else -1 for o in owner])
            sn = np.array([nets.index(partners[o]) if o >= 0 and partners[o] in nets else -1 for o in owner])
            s = PartnerSeats(partners, np.nonzero(owner < 0)[0], sb, 0, sn if nets else None)
        out.append((s, G, P, 5, 0))
        rows, sb = s.rows.copy(), s.seat_bot.copy()
        sn = None if s.seat_net is None else s.seat_net.copy()
        what = int(rng.randint(6))
        if what == 0:
            rows[rng.randint(len(rows))] = rng.randint(-2, N + 2)
        elif what == 1:
            sb[rng.randint(N)] = rng.randint(-2, nb + 2)
        elif what == 2 and sn is not None:
            sn[rng.randint(N)] = rng.randint(-2, nn + 2)
        elif what == 3 and sn is not None:
            sn, sb = sb, sn
        elif what == 4 and nn:
            bad = fake_net("bad", F_ENV + int(rng.randint(2)), A_ENV + 1)
            partners = [bad if x is s.nets[-1] else x for x in partners]
        else:
            sb = sb[::-1].copy()
        out.append((PartnerSeats(partners, rows, sb, 0, sn), G, P, 5, 0))
    return out


def test_header_agrees_with_the_python_helper_under_sanitizers(tmp_path):
    """partner_layout_verdict_nets of csrc/hsad_partner.h -- the check hsad_actor_create_partnered_nets runs -- compiled alone with the
    address and undefined-behaviour sanitizers into a stand-alone program (tests/partner_net/partner_net_main.cc): verdict and text,
    line for line what PartnerSeats says, over the new refusal table, the old table (through the new function: the old verdicts) and
    seeded valid and spoiled mixed layouts."""
    exe = str(tmp_path / "partner_net_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hanabi_sad_amd", "csrc"), os.path.join(ROOT, "tests", "partner_net", "partner_net_main.cc"),
                           "-o", exe])
    table, G, P = _net_refusals()
    layouts = [(c[1], G, P, 5, int(c[0] == "vdn")) for c in table]
    old = [(c[1], c[2], c[3], c[4], c[5]) for c in _old_refusals()]
    seeded = _seeded_layouts(20261019, 70)
    assert len(seeded) >= 60
    layouts += old + seeded
    want, verdicts = [], []
    for s, g, p, H, vdn in layouts:
        v = s.verdict(g, p, H, vdn, F_ENV, A_ENV)
        verdicts.append(v)
        want += ["%d %d %d" % v, s.explain(v, g, p, F_ENV, A_ENV)]
    assert [v for v in verdicts[len(table):len(table) + len(old)]] == [c[6] for c in _old_refusals()]      # the old verdicts, code for code
    seeded_codes = [v[0] for v in verdicts[len(table) + len(old):]]
    assert seeded_codes.count(0) >= 20, seeded_codes
    assert set(range(12, 20)) <= {v[0] for v in verdicts}                                                   # every new verdict occurs
    text = "%d\n" % len(layouts) + "\n".join(_layout_text(*l) for l in layouts) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]


def test_driver_flags(tmp_path):
    from hanabi_sad_amd.selfplay import init_weights, parse_args, partner_seats
    f = str(tmp_path / "frozen.pthw")
    torch.save(init_weights(F_ENV, 64, A_ENV, 5, 11), f)
    a = parse_args(["--partner", "piers", f, "--num_game", "8"])
    s = partner_seats(a, 8)
    assert [b.name for b in s.bots] == ["piers"] and [n.name for n in s.nets] == ["frozen.pthw"] and not s.nets[0].skip_connect
    assert s.nets[0].dims() == (F_ENV, A_ENV) and s.verdict(8, 2, 5, False, F_ENV, A_ENV) == (0, 0, 0)
    assert (s.seat_net.reshape(8, 2).max(1) == [-1, -1, 0, 0, -1, -1, 0, 0]).all()      # partner j = 1 gets the games bot 1 would get
    s = partner_seats(parse_args(["--partner", f + ":skip", "--partner_seats", "1", "--num_game", "4"]), 4)
    assert s.bots == [] and s.nets[0].skip_connect and s.nets[0].name == "frozen.pthw" and (s.rows % 2 == 1).all()
    with pytest.raises(SystemExit) as e:
        parse_args(["--partner", "piers", str(tmp_path / "missing.pthw")])
    assert "no rule-bot preset of that name" in str(e.value) and "no weight file at" in str(e.value)
    with pytest.raises(SystemExit, match="at most 8 bots and 8 nets"):
        parse_args(["--partner"] + [f] * 9)
    with pytest.raises(SystemExit, match="--method iql"):
        parse_args(["--partner", f, "--method", "vdn"])
    assert parse_args(["--partner"] + [f] * 8 + ["piers"] * 8).partner[0] == f
