"""CPU: the seat layouts of a partnered actor (actor.PartnerSeats), every host refusal with its message, the validation header
csrc/hsad_partner.h under the sanitizers against the Python restatement, and the driver's new flags."""
import os
import subprocess

import numpy as np
import pytest

from hanabi_sad_amd import rulebot as rbt
from hanabi_sad_amd.actor import PartnerSeats, PartnerSeatsError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(6, 2), (7, 3), (5, 5)]
BOTS = [rbt.PRESETS["cautious"], rbt.PRESETS["piers"], rbt.PRESETS["flawed"]]


def _check_layout(s, G, P, n_bot):
    rows, sb = s.rows, s.seat_bot.reshape(G, P)
    assert rows.dtype == np.int32 and s.seat_bot.dtype == np.int32
    assert (np.diff(rows) > 0).all()                                   # ascending
    assert rows.shape == (G,) and (rows // P == np.arange(G)).all()    # one learner row per game
    want = np.zeros(G * P, dtype=bool)
    want[rows] = True
    assert ((s.seat_bot == -1) == want).all()                          # -1 exactly on the learner's rows
    assert ((s.seat_bot[~want] >= 0) & (s.seat_bot[~want] < n_bot)).all()
    for g in range(G):                                                 # one bot per game
        assert len(set(sb[g][sb[g] >= 0].tolist())) == 1
    assert s.verdict(G, P) == (0, 0, 0)
    return rows % P, np.array([sb[g][sb[g] >= 0][0] for g in range(G)])


@pytest.mark.parametrize("G,P", SHAPES)
@pytest.mark.parametrize("n_bot", [1, 2, 3])
def test_alternate_layout(G, P, n_bot):
    """alternate: the learner on seat g % P, the others of game g on bot (g // P) % n_bot.  The bots take turns by BLOCKS of P
    consecutive games (so that every bot meets the learner on every seat): the balance that formula gives, and that is asserted, is
    within one block between any two bots -- and within one game where the blocks divide evenly."""
    s = PartnerSeats.alternate(G, P, BOTS[:n_bot])
    seat, bot = _check_layout(s, G, P, n_bot)
    assert (seat == np.arange(G) % P).all() and (bot == (np.arange(G) // P) % n_bot).all()
    seats = np.bincount(seat, minlength=P)
    assert seats.max() - seats.min() <= 1                              # seats balanced within one
    blocks = np.bincount(bot[::P], minlength=n_bot)                    # blocks of P games each bot plays
    assert blocks.max() - blocks.min() <= 1
    games = np.bincount(bot, minlength=n_bot)
    assert games.max() - games.min() <= P
    if G % (P * n_bot) == 0:
        assert games.max() == games.min()


@pytest.mark.parametrize("G,P", SHAPES)
@pytest.mark.parametrize("n_bot", [1, 2, 3])
def test_fixed_seat_layout(G, P, n_bot):
    for seat_no in range(P):
        s = PartnerSeats.fixed_seat(G, P, seat_no, BOTS[:n_bot])
        seat, bot = _check_layout(s, G, P, n_bot)
        assert (seat == seat_no).all()
        games = np.bincount(bot, minlength=n_bot)
        assert games.max() - games.min() <= 1                          # bots balanced within one game
    with pytest.raises(PartnerSeatsError, match="seat = %d" % P):
        PartnerSeats.fixed_seat(G, P, P, BOTS[:n_bot])


def _refusals(G=4, P=2):
    """(what, PartnerSeats, G, P, hand_size, vdn, verdict, text the message must hold)"""
    ok = PartnerSeats.alternate(G, P, BOTS[:2])
    rows, sb = ok.rows.copy(), ok.seat_bot.copy()      # rows 0 3 4 7
    out = [("vdn", ok, G, P, 5, 1, (1, 0, 1), "cfg->vdn = 1"),
           ("players", PartnerSeats.alternate(2, 6, BOTS[:1]), 2, 6, 5, 0, (2, 0, 6), "players = 6"),
           ("no rows", PartnerSeats(BOTS[:1], [], np.zeros(G * P)), G, P, 5, 0, (3, 0, 0), "M = 0"),
           ("too many rows", PartnerSeats(BOTS[:1], np.arange(G * P + 1), np.zeros(G * P)), G, P, 5, 0, (3, 0, G * P + 1), "M = %d" % (G * P + 1))]
    r = rows.copy(); r[3] = G * P
    out.append(("row out of range", PartnerSeats(BOTS[:2], r, sb), G, P, 5, 0, (4, 3, G * P), "rows[3] = %d" % (G * P)))
    r = rows.copy(); r[0] = -1
    out.append(("negative row", PartnerSeats(BOTS[:2], r, sb), G, P, 5, 0, (4, 0, -1), "rows[0] = -1"))
    r = rows.copy(); r[1], r[2] = rows[2], rows[1]
    out.append(("unsorted", PartnerSeats(BOTS[:2], r, sb), G, P, 5, 0, (5, 2, 3), "rows[2] = 3 is not above rows[1]"))
    r = rows.copy(); r[2] = rows[1]
    out.append(("duplicate", PartnerSeats(BOTS[:2], r, sb), G, P, 5, 0, (5, 2, 3), "rows[2] = 3 is not above rows[1]"))
    out.append(("no bot for the partner rows", PartnerSeats([], rows, sb), G, P, 5, 0, (6, 0, 0), "n_bot = 0"))
    out.append(("nine bots", PartnerSeats([BOTS[0]] * 9, rows, sb), G, P, 5, 0, (6, 0, 9), "n_bot = 9"))
    out.append(("empty list", PartnerSeats([BOTS[0], rbt.RuleBot([])], rows, sb), G, P, 5, 0, (7, 1, 0), "bot 1 has 0 rules"))
    out.append(("nine rules", PartnerSeats([rbt.RuleBot([rbt.PLAY_CERTAIN] * 9), BOTS[0]], rows, sb), G, P, 5, 0, (7, 0, 9), "bot 0 has 9 rules"))
    out.append(("unknown code", PartnerSeats([BOTS[0], rbt.RuleBot([rbt.PLAY_CERTAIN, 14])], rows, sb), G, P, 5, 0, (8, 1, 0),
                "bot 1 names an unknown rule code"))
    out.append(("k out of range", PartnerSeats([BOTS[0], rbt.RuleBot([(rbt.PLAY_PROBABLE, 101)])], rows, sb), G, P, 5, 0, (9, 1, 0), "bot 1: k must be"))
    b = sb.copy(); b[3] = 1
    out.append(("learner row with a bot", PartnerSeats(BOTS[:2], rows, b), G, P, 5, 0, (10, 3, 1), "seat_bot[3] = 1 on a learner row"))
    b = sb.copy(); b[5] = -1
    out.append(("partner row without a bot", PartnerSeats(BOTS[:2], rows, b), G, P, 5, 0, (11, 5, -1), "seat_bot[5] = -1 on a partner row"))
    b = sb.copy(); b[6] = 2
    out.append(("partner row names no bot", PartnerSeats(BOTS[:2], rows, b), G, P, 5, 0, (11, 6, 2), "seat_bot[6] = 2 on a partner row"))
    return out


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0].replace(" ", "_"))
def test_every_host_refusal_names_the_entry(case):
    what, s, G, P, H, vdn, verdict, text = case
    assert s.verdict(G, P, H, vdn) == verdict, what
    with pytest.raises(PartnerSeatsError) as e:
        s.check(G, P, H, vdn)
    assert text in str(e.value) and e.value.verdict == verdict


def test_all_rows_without_bots_is_a_layout():
    s = PartnerSeats([], np.arange(10), np.full(10, -1))
    assert s.verdict(5, 2) == (0, 0, 0)


def _layout_text(s, G, P, H, vdn):
    t = ["%d %d %d %d %d %d" % (G, P, H, int(vdn), s.M, len(s.bots)), " ".join(str(int(r)) for r in s.rows)]
    for bot in s.bots:
        t.append(" ".join([str(len(bot.rules))] + ["%d %d" % ck for ck in bot.rules[:rbt.MAX_RULES]]))
    t.append(" ".join(str(int(b)) for b in s.seat_bot))
    return "\n".join(t)


def _seeded_layouts(seed, n):
    """valid layouts of random shapes, and the same with one random entry spoiled"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        G, P, n_bot = int(rng.randint(1, 9)), int(rng.randint(2, 6)), int(rng.randint(1, 4))
        s = PartnerSeats.alternate(G, P, BOTS[:n_bot]) if k % 2 else PartnerSeats.fixed_seat(G, P, int(rng.randint(P)), BOTS[:n_bot])
        if k % 5 == 0:       # several learner seats in a game
            mask = rng.rand(G * P) < 0.5
            mask[0] = True
            sb = np.where(mask, -1, rng.randint(0, n_bot, G * P))
            s = PartnerSeats(BOTS[:n_bot], np.nonzero(mask)[0], sb) if not mask.all() else PartnerSeats([], np.arange(G * P), sb)
        out.append((s, G, P, 5, 0))
        rows, sb = s.rows.copy(), s.seat_bot.copy()
        what = int(rng.randint(4))
        if what == 0:
            rows[rng.randint(len(rows))] = rng.randint(-2, G * P + 2)
        elif what == 1:
            sb[rng.randint(G * P)] = rng.randint(-2, n_bot + 2)
        elif what == 2 and len(rows) > 1:
            rows = rows[rng.permutation(len(rows))]
        else:
            sb = sb[::-1].copy()
        out.append((PartnerSeats(s.bots, rows, sb), G, P, 5, 0))
    return out


def test_header_agrees_with_the_python_helper_under_sanitizers(tmp_path):
    """csrc/hsad_partner.h -- the check hsad_actor_create_partnered runs -- compiled alone with the address and undefined-behaviour
    sanitizers into a stand-alone program (tests/partner/partner_main.cc): verdict and text, line for line what PartnerSeats says,
    over the refusal table and seeded valid and spoiled layouts."""
    exe = str(tmp_path / "partner_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hanabi_sad_amd", "csrc"), os.path.join(ROOT, "tests", "partner", "partner_main.cc"),
                           "-o", exe])
    layouts = [(c[1], c[2], c[3], c[4], c[5]) for c in _refusals()] + _seeded_layouts(20261019, 60)
    layouts.append((PartnerSeats([], np.arange(10), np.full(10, -1)), 5, 2, 5, 0))
    want = []
    for s, G, P, H, vdn in layouts:
        v = s.verdict(G, P, H, vdn)
        want += ["%d %d %d" % v, s.explain(v, G, P)]
    assert sum(1 for w in want[::2] if w == "0 0 0") >= 20 and len({w.split()[0] for w in want[::2]}) == 12   # every verdict occurs
    text = "%d\n" % len(layouts) + "\n".join(_layout_text(*l) for l in layouts) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]


def test_driver_flags():
    from hanabi_sad_amd.selfplay import parse_args, partner_seats
    a = parse_args(["--partner", "cautious", "piers", "--num_game", "6"])
    assert a.partner == ["cautious", "piers"] and a.partner_seats == "alternate"
    s = partner_seats(a, 6)
    assert [b.name for b in s.bots] == ["cautious", "piers"] and s.verdict(6, 2) == (0, 0, 0)
    assert (s.rows == PartnerSeats.alternate(6, 2, s.bots).rows).all()
    a = parse_args(["--partner", "piers", "--partner_seats", "1", "--num_game", "6"])
    assert (partner_seats(a, 6).rows % 2 == 1).all()
    assert partner_seats(parse_args([]), 6) is None and parse_args([]).partner == []
    for bad in (["--partner", "piers", "--method", "vdn"], ["--partner", "nobody"], ["--partner", "piers", "--partner_seats", "2"],
                ["--partner", "piers", "--native_actor", "0"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_python_actor_path_refuses_partners():
    """DeviceActor(native=False, partners=...) is refused by name before anything touches a device"""
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.actor import DeviceActor

    class Env:
        G, P, H, F, A, device, knowledge_mode = 4, 2, 5, 838, 21, "cpu", 0

    class Agent:
        cached_q = True

        def get_h0(self, n):
            return {}
    with pytest.raises(_lib.HsadError, match="PartnerSeats need the library's loop body"):
        DeviceActor(Env(), Agent(), None, 3, 0.99, 0.9, 80, native=False, partners=PartnerSeats.alternate(4, 2, BOTS[:1]))
