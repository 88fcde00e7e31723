"""GPU: positions in and out of an env -- hsad_env_import_state, hsad_env_snapshot, hsad_env_restore (BatchedHanabiEnv.import_state /
snapshot / restore / save / load).  An imported record is the exported one and observes like it; a refused or untaken game is
untouched to the byte; the device's reasons are position.validate's; accepted positions play to a legal end; a restored env goes
on bit for bit, in the same object, a fresh one, another file, other slots.  Shapes: 65 and 33 games (two workgroups, the second
partial, for 64- and 32-game workgroups).

Empty decks.  Under random play only c3r4 (12 cards left after the deal, 2 lives) reaches an empty deck with the game still live:
its deep rollouts do (asserted), and those games are stepped in lockstep with their imported copies until they end.  In full,
small and p5h4 random play loses its lives long before the deck runs out (0 of 200 oracle games each), so for every rule set the
empty-deck checks also run on hand-written endgames (tests/position_cases.endgame), imported, exported and imported again under
another generator."""
import ctypes as C

import numpy as np
import pytest
import torch

from hanabi_sad_amd import position as pos
from tests import position_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q_TERM, Q_SCORE, Q_LIFE, Q_LAST_SCORE, Q_DECK, Q_FW = 0, 2, 3, 5, 7, 8

#        rules   sad    shuffle G   games per workgroup
CASES = [("full", False, False, 65, 64), ("full", True, True, 33, 32), ("small", True, False, 65, 64), ("small", False, True, 33, 32),
         ("c3r4", True, True, 65, 64), ("c3r4", False, False, 33, 32), ("p5h4", True, False, 33, 32), ("p5h4", False, True, 65, 64)]
IDS = ["%s-sad%d-sc%d-G%d" % (c[0], c[1], c[2], c[3]) for c in CASES]
SAD_CASES = [c for c in CASES if c[1]]
SAD_IDS = [i for i, c in zip(IDS, CASES) if c[1]]


def make_env(name, sad, sc, G, gpw, seed, packed=True, **extra):
    from hanabi_sad_amd import BatchedHanabiEnv
    env = BatchedHanabiEnv(G, seed=seed, eps_list=(0.1, 0.05), device=DEV, games_per_workgroup=gpw, sad=sad, shuffle_color=sc,
                           knowledge_mode=0, bomb=0, max_len=pc.MAX_LEN, **pc.RULESETS[name], **extra)
    env.packed = packed
    if packed:
        env.enable_packed((env.F + 63) // 64 * 64, keep_float32=True)
    return env


def rows(env):
    out = {"priv_s": env.priv_s, "legal_move": env.legal_move, "own_hand": env.own_hand, "eps": env.eps}
    if env.packed:
        out.update(priv_bits=env.priv_bits, legal_bits=env.legal_bits, own_bits=env.own_bits, priv_s_bf16=env.priv_s_bf16)
    return out


def clone(d):
    return {k: v.clone() for k, v in d.items()}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def errors(env):
    n, g, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert env.lib.hsad_env_error_count(env.h, C.byref(n), C.byref(g), C.byref(c)) == 0
    return n.value, g.value, c.value


def flags_of(env):
    return dict(max_len=pc.MAX_LEN, shuffle_color=bool(env.config["shuffle_color"]))


def sad_len(env):
    P, H, nC, nR = env.P, env.H, env.colors, env.ranks
    return (P + 4 + P + nC + nR + H + H + nC * nR + 2) if env.sad else 0


def pack_bits(x):
    """float32 [..., F] of 0/1 -> int64 [..., ceil(F / 64)], bit j of word w = column 64 w + j"""
    F = x.shape[-1]
    b = torch.nn.functional.pad((x != 0).to(torch.int64), (0, (-F) % 64)).view(*x.shape[:-1], -1, 64)
    return (b << torch.arange(64, device=x.device)).sum(-1)


def rows_without_sad(env, r, sel):
    """the rows of games sel with the SAD section cut out of every form of priv_s (and shown to be all-zero)"""
    F0 = env.F - sad_len(env)
    out = {k: v[sel] for k, v in r.items() if not k.startswith("priv")}
    ps = r["priv_s"][sel]
    out["priv_s"] = ps[..., :F0]
    assert not bool(ps[..., F0:].any()), "the SAD section of an imported game is not all-zero"
    if "priv_bits" in r:
        assert same(r["priv_bits"][sel], pack_bits(ps)), "the bit words are not the float32 row"
        bf = r["priv_s_bf16"][sel]
        assert same(bf[..., :env.F].float(), ps) and not bool(bf[..., env.F:].any()), "the bf16 row is not the float32 row"
    return out


def conserved(records, rules):
    want = np.asarray(pos.full_deck(rules))
    return all((pc.type_counts(r, rules) == want).all() for r in np.asarray(records))


def scores_are_fireworks(env, sel):
    q = env.query()[sel]
    assert bool((q[:, Q_TERM] == 1).all())
    fw = q[:, Q_FW:Q_FW + 5].sum(1)
    return bool((q[:, Q_SCORE] == fw).all()) and bool((q[:, Q_LAST_SCORE] == fw).all())   # bomb = 0


def lockstep_on_an_empty_deck(src, dst, alive, drawn):
    """games `alive` of src and dst hold the same live position on an empty deck, under different generators.  Nothing is dealt
    from an empty deck, so no draw is consumed (env_logic deals only while the chance player is on turn, advance_player puts it
    there only over a non-empty deck): the same actions keep every word but [73] and every row equal until the games end."""
    alive = alive.clone()
    for it in range(src.P + 1):
        if not bool(alive.any()):
            break
        src.reset()   # finished games elsewhere in the batch restart (a step on one is an error); a live game is left alone
        dst.reset()
        a, ga = src.policy_random(3)
        b, gb = dst.policy_random(3)
        b[alive], gb[alive] = a[alive], ga[alive]
        src.step(a, ga)
        dst.step(b, gb)
        sa, sb = src.export_state(), dst.export_state()
        assert same(sa[alive, 73], drawn[alive]) and not bool(sb[alive, 73].any()), "a draw was consumed on an empty deck"
        sa[:, 73] = 0
        assert same(sa[alive], sb[alive]), "states differ %d steps into the empty deck" % (it + 1)
        ra, rb = rows(src), rows(dst)
        for k2 in ra:
            assert same(ra[k2][alive], rb[k2][alive]), "%s differs %d steps into the empty deck" % (k2, it + 1)
        assert same(src.reward[alive], dst.reward[alive]) and same(src.terminal[alive], dst.terminal[alive])
        alive &= ~src.terminal.bool()
    assert not bool(alive.any()), "a game outlived its turns"


# ---- 1 + 2: the round trip of import, and untouched means untouched -------------------------------------------------------------------
@pytest.mark.parametrize("name,sad,sc,G,gpw", CASES, ids=IDS)
def test_an_imported_record_is_the_exported_one(name, sad, sc, G, gpw):
    rules = pc.RULESETS[name]
    n_empty = 0
    for k in (0, 1, 7, 23, 31, 40):
        src = make_env(name, sad, sc, G, gpw, 8000 + k)
        src.reset()
        if k:
            src.rollout_random(k, 13)
        dst = make_env(name, sad, sc, G, gpw, 777)
        dst.reset()
        dst.rollout_random(3, 5)
        rec = src.export_state()
        done = src.terminal.bool()
        empty = ((rec[:, 61] == 0) & ~done).tolist()     # live on an empty deck: always taken
        games = torch.tensor([g for g in range(G) if g % 7 != 3 or empty[g]], device=DEV)
        taken = torch.zeros(G, dtype=torch.bool, device=DEV)
        taken[games] = True
        before_snap, before_rows, before_term = dst.snapshot(), clone(rows(dst)), dst.terminal.clone()
        status = dst.import_state(rec[games], games, seeds=1000 + games, eps=src.eps[games])
        want = torch.full((G,), -1, dtype=torch.int32, device=DEV)
        want[taken & done], want[taken & ~done] = pos.TERMINAL, 0
        assert same(status, want), "k=%d: status %s, want %s" % (k, status.tolist(), want.tolist())
        host = [pos.validate(r, rules, flags_of(src)) for r in rec.cpu().numpy()]
        assert host == [pos.TERMINAL if t else 0 for t in done.tolist()], "validate disagrees with the env about its own states"
        n_ref = int((taken & done).sum())
        n, g, c = errors(dst)
        assert n == n_ref and (n == 0 or (c == 6 and bool((taken & done)[g]))), (n, g, c, n_ref)
        live = taken & ~done
        assert int(live.sum()) > G // 2
        got = dst.export_state()
        want_rec = rec.clone()
        want_rec[:, 73] = 0
        assert same(got[live], want_rec[live]), "k=%d: the imported state is not the record" % k
        assert not bool(dst.terminal[live].any()) and not bool(dst.reward[live].any())
        s_rows, d_rows = rows(src), rows(dst)
        if sad:
            cut = rows_without_sad(dst, d_rows, live)    # equal outside the section; the section itself all-zero
            for k2 in cut:
                b = s_rows[k2][live][..., :src.F - sad_len(src)] if k2 == "priv_s" else s_rows[k2][live]
                assert same(cut[k2], b), "k=%d: %s of the imported games differs from the source's" % (k, k2)
        else:
            for k2 in d_rows:
                assert same(d_rows[k2][live], s_rows[k2][live]), "k=%d: %s of the imported games differs from the source's" % (k, k2)
        # untaken and refused games: not a byte of the game, not a bit of its rows
        assert same(dst.snapshot()[~live], before_snap[~live]), "k=%d: a game that was not imported changed" % k
        for k2 in d_rows:
            assert same(d_rows[k2][~live], before_rows[k2][~live]), "k=%d: %s of a game that was not imported changed" % (k, k2)
        assert same(dst.terminal[~live], before_term[~live])
        # the source's live games on an empty deck, and their imported copies under another generator
        ed = live & (rec[:, 61] == 0)
        n_empty += int(ed.sum())
        if bool(ed.any()):
            lockstep_on_an_empty_deck(src, dst, ed, rec[:, 73].clone())
        # the imported games play on like any other: no errors, every card accounted for, scores what the fireworks say
        for it in range(6):
            dst.reset()
            a, ga = dst.policy_random(31)
            dst.step(a, ga)
            assert conserved(dst.export_state().cpu(), rules), "k=%d: a card went missing %d steps after the import" % (k, it + 1)
        dst.playout_random(120, 9)
        assert conserved(dst.export_state().cpu(), rules)
        assert scores_are_fireworks(dst, torch.ones(G, dtype=torch.bool, device=DEV))
        assert errors(dst)[0] == 0 and errors(src)[0] == 0
        src.close()
        dst.close()
    if name == "c3r4":
        assert n_empty >= 1, "the deep rollouts of c3r4 should leave a live game on an empty deck"


# ---- 3: the device's reasons are validate's ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sad,sc,G,gpw", CASES, ids=IDS)
def test_status_is_what_validate_says(name, sad, sc, G, gpw):
    rules = pc.RULESETS[name]
    env = make_env(name, sad, sc, G, gpw, 4321)
    env.reset()
    env.rollout_random(2, 3)
    table = pc.corruptions(rules, sc)
    good = [pc.opening(rules, info=0).to_record(), pc.endgame(rules).to_record(), pc.opening(rules, life=1).to_record()]
    recs = []
    for i in range(G):   # a valid record between the bad ones, the whole table at least once where G allows
        recs.append(good[(i // 2) % 3] if i % 2 == 0 else table[(i // 2) % len(table)][1])
    want = [pos.validate(r, rules, flags_of(env)) for r in recs]
    assert [w for w in want[1::2]] == [table[(i // 2) % len(table)][2] for i in range(1, G, 2)] and not any(want[0::2])
    before_snap, before_rows = env.snapshot(), clone(rows(env))
    status = env.import_state(np.stack(recs), seeds=np.arange(G) + 5)
    assert status.tolist() == want, [(i, s, w) for i, (s, w) in enumerate(zip(status.tolist(), want)) if s != w]
    bad = torch.tensor([w != 0 for w in want], device=DEV)
    n, g, c = errors(env)
    assert n == int(bad.sum()) and c == 6 and bool(bad[g])
    with pytest.raises(Exception, match="position refused"):   # what check_errors makes of code 6
        env.import_state(table[0][1], games=[2], seeds=[1])
        env.check_errors()
    got = env.export_state()
    for i in range(0, G, 2):
        w = torch.from_numpy(recs[i]).to(DEV)
        w[73] = 0
        assert same(got[i], w), "valid record %d of the mixed batch was not imported" % i
    assert same(env.snapshot()[bad], before_snap[bad]), "a refused game changed"
    r = rows(env)
    for k2 in r:
        assert same(r[k2][bad], before_rows[k2][bad]), "%s of a refused game changed" % k2
    # one refused record alone: the log names the game
    st = env.import_state(table[3][1], games=[G - 1], seeds=[1])
    assert st[G - 1].item() == table[3][2] and int((st == -1).sum()) == G - 1
    assert errors(env) == (1, G - 1, 6)
    # seeds = None: a started game keeps its generator, a game that was never started has none
    fresh = make_env(name, sad, sc, G, gpw, 99)
    st = fresh.import_state(good[0], games=[1])
    assert st[1].item() == pos.NO_GENERATOR and errors(fresh) == (1, 1, 6)
    draws = env.query()[:, 13].clone()
    st = env.import_state(good[1], games=[4])
    assert st[4].item() == 0 and same(env.query()[:, 13], draws)
    env.close()
    fresh.close()


# ---- 4: accepted positions play -------------------------------------------------------------------------------------------------------------
def built_positions(rules):
    P, H, nC, nR = rules["players"], rules["hand_size"], rules["colors"], rules["ranks"]
    out = []
    for t in range(1, P + 1):       # an empty deck with t turns left: the seats that moved on it hold one card fewer
        mover = t % P
        out.append(("empty deck, %d turns" % t, pc.endgame(rules, turns_to_play=t, mover=mover,
                                                           short=[(mover - k) % P for k in range(1, P - t + 1)], life=rules["max_life_tokens"])))
    out.append(("no hint token", pc.opening(rules, info=0)))
    out.append(("every hint token", pc.opening(rules)))
    out.append(("one life", pc.opening(rules, life=1)))
    out.append(("a short hand on the mover", pc.endgame(rules, turns_to_play=P - 1, mover=0, short=[0])))
    # every firework one short of complete: the top cards in the hands
    cards = pc.all_cards(rules)
    for c in range(nC):
        for r in range(nR - 1):
            cards.remove((c, r))
    cards.sort(key=lambda cr: (-cr[1], cr[0]))
    out.append(("one card from every firework", pos.Position(rules, [cards[p * H:(p + 1) * H] for p in range(P)], fireworks=[nR - 1] * nC)))
    return out


@pytest.mark.parametrize("name,sad,sc,G,gpw", CASES, ids=IDS)
def test_accepted_positions_play(name, sad, sc, G, gpw):
    rules = pc.RULESETS[name]
    P, H, nC = rules["players"], rules["hand_size"], rules["colors"]
    built = built_positions(rules)
    recs = np.stack([built[i % len(built)][1].to_record() for i in range(G)])
    for what, p in built:
        assert pos.validate(p.to_record(), rules, dict(max_len=pc.MAX_LEN, shuffle_color=sc)) == 0, what
    env = make_env(name, sad, sc, G, gpw, 600)
    env.reset()
    status = env.import_state(recs, seeds=np.arange(G) * 3 + 1)
    assert not bool(status.any()), [(built[i % len(built)][0], pos.explain(s)) for i, s in enumerate(status.tolist()) if s]
    assert errors(env)[0] == 0
    # a hint that would touch nothing is not offered: the colour hints to the next seat are exactly the colours it holds
    for i, (what, p) in enumerate(built):
        held = {c.colour for c in p.hands[(p.mover + 1) % P]}
        offered = env.legal_move[i, p.mover, 2 * H:2 * H + nC].tolist()
        assert offered == [float(p.info > 0 and c in held) for c in range(nC)], what
        assert env.legal_move[i, p.mover, :H].tolist() == [float(p.info < rules["max_information_tokens"] and s < len(p.hands[p.mover])) for s in range(H)], what
    start = env.snapshot()
    seen_end = torch.zeros(G, dtype=torch.bool, device=DEV)
    for it in range(40):
        a, ga = env.policy_random(77)
        env.step(a, ga)
        assert conserved(env.export_state().cpu(), rules), "a card went missing at step %d" % (it + 1)
        ended = env.terminal.bool()
        if bool(ended.any()):
            assert scores_are_fireworks(env, ended)
        seen_end |= ended
        env.reset()   # finished games start afresh (a step on a finished game is an error) and play on
    assert int(seen_end.sum()) > G // 2 and errors(env)[0] == 0
    assert not bool(env.restore(start).any())
    env.playout_random(120, 5)
    assert scores_are_fireworks(env, torch.ones(G, dtype=torch.bool, device=DEV))
    assert conserved(env.export_state().cpu(), rules) and errors(env)[0] == 0
    env.close()


@pytest.mark.parametrize("name,sad,sc,G,gpw", CASES, ids=IDS)
def test_an_empty_deck_position_needs_no_generator(name, sad, sc, G, gpw):
    """nothing is dealt from an empty deck, so no draw is consumed: an imported copy under another generator stays equal to its
    source in every word but [73] and in every row until the game ends"""
    rules = pc.RULESETS[name]
    P = rules["players"]
    ends = [p for what, p in built_positions(rules) if what.startswith("empty deck")]
    recs = np.stack([ends[i % len(ends)].to_record() for i in range(G)])
    a_env, b_env = make_env(name, sad, sc, G, gpw, 1), make_env(name, sad, sc, G, gpw, 2)
    a_env.reset()
    b_env.reset()
    assert not bool(a_env.import_state(recs, seeds=np.arange(G) + 10).any())
    assert not bool(b_env.import_state(a_env.export_state(), seeds=np.arange(G) + 5000, eps=a_env.eps).any())
    alive = torch.ones(G, dtype=torch.bool, device=DEV)
    for it in range(P):
        a, ga = a_env.policy_random(3)
        b, gb = b_env.policy_random(3)    # (a restarted game has its own deal and needs its own legal action)
        assert same(a[alive], b[alive]) and same(ga[alive], gb[alive]), "equal positions and counters, different actions"
        a_env.step(a, ga)
        b_env.step(b, gb)
        sa, sb = a_env.export_state(), b_env.export_state()
        assert same(sa[alive, 73], torch.zeros_like(sa[alive, 73])) and same(sb[alive, 73], sa[alive, 73]), "a draw was consumed on an empty deck"
        assert same(sa[alive], sb[alive]), "states differ after %d steps" % (it + 1)
        ra, rb = rows(a_env), rows(b_env)
        for k2 in ra:
            assert same(ra[k2][alive], rb[k2][alive]), "%s differs after %d steps" % (k2, it + 1)
        assert same(a_env.reward[alive], b_env.reward[alive]) and same(a_env.terminal[alive], b_env.terminal[alive])
        alive &= ~a_env.terminal.bool()
        a_env.reset()   # the finished games restart, each from its own generator: they leave the comparison
        b_env.reset()
    assert not bool(alive.any()), "a game outlived its turns"
    assert errors(a_env)[0] == 0 and errors(b_env)[0] == 0
    a_env.close()
    b_env.close()


# ---- 5 + 6: a restored env goes on bit for bit ----------------------------------------------------------------------------------------------
def mixed_history(env):
    """rollouts and single steps, games finishing and restarting on the way; stops on a step that finished some game"""
    env.reset()
    env.rollout_random(9, 3)
    for it in range(60):
        env.reset()
        a, ga = env.policy_random(8)
        env.step(a, ga)
        if it >= 2 and bool(env.terminal.any()):
            break


def five_steps(env):
    out = []
    for _ in range(5):
        env.reset()
        a, ga = env.policy_random(55)
        env.step(a, ga)
        out.append(dict(clone(rows(env)), a=a.clone(), ga=ga.clone(), reward=env.reward.clone(), terminal=env.terminal.clone(),
                        state=env.export_state(), history=env.deck_history()[0]))
    return out


def assert_same_runs(x, y, what):
    assert len(x) == len(y)
    for i, (p, q) in enumerate(zip(x, y)):
        for k2 in p:
            if k2 in q:
                assert same(p[k2], q[k2]), "%s: %s differs at iteration %d" % (what, k2, i + 1)


@pytest.mark.parametrize("name,sad,sc,G,gpw", SAD_CASES, ids=SAD_IDS)
def test_restore_continues_bit_for_bit(name, sad, sc, G, gpw, tmp_path):
    env = make_env(name, sad, sc, G, gpw, 3100)
    mixed_history(env)
    q = env.query()
    assert bool((q[:, Q_TERM] == 1).any()) and bool((q[:, Q_TERM] == 0).any()), "the history should leave finished and live games"
    snap = env.snapshot()
    assert snap.shape == (G, env.snapshot_record_bytes()) and snap.dtype == torch.uint8
    at = dict(clone(rows(env)), terminal=env.terminal.clone(), state=env.export_state(), history=env.deck_history()[0])
    first = five_steps(env)

    def never_restored():
        """another env brought to the very state of the snapshot by the same history: what it does next is the reference"""
        e = make_env(name, sad, sc, G, gpw, 3100)
        mixed_history(e)
        assert same(e.snapshot(), snap), "the same history did not lead to the same snapshot"
        return e

    def after_rollout(e, chunk):
        e.set_rollout_chunk(chunk)
        e.rollout_random(4, 21)
        return [dict(clone(rows(e)), a=e.a.clone(), ga=e.greedy_a.clone(), reward=e.reward.clone(), terminal=e.terminal.clone(),
                     state=e.export_state(), snap=e.snapshot())]

    def after_playout(e):
        # (a playout leaves a finished game alone, its rows of a / greedy_a included: those hold whatever was there before)
        live = at["terminal"] == 0
        e.playout_random(100, 33)
        return [dict(a=e.a[live].clone(), ga=e.greedy_a[live].clone(), terminal=e.terminal.clone(), state=e.export_state(), q=e.query(),
                     snap=e.snapshot())]

    def back(e):
        status = e.restore(snap)
        assert not bool(status.any()), status.tolist()
        now = dict(rows(e), terminal=e.terminal, state=e.export_state(), history=e.deck_history()[0])
        for k2 in now:
            assert same(now[k2], at[k2]), "%s after restore is not what it was at the snapshot" % k2
        assert not bool(e.reward.any())
        assert same(e.snapshot(), snap), "a snapshot of the restored env is not the snapshot"

    back(env)
    assert_same_runs(five_steps(env), first, "same env")
    for chunk in (0, 4):    # one launch per iteration (the default), and persistent launches: pipeline, delta and compaction as they default
        ref_env = never_restored()
        ref = after_rollout(ref_env, chunk)
        ref_env.close()
        for _ in range(2):
            back(env)
            assert_same_runs(after_rollout(env, chunk), ref, "rollout_random, chunk %d" % chunk)
    env.set_rollout_chunk(0)
    ref_env = never_restored()
    ref = after_playout(ref_env)
    ref_env.close()
    for _ in range(2):
        back(env)
        assert_same_runs(after_playout(env), ref, "playout_random")

    # another object of the same configuration
    other = make_env(name, sad, sc, G, gpw, 17)
    other.reset()
    back(other)
    assert_same_runs(five_steps(other), first, "fresh env")
    other.close()

    # another file: save -> load (float32 rows only: load binds no packed outputs)
    back(env)
    path = str(tmp_path / "env.pt")
    env.save(path)
    from hanabi_sad_amd import BatchedHanabiEnv
    loaded = BatchedHanabiEnv.load(path, device=DEV)
    loaded.packed = False
    assert loaded.config == env.config and loaded.G == G
    for k2, v in rows(loaded).items():
        assert same(v, at[k2]), "%s of the loaded env is not what was saved" % k2
    assert same(loaded.snapshot(), snap)
    assert_same_runs(five_steps(loaded), first, "loaded env")
    loaded.close()

    # other slots: what restore puts into slot j is what fork_from puts there
    back(env)
    rng = np.random.RandomState(5)
    idx = rng.randint(0, G, size=G).astype(np.int32)
    idx[0], idx[1], idx[2], idx[3], idx[G - 1] = -1, G - 1, G - 1, G + 4, 0
    d1, d2 = make_env(name, sad, sc, G, gpw, 40), make_env(name, sad, sc, G, gpw, 40)
    for d in (d1, d2):
        d.reset()
        d.rollout_random(3, 6)
    status = d1.restore(snap, idx)
    d2.fork_from(env, idx)
    assert status.tolist() == [0 if 0 <= i < G else -1 for i in idx.tolist()]
    assert errors(d1) == (1, 3, 4) and errors(d2) == (1, 3, 4)
    assert same(d1.export_state(), d2.export_state())
    for k2, v in rows(d1).items():
        assert same(v, rows(d2)[k2]), "%s: restore into other slots is not fork_from" % k2
    assert same(d1.terminal, d2.terminal) and same(d1.snapshot(), d2.snapshot())
    for e in (env, d1, d2):
        assert errors(e)[0] == 0
        e.close()


# ---- 6 (scripts) + 7: a scripted env restores scripted; what restore refuses ------------------------------------------------------------------
def scripted_env(name, sad, sc, G, gpw, seed):
    env = make_env(name, sad, sc, G, gpw, seed)
    env.reset()
    env.rollout_random(6, 3)
    env.reset()
    hist, n = env.deck_history()
    env.rewind_scripted(hist, n)       # every game again from its own deal, now dealt from the script
    for _ in range(2):
        a, ga = env.policy_random(8)
        env.step(a, ga)
    return env, n


@pytest.mark.parametrize("name,sad,sc,G,gpw", [CASES[1], CASES[4], CASES[5]], ids=[IDS[1], IDS[4], IDS[5]])
def test_a_scripted_env_restores_scripted(name, sad, sc, G, gpw):
    env, _ = scripted_env(name, sad, sc, G, gpw, 2200)
    snap = env.snapshot()
    twin = make_env(name, sad, sc, G, gpw, 9)
    twin.reset()
    plain = twin.snapshot_record_bytes()
    assert snap.shape[1] == plain + 56
    assert not bool(twin.restore(snap).any())
    assert twin.snapshot_record_bytes() == plain + 56 and same(twin.snapshot(), snap)
    dealt = False
    for it in range(8):
        # no reset (it would drop the scripts).  A game that has ended is stepped all the same: the env logs it (code 3) and leaves
        # it alone, in both envs alike
        deck = env.query()[:, Q_DECK].clone()
        a, ga = env.policy_random(12)
        b, gb = twin.policy_random(12)    # the restored policy counter and legal masks: the twin picks what the source picks
        assert same(a, b) and same(ga, gb), "the restored env chose other actions at step %d" % (it + 1)
        env.step(a, ga)
        twin.step(b, gb)
        for k2, v in rows(env).items():
            assert same(v, rows(twin)[k2]), "%s differs %d steps after the restore" % (k2, it + 1)
        assert same(env.export_state(), twin.export_state()) and same(env.reward, twin.reward) and same(env.terminal, twin.terminal)
        dealt |= bool((env.query()[:, Q_DECK] < deck).any())
    assert dealt, "no card was dealt from the script"
    assert same(env.query()[:, 13], twin.query()[:, 13]), "generator draws differ: a scripted deal consumed one"
    (n1, _, c1), (n2, _, c2) = errors(env), errors(twin)
    assert n1 == n2 and c1 == c2 and c1 in (0, 3)
    assert same(env.snapshot(), twin.snapshot())
    env.close()
    twin.close()


@pytest.mark.parametrize("name,sad,sc,G,gpw", [CASES[1], CASES[4], CASES[5]], ids=[IDS[1], IDS[4], IDS[5]])
def test_restore_refuses(name, sad, sc, G, gpw, tmp_path):
    from hanabi_sad_amd import BatchedHanabiEnv, _lib
    env, n_script = scripted_env(name, sad, sc, G, gpw, 2300)
    P, H = env.P, env.H
    npl = 10 + 6 * P
    off_sc = npl + 1 + 624 + 13
    snap = env.snapshot()
    assert snap.shape[1] == 4 * (off_sc + 14 + 2 * P)
    q, state = env.query().cpu().numpy(), env.export_state().cpu().numpy()
    di = env.max_deck_size() - q[:, Q_DECK]
    ok = (q[:, Q_TERM] == 0) & (n_script.cpu().numpy() > di) & (q[:, Q_DECK] > 4)
    cand = [int(g) for g in np.nonzero(ok)[0]]
    empty_type = [g for g in cand if (state[g, 0:25] == 0).any()]     # the deck has run out of some card type (or never had it)
    assert empty_type and len(cand) >= 5, "the fixture should leave five live games with scripted deals to come"
    picks = [g for g in cand if g != empty_type[0]][:4] + [empty_type[0]]
    bad = snap.clone()
    w = bad.view(torch.int32)
    g0, g1, g2, g3, g4 = picks
    w[g0, 0] = (w[g0, 0] & ~3) | ((w[g0, 0] + 1) & 3)                 # one deck count: a copy too many or too few
    w[g1, 10] = w[g1, 10] | (7 << 25)                                  # seat 0's hand of length 7
    w[g2, 5] = w[g2, 5] | (3 << 22)                                    # three look-ahead words
    bad[g3, 4 * off_sc] = 31                                           # the script's first card is no card
    absent = int(np.nonzero(state[g4, 0:25] == 0)[0][0])
    bad[g4, 4 * off_sc + int(di[g4])] = absent                         # the next scripted deal is a card the deck has run out of
    want = {g0: pos.CONSERVATION, g1: pos.HANDS, g2: pos.LOOKAHEAD, g3: pos.HISTORY, g4: pos.SCRIPT}
    for _ in range(2):     # move on, so that a restored game shows (a finished game is logged, code 3, and left alone)
        a, ga = env.policy_random(8)
        env.step(a, ga)
    assert errors(env)[2] in (0, 3)
    before = env.snapshot()
    assert not same(before, snap)
    status = env.restore(bad)
    assert status.tolist() == [want.get(g, 0) for g in range(G)], [(g, pos.explain(s)) for g, s in enumerate(status.tolist()) if s]
    n, g, c = errors(env)
    assert n == 5 and c == 6 and g in want
    after = env.snapshot()
    refused = torch.tensor([g in want for g in range(G)], device=DEV)
    assert same(after[refused], before[refused]), "a refused game changed"
    assert same(after[~refused], snap[~refused]), "a neighbour of a refused game was not restored"

    # host-side refusals: nothing is launched, nothing changes
    lib = env.lib
    st = torch.zeros(G, dtype=torch.int32, device=DEV)
    rc = lib.hsad_env_restore(env.h, snap.data_ptr(), int(snap.shape[1]) - 4, G, None, st.data_ptr(), env._stream())
    assert rc == -1 and b"bytes" in lib.hsad_last_error()   # HSAD_ERR_INVALID
    assert lib.hsad_env_restore(env.h, snap.data_ptr(), int(snap.shape[1]), G - 1, None, st.data_ptr(), env._stream()) == -1
    assert same(env.snapshot(), after)
    path = str(tmp_path / "env.pt")
    env.save(path)
    d = torch.load(path)
    for name2, edit in (("version", lambda x: x.update(version=d["version"] + 1)),
                        ("truncated", lambda x: x.update(snapshot=d["snapshot"][:, :-4].clone())),
                        ("short", lambda x: x.update(snapshot=d["snapshot"][:-1].clone())),
                        ("hand size", lambda x: x.update(config=dict(d["config"], hand_size=H - 1))),
                        ("players", lambda x: x.update(config=dict(d["config"], players=P + 1)))):
        x = dict(d)
        edit(x)
        p2 = str(tmp_path / ("bad_%s.pt" % name2.replace(" ", "_")))
        torch.save(x, p2)
        with pytest.raises(ValueError):
            BatchedHanabiEnv.load(p2, device=DEV)
    ok_env = BatchedHanabiEnv.load(path, device=DEV)
    assert same(ok_env.snapshot(), after)
    ok_env.close()
    env.close()
