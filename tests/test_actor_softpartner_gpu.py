"""GPU: a frozen network partner that plays its softmax policy (actor.NetPartner(temperature=),
hsad_actor_set_partner_temperature).  One partnered actor, G = 64 two-player games, the learner and the frozen net alternating seats,
12 steps (max_len 8: every game ends once inside them, so every learner row stores one sequence).  At temperature 0 the actor is the one
built without the keyword, bit for bit; at temperature 1 the partner leaves its greedy move on some rows, the replay still holds the
learner's rows only, and one seed gives one run."""
import pytest
import torch

from tests.test_actor_netpartner_gpu import frozen_net
from tests.test_actor_partner_gpu import BOT_SEED, FULL, Side, make_actor

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
G, P, STEPS, MAX_LEN = 64, 2, 12, 8


class Run:
    """12 steps of a partnered actor; kw: the keywords of NetPartner under test"""

    def __init__(self, nets, **kw):
        from hanabi_sad_amd.actor import NetPartner, PartnerSeats
        self.side = Side(G, P, 5, 1, FULL, MAX_LEN, nets=nets)
        self.partner = frozen_net(self.side, 21)
        self.seats = PartnerSeats.alternate(G, P, [NetPartner(self.partner, name="frozen", **kw)], bot_seed=BOT_SEED)
        ac = make_actor(self.side, self.seats)
        self.a, self.greedy = [], []
        for _ in range(STEPS):
            ac.step()
            last = ac.last_reply
            self.a.append(last["a"].clone())
            self.greedy.append(last["greedy_a"].clone())
        torch.cuda.synchronize()
        self.state = [x.clone() for x in ac.state]
        self.pstate = [x.clone() for x in ac.partner_state(0)]
        self.num_act = ac.num_act
        self.side.env.check_errors()
        ac.close()

    def same_as(self, other):
        assert all(torch.equal(x, y) for x, y in zip(self.a, other.a)), "actions differ"
        assert all(torch.equal(x, y) for x, y in zip(self.greedy, other.greedy)), "greedy actions differ"
        assert all(torch.equal(x, y) for x, y in zip(self.state, other.state)), "the learner's state differs"
        assert all(torch.equal(x, y) for x, y in zip(self.pstate, other.pstate)), "the partner's state differs"
        ra, rb = self.side.replay, other.side.replay
        assert (ra.size(), ra.num_add()) == (rb.size(), rb.num_add()) and ra.size() > 0
        for i in range(ra.size()):
            fa, fb = ra.get(i), rb.get(i)
            for k in fa[0]:
                assert torch.equal(fa[0][k], fb[0][k]), (i, k)
            for x, y, what in zip(fa[1:], fb[1:], ("reward", "terminal", "bootstrap", "seq_len")):
                assert torch.equal(x, y), (i, what)
        assert ra.priority_sum()[0] == rb.priority_sum()[0]


@pytest.fixture(scope="module")
def plain():
    return Run(None)


def test_temperature_zero_is_the_actor_without_the_keyword(plain):
    Run(plain.side.nets, temperature=0.0).same_as(plain)


def test_a_warm_partner_samples_and_stays_out_of_the_replay(plain):
    warm = Run(plain.side.nets, temperature=1.0)
    rows = torch.as_tensor(warm.seats.net_rows[0], dtype=torch.long, device=warm.a[0].device)
    mine = torch.as_tensor(warm.seats.rows, dtype=torch.long, device=warm.a[0].device)
    left = sum(int((a[rows] != g[rows]).sum()) for a, g in zip(warm.a, warm.greedy))
    print("the partner left its greedy move on %d of %d row-steps" % (left, STEPS * len(rows)))
    assert left > 0
    # the learner's rows explore by eps alone, exactly as the greedy-partner run's do on the first step (the same observations)
    assert torch.equal(warm.a[0][mine], plain.a[0][mine]) and torch.equal(warm.greedy[0], plain.greedy[0])
    # what is stored: sequences of the learner's M = G rows only (every game ends once; the few that lose their lives early may end
    # twice -- were the partner's G rows stored too, there would be 2 G or more), acts counted on the learner's rows only
    assert warm.num_act == STEPS * warm.seats.M == plain.num_act and warm.seats.M == G
    assert G <= warm.side.replay.num_add() < 2 * G and G <= plain.side.replay.num_add() < 2 * G
    # ... and the stored rows themselves: every sequence's (a, greedy_a) series is the series of a LEARNER row of the run, from some
    # step on; the partner's sampled rows (a != greedy_a without any eps) are nowhere in it
    A, Gr = torch.stack(warm.a).cpu()[:, mine.cpu()], torch.stack(warm.greedy).cpu()[:, mine.cpu()]      # [STEPS, M]
    rp = warm.side.replay
    assert rp.size() >= G
    for i in range(rp.size()):
        f, _, _, _, seq_len = rp.get(i)
        L = int(seq_len.item())
        sa, sg = f["a"][:L, 0].cpu().view(-1, 1), f["greedy_a"][:L, 0].cpu().view(-1, 1)
        assert 1 <= L <= MAX_LEN
        assert any(bool(((A[s:s + L] == sa) & (Gr[s:s + L] == sg)).all(0).any()) for s in range(STEPS - L + 1)), \
            "stored sequence %d (%d steps) is no learner row's series" % (i, L)
    # one seed, one run
    Run(plain.side.nets, temperature=1.0).same_as(warm)
