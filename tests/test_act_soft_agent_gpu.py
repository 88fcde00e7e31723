"""GPU: CompositeAgent.act with obs["temp"] (hsad_r2d2_act_soft) on a small random net (hid_dim 64), at N = 96 and N = 1,024 -- the two
acting regimes (from 1,024 rows on the bf16 copy of the state is carried) -- with packed bf16 observation rows and with float32 rows.
Without obs["temp"] and with zeros the reply is the plain call's bit for bit; at temperature 1 the greedy action and the new state still
are, every action is legal and some leave the greedy one."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = "cuda:0"
F, A, HAND, HID = 838, 21, 5, 64


@pytest.fixture(scope="module")
def net():
    from hanabi_sad_amd.composite import CNet
    from hanabi_sad_amd.selfplay import init_weights
    return CNet(init_weights(F, HID, A, HAND, 5), DEV)


def inputs(net, N, packed):
    g = torch.Generator().manual_seed(N)
    priv = (torch.rand(N, F, generator=g) < 0.1).float()
    legal = (torch.rand(N, A, generator=g) < 0.5).float()
    legal[:, 0] = 1.0
    legal[1] = 0.0
    legal[1, 7] = 1.0                      # one legal action
    obs = {"legal_move": legal.to(DEV), "eps": torch.where(torch.rand(N, generator=g) < 0.3, 0.25, 0.0).to(DEV)}
    if packed:
        p16 = torch.zeros(N, net.Fp, dtype=torch.bfloat16)
        p16[:, :F] = priv.to(torch.bfloat16)
        obs["priv_s_bf16"] = p16.to(DEV)
    else:
        obs["priv_s"] = priv.to(DEV)
    hid = {"h0": (torch.randn(net.L, N, HID, generator=g) * 0.3).to(DEV), "c0": (torch.randn(net.L, N, HID, generator=g) * 0.3).to(DEV)}
    if N >= 1024:
        hid["h0_16"] = hid["h0"].to(torch.bfloat16)
    return obs, hid


def act(net, obs, hid, **extra):
    from hanabi_sad_amd.composite import CompositeAgent
    agent = CompositeAgent(net, net, 1, 0.99, seed=77)
    agent.counter = 3
    reply, new = agent.act(dict(obs, **extra), hid)
    torch.cuda.synchronize()
    assert agent.counter == 4
    return reply, new


def same(x, y, keys):
    return all(torch.equal(x[k], y[k]) for k in keys)


@pytest.mark.parametrize("packed", [True, False], ids=["bf16_rows", "float32_rows"])
@pytest.mark.parametrize("N", [96, 1024])
def test_act_with_a_temperature(net, N, packed):
    obs, hid = inputs(net, N, packed)
    state = ("h0", "c0", "h0_16") if N >= 1024 else ("h0", "c0")
    plain, plain_hid = act(net, obs, hid)
    assert set(plain_hid) == set(state)
    key = torch.arange(N, dtype=torch.int64, device=DEV) * 31 + 5
    for extra in ({"temp": torch.zeros(N, device=DEV)}, {"temp": torch.zeros(N, device=DEV), "sample_key": key}):
        cold, cold_hid = act(net, obs, hid, **extra)
        assert same(cold, plain, ("a", "greedy_a")) and same(cold_hid, plain_hid, state)
    legal = obs["legal_move"]
    for extra in ({"temp": torch.ones(N, device=DEV)}, {"temp": torch.ones(N, device=DEV), "sample_key": key}):
        warm, warm_hid = act(net, obs, hid, **extra)
        assert same(warm, plain, ("greedy_a",)) and same(warm_hid, plain_hid, state)
        assert bool((legal.gather(1, warm["a"].view(-1, 1)) == 1).all()) and int(warm["a"][1]) == 7
        left = int((warm["a"] != warm["greedy_a"]).sum())
        print("N %d: %d rows left their greedy action" % (N, left))
        assert left > N // 8
    # Q_online at the sampled action is hsad_q_at's value there: asked through with_q on the deferred-target path
    from hanabi_sad_amd.composite import CompositeAgent
    agent = CompositeAgent(net, net, 1, 0.99, seed=77)
    agent.counter = 3
    r, _ = agent.act(dict(obs, temp=torch.ones(N, device=DEV)), hid, with_q=True, defer_target=True)
    assert torch.equal(r["a"], act(net, obs, hid, temp=torch.ones(N, device=DEV))[0]["a"]) and bool(torch.isfinite(r["q_online_a"]).all())
    with pytest.raises(Exception, match="defer_target"):
        agent.act(dict(obs, temp=torch.ones(N, device=DEV)), hid, with_q=True)
