"""TEST INFRASTRUCTURE: the per-slot stratified uniforms of the learned belief's worlds (include/hsad.h,
hsad_env_determinize_belief_worlds; hanabi_sad_amd/csrc/hsad_belief_world.h), restated from the specification in Python integers.
Never imported by the product package.

    h(c) = policy_hash(seed, group, c, 67);  W = n_worlds, w = the world;  slot i = 0 .. 4:
    a_i = the first cand_k = 1 + ((h(16 + 8 i + k) (W - 1)) >> 32), k = 0 .. 7, coprime to W; 1 if none
    o_i = (h(2 i) W) >> 32;  s_i = (a_i w + o_i) mod W;  j_i = h((1 << 8) | i) >> 8 (one per group and slot);  k_i = ((s_i << 24) + j_i) // W;  u_i = k_i << 8

sample / row_f32 are belief_head_ref's with these uniforms: the float64 reference and the fp32 restatement of a world's hand."""
import math

from tests import belief_head_ref as R
from tests.determinize_ref import M64, policy_hash

STREAM = 67
SLOTS = 5
MAX_WORLDS = 1 << 20


def h(seed, group, c):
    return policy_hash(seed & M64, group & M64, c, STREAM)


def stride(seed, group, W, i):
    for k in range(8):
        cand = 1 + ((h(seed, group, 16 + 8 * i + k) * (W - 1)) >> 32)
        if math.gcd(cand, W) == 1:
            return cand
    return 1


def offset(seed, group, W, i):
    return (h(seed, group, 2 * i) * W) >> 32


def strata(seed, group, W, w):
    """[s_0 .. s_4]"""
    return [(stride(seed, group, W, i) * w + offset(seed, group, W, i)) % W for i in range(SLOTS)]


def ks(seed, group, W, w):
    """[k_0 .. k_4], 24-bit"""
    out = []
    for i, s in enumerate(strata(seed, group, W, w)):
        j = h(seed, group, (1 << 8) | i) >> 8
        out.append(((s << 24) + j) // W)
    return out


def uniforms(seed, group, W, w):
    """[u_0 .. u_4] as bh_slot_pick takes them; None when W or w is out of range"""
    if not (1 <= W <= MAX_WORLDS and 0 <= w < W):
        return None
    return [k << 8 for k in ks(seed, group, W, w)]


def sample(z, pool, cms, seed, group, W, w):
    """belief_head_ref.sample (float64) of world w of W of `group`; cms = the occupied slots' compat lists"""
    us = uniforms(seed, group, W, w)
    return None if us is None else R.sample(z, pool, cms, us[:len(cms)])


def row_f32(z, pool, cms, n, seed, group, W, w):
    """belief_head_ref.row_f32 (sample mode) of world w of W of `group`"""
    us = uniforms(seed, group, W, w)
    return None if us is None else R.row_f32(z, pool, cms, None, us, n)


def slot0_counts(z, pool, cms, seed, group, W):
    """slot 0 of a game's W worlds: its conditional is the same in every world (nothing has been drawn yet), and the W uniforms
    u_0 = k_0 2^-24 lie one in each part [s / W, (s + 1) / W).  -> (count [25]: how many worlds the float64 reference gives type
    t; p [25]: p_0[t]; near [25]: how many worlds lie within the fp32 sampler's margin (belief_head_ref.sample: (2 E_S + 2 U) S) of
    one of the two boundaries of t's interval of the cumulative distribution -- a device draw may fall on either side of those)"""
    w0 = R.weights(list(pool), cms, 0)
    s = R.slot(z[:25], w0)
    e_s = 25 * R.U + 2 * R.U + (4 + 2 * s["dmax"]) * R.U
    margin = (2 * e_s + 2 * R.U) * s["S"]
    count, near = [0] * 25, [0] * 25
    for w in range(W):
        thr = (ks(seed, group, W, w)[0] * 2.0 ** -24) * s["S"]
        run, c = 0.0, None
        for k, t in enumerate(s["F"]):
            run += s["v"][t]
            if abs(run - thr) <= margin and t != s["F"][-1]:
                near[t] += 1
                near[s["F"][k + 1]] += 1
            if c is None and run > thr:
                c = t
        count[c if c is not None else s["F"][-1]] += 1
    return count, s["p"], near
