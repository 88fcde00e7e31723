"""CPU: the compacted delta stream in half-line units, as a lock-step model of one 64-lane wave (tests/delta_subline_ref.py; the kernel
is stream_bits_f32_compact<NT, 16> in csrc/hsad_env.hip).  The list of changed half lines is written in place into `old` as 16-bit
entries, so for every case:

* no read of `old` returns a list entry: every read sees the original word,
* the list is exactly the changed halves, in order, each once (so the two halves of a line are neighbours),
* the set of float4 chunks stored equals the chunks of the changed halves, plus the partial last word handled directly, with the
  nibbles the bits give, no chunk twice and none >= nch,
* a store instruction's lanes cover whole halves: lanes 4q .. 4q + 3 hold the four consecutive chunks of one half.

Run for unroll factors 1-8 of both loops, for the word counts of a configs[1] workgroup (3,132), the largest workgroup (14,390:
five players with SAD, 64 games), a one-game workgroup (48 full words and a partial one), 64 and 65, and for the masks none / all
(the invariant's worst case: two entries per lane in every step) / only lo / only hi / random at 0.1, 0.274 and 0.9."""
import random

import pytest

from tests import delta_subline_ref as R

F2 = 2 * 783           # floats of one two-player game: 391 chunks + 2 tail floats, the last word owns 7 chunks
SIZES = [32 * 3132, 32 * 14390, F2, 32 * 64, 32 * 65]
MASKS = ["none", "all", "lo", "hi", 0.1, 0.274, 0.9]


def make_case(n, mask):
    """bits, old: one spare word behind the used ones, never read, never written"""
    nw_used = (n // 4 + 7) // 8
    bits = [random.getrandbits(32) for _ in range(nw_used + 1)]
    old = list(bits)
    for w in range(nw_used):
        if mask == "none":
            x = 0
        elif mask == "all":
            x = (1 << random.randrange(16)) | (0x10000 << random.randrange(16))
        elif mask == "lo":
            x = 1 << random.randrange(16)
        elif mask == "hi":
            x = 0x10000 << random.randrange(16)
        else:   # each half on its own at the given density
            x = ((1 << random.randrange(16)) if random.random() < mask else 0) | \
                ((0x10000 << random.randrange(16)) if random.random() < mask else 0)
        old[w] = bits[w] ^ x
    return bits, old


def check(n, mask, scan_steps, store_groups):
    bits, old = make_case(n, mask)
    nch = n // 4
    nfull = nch // 8
    assert 2 * nfull <= 65536, "a half-line index must fit 16 bits"
    got, lines, units, old_reads, entries, instrs = R.compact16(bits, old, n, scan_steps, store_groups)
    for pos, seen in old_reads:
        assert seen == old[pos], "a read of old[%d] saw %#x, not the original word" % (pos, seen)
    halves = R.changed_halves(bits, old, n)
    assert entries == halves
    assert len(set(entries)) == len(entries)
    want = [(4 * h + c, (bits[h >> 1] >> (16 * (h & 1) + 4 * c)) & 15) for h in halves for c in range(4)]
    part_changed = nch > 8 * nfull and bits[nfull] != old[nfull]
    if part_changed:
        want += [(k, (bits[nfull] >> (4 * (k & 7))) & 15) for k in range(8 * nfull, nch)]
    assert sorted(got) == sorted(want)
    assert len({k for k, _ in got}) == len(got), "a chunk stored twice"
    assert all(0 <= k < nch for k, _ in got)
    assert lines == len({h >> 1 for h in halves}) + part_changed
    assert units == len(halves) + part_changed * (1 if (nch & 7) <= 4 else 2)
    for ins in instrs:
        by_lane = dict(ins)
        for q in range(16):
            ks = [by_lane.get(4 * q + c) for c in range(4)]
            if ks[0] is None:
                assert ks == [None] * 4, "a half stored in part"
            else:
                assert ks[0] % 4 == 0 and ks == list(range(ks[0], ks[0] + 4)), "the lanes of a half do not hold its four chunks"
    if mask in ("none", "all", "lo", "hi"):
        per_word = {"none": 0, "all": 2, "lo": 1, "hi": 1}[mask]
        assert len(halves) == per_word * nfull


@pytest.mark.parametrize("unroll", range(1, 9))
def test_half_line_list_and_stores_at_every_size_and_mask(unroll):
    random.seed(500 + unroll)
    for n in SIZES:
        for mask in MASKS:
            check(n, mask, unroll, unroll)


@pytest.mark.parametrize("scan_steps,store_groups", [(1, 8), (8, 1), (4, 4), (3, 5)])
def test_mixed_unroll_factors(scan_steps, store_groups):
    random.seed(77)
    for n in (F2, 32 * 65, 32 * 3132):
        for mask in MASKS:
            check(n, mask, scan_steps, store_groups)


def test_halves_of_a_line_are_neighbours_in_a_store():
    """both halves of a changed line sit in lanes 8q .. 8q + 7 of one store or in the last and first four lanes of two: the eight
    chunks stay consecutive in the list order, so the stores still form 128-byte segments"""
    random.seed(5)
    n = 32 * 3132
    bits, old = make_case(n, 0.9)
    _, _, _, _, entries, _ = R.compact16(bits, old, n)
    listed = set(entries)
    both = 0
    for a, b in zip(entries, entries[1:]):
        if a % 2 == 0 and (a + 1) in listed:
            assert b == a + 1
            both += 1
    assert both > 0


def test_partial_last_word_of_one_game():
    """one game at P = 2, F = 783: word 48 owns chunks 384 .. 390 only and is stored whole, whichever half changed"""
    random.seed(3)
    n = F2
    bits, old = make_case(n, "none")
    old[48] ^= 1 << 30                   # a bit of the tail floats: the whole word compares unequal, as in the direct form
    got, lines, units, _, entries, _ = R.compact16(bits, old, n)
    assert entries == [] and lines == 1 and units == 2
    assert sorted(k for k, _ in got) == list(range(384, 391))
