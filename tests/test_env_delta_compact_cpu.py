"""CPU: the compacted delta stream's scan / store, as a lock-step model of one 64-lane wave (tests/delta_compact_ref.py; the kernel is
stream_bits_f32_compact in csrc/hsad_env.hip).  The list of changed words is written in place into `old`, so on random `bits` / `old`:

* every read of `old` sees the original word (no list entry is ever read as an old word),
* the multiset of stored (chunk index, nibble) pairs equals the direct form's, and no chunk is stored twice,
* no chunk >= nch is stored, the list names the changed words in order, and the line count equals the direct form's.

The epilogue keeps the direct form, so there is no two-wave split to model."""
import random

import pytest

from tests import delta_compact_ref as R

F2 = 2 * 783           # floats of one two-player game: 391 chunks + 2 tail floats, the last word owns 7 chunks
SIZES = [32 * w for w in (1, 63, 64, 65, 255, 256, 257, 3132, 3133)] + [F2, 64 * F2 + F2, 4, 28, 32 + 12]


def words_for(n):
    return (n // 4 + 7) // 8 + 1       # one spare word behind: never read, never written


def patterns(nw_used):
    """which of the words that own a chunk differ"""
    last = nw_used - 1
    yield "none", set()
    yield "all", set(range(nw_used))
    yield "last", {last}
    yield "first", {0}
    for c in (1, 7, 8, 9, 31, 32, 33):
        if c <= nw_used:
            yield "%d random" % c, set(random.sample(range(nw_used), c))
            yield "%d leading" % c, set(range(c))
            yield "%d trailing" % c, set(range(nw_used - c, nw_used))
    yield "0.37", {w for w in range(nw_used) if random.random() < 0.37}


def check(n, changed, scan_steps=R.SCAN_STEPS, store_groups=R.STORE_GROUPS):
    nw = words_for(n)
    nch = n // 4
    bits = [random.getrandbits(32) for _ in range(nw)]
    old = list(bits)
    for w in changed:
        old[w] = bits[w] ^ (1 << random.randrange(32))
    want, want_lines = R.direct(bits, old, n)
    got, lines, old_reads, entries = R.compact(bits, old, n, scan_steps, store_groups)
    for pos, seen in old_reads:
        assert seen == old[pos], "a read of old[%d] saw %#x, not the original word" % (pos, seen)
    assert sorted(got) == sorted(want)
    assert len({k for k, _ in got}) == len(got), "a chunk stored twice"
    assert all(0 <= k < nch for k, _ in got)
    assert entries == sorted(w for w in changed if w < nch // 8)
    assert lines == want_lines == len([w for w in changed if 8 * w < nch])
    # whole lines only: a word's chunks are stored all or none (the partial last word: all the chunks it owns)
    per_word = {}
    for k, _ in got:
        per_word[k >> 3] = per_word.get(k >> 3, 0) + 1
    for w, c in per_word.items():
        assert c == min(8, nch - 8 * w)


@pytest.mark.parametrize("n", SIZES)
def test_compact_equals_direct_and_never_reads_a_list_entry_as_old(n):
    random.seed(1000 + n)
    nw_used = (n // 4 + 7) // 8
    if nw_used == 0:
        check(n, set())
        return
    for name, changed in patterns(nw_used):
        check(n, changed)


@pytest.mark.parametrize("scan_steps,store_groups", [(1, 1), (2, 4), (4, 2), (8, 8)])
def test_invariant_holds_for_other_unroll_factors(scan_steps, store_groups):
    random.seed(7)
    for n in (32 * 65, 32 * 3133, 64 * F2 + F2):
        for name, changed in patterns((n // 4 + 7) // 8):
            check(n, changed, scan_steps, store_groups)


def test_partial_last_word_of_one_game():
    """one game at P = 2, F = 783: 1,566 floats = 391 chunks + 2 tail floats; word 48 owns chunks 384 .. 390 only"""
    random.seed(3)
    n = F2
    assert n // 4 == 391 and n % 4 == 2
    nw = words_for(n)
    bits = [random.getrandbits(32) for _ in range(nw)]
    old = list(bits)
    old[48] ^= 1 << 30                   # a bit of the tail floats: the whole word compares unequal, as in the direct form
    got, lines, _, entries = R.compact(bits, old, n)
    assert entries == [] and lines == 1
    assert sorted(k for k, _ in got) == list(range(384, 391))
    assert got == R.direct(bits, old, n)[0]
