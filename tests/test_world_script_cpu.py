"""CPU: the plain-Python slot tracking of tests/world_script_ref.py on hand-written histories (what the GPU test holds
hsad_search_world_script to), and the three entry points of the replay stage in include/hsad.h and the ctypes table."""
import ctypes as C
import os
import re

from tests import world_script_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_discard_of_a_middle_slot_shifts_the_later_slots_down():
    # 2 players, hand 5: seat 0 holds deal indices 0..4, the next card dealt is index 10
    assert W.viewer_slots([2], 0, 11, 2, 5) == [0, 1, 3, 4, 10]
    # the partner's play (uid H + 1) takes index 11; seat 0 then plays its slot 3 (index 4) and draws index 12
    assert W.viewer_slots([2, 6, 8], 0, 13, 2, 5) == [0, 1, 3, 10, 12]
    # seen from seat 1: only its own play moved its hand
    assert W.viewer_slots([2, 6, 8], 1, 13, 2, 5) == [5, 7, 8, 9, 11]
    # hints (uid >= 2H) and the noop move no card
    assert W.viewer_slots([10, 15, 20, 12], 0, 10, 2, 5) == [0, 1, 2, 3, 4]


def test_plays_after_the_deck_is_empty_draw_nothing():
    # Hanabi-Small shape: 2 players, hand 2, 20 cards.  Seat 0 discards slot 0, seat 1 plays slot 1, eight times each: 16 deals
    moves = [0, 3] * 8
    assert W.viewer_slots(moves, 0, 20, 2, 2) == [16, 18]
    assert W.viewer_slots(moves, 1, 20, 2, 2) == [2, 19]
    # the deck is empty now (deal index 20 = root_count): a play shortens the hand and nothing is appended
    assert W.viewer_slots(moves + [3], 0, 20, 2, 2) == [16]
    assert W.viewer_slots(moves + [3, 2], 1, 20, 2, 2) == [19]
    assert W.viewer_slots(moves + [3, 2, 0], 0, 20, 2, 2) == []
    # a game that ended on a move that dealt no card although the deck still held some: root_count says so
    assert W.viewer_slots([0, 3, 1], 0, 6, 2, 2) == [1]


def test_a_viewer_who_never_moved_keeps_the_initial_deal():
    # 3 players, hand 5: seats 0 and 1 moved, seat 2 did not
    assert W.viewer_slots([0, 6], 2, 17, 3, 5) == [10, 11, 12, 13, 14]
    assert W.viewer_slots([], 1, 15, 3, 5) == [5, 6, 7, 8, 9]
    # ... and its cards stay put while the others draw: the indices 15 and 16 went to seats 0 and 1
    assert W.viewer_slots([0, 6], 0, 17, 3, 5) == [1, 2, 3, 4, 15]
    assert W.viewer_slots([0, 6], 1, 17, 3, 5) == [5, 7, 8, 9, 16]


def test_a_viewer_whose_every_card_is_newer_than_the_initial_deal():
    # 2 players, hand 2: seat 0 only hints (uid 4), seat 1 discards slot 0 twice
    assert W.viewer_slots([4, 0, 4, 0], 1, 6, 2, 2) == [4, 5]
    script, count = W.world_script_ref([7, 8, 9, 5, 6, 1], 6, [4, 0, 4, 0], 1, [20, 21], 2, 2)
    assert count == 6 and script[:6] == [7, 8, 9, 5, 20, 21] and script[6:] == [0] * 46


def test_the_script_replaces_exactly_the_viewers_current_cards():
    dh = list(range(11)) + [0] * 41
    script, count = W.world_script_ref(dh, 11, [2], 0, [24, 23, 22, 21, 20], 2, 5)
    assert count == 11 and script[:11] == [24, 23, 2, 22, 21, 5, 6, 7, 8, 9, 20] and len(script) == 52
    # skipped: no viewer, a root that was never started, a hand of another length than the history gives, a slot that does not exist
    assert W.world_script_ref(dh, 11, [2], -1, [1] * 5, 2, 5) == ([0] * 52, 0)
    assert W.world_script_ref(dh, 0, [], 0, [1] * 5, 2, 5) == ([0] * 52, 0)
    assert W.world_script_ref(dh, 11, [2], 0, [1] * 4, 2, 5) == ([0] * 52, 0)
    assert W.world_script_ref([0] * 52, 20, [0, 3] * 8 + [3, 2, 1], 0, [], 2, 2) == ([0] * 52, 0)


DECLARED = {
    "hsad_env_rewind_scripted": "int hsad_env_rewind_scripted(hsad_env* env, const uint8_t* script, const int32_t* count, void* stream);",
    "hsad_search_world_script": "int hsad_search_world_script(const hsad_env* world_env, const int32_t* src_index, const int32_t* viewer, "
                                "const uint8_t* root_deck_hist, const int32_t* root_count, int G_root, const int64_t* log_a, int n_moves, "
                                "uint8_t* script_out, int32_t* count_out, void* stream);",
    "hsad_search_replay_actions": "int hsad_search_replay_actions(const hsad_env* env, const int32_t* src_index, const int32_t* viewer, "
                                  "const int64_t* log_a_t, const int64_t* log_greedy_t, int G_root, const int64_t* greedy_src, int64_t* a, "
                                  "int64_t* greedy_a, int32_t* mismatch, void* stream);",
}


def test_header_and_ctypes_table_carry_the_replay_entry_points():
    from hanabi_sad_amd import _lib
    txt = open(os.path.join(ROOT, "include", "hsad.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, want in DECLARED.items():
        found = re.findall(r"\bint\s+%s\s*\([^;]*\);" % name, txt)
        assert len(found) == 1, "%s: declared %d times in include/hsad.h" % (name, len(found))
        assert re.sub(r"\s+", " ", found[0]) == want
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        # every pointer is a void pointer in the table; the two sizes are plain ints
        args = want[want.index("(") + 1:want.rindex(")")].split(", ")
        assert argtypes == [C.c_void_p if "*" in a else C.c_int for a in args], name
    # the error log names the new code
    assert re.search(r"5 a deal\s+\*?\s*script names a card the deck does not hold", open(os.path.join(ROOT, "include", "hsad.h")).read())
