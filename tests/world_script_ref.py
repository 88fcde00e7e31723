"""Plain-Python restatement of hsad_search_world_script (include/hsad.h), written from its specification: which deal index fills
each slot of the viewer's hand after a logged history, and the deal script of a sampled world that follows from it.

A history is a list of moves, move t made by seat t mod P, given as the uid the env was stepped with: uid in [0, H) discards and
uid in [H, 2H) plays hand slot uid mod H; anything else (hints, the noop) moves no card."""


def viewer_slots(moves, viewer, root_count, P, H):
    """moves: per move t the uid of seat t mod P.  -> the deal indices of the viewer's hand slots, in slot order, or None when the
    history names a slot the viewer's hand does not have"""
    slots = [viewer * H + i for i in range(H)]
    d = P * H
    for t, uid in enumerate(moves):
        mover = t % P
        uid = int(uid)
        if not 0 <= uid < 2 * H:
            continue
        i = uid % H
        if mover == viewer:
            if i >= len(slots):
                return None
            del slots[i]
        if d < root_count:
            if mover == viewer:
                slots.append(d)
            d += 1
    return slots


def world_script_ref(deck_hist, root_count, moves, viewer, world_hand, P, H):
    """deck_hist: the root's card types in deal order (at least root_count entries); world_hand: the card types of the hand the
    world holds for the viewer, in slot order.  -> (script: 52 ints, count); ([0] * 52, 0) for a slot that is skipped"""
    skip = ([0] * 52, 0)
    if not (0 <= viewer < P) or root_count < P * H or root_count > 50:
        return skip
    slots = viewer_slots(moves, viewer, root_count, P, H)
    if slots is None or len(slots) != len(world_hand):
        return skip
    script = [int(deck_hist[i]) if i < root_count else 0 for i in range(52)]
    for k, di in enumerate(slots):
        script[di] = int(world_hand[k])
    return script, int(root_count)
