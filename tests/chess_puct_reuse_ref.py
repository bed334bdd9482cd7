"""Tree reuse of the chess PUCT search (zc_chess_puct_begin_reuse, chess_puct.hip's re-root
kernel) in executable form (TEST INFRASTRUCTURE ONLY).  The search loop is
puct_reuse_ref.search with rules=puct_ref.ChessRules; this file adds what differs on chess:
the position key, the rule that picks the new root with both halves of the room rule, and the
re-root of a zc_debug_chess_tree dump (node records plus the mv / prior / na / w / child slot
arrays) as a pure function."""
import numpy as np

from oracle.puct_ref import ChessRules, Node
from puct_reuse_ref import count_nodes, count_slots, search  # noqa: F401  (re-exported for the tests)

SLOTS_PER_NODE = 64   # kChessSlotsPerNode: a tree of M nodes has S = 64 * M child slots
SLOT_ARRAYS = ("mv", "prior", "na", "w", "child")


def key(state):
    """What "holds the position" compares: board, turn, fifty, castle."""
    return bytes(bytearray(state.board)[:64]), int(state.turn), int(state.fifty), int(state.castle)


def advance(root, k):
    """The node of `root`'s tree whose position has key `k`: the first child in slot order,
    else the first grandchild (child slot, then grandchild slot); None when there is none, when
    it was never evaluated or has no moves.  The root itself never matches."""
    found = next((ch for ch in root.child if ch is not None and key(ch.s) == k), None)
    if found is None:
        found = next((gc for ch in root.child if ch is not None for gc in ch.child
                      if gc is not None and key(gc.s) == k), None)
    if found is None or not found.evaluated or len(found.moves) == 0:
        return None
    return found


def next_root(root, state, sims, max_nodes):
    """(root of the next search of `state`, nodes kept): the kept subtree when advance() finds
    one and both kept_nodes + sims - 1 <= M and kept_slots + 64 * (sims - 1) <= 64 * M hold
    (M = max_nodes), else a fresh Node and 0."""
    if root is not None:
        nr = advance(root, key(state))
        if nr is not None:
            kept = count_nodes(nr)
            if (kept + sims - 1 <= max_nodes and
                    count_slots(nr) + SLOTS_PER_NODE * (sims - 1) <= SLOTS_PER_NODE * max_nodes):
                return nr, kept
    return Node(state, ChessRules), 0


def dump_key(dump, i):
    st = dump["nodes"]["st"][i]
    return bytes(bytearray(st[:64])), int(st[64]), int(st[65]), int(st[66])


def find(dump, k):
    """advance() on a dump: the id of the node to re-root at, or None."""
    nodes = dump["nodes"]

    def children(i):
        b, n = int(nodes["base"][i]), int(nodes["nmoves"][i])
        return [int(c) for c in dump["child"][b:b + n] if int(c) != 0xFFFF]

    hit = next((c for c in children(0) if dump_key(dump, c) == k), None)
    if hit is None:
        hit = next((g for c in children(0) for g in children(c) if dump_key(dump, g) == k), None)
    if hit is None or not int(nodes["evaluated"][hit]) or int(nodes["nmoves"][hit]) == 0:
        return None
    return hit


def compact(dump, new_root):
    """The dump that the re-root at node `new_root` must leave: the nodes of its subtree in
    increasing old id, renumbered from 0, their bases the running sums of nmoves in the new
    numbering and their slot ranges moved there; parents and children renumbered, the new root
    without parent or parent slot, depths counted from it; every other field as it was."""
    nodes = dump["nodes"]
    remap = {}
    for i in range(len(nodes)):
        if i == new_root or int(nodes["parent"][i]) in remap:
            remap[i] = len(remap)
    old = sorted(remap)
    out = nodes[old].copy()
    total = sum(int(nodes["nmoves"][o]) for o in old)
    slots = {f: np.zeros(total, dump[f].dtype) for f in SLOT_ARRAYS}
    d0, base = int(nodes["depth"][new_root]), 0
    for new, o in enumerate(old):
        n, ob = int(nodes["nmoves"][o]), int(nodes["base"][o])
        out["base"][new] = base
        if new == 0:
            out["parent"][new], out["pact"][new], out["depth"][new] = 0xFFFF, 0xFFFF, 0
        else:
            out["parent"][new] = remap[int(nodes["parent"][o])]
            out["depth"][new] = int(nodes["depth"][o]) - d0
        for f in SLOT_ARRAYS:
            slots[f][base:base + n] = dump[f][ob:ob + n]
        for k in range(n):
            ch = int(dump["child"][ob + k])
            if ch != 0xFFFF:
                slots["child"][base + k] = remap[ch]   # a kept node's children are all kept
        base += n
    return {"nodes": out, **slots}
