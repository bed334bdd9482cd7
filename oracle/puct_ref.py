"""A plain-Python restatement of the PUCT searches of zeroclone_amd/csrc/chess_puct.hip and
c4_puct.hip, for the parity tests and bench.py's C5 CPU baseline (TEST INFRASTRUCTURE ONLY;
the rules come from the oracle).  The search has no
reference counterpart, so this file is its specification in executable
form: same arithmetic order in fp64, same tie-breaking, same flush / virtual-loss protocol.
"""
import math

import oracle


class ChessRules:
    """chess_puct.hip: the reference's chess rules (oracle restatement of chess_backend.cpp)."""
    moves = staticmethod(oracle.chess_moves)
    play = staticmethod(oracle.chess_play)
    win = staticmethod(oracle.chess_win)


class C4Rules:
    """c4_puct.hip: Connect4 (c4_backend.py) on state = (42-char board, side to move): moves
    are the legal columns in CPython set order, none once the last mover has four or the
    board is full; win = the last mover has four."""

    @staticmethod
    def moves(s):
        b, t = s
        if oracle.check_win(b, t) or oracle.check_draw(b):
            return []
        return oracle.set_order(sum(1 << col for col in range(7) if b[col] == "."))

    @staticmethod
    def play(s, col):
        return oracle.play(s[0], s[1], col)

    @staticmethod
    def win(s):
        return oracle.check_win(s[0], s[1])


class Capacity(Exception):
    """The search ended with status CAPACITY (no move) in flush `flush`; kind "depth": a walk
    stood on an evaluated, non-terminal node at level max_level (the flush selects no leaf);
    kind "slots": a node created in the flush did not fit in slot_cap (the flush's leaves are
    selected, none is backed up).  Visit counts are then unspecified: the device leaves the
    virtual losses of the flush's walks in place."""

    def __init__(self, flush, kind):
        super().__init__(f"CAPACITY ({kind}) in flush {flush}")
        self.flush, self.kind = flush, kind


class Node:
    def __init__(self, state, rules=ChessRules):
        self.s = state
        self.moves = rules.moves(state)
        n = len(self.moves)
        self.N = [0] * n
        self.W = [0.0] * n
        self.P = [0.0] * n
        self.child = [None] * n
        self.evaluated = False


def search(state, sims, bs, c, value_fn, prior_fn, rules=ChessRules, flush_fn=None, max_level=None, slot_cap=None):
    """value_fn(state) -> value for the side to move; prior_fn(node) -> priors (list,
    float) for the node's moves.  flush_fn(states), if given, is called once per flush with
    the states of its non-terminal leaves before any value_fn / prior_fn call of that flush
    (a batched network fills the cache they read).  Returns (root moves, root visits,
    chosen index).

    The two limits of the chess kernel, off by default (None): max_level (the kernel's 62) — a
    walk standing on an evaluated, non-terminal node at this level raises Capacity; slot_cap
    (the kernel's 64 * (max_sims + 1)) — the nodes take len(moves) slots in creation order, the
    root first, and a flush that created a node that does not fit raises Capacity after its
    walks."""
    root = Node(state, rules)
    slots = len(root.moves)
    flushes = 1 + (sims - 1 + bs - 1) // bs
    for f in range(flushes):
        nb = 1 if f == 0 else max(0, min(bs, sims - 1 - (f - 1) * bs))
        leaves, made = [], []
        for _ in range(nb):
            if f == 0:
                leaves.append((root, []))
                continue
            node, path = root, []
            while len(node.moves) and node.evaluated:
                if max_level is not None and len(path) >= max_level:
                    raise Capacity(f, "depth")
                sq = math.sqrt(float(sum(node.N)))
                best, bv = -1, -math.inf
                for j in range(len(node.moves)):
                    q = node.W[j] / node.N[j] if node.N[j] > 0 else 0.0
                    v = q + c * node.P[j] * sq / float(1 + node.N[j])
                    if v > bv:
                        bv, best = v, j
                node.N[best] += 1
                node.W[best] -= 1.0
                path.append((node, best))
                if node.child[best] is None:
                    node.child[best] = Node(rules.play(node.s, node.moves[best]), rules)
                    node = node.child[best]
                    made.append(node)
                    break
                node = node.child[best]
            leaves.append((node, path))
        for node in made:
            slots += len(node.moves)
            if slot_cap is not None and slots > slot_cap:
                raise Capacity(f, "slots")
        if flush_fn is not None:
            flush_fn([node.s for node, _ in leaves if len(node.moves)])
        for node, path in leaves:
            if len(node.moves) == 0:
                v = -1.0 if rules.win(node.s) else 0.0
            else:
                v = value_fn(node.s)
                if not node.evaluated:
                    node.P = prior_fn(node)
                    node.evaluated = True
            d = len(path)
            for l, (par, a) in enumerate(path, start=1):
                r = v if (d - l) % 2 == 0 else -v
                par.W[a] = par.W[a] + 1.0 - r
    best, bn = -1, -1
    for j, n in enumerate(root.N):
        if n > bn:
            bn, best = n, j
    return root.moves, root.N, best
