"""Non-uniform priors for the PUCT searches' parity tests (TEST INFRASTRUCTURE ONLY): logits as
a pure function of (position, move), so that the host callback of a device search and the
specification's prior_fn see the same numbers and a repeated or transposed position gets the
same row; the trees of a device dump and of the specification in one form, and the two
comparisons test_gpu_puct_priors.py makes on them (test_puct_priors_cpu.py shows that they
reject wrong searches).

Logit variants (Logits.kind), a row = the 4096 (chess, from * 64 + to) or 7 (Connect4, column)
logits of one position:

    hash   scale * u(position, move), u in [-1, 1): scale 0.05 flat, 3 moderate, 12 peaked
    line   +40 on the position's first listed move, 0 on the others; every value 0
    tie    one number (of the position) on every legal move
    mask   hash at scale 3 with -inf on a strict subset of the legal moves (about a third of
           them, never the first listed one)

Every ILLEGAL entry of a row holds 40 * u'(position, entry), another hash: a gather with a wrong
index reads something plausible but wrong.  Values are the existing position hashes
(test_gpu_puct.hv, c4_values.hash_value), or 0 everywhere (zero_values).  half=True rounds the logits to fp16 first; the
specification reads the rounded numbers.  Finite logits stay within |x| <= 40 and within 64 of
each other in a row, so no prior of the float32 restatement is denormal."""
import numpy as np

import oracle
from oracle import puct_ref
import puct_noise_ref as noise_ref
import puct_reuse_ref
from c4_values import bits_from_rows, hash_value

M64 = (1 << 64) - 1
SALT_LEGAL, SALT_ILLEGAL, SALT_TIE, SALT_MASK, SALT_FILL = 0x1F83D9ABFB41BD6B, 0x5BE0CD19137E2179, 0x3C6EF372FE94F82B, \
    0x510E527FADE682D1, 0xA54FF53A5F1D36F1
MAX_LEVEL = 62   # chess_puct.hip: a walk on an evaluated node at this level is CAPACITY (kChessPath - 2)


def hv(board: bytes, turn: int) -> float:
    """test_gpu_puct.hv."""
    h = 0x84222325CBF29CE4
    for b in board:
        h = ((h ^ b) * 0x100000001B3) & M64
    h = (h ^ (turn * 0x9E3779B97F4A7C15)) & M64
    h ^= h >> 31
    return ((h % 400001) - 200000) / 200003.0


def _mix(x):
    """splitmix64's finaliser on uint64 arrays."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def unit(h, idx, salt):
    """u(h, idx) in [-1, 1), float64 with 52 random bits."""
    x = _mix(np.uint64(h & M64) ^ _mix(np.asarray(idx, dtype=np.uint64) ^ np.uint64(salt)))
    return (x >> np.uint64(12)).astype(np.float64) * 2.0 ** -51 - 1.0


class Chess:
    name, width, rules = "chess", 4096, puct_ref.ChessRules

    @staticmethod
    def key(s):
        return bytes(bytearray(s.board)[:64]), int(s.turn), int(s.fifty), int(s.castle)

    @staticmethod
    def state(key):
        return oracle.chess_state(key[0].decode("latin-1"), key[1], key[2], key[3])

    @staticmethod
    def row_key(row):
        """A zc_chess_state row (72 bytes) -> key."""
        return bytes(bytearray(row[:64])), int(row[64]), int(row[65]), int(row[66])

    @staticmethod
    def pos_hash(key):
        h = 0xCBF29CE484222325
        for b in key[0] + bytes((key[1], key[3])):
            h = ((h ^ b) * 0x100000001B3) & M64
        return h

    @staticmethod
    def value(key):
        return hv(key[0], key[1])

    @staticmethod
    def index(move):
        return (move[0] * 8 + move[1]) * 64 + move[2] * 8 + move[3]

    @staticmethod
    def wrong_index(move):
        """The gather transposed: to * 64 + from."""
        return (move[2] * 8 + move[3]) * 64 + move[0] * 8 + move[1]


class C4:
    name, width, rules = "c4", 7, puct_ref.C4Rules

    @staticmethod
    def key(s):
        return bits_from_rows(s[0]) + (int(s[1]),)

    @staticmethod
    def state(key):
        s0, s1, turn = key
        cells = ["."] * 42
        for r in range(6):
            for c in range(7):
                bit = 1 << (7 * c + 5 - r)
                if s0 & bit:
                    cells[r * 7 + c] = "X"
                elif s1 & bit:
                    cells[r * 7 + c] = "O"
        return "".join(cells), turn

    @staticmethod
    def row_key(row):
        """A zc_c4_state row (3 int64) -> key."""
        return int(row[0]) & M64, int(row[1]) & M64, int(row[2]) & 1

    @staticmethod
    def pos_hash(key):
        return (key[0] * 0x9E3779B97F4A7C15 + key[1] * 0xC2B2AE3D27D4EB4F + key[2] * 0x165667B19E3779F9) & M64

    @staticmethod
    def value(key):
        return hash_value(*key)

    @staticmethod
    def index(col):
        return int(col)

    @staticmethod
    def wrong_index(col):
        """The gather mirrored: column 6 - col."""
        return 6 - int(col)


class Logits:
    def __init__(self, game, kind, scale=3.0, half=False, zero_values=False):
        assert kind in ("hash", "line", "tie", "mask") and abs(scale) <= 40
        self.game, self.kind, self.scale, self.half = game, kind, float(scale), half
        self.zero_values = zero_values or kind == "line"
        self._rows, self._moves = {}, {}

    @property
    def name(self):
        return f"{self.game.name}-{self.kind}{self.scale:g}-{'f16' if self.half else 'f32'}"

    def moves(self, key):
        """The position's legal moves in list order (the rules' own)."""
        m = self._moves.get(key)
        if m is None:
            m = self._moves[key] = self.game.rules.moves(self.game.state(key))
        return m

    def _round(self, x):
        x = np.asarray(x, dtype=np.float64)
        return (x.astype(np.float16) if self.half else x).astype(np.float32)

    def filler(self, h):
        """A row that belongs to no position (a stale or neighbouring row of the buffer)."""
        return self._round(40.0 * unit(h, np.arange(self.game.width), SALT_FILL))

    def row(self, key):
        """float32 [width]: the logits of the position, as the device reads them."""
        r = self._rows.get(key)
        if r is not None:
            return r
        g, h = self.game, self.game.pos_hash(key)
        every = np.arange(g.width)
        x = 40.0 * unit(h, every, SALT_ILLEGAL)
        legal = np.array([g.index(m) for m in self.moves(key)], dtype=np.int64)
        if legal.size:
            if self.kind == "hash":
                x[legal] = self.scale * unit(h, legal, SALT_LEGAL)
            elif self.kind == "line":
                x[legal] = 0.0
                x[legal[0]] = 40.0
            elif self.kind == "tie":
                x[legal] = 3.0 * unit(h, 0, SALT_TIE)
            else:
                x[legal] = 3.0 * unit(h, legal, SALT_LEGAL)
                off = unit(h, legal, SALT_MASK) < -0.3   # about a third of the moves
                off[0] = False   # a strict subset
                x[legal[off]] = -np.inf
        r = self._rows[key] = self._round(x)
        return r

    def value(self, key):
        return 0.0 if self.zero_values else self.game.value(key)

    def listed(self, key, moves=None, wrong=False):
        """The logits of the moves in list order (float32)."""
        g = self.game
        moves = self.moves(key) if moves is None else moves
        return self.row(key)[[g.wrong_index(m) if wrong else g.index(m) for m in moves]]

    def prior32(self, key, mutation=None):
        """The float32 restatement of the backup kernels' softmax (puct_noise_ref.softmax) on the
        position's row: what a device search is expected to hold, as a list of floats.  mutation:
        a deliberately wrong gather for the mutation checks — "transposed" (the index of the move
        mirrored), "row" (the row of another leaf) or "all" (the softmax over the whole row)."""
        moves = self.moves(key)
        lg = self.listed(key, wrong=mutation == "transposed")
        if mutation == "row":
            lg = self.filler(self.game.pos_hash(key))[[self.game.index(m) for m in moves]]
        if mutation == "all":
            row = self.row(key).astype(np.float32)
            e = np.exp(lg - row.max())
            p = e / np.exp(row - row.max()).sum(dtype=np.float32)
        else:
            p = noise_ref.softmax(lg[None, :], [len(moves)], np.float32)[0]
        return [float(x) for x in p.astype(np.float32)]


# ---- trees in one form: a list of records in creation order

def spec_tree(game, root, order):
    """`order`: the tree's nodes in creation order, the root first."""
    ids = {id(n): i for i, n in enumerate(order)}
    out = []
    for n in order:
        out.append(dict(key=game.key(n.s), parent=None, edge=None, moves=[tuple(m) if isinstance(m, tuple) else int(m)
                                                                          for m in n.moves],
                        N=[int(x) for x in n.N], W=[float(x) for x in n.W], child=[c is not None for c in n.child],
                        evaluated=bool(n.evaluated), P=np.array(n.P if n.evaluated else [], dtype=np.float32)))
    for i, n in enumerate(order):
        for k, c in enumerate(n.child):
            if c is not None:
                out[ids[id(c)]]["parent"], out[ids[id(c)]]["edge"] = i, k
    assert order[0] is root and all(r["parent"] is not None for r in out[1:])
    return out


def chess_dump_tree(d):
    """NativeEngine.debug_chess_tree's dump."""
    from zeroclone_amd._native import unpack_chess_move
    nd, out = d["nodes"], []
    for i in range(len(nd)):
        b, n = int(nd["base"][i]), int(nd["nmoves"][i])
        mv = []
        for m in d["mv"][b:b + n]:
            sq, val = unpack_chess_move(int(m))
            mv.append(sq + (val,))
        par, root = int(nd["parent"][i]), i == 0
        out.append(dict(key=Chess.row_key(nd["st"][i]), parent=None if root else par,
                        edge=None if root else int(nd["pact"][i]), moves=mv, N=[int(x) for x in d["na"][b:b + n]],
                        W=[float(x) for x in d["w"][b:b + n]], child=[int(c) != 0xFFFF for c in d["child"][b:b + n]],
                        evaluated=bool(nd["evaluated"][i]),
                        P=d["prior"][b:b + n].copy() if nd["evaluated"][i] else np.zeros(0, np.float32)))
        for k, c in enumerate(d["child"][b:b + n]):   # the child ids agree with the parent links
            if int(c) != 0xFFFF:
                assert int(nd["parent"][int(c)]) == i and int(nd["pact"][int(c)]) == k
    return out


def c4_dump_tree(nodes):
    """NativeEngine.debug_c4_puct_tree's records."""
    out = []
    for i, nd in enumerate(nodes):
        n, root = int(nd["nmoves"]), i == 0
        out.append(dict(key=(int(nd["s0"]), int(nd["s1"]), int(nd["turn"])), parent=None if root else int(nd["parent"]),
                        edge=None if root else int(nd["pact"]),
                        moves=[(int(nd["order"]) >> (3 * k)) & 7 for k in range(n)], N=[int(x) for x in nd["na"][:n]],
                        W=[float(x) for x in nd["w"][:n]], child=[int(c) != 0xFFFF for c in nd["child"][:n]],
                        evaluated=bool(nd["evaluated"]),
                        P=nd["pr"][:n].copy() if nd["evaluated"] else np.zeros(0, np.float32)))
        for k, c in enumerate(nd["child"][:n]):
            if int(c) != 0xFFFF:
                assert int(nodes[int(c)]["parent"]) == i and int(nodes[int(c)]["pact"]) == k
    return out


def levels(tree):
    lv = []
    for r in tree:
        lv.append(0 if r["parent"] is None else lv[r["parent"]] + 1)
    return lv


def compare_trees(got, want, what=""):
    """The whole tree, node by node in creation order: position, parent and edge, move list, every
    edge's N, every edge's W bit for bit, child presence, the evaluated flag."""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        for f in ("key", "parent", "edge", "moves", "N", "child", "evaluated"):
            assert a[f] == b[f], (what, i, f, a[f], b[f])
        assert np.array(a["W"], np.float64).tobytes() == np.array(b["W"], np.float64).tobytes(), (what, i, a["W"], b["W"])


def check_priors(tree, logits, what="", masked_unvisited=False):
    """The priors of every evaluated node of `tree` against the float64 softmax of the supplied
    logits over the node's moves in list order.  The error is measured against the float32
    restatement (Logits.prior32's arithmetic): 8 of its floors, absolute and relative; bit
    equality where the restatement is exact (every legal logit equal: 1 / n in float32); a masked
    move's prior exactly 0; positive wherever the restatement's is.  masked_unvisited: no masked
    move was ever selected (no visit, no child).  That is a property of the specification only
    where every score of an unmasked move stays positive — values 0 (no mate backed up past a
    masked move either: the chess case of this kind; Connect4's wins are too near), one leaf a
    flush, the first listed move unmasked; elsewhere a move of prior 0 scores Q + 0 = 0 and wins the argmax against
    moves whose Q is negative, by their values or by the virtual loss of a pending flush, and the
    tree comparison pins those visits one by one.
    Returns (abs error, abs floor, rel error, rel floor, nodes checked)."""
    ev = [r for r in tree if r["evaluated"]]
    assert ev and all(len(r["moves"]) for r in ev)
    K = max(len(r["moves"]) for r in ev)
    nm = np.array([len(r["moves"]) for r in ev])
    lg = np.full((len(ev), K), -np.inf, np.float32)
    dev = np.zeros((len(ev), K), np.float32)
    for i, r in enumerate(ev):
        assert len(r["P"]) == nm[i], (what, i)
        lg[i, :nm[i]] = logits.listed(r["key"], r["moves"])
        dev[i, :nm[i]] = r["P"]
    valid = np.arange(K)[None, :] < nm[:, None]
    assert not np.isnan(lg[valid]).any() and (lg[valid] < np.inf).all()
    with np.errstate(invalid="ignore"):
        p64 = noise_ref.softmax(lg, nm, np.float64)
        p32 = noise_ref.softmax(lg, nm, np.float32)
    assert p32.dtype == np.float32
    masked = valid & np.isneginf(lg)
    live = valid & ~masked
    assert (dev[masked] == 0).all(), what
    if masked_unvisited:
        for i, r in enumerate(ev):
            for k in np.nonzero(masked[i])[0]:
                assert r["N"][k] == 0 and not r["child"][k], (what, i, k)
    assert np.isfinite(dev[valid]).all() and (dev[valid] >= 0).all(), what
    assert (dev[live & (p32 > 0)] > 0).all(), what
    np.testing.assert_allclose(dev.astype(np.float64).sum(axis=1), 1.0, atol=1e-5)
    lo = np.where(live, lg, np.inf).min(axis=1)
    hi = np.where(live, lg, -np.inf).max(axis=1)
    exact = lo == hi   # all live logits equal (one move included): e = 1 each, the sum an integer
    cnt = live.sum(axis=1).astype(np.float32)
    want = np.where(live, (np.float32(1.0) / cnt)[:, None], np.float32(0)).astype(np.float32)
    assert (dev[exact] == want[exact]).all(), what
    assert (p32[exact] == want[exact]).all()
    d64 = dev.astype(np.float64)
    err = float(np.abs(d64 - p64)[live].max())
    floor = float(np.abs(p32.astype(np.float64) - p64)[live].max())
    big = live & (p64 >= 2.0 ** -100)   # a float32 normal number with room to spare
    rerr = float((np.abs(d64 - p64)[big] / p64[big]).max())
    rfloor = float((np.abs(p32.astype(np.float64) - p64)[big] / p64[big]).max())
    print(f"priors {what}: {len(ev)} nodes, widest {K}; device-spec64 abs {err:.3e} floor {floor:.3e} "
          f"({err / floor if floor else 0:.2f} floors), rel {rerr:.3e} floor {rfloor:.3e} "
          f"({rerr / rfloor if rfloor else 0:.2f} floors); exact nodes {int(exact.sum())}")
    assert err <= 8 * floor, (what, err, floor)
    assert rerr <= 8 * rfloor, (what, rerr, rfloor)
    return err, floor, rerr, rfloor, len(ev)


# ---- the specification on a case

class SpecRun:
    """One specification search of `state` (spec state) with the case's logits.  priors: key ->
    list of floats (a device's own priors replayed); default: Logits.prior32.  Holds the tree
    (records), root moves / visits / chosen index, the flush counts, or `capacity` (the
    puct_ref.Capacity raised)."""

    def __init__(self, logits, state, sims, bs, c, priors=None, prior_mutation=None, search_mutation=None,
                 max_level=None, slot_cap=None, root=None, order=None, reused=False):
        g = logits.game
        self.value_calls = self.prior_calls = 0

        def value_fn(s):
            self.value_calls += 1
            return logits.value(g.key(s))

        def prior_fn(node):
            self.prior_calls += 1
            k = g.key(node.s)
            return list(priors[_prior_key(g, k)]) if priors is not None else logits.prior32(k, prior_mutation)

        self.root = root if root is not None else puct_ref.Node(state, g.rules)
        self.order = order if order is not None else [self.root]
        self.capacity = None
        self.moves = self.N = self.best = None
        try:
            self.moves, self.N, self.best = puct_reuse_ref.search(
                self.root, sims, bs, c, value_fn, prior_fn, rules=g.rules, reused=reused, max_level=max_level,
                slot_cap=slot_cap, created=self.order, mutation=search_mutation)
        except puct_ref.Capacity as e:
            self.capacity = e
        self.tree = spec_tree(g, self.root, self.order)
        self.repeats = self.value_calls - self.prior_calls   # leaves pending more than once in a flush

    def flush_counts(self, sims, bs):
        """The leaves the device selects per flush (the `counts` its callback sees)."""
        out = [1] + [max(0, min(bs, sims - 1 - f * bs)) for f in range((sims - 1 + bs - 1) // bs)]
        if self.capacity is not None:
            first_empty = self.capacity.flush + (self.capacity.kind == "slots")
            out = [n if f < first_empty else 0 for f, n in enumerate(out)]
        return out


def _prior_key(game, key):
    """What a position's priors depend on: the row's position hash inputs and the move list."""
    return (key[0], key[1], key[3]) if game is Chess else key


def device_priors(game, tree):
    """key -> the device's priors of an evaluated position.  Positions that repeat in a tree hold
    the same row and move list, hence the same priors bit for bit (asserted)."""
    out = {}
    for r in tree:
        if r["evaluated"]:
            k = _prior_key(game, r["key"])
            p = [float(x) for x in r["P"]]
            assert out.setdefault(k, p) == p, k
    return out


# ---- the cases both test files run

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
KIWIPETE = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
POS3 = "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1"
LINE_FENS = [START, KIWIPETE, POS3]   # the line logits grow one level a flush from these
WIDE218 = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"   # test_gpu_puct_noise's wide roots
WIDE194 = "R6R/3Q4/1Q4Q1/4Q3/2Q5/5Q2/pp1Q4/kBNN1KB1 w - - 0 1"
SLOT_FEN = "kr6/pp1Q1q2/2Q2q2/3Q1q2/2Q1q3/1Q2q3/5QPP/6RK w - - 0 1"   # 73 moves a node on average
CHESS_FENS = LINE_FENS + [WIDE218, WIDE194, SLOT_FEN, "r1bqkbnr/pppp1ppp/2n5/4p3/2B1P3/5Q2/PPPP1PPP/RNB1K1NR w KQkq - 2 3",
                          "6k1/5ppp/8/8/8/8/5PPP/3R2K1 w - - 0 1"]


def c4_board(cols):
    b, t = "." * 42, 0
    for col in cols:
        b, t = oracle.play(b, t, col)
    return b, t


# 36 stones, nobody has four, columns 1, 3 and 6 full: full boards and wins a few plies below
C4_LATE = [0, 2, 6, 1, 3, 3, 3, 4, 6, 5, 1, 6, 6, 3, 3, 3, 4, 6, 5, 1, 1, 2, 6, 1, 1, 0, 0, 5, 5, 0, 2, 0, 5, 2, 0, 2]
C4_COLS = [[], [3, 3, 2, 4], [0, 0, 0, 0, 0, 0, 1, 2], C4_LATE, [1, 1, 2, 2, 4, 4, 5, 6, 6, 5, 0], C4_LATE[:34]]


class Case:
    """One launch: every root of the game under one kind of logits and one (sims, bs, c);
    roots_only: flush 0 runs on the roots alone (the backup's rows = 1 path)."""

    def __init__(self, game, kind, scale, half, sims, bs, c, roots_only, zero_values=False):
        self.game, self.kind, self.scale, self.half = game, kind, scale, half
        self.sims, self.bs, self.c, self.roots_only = sims, bs, c, roots_only
        self.zero_values = zero_values or kind == "line"
        # no masked move is ever selected: see check_priors
        self.masked_unvisited = kind == "mask" and zero_values and bs == 1

    def logits(self):
        return Logits(self.game, self.kind, self.scale, self.half, self.zero_values)

    def roots(self):
        if self.game is Chess:
            return [oracle.chess_from_fen(f) for f in CHESS_FENS]
        return [c4_board(cols) for cols in C4_COLS]

    @property
    def name(self):
        return f"{self.game.name}-{self.kind}{self.scale:g}-{'f16' if self.half else 'f32'}-{self.sims}x{self.bs}-c{self.c:g}" \
               f"{'-roots' if self.roots_only else ''}{'-v0' if self.zero_values else ''}"

    def spec(self, **kw):
        lg = self.logits()
        return [SpecRun(lg, s, self.sims, self.bs, self.c, **kw) for s in self.roots()]


CHESS_CASES = [Case(Chess, "hash", 3, False, 129, 8, 1.5, False), Case(Chess, "hash", 12, True, 131, 32, 2.5, True),
               Case(Chess, "hash", 0.05, False, 100, 1, 0.7, False), Case(Chess, "line", 40, True, 130, 8, 1.5, False),
               Case(Chess, "tie", 3, False, 67, 8, 1.5, True), Case(Chess, "mask", 3, True, 131, 32, 2.5, False),
               Case(Chess, "mask", 3, False, 90, 1, 1.5, False, zero_values=True)]
C4_CASES = [Case(C4, "hash", 3, False, 65, 8, 1.5, False), Case(C4, "hash", 12, True, 131, 32, 2.5, True),
            Case(C4, "mask", 3, False, 100, 1, 0.7, False), Case(C4, "tie", 3, True, 67, 8, 1.5, False),
            Case(C4, "line", 40, False, 130, 8, 1.5, True)]
CASES = CHESS_CASES + C4_CASES
