"""The trajectory recorder (include/zeroclone.h, "self-play trajectories on the device" and "root
visit counts as policy targets") in plain Python ints and lists, and a generator of scripted
self-play tables for it.  No GPU, no library: tests/test_gpu_traj_scripted.py holds the kernels
of csrc/selfplay.hip to this file, tests/test_traj_ref_cpu.py holds this file to the reference's
rules (Engine.play_move's history append, Engine.get_dataset's labels, Engine._evaluate's result,
scripts/train.py:simulate_games's refill and quota).
"""
from __future__ import annotations

import copy

import numpy as np

ONGOING, IDLE, SKIP = 2, 3, 4                 # ZC_C4_ONGOING, ZC_SLOT_IDLE, ZC_SLOT_SKIP
WIN, STALEMATE, FIFTY = 1, 2, 4               # ZC_CHESS_WIN / STALEMATE / FIFTY
UNLIMITED = 1 << 62
OV_POOL, OV_MAXLEN, OV_QUOTA = 1, 2, 4        # ZC_TRAJ_OVERFLOW bits
PI_SLOT, PI_POOL, PI_SAT = 1, 2, 4            # ZC_TRAJ_PI_OVERFLOW bits
MAX_COUNT = 65535


def labels_of(length: int, result: int) -> list[int]:
    """Engine.get_dataset: the factor starts at 0 (draw) or -1 at the opening, alternates, and the
    game's list is reversed: position i of `length` gets f * (-1)^(length - 1 - i)."""
    entry, f = [], (0 if result == 0 else -1)
    for _ in range(length):
        entry.append(f)
        f = -f
    return entry[::-1]


def chess_result(turn: int, flags: int, rep) -> int:
    """Engine._evaluate of the position after the move: check_win -> turn * 2 - 1 (the side to
    move now), first; check_draw (stalemate, fifty moves, a threefold repetition) -> 0."""
    if flags & WIN:
        return turn * 2 - 1
    if flags & (STALEMATE | FIFTY) or (rep is not None and rep == 3):
        return 0
    return ONGOING


def _row(r) -> tuple:
    return tuple(int(x) for x in r)


class TrajModel:
    """One trajectory pool and, with `slot_cap` given, the policy record beside it.

    State (Python ints, lists and tuples; a row is a tuple of row_bytes / 8 words):
      slot[g] = [positions so far, game number or -1]   d_slot[g][0:2]
      hist[g], hmoves[g]       the slot's game: len rows, len - 1 moves
      pool, labels, pool_moves [pool_cap], None = never written
      games                    [games_cap] of (game, slot, result, first, positions), None = never
      positions, n_games, next, quota, finished, overflow      d_ctl[0:6]
      slot_pi[g], slot_off[g]  the slot's entries and off[0 .. len - 1]
      pool_pi [pi_pool_cap], pool_first, pool_count [pool_cap], None = never written
      entries, pi_overflow     d_pctl[0:2]

    Always specified, whatever overflows: nothing is written outside the buffers; a slot that a
    step leaves alone (ZC_SLOT_SKIP, or idle apart from its row and result) keeps every word; the
    counters count every finished game, dropped ones included (POSITIONS adds its positions,
    GAMES, NEXT and FINISHED add one: NEXT keeps counting past the quota, and POSITIONS / GAMES
    may pass pool_cap / games_cap); a game that is not dropped has its record, rows, labels and
    moves exactly as without the overflow.

    ZC_TRAJ_OVERFLOW
      bit 0, a game dropped (first + positions > pool_cap, or its record's place >= games_cap,
        both taken from the counters, so every later game is dropped too): the dropped game writes
        nothing to d_pool, d_labels, d_pool_moves, d_games or the policy pool and reserves no
        policy entries; its slot restarts like any finished slot (opening, next game number or
        idle).  Everything stays specified.
      bit 1, a slot's game got a position past max_len: the slot keeps fill max_len and its game
        number, its rows below max_len - 1 and moves below max_len - 2.  Unspecified: that slot's
        last row and move, its policy CSR, and, once that game finishes, the pool (the single step
        pools it with max_len positions, the multi-step call with its true length, so places and
        counters differ).  Other slots stay specified until then.
      bit 2, a multi-step call met a refill at or past the quota: the slot goes idle as in single
        steps.  What the table holds for that slot after that step is not a recorded game, so the
        counters and places stay specified only if the slot has no later step (the call's last
        step, or ZC_SLOT_SKIP from there on).

    ZC_TRAJ_PI_OVERFLOW
      bit 0, a slot's entries passed slot_cap: the entries below slot_cap are kept, the others are
        lost and every offset is clamped to slot_cap; the pooled game carries the clamped record.
        Specified, and the same through single steps and the multi-step call.
      bit 1, a finished game's entries do not fit below pi_pool_cap (the place comes from the
        ENTRIES counter, which still adds them, so every later game with entries is dropped too):
        d_pool_first / d_pool_count of all the game's positions are 0 and d_pool_pi is not written.
        Everything stays specified.
      bit 2, a count above 65535: stored as 65535.  Everything stays specified.
    """

    def __init__(self, n, init, max_len, pool_cap, games_cap, quota=None, slot_cap=None, pi_pool_cap=0):
        self.n, self.init, self.max_len = n, _row(init), max_len
        self.pool_cap, self.games_cap = pool_cap, games_cap
        q = UNLIMITED if quota is None else int(quota)
        self.quota = q
        self.slot = [[1, g if g < min(q, n) else -1] for g in range(n)]
        self.hist = [[self.init] for _ in range(n)]
        self.hmoves = [[] for _ in range(n)]
        self.pool, self.labels, self.pool_moves = [None] * pool_cap, [None] * pool_cap, [None] * pool_cap
        self.games = [None] * games_cap
        self.positions = self.n_games = self.finished = self.overflow = 0
        self.next = min(q, n)
        self.unspecified = set()          # slots whose game passed max_len
        self.slot_cap = slot_cap
        if slot_cap is not None:
            self.pi_pool_cap = pi_pool_cap
            self.slot_pi = [[] for _ in range(n)]
            self.slot_off = [[0] for _ in range(n)]
            self.pool_pi = [None] * pi_pool_cap
            self.pool_first, self.pool_count = [None] * pool_cap, [None] * pool_cap
            self.entries = self.pi_overflow = 0
        self._placed = []

    # ------------------------------------------------------------------ one step
    def record(self, states, moves, results, flags=None, rep=None, _multi=False):
        """zc_traj_record_async.  `states` (n rows) and `results` (n ints) are lists and are
        updated in place as the call updates d_states and d_results."""
        fins = []
        for g in range(self.n):
            ln, game = self.slot[g]
            if game < 0:                                   # idle: held at the opening
                states[g] = self.init
                results[g] = IDLE
                continue
            if flags is None and int(results[g]) == SKIP:  # no move at this step
                if self.slot_cap is not None:              # an append before it counts for nothing
                    del self.slot_off[g][ln:]
                    del self.slot_pi[g][self.slot_off[g][ln - 1]:]
                continue
            row = _row(states[g])
            if flags is not None:
                r = chess_result(row[8] & 0xFF, int(flags[g]), None if rep is None else int(rep[g]))
                results[g] = r
            else:
                r = int(results[g])
            if ln >= self.max_len:
                self.overflow |= OV_MAXLEN
                self.unspecified.add(g)
                self.hist[g][self.max_len - 1] = row
                self.hmoves[g][self.max_len - 2] = int(moves[g])
            else:
                self.hist[g].append(row)
                self.hmoves[g].append(int(moves[g]))
                self.slot[g][0] = ln + 1
            if r != ONGOING:
                fins.append((g, r))
        self._placed = []
        for rank, (g, r) in enumerate(fins):               # slot order: numbers and places
            ln, game = self.slot[g]
            G, P = self.n_games, self.positions
            if P + ln > self.pool_cap or G >= self.games_cap:
                self.overflow |= OV_POOL
            else:
                lab = labels_of(ln, r)
                for i in range(ln):
                    self.pool[P + i] = self.hist[g][i]
                    self.labels[P + i] = lab[i]
                    self.pool_moves[P + i] = self.hmoves[g][i] if i + 1 < ln else -1
                self.games[G] = (game, g, r, P, ln)
                if self.slot_cap is not None:              # the commit takes the game's entries along
                    self._placed.append((g, P, ln, self.slot_off[g], self.slot_pi[g]))
            self.positions += ln
            self.n_games += 1
            self.finished += 1
            nx = self.next                                  # the refill: train.py:165-167
            self.next += 1
            if nx < self.quota:
                self.slot[g] = [1, nx]
            else:
                self.slot[g] = [1, -1]
                if _multi:
                    self.overflow |= OV_QUOTA
            self.hist[g], self.hmoves[g] = [self.init], []
            if self.slot_cap is not None:                  # its policy record starts over
                self.slot_off[g], self.slot_pi[g] = [0], []
            states[g] = self.init
            self.unspecified.discard(g)
        return states, results

    def policy_append(self, na, root_moves=None):
        """zc_traj_policy_append_async: before the step's record()."""
        for g in range(self.n):
            ln, game = self.slot[g]
            if game < 0:
                continue
            off, ent = self.slot_off[g], self.slot_pi[g]
            del off[ln:]
            base = off[ln - 1]
            del ent[base:]
            cnt = 0
            for j, c in enumerate(na[g]):
                c = int(c)
                if c <= 0:
                    continue
                if c > MAX_COUNT:
                    self.pi_overflow |= PI_SAT
                mid = int(root_moves[g][j]) & 0xFFFF if root_moves is not None else j
                if base + cnt < self.slot_cap:
                    ent.append(mid | min(c, MAX_COUNT) << 16)
                else:
                    self.pi_overflow |= PI_SLOT
                cnt += 1
            off.append(min(base + cnt, self.slot_cap))

    def policy_commit(self):
        """zc_traj_policy_commit_async: after the step's record().  The games that record() pooled
        get their entries' places in slot order."""
        for g, P, ln, off, ent in self._placed:
            total = off[ln - 1]
            at = self.entries
            self.entries += total
            if at + total > self.pi_pool_cap:
                self.pi_overflow |= PI_POOL
                for i in range(ln):
                    self.pool_first[P + i], self.pool_count[P + i] = 0, 0
                continue
            for i in range(ln):
                self.pool_first[P + i] = at + off[i]
                self.pool_count[P + i] = off[i + 1] - off[i] if i + 1 < ln else 0
            self.pool_pi[at:at + total] = ent[:total]
        self._placed = []

    def step(self, states, moves, results, na=None, root_moves=None, flags=None, rep=None, _multi=False):
        """One self-play step as the pools run it: append, record, commit."""
        if self.slot_cap is not None and na is not None:
            self.policy_append(na, root_moves)
        out = self.record(states, moves, results, flags, rep, _multi)
        if self.slot_cap is not None:
            self.policy_commit()
        return out

    # ------------------------------------------------------------------ a launch's steps
    @staticmethod
    def reached_steps(steps, reached):
        return steps if reached is None else min(steps, max(int(reached), 0))

    def record_steps(self, states, moves, results, steps, reached=None, na=None, root_moves=None):
        """zc_traj_policy_record_steps_async + zc_traj_record_steps_async: `steps` rounds of the
        single-step calls in step order over the steps below min(steps, max(reached, 0)).  The
        tables are not modified; a slot's ZC_SLOT_SKIP steps take no visit counts."""
        for k in range(self.reached_steps(steps, reached)):
            res = [int(x) for x in results[k]]
            nak = None
            if na is not None:
                nak = [na[k][g] if res[g] != SKIP else () for g in range(self.n)]
            self.step([_row(r) for r in states[k]], moves[k], res, nak,
                      None if root_moves is None else root_moves[k], _multi=True)

    def policy_record_steps(self, results, na, root_moves, steps, reached=None):
        """zc_traj_policy_record_steps_async alone, called before record_steps of the same launch:
        the policy record of those rounds; the trajectory pool is not changed."""
        twin = copy.deepcopy(self)
        blank = [[self.init] * self.n] * steps
        twin.record_steps(blank, [[0] * self.n] * steps, results, steps, reached, na, root_moves)
        for f in ("slot_pi", "slot_off", "pool_pi", "pool_first", "pool_count", "entries", "pi_overflow"):
            setattr(self, f, getattr(twin, f))

    def record_steps_after_policy(self, states, moves, results, steps, reached=None):
        """record_steps for a launch whose policy record was made by policy_record_steps."""
        keep = {f: getattr(self, f) for f in ("slot_pi", "slot_off", "pool_pi", "pool_first", "pool_count",
                                              "entries", "pi_overflow")}
        cap, self.slot_cap = self.slot_cap, None
        self.record_steps(states, moves, results, steps, reached)
        self.slot_cap = cap
        for f, v in keep.items():
            setattr(self, f, v)

    # ------------------------------------------------------------------ the batch
    def take(self):
        """Trajectories.take: the pooled games by game number, rows re-based game after game, the
        policy entries re-based to the batch's rows; the pool is emptied."""
        if self.overflow or (self.slot_cap is not None and self.pi_overflow):
            raise RuntimeError("overflow")
        recs = sorted(self.games[:self.n_games])
        out = {"rows": [], "labels": [], "moves": [], "games": []}
        if self.slot_cap is not None:
            out["pi_off"], out["pi"] = [0], []
        for game, g, r, first, ln in recs:
            out["games"].append((game, g, r, len(out["rows"]), ln))
            for p in range(first, first + ln):
                out["rows"].append(self.pool[p])
                out["labels"].append(self.labels[p])
                out["moves"].append(self.pool_moves[p])
                if self.slot_cap is not None:
                    f, c = self.pool_first[p], self.pool_count[p]
                    out["pi"] += self.pool_pi[f:f + c]
                    out["pi_off"].append(len(out["pi"]))
        self.positions = self.n_games = 0
        if self.slot_cap is not None:
            self.entries = 0
        return out


# ---------------------------------------------------------------------- scripted tables
def init_row(words: int) -> tuple:
    return tuple(0x1111111111110000 + w for w in range(words))


def row_of(g: int, j: int, p: int, words: int) -> tuple:
    """Position p >= 1 of the j-th game the table plays on slot g: every word names all four."""
    row = [(g + 1) << 48 | (j + 1) << 32 | p << 16 | w << 8 | 0xA5 for w in range(words)]
    if words == 9:                         # a zc_chess_state: byte 64 is the side to move
        row[8] = (row[8] & ~0xFF) | (p & 1)
    return tuple(row)


def move_of(g: int, j: int, p: int) -> int:
    """The move that made position p (int16, positive): injective for p < 37, j < 9 and g < 98,
    and never equal between neighbours in slot, game or position beyond that."""
    return (g * 331 + j * 37 + p) % 32749 + 1


def result_of(g: int, j: int) -> int:
    return (g + j) % 3 - 1


def na_row(g: int, j: int, p: int, stride: int, nnz: int, with_ids: bool):
    """The visit counts of the search from position p (p >= 0) with `nnz` non-zero cells spread
    over the row, every count and id a function of (slot, game, position, cell)."""
    na, ids = [0] * stride, [0] * stride
    for t in range(nnz):
        c = t * stride // nnz
        na[c] = 1 + (g * 3 + j * 5 + p * 7 + c * 11) % 1000
    if with_ids:
        # the low 12 bits (from / to) differ between the cells of a row of up to 256
        ids = [((g + 3 * p) & 15) << 12 | (c & 255) << 4 | ((g * 5 + j * 3 + p) & 15) for c in range(stride)]
    return na, ids


def default_nnz(g, j, p, stride):
    return (g + 2 * j + 3 * p) % (stride + 1)


def scripted(n, steps, row_bytes, lengths, stride=None, with_ids=False, nnz=default_nnz, chess=False,
             skip_after=None, skip_move=-1):
    """Tables [steps][n] for slots that play the games of `lengths[g]` (positions each, opening
    included, >= 2) one after the other and then go on without finishing.  `skip_after[g]` = k:
    slot g has no move from step k on (ZC_SLOT_SKIP, move `skip_move`).  Returns a dict of numpy
    arrays: states [steps][n][words] int64, moves int16, results int32; chess: flags and rep
    instead of meaningful results; with `stride`: na [steps][n][stride] int32 and root_moves
    uint16 (with_ids) of the search each step's move came from."""
    words = row_bytes // 8
    out = {"states": np.zeros((steps, n, words), np.int64), "moves": np.zeros((steps, n), np.int16),
           "results": np.full((steps, n), ONGOING, np.int32)}
    if chess:
        out["flags"] = np.zeros((steps, n), np.int32)
        out["rep"] = np.zeros((steps, n), np.int32)
    if stride:
        out["na"] = np.zeros((steps, n, stride), np.int32)
        out["root_moves"] = np.zeros((steps, n, stride), np.uint16) if with_ids else None
    for g in range(n):
        j, p = 0, 0                        # the game and the position the slot is at
        for k in range(steps):
            if skip_after is not None and skip_after[g] is not None and k >= skip_after[g]:
                out["results"][k, g] = SKIP
                out["moves"][k, g] = skip_move
                out["states"][k, g] = row_of(g, j, p, words) if p else init_row(words)
                continue
            if stride:
                na, ids = na_row(g, j, p, stride, nnz(g, j, p, stride), with_ids)
                out["na"][k, g] = na
                if with_ids:
                    out["root_moves"][k, g] = ids
            p += 1
            out["states"][k, g] = row_of(g, j, p, words)
            out["moves"][k, g] = move_of(g, j, p)
            ends = j < len(lengths[g]) and p + 1 == lengths[g][j]
            if ends:
                r = result_of(g, j)
                if chess and r:            # a decisive chess game: the side to move has lost
                    r = (p & 1) * 2 - 1
                out["results"][k, g] = r
                if chess:                  # the flags and repetition count that give r
                    if r == 0:
                        kind = (g + j + k) % 4
                        out["flags"][k, g] = (STALEMATE, FIFTY, STALEMATE | FIFTY, 0)[kind]
                        out["rep"][k, g] = 3 if kind == 3 else (g + k) % 3
                    else:                  # a win, whatever the draw bits say
                        out["flags"][k, g] = WIN | ((g + k) % 2) * FIFTY
                j, p = j + 1, 0
            elif chess:
                out["rep"][k, g] = (g + k) % 3
    return out
