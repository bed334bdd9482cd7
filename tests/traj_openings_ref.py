"""zc_traj_openings_async (include/zeroclone.h) in plain Python, on top of tests/traj_ref.py's
model of the recorder: a book of openings in place of the one d_init row.  No GPU, no library:
tests/test_gpu_openings.py holds the kernel to this file, tests/test_openings_cpu.py holds this
file to hand-written cases.

The rule.  After a step's record (and policy commit), and after the pool is started, every slot g
with a game number `game` >= 0 whose game has only its first position takes row
(game // share) % len(book) of the book as its root and as position 0 of its history.  Idle slots
stay at the opening the recorder gave them, games in progress are not touched, and the call can be
repeated.  share = 1: game g starts from opening g % N; share = 2: games 2k and 2k + 1 start from
opening k % N (an arena's pair of colours).
"""
from __future__ import annotations

from traj_ref import TrajModel, _row


def opening_of(game: int, book_rows: int, share: int) -> int:
    """The book's row of game number `game`."""
    return (game // share) % book_rows


class OpeningsModel(TrajModel):
    """`TrajModel` with a book: `seed(roots)` is the call; `start_roots()` gives the roots a
    started pool holds before it (every slot at d_init)."""

    def __init__(self, *args, book, share=1, **kw):
        super().__init__(*args, **kw)
        if len(book) < 1 or share < 1:
            raise ValueError("book_rows and share must be >= 1")
        self.book, self.share = [_row(r) for r in book], int(share)

    def start_roots(self) -> list:
        return [self.init] * self.n

    def seed(self, roots: list) -> list:
        """zc_traj_openings_async: `roots` (n rows) is updated in place as the call updates d_roots."""
        for g in range(self.n):
            ln, game = self.slot[g]
            if game < 0 or ln != 1:
                continue
            row = self.book[opening_of(game, len(self.book), self.share)]
            roots[g] = row
            self.hist[g][0] = row
        return roots

    def step_seeded(self, states, moves, results, roots, **kw):
        """One step as a pool with a book runs it: append, record, commit, seed.  `roots` are the
        positions the next search starts from: where the record restarted a slot (its row of
        `states` is d_init again) the play kernel has put d_init, elsewhere the position played."""
        out = self.step(states, moves, results, **kw)
        for g in range(self.n):
            roots[g] = _row(states[g])
        self.seed(roots)
        return out
